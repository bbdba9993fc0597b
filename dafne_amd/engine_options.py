"""The switches that choose a model's kernels and fusions, as ONE record.

EngineOptions.from_env() is the only reader of these environment variables.  The weight packers (engine.pack_model_weights /
pack_backbone_weights / pack_head_weights) call it once and keep the record as P["options"], next to P["fp8_kernel"]: every
plan a model builds over its life -- one-stream, pipelined sub-batches, TTA groups, calibration -- follows the same record,
whatever the environment says by then.  INTEGRATION.md ("Engine switches") has the table.

"bits": the field changes result bits.  "launches": it changes the launch list only; results are bit-identical.
"""
import os
from dataclasses import dataclass, field, fields


def _switch(env, default, only_1=False):
    """A field read from the variable `env`: on unless the variable is "0"; only_1: on only when it is "1"."""
    return field(default=default, metadata={"env": env, "only_1": only_1})


@dataclass(frozen=True)
class EngineOptions:
    # bits (<= 1 bf16 ulp per layer): the resident-operand kernels' matrix instruction: towers and res4.  16x16x32 (conv3x3_rp: weights
    # pack_conv3x3_frag16, flag F_FRAG16; conv_bneck: weights pack_bneck16, dafne_bottleneck_body16_hip); off: 32x32x16 in both
    rp_mfma16: bool = _switch("DAFNE_RP_MFMA16", True)
    # launches: the 256-channel 3x3 layers (towers, FPN outputs) on conv3x3_rp; off: conv3x3_patch
    conv_rp: bool = _switch("DAFNE_CONV_RP", True)
    # launches: the small-M layers engine.wr_takes names on conv_wr; off: conv_igemm / conv_stream
    conv_wr: bool = _switch("DAFNE_CONV_WR", True)
    # launches: the F_EXCL hint also on the launches of plans that share the GPU (the pipelined sub-batches)
    shared_excl: bool = _switch("DAFNE_SHARED_EXCL", False, only_1=True)
    # launches: res2's conv2 on the persistent conv3x3_c64 kernel
    conv_c64: bool = _switch("DAFNE_CONV_C64", False, only_1=True)
    # launches: whole-block kernels write their output over a shortcut operand that is dead after the block
    inplace_res: bool = _switch("DAFNE_INPLACE_RES", True)
    # launches: conv7x7/s2 + ReLU + max-pool in one kernel (stem_pool); off: convolution, then maxpool
    fuse_stem: bool = _switch("DAFNE_FUSE_STEM", True)
    # launches: ... and res2.0's conv1 on the pooled tile (stem_pool_conv1)
    fuse_stem_conv1: bool = _switch("DAFNE_FUSE_STEM_CONV1", True)
    # launches: conv3 + residual + ReLU + the next block's conv1 in one kernel (conv_b2b); gates the five fusions below it
    fuse_b2b: bool = _switch("DAFNE_FUSE_B2B", True)
    # launches: the same pair in res2 (conv_b2b_narrow, and res2.0's fused projection)
    fuse_b2b_narrow: bool = _switch("DAFNE_FUSE_B2B_NARROW", True)
    # launches: the same pair in res3 (conv_b2b_mid)
    fuse_b2b_mid: bool = _switch("DAFNE_FUSE_B2B_MID", True)
    # launches: res4's conv2 + conv3 + residual + next conv1 in one kernel (conv_bneck).  While rp_mfma16 is on the kernel runs its
    # 16x16x32 form, so 0 (the separate 32x32x16 launches) then also changes res4's bits; likewise fuse_bneck_last for the last block
    fuse_bneck: bool = _switch("DAFNE_FUSE_BNECK", True)
    # launches: a whole res3 block in one kernel (conv_blk_mid)
    fuse_blk_mid: bool = _switch("DAFNE_FUSE_BLK_MID", True)
    # launches: a whole res2 block in one kernel (conv_blk_narrow)
    fuse_blk_narrow: bool = _switch("DAFNE_FUSE_BLK_NARROW", True)
    # launches: res2's last block only at the pixels res3.0's stride-2 layers read (conv_blk_narrow_s2)
    res2_tail_s2: bool = _switch("DAFNE_RES2_TAIL_S2", True)
    # launches: res4's last block on conv_bneck's no-head form (conv_bneck_last)
    fuse_bneck_last: bool = _switch("DAFNE_FUSE_BNECK_LAST", True)
    # launches: P7 rectifies P6 on load (F_RELU_INPUT); off: a relu_copy launch and a rectified copy of P6
    p7_relu_in: bool = _switch("DAFNE_P7_RELU_IN", True)
    # launches: a tower layer's GroupNorm + ReLU applied by its consumer on load (F_GNIN); off: a groupnorm pass per layer
    fuse_gn: bool = _switch("DAFNE_FUSE_GN", True)
    # launches: the GroupNorm statistics finalised inside the producing convolution (F_GNFIN); off: groupnorm_finalize launches
    fuse_gnfin: bool = _switch("DAFNE_FUSE_GNFIN", True)
    # launches: cls_tower.i and its partner tower's layer i as one launch of conv3x3_rp
    rp_pair: bool = _switch("DAFNE_RP_PAIR", True)
    # launches: ... in the plans that share the GPU as well
    rp_pair_shared: bool = _switch("DAFNE_RP_PAIR_SHARED", True, only_1=True)
    # launches: the FPN-fed tower layer 0 of a small plan on conv3x3_rp (otherwise the generic tile + groupnorm_finalize)
    rp_layer0: bool = _switch("DAFNE_RP_LAYER0", False, only_1=True)
    # launches: the prediction convolutions (and corners_tower.0) normalise the towers' last layer on load
    fuse_gn_pred: bool = _switch("DAFNE_FUSE_GN_PRED", True)

    @classmethod
    def from_env(cls, env=os.environ):
        kw = {}
        for f in fields(cls):
            v = env.get(f.metadata["env"])
            if v is not None:
                kw[f.name] = (v == "1") if f.metadata["only_1"] else (v != "0")
        return cls(**kw)

    # what the plan builders ask: a fusion runs when its own switch and the ones it depends on are on
    @property
    def b2b_narrow_on(self):
        return self.fuse_b2b and self.fuse_b2b_narrow

    @property
    def b2b_mid_on(self):
        return self.fuse_b2b and self.fuse_b2b_mid

    @property
    def bneck_on(self):
        return self.fuse_b2b and self.fuse_bneck

    @property
    def blk_mid_on(self):
        return self.b2b_mid_on and self.fuse_blk_mid

    @property
    def blk_narrow_on(self):
        return self.b2b_narrow_on and self.fuse_blk_narrow

    def pair_towers(self, shared_gpu):
        return self.rp_pair and (not shared_gpu or self.rp_pair_shared)
