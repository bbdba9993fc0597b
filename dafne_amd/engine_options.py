"""The switches that choose a model's kernels and fusions, as ONE record.

EngineOptions.from_env() is the only reader of these environment variables.  The weight packers (engine.pack_model_weights /
pack_backbone_weights / pack_head_weights) call it once and keep the record as P["options"], next to P["fp8_kernel"]: every
plan a model builds over its life -- one-stream, pipelined sub-batches, TTA groups, calibration -- follows the same record,
whatever the environment says by then.  INTEGRATION.md ("Engine switches") has the table.

"bits": the field changes result bits.  "launches": it changes the launch list only; results are bit-identical.
tests/test_gpu_engine_switches.py holds every label on whole models: a "launches" flip reproduces the defaults' FPN maps, head outputs
and detections bit for bit; a "bits" flip is anchored on either side of the rounding it changes.
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
    # bits (last-place roundings): the 256-channel 3x3 layers (towers, FPN outputs) on conv3x3_rp; off: conv3x3_patch.  conv3x3_rp
    # groups the fp32 K sum unlike conv3x3_patch and normalises on load as max(a x + b, 0), a = rstd gamma, b = beta - mean a, where
    # every other kernel evaluates (x - mean) rstd gamma + beta: tower layers 1-3, corners_tower.0, an FPN output it takes
    conv_rp: bool = _switch("DAFNE_CONV_RP", True)
    # bits (<= 1 bf16 ulp per layer): the small-M layers engine.wr_takes names on conv_wr, which splits K into slices and adds the
    # fp32 partial slabs in slice order (res5, res4.0 conv1, FPN laterals 5 / 4, FPN outputs, P6, P7; res4's conv1 / conv2 when
    # they are launches of their own); off: conv_igemm / conv_stream, K in one pass
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
    # launches: conv3 + residual + ReLU + the next block's conv1 in one kernel (conv_b2b); gates the five fusions below it.  With
    # conv_wr on also bits: off, res4's conv1 (up to 5000 pixels per image) and conv2 (up to 1250) are launches conv_wr takes
    fuse_b2b: bool = _switch("DAFNE_FUSE_B2B", True)
    # launches: the same pair in res2 (conv_b2b_narrow, and res2.0's fused projection)
    fuse_b2b_narrow: bool = _switch("DAFNE_FUSE_B2B_NARROW", True)
    # launches: the same pair in res3 (conv_b2b_mid)
    fuse_b2b_mid: bool = _switch("DAFNE_FUSE_B2B_MID", True)
    # launches: res4's conv2 + conv3 + residual + next conv1 in one kernel (conv_bneck).  While rp_mfma16 is on the kernel runs its
    # 16x16x32 form, so 0 (the separate 32x32x16 launches) then also changes res4's bits; likewise fuse_bneck_last for the last block.
    # With conv_wr on also bits: off, res4's conv2 (up to 1250 pixels per image) is a launch conv_wr takes
    fuse_bneck: bool = _switch("DAFNE_FUSE_BNECK", True)
    # launches: a whole res3 block in one kernel (conv_blk_mid)
    fuse_blk_mid: bool = _switch("DAFNE_FUSE_BLK_MID", True)
    # launches: a whole res2 block in one kernel (conv_blk_narrow)
    fuse_blk_narrow: bool = _switch("DAFNE_FUSE_BLK_NARROW", True)
    # launches: res2's last block only at the pixels res3.0's stride-2 layers read (conv_blk_narrow_s2)
    res2_tail_s2: bool = _switch("DAFNE_RES2_TAIL_S2", True)
    # launches: res4's last block on conv_bneck's no-head form (conv_bneck_last).  With conv_wr on also bits: off, that block's
    # conv2 (up to 1250 pixels per image) is a launch conv_wr takes
    fuse_bneck_last: bool = _switch("DAFNE_FUSE_BNECK_LAST", True)
    # launches: P7 rectifies P6 on load (F_RELU_INPUT); off: a relu_copy launch and a rectified copy of P6
    p7_relu_in: bool = _switch("DAFNE_P7_RELU_IN", True)
    # bits (last-place roundings): a tower layer's GroupNorm + ReLU applied by its consumer on load (F_GNIN); off: a groupnorm pass per
    # layer, which evaluates (x - mean) rstd gamma + beta where conv3x3_rp computes a x + b (conv_rp), and the towers of a small plan
    # on the generic tile: tower layers 1-3
    fuse_gn: bool = _switch("DAFNE_FUSE_GN", True)
    # launches: the GroupNorm statistics finalised inside the producing convolution (F_GNFIN); off: groupnorm_finalize launches
    fuse_gnfin: bool = _switch("DAFNE_FUSE_GNFIN", True)
    # launches: cls_tower.i and its partner tower's layer i as one launch of conv3x3_rp
    rp_pair: bool = _switch("DAFNE_RP_PAIR", True)
    # launches: ... in the plans that share the GPU as well
    rp_pair_shared: bool = _switch("DAFNE_RP_PAIR_SHARED", True, only_1=True)
    # bits (last bits of mean / rstd): the FPN-fed tower layer 0 of a small plan on conv3x3_rp (otherwise the generic tile +
    # groupnorm_finalize): the GroupNorm statistics are summed tile by tile in fp32, and the two kernels tile the maps differently
    rp_layer0: bool = _switch("DAFNE_RP_LAYER0", False, only_1=True)
    # bits (last-place roundings): the prediction convolutions (and corners_tower.0) normalise the towers' last layer on load.  The
    # prediction kernels evaluate the groupnorm pass's expression (same bits); corners_tower.0 on conv3x3_rp does not (conv_rp)
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
