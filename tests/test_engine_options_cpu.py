"""CPU: EngineOptions, the one record of the engine's kernel / fusion switches (dafne_amd/engine_options.py): defaults and the
meaning of "0" / "1" per variable as the plan builders' inline comparisons had them, the dependent switches, and the record's place
in the packed weights.  No kernel runs."""
import dataclasses
import itertools
import os
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (variable, field, the comparison the builders made): "ne0" = env.get(NAME, "1") != "0", "eq1" = env.get(NAME, <default>) == "1"
SWITCHES = [
    ("DAFNE_RP_MFMA16", "rp_mfma16", "1", "ne0"),
    ("DAFNE_CONV_RP", "conv_rp", "1", "ne0"),
    ("DAFNE_CONV_WR", "conv_wr", "1", "ne0"),
    ("DAFNE_SHARED_EXCL", "shared_excl", "0", "eq1"),
    ("DAFNE_CONV_C64", "conv_c64", "0", "eq1"),
    ("DAFNE_INPLACE_RES", "inplace_res", "1", "ne0"),
    ("DAFNE_FUSE_STEM", "fuse_stem", "1", "ne0"),
    ("DAFNE_FUSE_STEM_CONV1", "fuse_stem_conv1", "1", "ne0"),
    ("DAFNE_FUSE_B2B", "fuse_b2b", "1", "ne0"),
    ("DAFNE_FUSE_B2B_NARROW", "fuse_b2b_narrow", "1", "ne0"),
    ("DAFNE_FUSE_B2B_MID", "fuse_b2b_mid", "1", "ne0"),
    ("DAFNE_FUSE_BNECK", "fuse_bneck", "1", "ne0"),
    ("DAFNE_FUSE_BLK_MID", "fuse_blk_mid", "1", "ne0"),
    ("DAFNE_FUSE_BLK_NARROW", "fuse_blk_narrow", "1", "ne0"),
    ("DAFNE_RES2_TAIL_S2", "res2_tail_s2", "1", "ne0"),
    ("DAFNE_FUSE_BNECK_LAST", "fuse_bneck_last", "1", "ne0"),
    ("DAFNE_P7_RELU_IN", "p7_relu_in", "1", "ne0"),
    ("DAFNE_FUSE_GN", "fuse_gn", "1", "ne0"),
    ("DAFNE_FUSE_GNFIN", "fuse_gnfin", "1", "ne0"),
    ("DAFNE_RP_PAIR", "rp_pair", "1", "ne0"),
    ("DAFNE_RP_PAIR_SHARED", "rp_pair_shared", "1", "eq1"),
    ("DAFNE_RP_LAYER0", "rp_layer0", "0", "eq1"),
    ("DAFNE_FUSE_GN_PRED", "fuse_gn_pred", "1", "ne0"),
]
DEFAULTS = dict(rp_mfma16=True, conv_rp=True, conv_wr=True, shared_excl=False, conv_c64=False, inplace_res=True, fuse_stem=True,
                fuse_stem_conv1=True, fuse_b2b=True, fuse_b2b_narrow=True, fuse_b2b_mid=True, fuse_bneck=True, fuse_blk_mid=True,
                fuse_blk_narrow=True, res2_tail_s2=True, fuse_bneck_last=True, p7_relu_in=True, fuse_gn=True, fuse_gnfin=True,
                rp_pair=True, rp_pair_shared=True, rp_layer0=False, fuse_gn_pred=True)


def _builders_value(env, name, default, rule):
    return env.get(name, default) != "0" if rule == "ne0" else env.get(name, default) == "1"


def test_defaults_and_the_field_list():
    from dafne_amd.engine_options import EngineOptions
    assert [f.name for f in dataclasses.fields(EngineOptions)] == [s[1] for s in SWITCHES] == list(DEFAULTS)
    assert dataclasses.asdict(EngineOptions.from_env({})) == DEFAULTS
    assert EngineOptions.from_env({}) == EngineOptions()
    assert dataclasses.asdict(EngineOptions.from_env({"DAFNE_HIP_GRAPHS": "0", "PATH": "/bin"})) == DEFAULTS      # not its variables
    with pytest.raises(dataclasses.FrozenInstanceError):
        EngineOptions().rp_mfma16 = False


@pytest.mark.parametrize("name,field,default,rule", SWITCHES)
def test_one_variable_at_a_time(name, field, default, rule):
    from dafne_amd.engine_options import EngineOptions
    for value in ("0", "1", "", "2"):
        env = {name: value}
        want = dict(DEFAULTS)
        want[field] = _builders_value(env, name, default, rule)
        assert dataclasses.asdict(EngineOptions.from_env(env)) == want, (name, value)
    assert EngineOptions.from_env({name: "0"}) == dataclasses.replace(EngineOptions(), **{field: False})
    assert EngineOptions.from_env({name: "1"}) == dataclasses.replace(EngineOptions(), **{field: True})


def test_from_env_reads_the_process_environment_by_default(monkeypatch):
    from dafne_amd.engine_options import EngineOptions
    for name, *_ in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    assert EngineOptions.from_env() == EngineOptions()
    monkeypatch.setenv("DAFNE_RP_MFMA16", "0")
    monkeypatch.setenv("DAFNE_RP_LAYER0", "1")
    assert EngineOptions.from_env() == dataclasses.replace(EngineOptions(), rp_mfma16=False, rp_layer0=True)


def test_dependent_switches_are_the_builders_and_chains():
    from dafne_amd.engine_options import EngineOptions
    names = ("fuse_b2b", "fuse_b2b_narrow", "fuse_b2b_mid", "fuse_bneck", "fuse_blk_mid", "fuse_blk_narrow")
    for bits in itertools.product((False, True), repeat=len(names)):
        o = EngineOptions(**dict(zip(names, bits)))
        b2b, narrow, mid, bneck, blk_mid, blk_narrow = bits
        fuse_narrow = b2b and narrow
        fuse_mid = b2b and mid
        assert o.b2b_narrow_on is fuse_narrow and o.b2b_mid_on is fuse_mid and o.bneck_on is (b2b and bneck)
        assert o.blk_mid_on is (fuse_mid and blk_mid) and o.blk_narrow_on is (fuse_narrow and blk_narrow)
    for pair, pair_shared, shared_gpu in itertools.product((False, True), repeat=3):
        o = EngineOptions(rp_pair=pair, rp_pair_shared=pair_shared)
        assert o.pair_towers(shared_gpu) is (pair and (not shared_gpu or pair_shared))


def _head_state_dict():
    """A DAFNeHead's state dict as tests/test_ablation_head_cpu.py builds it."""
    from dafne_amd.config import load_cfg
    from dafne_amd.modeling.dafne.dafne import DAFNeHead
    from oracle.model import fill_params
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"),
                   ["MODEL.DAFNE.CORNER_PREDICTION", "direct", "MODEL.DAFNE.CENTERNESS", "none"])
    head = DAFNeHead(cfg, [types.SimpleNamespace(channels=256)] * 5)
    fill_params(head, seed=4)
    return head.state_dict()


def test_packed_weights_carry_the_record_of_pack_time(monkeypatch):
    from dafne_amd import engine
    from dafne_amd.engine_options import EngineOptions
    for name, *_ in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    sd = _head_state_dict()
    monkeypatch.setenv("DAFNE_FUSE_GN_PRED", "0")
    P = engine.pack_head_weights(sd, "cpu", prefix="")
    want = dataclasses.replace(EngineOptions(), fuse_gn_pred=False)
    assert P["options"] == want
    monkeypatch.setenv("DAFNE_FUSE_GN_PRED", "1")
    monkeypatch.setenv("DAFNE_RP_MFMA16", "0")
    assert P["options"] == want and dict(P)["options"] is P["options"]         # (calibrate_fp8's copy carries it along)
    assert engine.pack_head_weights(sd, "cpu", prefix="")["options"] == dataclasses.replace(EngineOptions(), rp_mfma16=False)
    given = EngineOptions(conv_rp=False)
    assert engine.pack_head_weights(sd, "cpu", prefix="", options=given)["options"] is given


def test_one_resident_patch_form_per_packed_weights(monkeypatch):
    from dafne_amd import engine
    from dafne_amd.engine_options import EngineOptions
    monkeypatch.delenv("DAFNE_RP_MFMA16", raising=False)
    w = torch.randn(256, 2304, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    f16, f32 = engine.pack_conv3x3_frag16(w), engine.pack_conv3x3_frag(w)
    assert not torch.equal(f16, f32)
    # pack_rp: the record's form; with one argument the form a model packed now would use
    for opt, want, flag in ((EngineOptions(), f16, engine.F_FRAG16), (EngineOptions(rp_mfma16=False), f32, 0)):
        got, fl = engine.pack_rp(w, opt)
        assert torch.equal(got, want) and fl == flag
    assert engine.pack_rp(w)[1] == engine.F_FRAG16
    monkeypatch.setenv("DAFNE_RP_MFMA16", "0")
    assert engine.pack_rp(w)[1] == 0 and torch.equal(engine.pack_rp(w)[0], f32)
    # the plans' cache: P["options"] names the key, whatever the environment says by now, and never both keys
    P = {"options": EngineOptions()}
    wf, frag16 = engine.rp_weights(P, "cls_tower.0", w)
    assert frag16 is True and torch.equal(wf, f16) and engine.rp_weights(P, "cls_tower.0", w)[0] is wf
    assert [k for k in P if k != "options"] == ["cls_tower.0.frag16"]
    P = {"options": EngineOptions(rp_mfma16=False)}
    wf, frag16 = engine.rp_weights(P, "cls_tower.0", w)
    assert frag16 is False and torch.equal(wf, f32) and [k for k in P if k != "options"] == ["cls_tower.0.frag"]
    P["cls_tower.0.frag16"] = f16
    with pytest.raises(AssertionError):
        engine.rp_weights(P, "cls_tower.0", w)
