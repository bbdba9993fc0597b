"""GPU: every engine switch held to its label on WHOLE models (dafne_amd/engine_options.py, INTEGRATION.md "Engine switches").

The kernel tests prove "fused kernel == the separate launches" on hand-made operands; this module proves it where DensePlan /
HeadPlan wire the kernels together -- pool recycling, in-place block outputs, the stem_y1 / y1_next hand-offs, the compact res2
map, the deferred maps of the paired towers, the GroupNorm-on-load triples -- by building a fresh model per switch record and
comparing everything a plan leaves behind, bit for bit:

 1a  rp_mfma16 off (every resident-operand kernel in the 32x32x16 form): each of the 14 "launches" switches flipped alone
     reproduces the defaults.  The 8 switches the matrix found to move last-place roundings (BITS_1A, with the cause of each) are
     anchored on either side of that rounding: the defaults with the switch flipped == the same record with all launches switches
     off, with conv_wr on and off; and "plain" (all 23 switches off: a chain of generic launches, each held to fp64 by
     tests/test_gpu_conv_matrix.py) == the defaults with rp_mfma16, conv_wr and the GroupNorm bits switches off.
 1b  rp_mfma16 on (production): a launches flip that leaves the number of 16x16x32 layer executions alone reproduces the
     defaults; the switches that change that number are a declared list, equal to the observed one.
 1c  R101, 1d one ablation head (direct corners, no centerness): the plain anchor and the launches-off anchor.
 2   a plan run again over NaN-filled buffers gives the same finite bits: nothing is read that the run did not write.

Each flip must change the launch list, a flag or the aliasing of some plan at some shape (a vacuous case fails)."""
import dataclasses
import os
import sys

import pytest
import torch

from dafne_amd import engine
from _engine_switches import (DEFAULT, FIELDS, PLAIN, describe, environment, flip, frag16_executions, gn_buffers, head_tensors,
                              mismatch_message, names, signature)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, h, w) with splits = 2 in the pipelined run.  R50 at the smallest sizes that reach the branches:
#   (2, 64, 96)    every level ragged, P7 one pixel, the small-M layers on conv_wr, sub-batches of one image
#   (1, 544, 544)  the smallest square at which an FPN output (fpn_output3) is on conv3x3_rp
#                  (test_one_resident_patch_form_per_model_whatever_the_environment_says_later)
#                  and the towers' layer 0 beside it, so that the towers run as pairs (rp_pair; rp_pair_shared in the shared-GPU
#                  plan of the pipelined run) -- in smaller plans layer 0 is on the generic tile and nothing pairs
#   (3, 128, 160)  sub-batch plans of 2 + 1 images that share the GPU (shared_excl), rp_layer0's small plans
SHAPES = [(2, 64, 96), (1, 544, 544), (3, 128, 160)]
SMALLEST = SHAPES[:1]
SPLITS = 2

B0 = dataclasses.replace(DEFAULT, rp_mfma16=False)
# a switch that acts only behind another one is flipped with that one off on both sides: conv_c64 takes res2's conv2 launches,
# which exist only when the whole-block kernels (fuse_blk_narrow) do not run them.  (B0 with fuse_blk_narrow off is itself a case.)
CONTEXT = {"conv_c64": {"fuse_blk_narrow": False}}
SWITCHES = [f for f in FIELDS if f != "rp_mfma16"]

# "bits" switches of 1a: the two sides legitimately round or group an fp32 sum differently (found by this matrix, cause read from
# the kernels), so the flip gets anchor pairs of its own (test_1a_bits_switch_anchor_pairs) instead of an equality with the defaults.
#   conv_wr          splits K over several workgroups where the launch is small and adds the fp32 partial slabs in slice order; the
#                    generic kernels run K in one pass (tests/test_gpu_conv.py::test_conv_wr_vs_igemm_and_torch: <= 1 bf16 ulp)
#   fuse_b2b, fuse_bneck, fuse_bneck_last
#                    launches by themselves (held with conv_wr off on both sides) -- but the res4 layers they leave to launches of
#                    their own are small-M layers engine.wr_takes names (conv1 1024 -> 256 up to 5000 pixels per image, conv2 up to
#                    1250), so with conv_wr on those layers move from the fused kernels' one-pass K sum to conv_wr's slices
#   conv_rp, fuse_gn, fuse_gn_pred
#                    conv3x3_rp normalises on load as max(a x + b, 0) with a = rstd gamma, b = beta - mean a (conv.hip, gn_piece);
#                    the groupnorm pass and the patch / slab / pred16 kernels evaluate (x - mean) rstd gamma + beta: a handful of
#                    bf16 roundings per map differ.  conv_rp also trades conv3x3_patch's fp32 grouping of the K sum for
#                    conv3x3_rp's (about 2 of 10 000 outputs round the other way on random maps); fuse_gn off moves the towers of
#                    a small plan from conv3x3_rp to the generic tile
#   rp_layer0        the FPN-fed layer on conv3x3_rp's 8 x 32 tiles instead of the generic tile: the GroupNorm statistics are
#                    summed tile by tile in fp32, so other tiles give other last bits of mean / rstd
WR_DEPENDENT = ("fuse_b2b", "fuse_bneck", "fuse_bneck_last")
GN_BITS = ("conv_rp", "fuse_gn", "fuse_gn_pred", "rp_layer0")
BITS_1A = ("conv_wr",) + WR_DEPENDENT + GN_BITS
LAUNCHES = [f for f in SWITCHES if f not in BITS_1A]          # "launches" switches: a flip reproduces the defaults bit for bit

# 1b: the switches whose flip changes how many layers run in the 16x16x32 form at SHAPES (a condition, not a tolerance: those
# flips are held in the neutral form by 1a)
FORM_CHANGING = {"conv_rp", "rp_layer0", "fuse_b2b", "fuse_bneck", "fuse_bneck_last", "fuse_gn", "fuse_gn_pred"}


def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------ models
def _released(depth):
    def make():
        sys.path.insert(0, ROOT)
        import bench
        return bench.build_model(depth, dev(), seed=0)[1]
    return make


def _direct_none():
    """CORNER_PREDICTION direct, CENTERNESS none, as tests/test_gpu_ablation_head.py::ablation_model builds it (uncached: the
    switches are read when a model packs its weights)."""
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.registry import build_model
    from oracle import model as om
    from oracle.model import fill_params
    from test_gpu_ablation_head import cfg_for
    cfg = cfg_for("direct", "none")
    m = build_model(cfg)
    fill_params(m.proposal_generator.dafne_head, seed=5)
    sd = m.state_dict()
    sd.update({k: v for k, v in om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=5).items()
               if k.startswith("backbone.")})
    m.load_state_dict(sd)
    m.to(dev())
    m.invalidate()
    return m


MODELS = {"r50": _released(50), "r101": _released(101), "direct_none": _direct_none}


def fresh_model(kind, opt, monkeypatch):
    for k, v in environment(opt).items():
        monkeypatch.setenv(k, v)
    m = MODELS[kind]()
    assert m._weights()["options"] == opt
    return m


def batch_of(n, h, w):
    g = torch.Generator().manual_seed(100 + n + h)
    return torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(dev())


def record_shape(model, n, h, w):
    batch = batch_of(n, h, w)
    rows, counts = model.detect_packed(batch)
    torch.cuda.synchronize()
    plan = model.plan(n, h, w)
    r = {"serial": (rows.clone(), counts.clone()), "feats": [[a.t.clone() for a in plan.features]], "head": head_tensors(plan.head)}
    rows, counts = model.detect_packed(batch, pipelined=True, splits=SPLITS)
    torch.cuda.synchronize()
    st = model._pipe[(n, h, w, min(SPLITS, n))]
    subs = st["plans"][0]
    r["pipelined"] = (rows.clone(), counts.clone())
    r["pipelined feats"] = [[a.t.clone() for a in p.features] for p in subs]
    r["pipelined head"] = head_tensors(st["ho"][0])
    r["names"], r["sub_names"] = names(plan), [names(p) for p in subs]
    r["sig"] = [signature(p) for p in [plan] + subs]
    r["frag16"] = tuple(frag16_executions(p) for p in [plan] + subs)
    assert all(float(f.float().abs().max()) > 0 for f in r["feats"][0])
    return r


_RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_records():
    yield
    _RECORDS.clear()            # (device tensors of every record: not kept for the rest of the session)


def record(kind, opt, shapes, monkeypatch):
    """{shape: what the model `kind` under `opt` leaves behind}: one model build per (kind, opt) and module."""
    key = (kind, opt)
    if key not in _RECORDS:
        model = fresh_model(kind, opt, monkeypatch)
        _RECORDS[key] = {s: record_shape(model, *s) for s in shapes}
        del model
        torch.cuda.synchronize()
    assert list(_RECORDS[key]) == list(shapes)
    return _RECORDS[key]


def assert_same(tag, base, other, shapes=None):
    for s in (shapes if shapes is not None else list(base)):
        msg = mismatch_message(tag, s, base[s], other[s])
        assert msg is None, msg


def assert_not_vacuous(tag, base, other):
    assert any(base[s]["sig"] != other[s]["sig"] for s in base), \
        "%s: no plan at %s differs in its launch list, its F_EXCL / F_GNIN / F_GNFIN / F_FRAG16 bits or its aliasing" % (tag, list(base))


def launches_off(opt):
    """`opt` with every "launches" switch off: the bits switches alone decide what this model computes."""
    return dataclasses.replace(opt, **{f: False for f in LAUNCHES})


def sides(mode, name):
    base = dataclasses.replace(mode, **CONTEXT.get(name, {}))
    return base, flip(base, name)


# ------------------------------------------------------------------------------------------------------------ 1. the matrix
def test_every_switch_has_a_case():
    from dafne_amd.engine_options import EngineOptions
    assert sorted(SWITCHES + ["rp_mfma16"]) == sorted(f.name for f in dataclasses.fields(EngineOptions))
    assert set(BITS_1A) <= set(SWITCHES) and FORM_CHANGING <= set(SWITCHES) and set(CONTEXT) <= set(LAUNCHES)
    assert sorted(LAUNCHES + list(BITS_1A)) == sorted(SWITCHES) and len(set(BITS_1A)) == len(BITS_1A)
    assert PLAIN == EngineOptions(**{f.name: False for f in dataclasses.fields(EngineOptions)})


@pytest.mark.parametrize("name", SWITCHES)
def test_1a_generic_form_one_flip_same_bits(name, monkeypatch):
    """rp_mfma16 off.  The defaults (B0) against B0 with `name` flipped: the five FPN maps, every head output, (rows, counts) of
    detect_packed serial and pipelined over 2 sub-batches -- and the sub-batch plans' own FPN maps and head outputs -- are
    torch.equal at every shape.  The switches of BITS_1A are held by test_1a_bits_switch_anchor_pairs instead; every flip must
    change some plan."""
    a, b = sides(B0, name)
    base, other = record("r50", a, SHAPES, monkeypatch), record("r50", b, SHAPES, monkeypatch)
    assert_not_vacuous(name, base, other)
    assert all(k == 0 for s in base for k in base[s]["frag16"] + other[s]["frag16"])
    if name not in BITS_1A:
        assert_same("%s (%s against %s)" % (name, describe(b), describe(a)), base, other)


def test_1a_generic_anchors(monkeypatch):
    """plain (every switch off: generic launches only, each held to fp64 by tests/test_gpu_conv_matrix.py) == the defaults with
    rp_mfma16, conv_wr and the GroupNorm bits switches off; plain with conv_wr on == the defaults with rp_mfma16, the GroupNorm
    bits switches and fuse_b2b off (so that res4's small-M layers are launches conv_wr takes on both sides)."""
    gn_off = {f: False for f in GN_BITS}
    plain = record("r50", PLAIN, SHAPES, monkeypatch)
    generic = record("r50", dataclasses.replace(B0, conv_wr=False, **gn_off), SHAPES, monkeypatch)
    for s in SHAPES:
        assert not any(n.startswith(("conv_b", "conv_wr", "conv3x3_rp", "conv3x3_c64", "stem_pool")) for n in plain[s]["names"]), plain[s]["names"]
        assert not any(f & ~engine.F_EXCL for _, fl, _ in plain[s]["sig"][0] for f in fl)
    assert_not_vacuous("plain", plain, generic)
    assert_same("plain against defaults rp_mfma16=0 conv_wr=0 conv_rp=0 fuse_gn=0 fuse_gn_pred=0", plain, generic)
    plain_wr = record("r50", dataclasses.replace(PLAIN, conv_wr=True), SHAPES, monkeypatch)
    generic_wr = record("r50", dataclasses.replace(B0, fuse_b2b=False, **gn_off), SHAPES, monkeypatch)
    assert all("conv_wr" in plain_wr[s]["names"] for s in SHAPES)
    assert_not_vacuous("plain + conv_wr", plain_wr, generic_wr)
    assert_same("plain + conv_wr against defaults rp_mfma16=0 fuse_b2b=0 conv_rp=0 fuse_gn=0 fuse_gn_pred=0", plain_wr, generic_wr)


@pytest.mark.parametrize("name", BITS_1A)
def test_1a_bits_switch_anchor_pairs(name, monkeypatch):
    """A bits switch S of 1a, with conv_wr on and with conv_wr off: the defaults with S flipped == the same record with every
    "launches" switch off.  So whatever S does to the bits, the 14 launches switches together still change none of them beside
    it (for conv_wr itself: the defaults and the defaults without it).  The res4 fusion switches are launches switches as long
    as conv_wr does not take the layers they set free: with conv_wr off the flip reproduces the defaults."""
    for wr in (True, False):
        x = dataclasses.replace(B0, conv_wr=wr)
        if name != "conv_wr":
            x = flip(x, name)
        full, bare = record("r50", x, SHAPES, monkeypatch), record("r50", launches_off(x), SHAPES, monkeypatch)
        assert_not_vacuous(describe(x), full, bare)
        assert_same("every launches switch off against %s" % describe(x), full, bare)
    if name in WR_DEPENDENT:
        w0 = dataclasses.replace(B0, conv_wr=False)
        base, other = record("r50", w0, SHAPES, monkeypatch), record("r50", flip(w0, name), SHAPES, monkeypatch)
        assert_not_vacuous(name, base, other)
        assert_same("%s (%s against %s)" % (name, describe(flip(w0, name)), describe(w0)), base, other)


def test_rp_mfma16_changes_the_form_of_every_resident_operand_launch(monkeypatch):
    """The mode axis itself: the defaults against rp_mfma16 off differ in F_FRAG16 / the conv_bneck entry and in nothing else of
    the launch lists."""
    d, b0 = record("r50", DEFAULT, SHAPES, monkeypatch), record("r50", B0, SHAPES, monkeypatch)
    assert_not_vacuous("rp_mfma16", b0, d)
    for s in SHAPES:
        assert d[s]["names"] == b0[s]["names"] and d[s]["sub_names"] == b0[s]["sub_names"]
        assert all(k > 0 for k in d[s]["frag16"]) and all(k == 0 for k in b0[s]["frag16"])


@pytest.mark.parametrize("name", SWITCHES)
def test_1b_production_form_neutral_flip_same_bits(name, monkeypatch):
    """rp_mfma16 on.  Where the flip leaves the count of 16x16x32 layer executions of every plan of a shape alone it must
    reproduce the defaults bit for bit; whether it does so at every shape is what FORM_CHANGING declares."""
    a, b = sides(DEFAULT, name)
    base, other = record("r50", a, SHAPES, monkeypatch), record("r50", b, SHAPES, monkeypatch)
    assert_not_vacuous(name, base, other)
    neutral = [s for s in SHAPES if base[s]["frag16"] == other[s]["frag16"]]
    print(name, "form-neutral at", neutral, {s: (base[s]["frag16"], other[s]["frag16"]) for s in SHAPES})
    assert (len(neutral) < len(SHAPES)) == (name in FORM_CHANGING), (name, neutral)
    if name not in BITS_1A:         # (a switch that moves bits in the generic form moves them here for the same reason)
        assert_same("%s (%s against %s)" % (name, describe(b), describe(a)), base, other, neutral)


# the direct head also at 544 x 544: only there its towers run as pairs (cls_tower with corners_tower, the non-stacked partner)
OTHER_MODELS = {"r101": SMALLEST, "direct_none": SHAPES[:2]}


@pytest.mark.parametrize("kind", sorted(OTHER_MODELS))
def test_1cd_anchors_on_the_other_models(kind, monkeypatch):
    """R101 (23 res4 blocks: the pool's recycling runs 17 blocks longer) and the direct / no-centerness head (cls tower paired
    with the corners tower, 8 prediction channels): plain == the defaults with rp_mfma16, conv_wr and the GroupNorm bits switches
    off, and the defaults with rp_mfma16 off == the same with every launches switch off."""
    shapes = OTHER_MODELS[kind]
    plain = record(kind, PLAIN, shapes, monkeypatch)
    generic = record(kind, dataclasses.replace(B0, conv_wr=False, **{f: False for f in GN_BITS}), shapes, monkeypatch)
    assert_not_vacuous(kind, plain, generic)
    assert_same("%s: plain against defaults rp_mfma16=0 conv_wr=0 conv_rp=0 fuse_gn=0 fuse_gn_pred=0" % kind, plain, generic)
    b0, bare = record(kind, B0, shapes, monkeypatch), record(kind, launches_off(B0), shapes, monkeypatch)
    assert_not_vacuous(kind, b0, bare)
    assert_same("%s: every launches switch off against defaults rp_mfma16=0" % kind, b0, bare)
    if kind == "direct_none":
        h = plain[shapes[0]]["head"]
        assert [n for n, l, _ in h if l == 0] == ["logits", "delta_ctr"] and h[-1][2].shape[-1] == 8
        assert b0[shapes[1]]["names"].count("conv3x3_rp") < bare[shapes[1]]["names"].count("conv3x3_rp")      # pairs


def test_1c_r101_defaults_twice_same_bits(monkeypatch):
    d1 = record("r101", DEFAULT, SMALLEST, monkeypatch)
    model = fresh_model("r101", DEFAULT, monkeypatch)
    d2 = {s: record_shape(model, *s) for s in SMALLEST}
    assert all(k > 0 for k in d1[SMALLEST[0]]["frag16"])
    assert_same("R101 defaults, a second model", d1, d2)


# ------------------------------------------------------------------------ 2. nothing is read that this run did not write
@pytest.mark.parametrize("n,h,w", SHAPES[:2])
@pytest.mark.parametrize("which", ["defaults", "plain"])
def test_2_second_run_over_nan_filled_buffers_same_bits(which, n, h, w, monkeypatch):
    """Run the plan, then fill the interior of every activation buffer the plan owns (engine.Act, recorded while the plan is
    built; halos stay zero, stem_in and the split-K workspace are left alone), the fp32 head outputs and the GroupNorm partial /
    statistics buffers with NaN, and run it again: every recorded tensor is finite and has the bits of the first run.  So a
    recycled pool buffer is never read before its new producer wrote it, the compact res2 map is read only where it was written,
    and an in-place block reads its own X before storing over it."""
    model = fresh_model("r50", DEFAULT if which == "defaults" else PLAIN, monkeypatch)
    acts = []

    class RecordedAct(engine.Act):
        def __init__(self, *a):
            super().__init__(*a)
            acts.append(self)

    batch = batch_of(n, h, w)
    with monkeypatch.context() as mp:
        mp.setattr(engine, "Act", RecordedAct)
        rows, counts = model.detect_packed(batch, graphs=False)
    torch.cuda.synchronize()
    plan = model.plan(n, h, w)
    assert plan.graph is None and len(acts) >= 20 and all(any(f is a for a in acts) for f in plan.features)
    first = {"feats": [[a.t.clone() for a in plan.features]], "head": head_tensors(plan.head), "serial": (rows.clone(), counts.clone())}
    nan = float("nan")
    for a in acts:
        a.t[:, 1:-1, 1:-1, :] = nan
    gn = gn_buffers(plan)
    assert len(gn) >= 24
    for t in gn + [t for v in (plan.head.logits, plan.head.delta_ctr, plan.head.center, plan.head.corners) if v is not None for t in v]:
        t.fill_(nan)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(f.t[:, 1:-1, 1:-1]).all()) for f in plan.features) and bool(torch.isnan(plan.head.logits[0]).all())
    plan.run()                      # (stem_in still holds the preprocessed batch)
    torch.cuda.synchronize()
    again = {"feats": [[a.t.clone() for a in plan.features]], "head": head_tensors(plan.head)}
    for l, f in enumerate(again["feats"][0]):
        assert bool(torch.isfinite(f.float()).all()), ("FPN level", l)
    for nme, l, t in again["head"]:
        assert bool(torch.isfinite(t).all()), (nme, l)
    rows, counts = model.detect_packed(batch, graphs=False)
    torch.cuda.synchronize()
    again["serial"] = (rows.clone(), counts.clone())
    for r in (first, again):
        r.update({"pipelined feats": [], "pipelined head": [], "pipelined": r["serial"], "names": names(plan), "sub_names": []})
    msg = mismatch_message("%s, second run over NaN" % which, (n, h, w), first, again)
    assert msg is None, msg
