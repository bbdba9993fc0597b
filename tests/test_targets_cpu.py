"""CPU: the numpy restatement of the reference's target assignment and losses (tests/_targets_np.py) against the reference's own
results (tests/golden/dafne_targets.npz, made by tests/golden/make_golden_targets.py), the C ABI of the two kernels, and the
host helpers.  The kernels themselves are compared with the restatement in tests/test_gpu_targets.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _targets_np as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "dafne_targets.npz"))


@pytest.fixture(scope="module")
def assigned():
    gts, shapes = tn.case_a()
    return {name: tn.assign(gts, shapes, tn.assign_config(name)) for name in tn.ASSIGN_CONFIGS}, shapes


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ C ABI
def test_abi_has_the_target_and_loss_kernels():
    from dafne_amd import _lib, build
    so = build.build()
    L = _lib.load()
    assert L.dafne_abi_version() >= 149
    header = open(os.path.join(ROOT, "include", "dafne_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    for sym in ("dafne_assign_targets_hip", "dafne_losses_hip"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES and hasattr(L, sym)
        assert re.search(r"\b%s\b" % sym, exported), sym
    # the kernels are compiled inside decode.hip: no contraction, no SLP vectoriser (fp32 in the reference's operation order)
    assert {"-ffp-contract=off", "-fno-slp-vectorize"} <= set(build.PER_FILE["decode.hip"])
    assert '#include "targets_kernels.h"' in open(os.path.join(build.CSRC, "decode.hip")).read()


def test_losses_has_no_cpu_path():
    """DAFNeOutputs.losses no longer refuses (NotImplementedError); on CPU tensors it fails as every entry point does."""
    from dafne_amd import _lib
    from dafne_amd.config import get_cfg
    from dafne_amd.data.targets import make_gt_instances
    from dafne_amd.modeling.dafne.dafne_outputs import DAFNeOutputs
    outs = DAFNeOutputs(get_cfg())
    shapes = tn.level_shapes(64, 64)
    z = lambda c: [torch.zeros(1, c, h, w) for h, w in shapes]  # noqa: E731
    gt = [make_gt_instances(np.array([[8, 8, 40, 8, 40, 30, 8, 30]], np.float32), [2], (64, 64))]
    with pytest.raises(_lib.DafneHipError):
        outs.losses(z(15), z(8), z(2), [], z(1), None, gt, top_feats=[])
    with pytest.raises(_lib.DafneHipError):
        outs._get_ground_truth([torch.zeros(h * w, 2) for h, w in shapes], gt)


def test_lambdas_as_the_reference():
    from dafne_amd.config import get_cfg
    from dafne_amd.modeling.dafne.dafne_outputs import DAFNeOutputs
    cfg = get_cfg()
    lam = cfg.MODEL.DAFNE.LOSS_LAMBDA
    lam.CLS, lam.CORNERS, lam.CENTER, lam.CTR = 10.0, 1.0, 1.0, 1.0
    cfg.MODEL.DAFNE.LOSS_LAMBDA_NORM = True
    outs = DAFNeOutputs(cfg)
    assert (outs.lambda_cls, outs.lambda_corners, outs.lambda_center, outs.lambda_ctr) == (10.0 / 13, 1.0 / 13, 1.0 / 13, 1.0 / 13)
    outs.update_lambdas(lambda_cls=2.0)
    assert (outs.lambda_cls, outs.lambda_corners, outs.lambda_center, outs.lambda_ctr) == (2.0, 1.0, 1.0, 1.0)
    outs.update_lambdas(lambda_cls=2.0, lambda_ctr=3.0, normalize=True)
    assert (outs.lambda_cls, outs.lambda_ctr, outs.lambda_corners) == (2.0 / 7, 3.0 / 7, 1.0 / 7)
    cfg.MODEL.DAFNE.CENTERNESS = "none"
    cfg.MODEL.DAFNE.CORNER_PREDICTION = "direct"
    outs = DAFNeOutputs(cfg)
    assert (outs.lambda_cls, outs.lambda_corners) == (10.0 / 11, 1.0 / 11)
    assert outs.sizes_of_interest == [[-1, 64], [64, 128], [128, 256], [256, 512], [512, 100000000]]


# ------------------------------------------------------------------------------------------------ ground truth
def test_make_gt_instances_by_hand():
    from dafne_amd.data.targets import make_gt_instances
    # a 4 x 3 rectangle given from its lower right corner, and a triangle-like quadrilateral
    c = np.array([[4, 3, 0, 3, 0, 0, 4, 0], [1, 1, 5, 1, 5, 4, 3, 6]], np.float32)
    inst = make_gt_instances(c, [7, 2], (32, 48))
    assert inst.image_size == (32, 48) and len(inst) == 2
    assert inst.gt_corners[0].tolist() == [0, 3, 4, 3, 4, 0, 0, 0]           # leftmost first, then the sense the reference walks
    assert inst.gt_boxes.tensor.tolist() == [[0, 0, 4, 3], [1, 1, 5, 6]]
    # shoelace: 12; (1,1),(5,1),(5,4),(3,6): 0.5 |(1 - 5) + (20 - 5) + (30 - 12) + (3 - 6)| = 13
    assert inst.gt_corners_area.tolist() == [12.0, 13.0] and inst.gt_corners_area.dtype == torch.float32
    assert inst.gt_classes.tolist() == [7, 2] and inst.gt_classes.dtype == torch.int64
    raw = make_gt_instances(c, [7, 2], (32, 48), sort=False)
    assert raw.gt_corners.tolist() == c.tolist()
    empty = make_gt_instances(np.zeros((0, 8)), [], (32, 48))
    assert len(empty.gt_classes) == 0 and empty.gt_boxes.tensor.shape == (0, 4) and empty.gt_corners.shape == (0, 8)


def test_gt_instances_from_label_objects():
    from dafne_amd.data.targets import gt_instances_from_objects
    objs = [{"name": "ship", "difficult": 0, "bbox": [0, 0, 8, 0, 8, 6, 0, 6]},
            {"name": "unknown-class", "difficult": 0, "bbox": [0, 0, 1, 0, 1, 1, 0, 1]},
            {"name": "plane", "difficult": 1, "bbox": [10, 10, 20, 10, 20, 30, 10, 30]}]
    inst = gt_instances_from_objects(objs, ["plane", "ship"], (100, 100), ratio=0.5)
    assert inst.gt_classes.tolist() == [1, 0]
    assert inst.gt_boxes.tensor.tolist() == [[0, 0, 4, 3], [5, 5, 10, 15]]
    assert inst.gt_corners_area.tolist() == [12.0, 50.0]


def test_host_corner_sort_vs_the_reference(golden):
    from dafne_amd.data.targets import sort_quadrilateral_np
    g = np.load(os.path.join(ROOT, "tests", "golden", "sort_corners.npz"))
    assert np.array_equal(bits(sort_quadrilateral_np(g["boxes"])), bits(g["sorted"]))


# ------------------------------------------------------------------------------------------------ assignment
def test_fixture_covers_what_it_should(golden):
    st = golden["a_stats"]
    assert (st[:5] > 0).sum() >= 4 and st[5] >= 20 and st[6] >= 1 and st[7] >= 1
    gts, shapes = tn.case_a()
    assert [g["cls"].shape[0] for g in gts] == [70, 0, 5] and sum(h * w for h, w in shapes) == 1706


@pytest.mark.parametrize("name", list(tn.ASSIGN_CONFIGS))
def test_assignment_vs_reference(golden, assigned, name):
    """Integers equal, and the targets that involve no square root (corners, ltrb) equal bit for bit."""
    t = assigned[0][name]
    assert np.array_equal(t["labels"], golden["a_%s_labels" % name])
    assert np.array_equal(t["target_inds"], golden["a_%s_target_inds" % name])
    for k in ("corners", "ltrb"):
        assert np.array_equal(bits(t[k]), bits(golden["a_%s_%s" % (name, k)])), k


@pytest.mark.parametrize("name", list(tn.ASSIGN_CONFIGS))
def test_assignment_abcd_vs_reference(golden, assigned, name):
    """The point-to-edge distances, bit for bit.  They go through a square root and a division: the fixture is made where both
    are verified correctly rounded (tests/golden/make_golden_targets.py stops otherwise -- torch's CPU sqrt is MKL's, and MKL's
    AVX512 path is one ulp off in about 0.6 % of values, among them sqrt(388.43658447265625f) of this very case), so these are
    the bits of the arithmetic the assignment is defined in on any machine."""
    t = assigned[0][name]
    got, want = bits(t["abcd"]), bits(golden["a_%s_abcd" % name])
    bad = np.argwhere(got != want)
    ulps = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(name, "abcd values that differ:", len(bad), "largest difference in ulp:", int(ulps.max()), "at", bad[:4].tolist())
    assert len(bad) == 0, (name, bad[:4].tolist(), int(ulps.max()))


@pytest.mark.parametrize("mode,key", [("oriented", "abcd"), ("plain", "ltrb")])
def test_centerness_targets_within_2_ulp(golden, mode, key):
    """torch's fp32 pow is within 1 ulp of the true power and the engine's (fp64 power of the same fp32 ratio, rounded once)
    within 1/2: at most 2 ulp apart.  The inputs are the fixture's own targets, so that this compares the power alone."""
    pos = golden["a_released_labels"] != 15
    mine = tn.ctrness_targets(golden["a_released_" + key][pos], 3.0).astype(np.float32)
    ref = golden["a_ctr_" + mode]
    d = np.abs(mine.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    print(mode, "largest difference in ulp:", int(d.max()))
    assert d.max() <= 2


# ------------------------------------------------------------------------------------------------ losses
# Relative deviation of the fp64 restatement from the reference's fp32 value, measured on the CPU over every case of the
# fixture (48 configurations, the batch without positives, the four hand-made sets), largest per term:
#     loss/cls 1.646e-07   loss/corners 1.497e-07   loss/center 2.814e-07   loss/ctr 1.247e-07   loss_denorm 7.894e-08
# This is the reference's own fp32 rounding (sums of thousands of fp32 terms), not the engine's.  Asserted: twice that.
MEASURED = {"cls": 1.646e-07, "corners": 1.497e-07, "center": 2.814e-07, "ctr": 1.247e-07, "loss_denorm": 7.894e-08}


def _loss_cases(assigned):
    tg, shapes = assigned[0]["released"], assigned[1]
    preds = tn.case_b_predictions(tg, seed=21)
    for name, Lc in tn.loss_configs():
        yield "b_" + name, tg, preds, Lc
    empty = [tn.gt_of(np.zeros((0, 8), np.float32), np.zeros(0, np.int64))] * 3
    tg0 = tn.assign(empty, shapes, tn.assign_config("released"))
    yield "b_nopos", tg0, tn.case_b_predictions(tg0, seed=22), tn.LOSS_RELEASED
    for kind in ("zero_ctr", "nan_ctr"):
        th = tn.handmade_targets(kind)
        for mode in ("oriented", "plain"):
            yield "b_%s_%s" % (kind, mode), th, tn.case_b_predictions(th, seed=23), dict(tn.LOSS_RELEASED, ctr_mode=mode)


def test_losses_restatement_vs_reference(golden, assigned):
    worst = dict.fromkeys(MEASURED, 0.0)
    n = 0
    for key, tg, preds, Lc in _loss_cases(assigned):
        o = tn.losses(preds[0], preds[1], preds[2], preds[3], tg, Lc)
        ref = golden[key]
        assert o["num_pos"] == ref[4], key
        for i, term in enumerate(("cls", "corners", "center", "ctr", None, "loss_denorm")):
            if term is None:
                continue
            if ref[i] == 0:
                assert o[term] == 0, (key, term, o[term])
                continue
            dev = abs(o[term] - ref[i]) / abs(ref[i])
            worst[term] = max(worst[term], dev)
            assert dev <= 2 * MEASURED[term], (key, term, o[term], ref[i], dev)
        n += 1
    print("cases", n, "largest relative deviation per term", worst)
    assert n == 48 + 1 + 4
    assert golden["b_nopos"][1:4].tolist() == [0, 0, 0] and golden["b_zero_ctr_oriented"][5] == 1e-6
