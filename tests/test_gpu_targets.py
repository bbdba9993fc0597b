"""GPU: the target-assignment and loss kernels (csrc/targets_kernels.h) against the numpy restatement of the reference
(tests/_targets_np.py), and OneStageDetector.validation_losses end to end.

  * assignment: every output equal bit for bit -- the restatement is fp32 in the reference's operation order, as the kernel is
  * losses: relative difference <= 1e-9 per term against the fp64 restatement (all summands are non-negative: only the order
    of summation and a few fp64 ulp of exp / log / pow differ), num_pos exact
  * two runs give equal bits
"""
import numpy as np
import pytest
import torch

import _targets_np as tn

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def make_outputs(T=None, Lc=None):
    from dafne_amd.config import get_cfg
    from dafne_amd.modeling.dafne.dafne_outputs import DAFNeOutputs
    cfg = get_cfg()
    d = cfg.MODEL.DAFNE
    T = T or tn.assign_config("released")
    Lc = Lc or tn.LOSS_RELEASED
    d.NUM_CLASSES = T["num_classes"]
    d.CENTER_SAMPLE, d.CENTER_SAMPLE_ONLY, d.COMBINE_CENTER_SAMPLE = T["center_sample"], T["center_sample_only"], T["combine"]
    d.POS_RADIUS, d.ENABLE_IN_BOX_CHECK, d.ENABLE_LEVEL_SIZE_FILTERING = T["radius"], T["in_box_check"], T["size_filter"]
    d.ENABLE_FPN_STRIDE_NORM = T["stride_norm"]
    d.SIZES_OF_INTEREST = [hi for _, hi in T["soi"][:-1]]
    d.LOSS_ALPHA, d.LOSS_GAMMA, d.LOSS_SMOOTH_L1_BETA = Lc["alpha"], Lc["gamma"], Lc["beta"]
    d.ENABLE_LOSS_LOG, d.ENABLE_LOSS_MODULATION = Lc["logspace"], Lc["modulation"]
    d.CENTERNESS, d.CENTERNESS_ALPHA, d.SORT_CORNERS = Lc["ctr_mode"], Lc["ctr_alpha"], Lc["sort_corners"]
    d.CORNER_PREDICTION = "center-to-corner" if Lc["has_center_reg"] else "direct"
    d.LOSS_LAMBDA.CLS, d.LOSS_LAMBDA.CORNERS = Lc["lambdas"]["cls"], Lc["lambdas"]["corners"]
    d.LOSS_LAMBDA.CENTER, d.LOSS_LAMBDA.CTR = Lc["lambdas"]["center"], Lc["lambdas"]["ctr"]
    d.LOSS_LAMBDA_NORM = Lc.get("lambda_norm", True)
    return DAFNeOutputs(cfg)


def gt_instances(gts, hw, device="cpu"):
    from dafne_amd.structures import Boxes, Instances
    out = []
    for g in gts:
        inst = Instances(hw)
        inst.gt_corners = torch.from_numpy(g["corners"]).to(device)
        inst.gt_boxes = Boxes(torch.from_numpy(g["hbox"]).to(device))
        inst.gt_corners_area = torch.from_numpy(g["area"]).to(device)
        inst.gt_classes = torch.from_numpy(g["cls"]).to(device)
        out.append(inst)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_assignment(tg, exp, tag):
    torch.cuda.synchronize()
    assert np.array_equal(tg.labels.cpu().numpy(), exp["labels"]), (tag, "labels")
    assert np.array_equal(tg.target_inds.cpu().numpy(), exp["target_inds"]), (tag, "target_inds")
    for k, t in (("corners", tg.corners), ("ltrb", tg.ltrb), ("abcd", tg.abcd)):
        got = bits(t.cpu().numpy())
        bad = np.nonzero((got != bits(exp[k])).any(1))[0]
        assert bad.size == 0, (tag, k, bad[:5], t.cpu().numpy()[bad[:2]], exp[k][bad[:2]])


@pytest.mark.parametrize("name", list(tn.ASSIGN_CONFIGS))
def test_assignment_case_a(name):
    gts, shapes = tn.case_a()
    T = tn.assign_config(name)
    exp = tn.assign(gts, shapes, T)
    outs = make_outputs(T)
    tg = outs.assign_targets(shapes, gt_instances(gts, tn.CASE_A_HW), dev())
    check_assignment(tg, exp, name)
    if name == "released":       # boxes that already live on the device, and run to run
        tg2 = outs.assign_targets(shapes, gt_instances(gts, tn.CASE_A_HW, dev()), dev())
        torch.cuda.synchronize()
        for a, b in ((tg.labels, tg2.labels), (tg.target_inds, tg2.target_inds), (tg.corners, tg2.corners), (tg.ltrb, tg2.ltrb),
                     (tg.abcd, tg2.abcd)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("seed", range(20))
def test_assignment_small_cases(seed):
    gts, shapes, T = tn.small_case(seed)
    exp = tn.assign(gts, shapes, T)
    tg = make_outputs(T).assign_targets(shapes, gt_instances(gts, (0, 0)), dev())
    check_assignment(tg, exp, seed)


def test_get_ground_truth_dict():
    """_get_ground_truth: the reference's keys, level-first lists in (image, location) order, views into the kernel's buffers."""
    from dafne_amd.modeling.dafne.dafne import compute_locations
    gts, shapes = tn.case_a()
    T = tn.assign_config("released")
    exp = tn.assign(gts, shapes, T)
    outs = make_outputs(T)
    locs = [compute_locations(h, w, s, dev()) for (h, w), s in zip(shapes, tn.STRIDES)]
    tt = outs._get_ground_truth(locs, gt_instances(gts, tn.CASE_A_HW))
    assert sorted(tt) == sorted(["labels", "target_inds", "reg_targets_corners", "reg_targets_ltrb", "reg_targets_abcd", "locations",
                                 "im_inds", "fpn_levels"])
    off = 0
    xs, ys, _ = tn.compute_locations(shapes)
    koff = 0
    for l, (h, w) in enumerate(shapes):
        n = 3 * h * w
        assert np.array_equal(tt["labels"][l].cpu().numpy(), exp["labels"][off:off + n])
        assert np.array_equal(bits(tt["reg_targets_abcd"][l].cpu().numpy()), bits(exp["abcd"][off:off + n]))
        assert tt["reg_targets_corners"][l].shape == (n, 8)
        for k in ("labels", "reg_targets_corners"):                   # views into one buffer, not copies
            assert tt[k][l].untyped_storage().data_ptr() == tt[k][0].untyped_storage().data_ptr()
        assert np.array_equal(tt["im_inds"][l].cpu().numpy(), np.repeat(np.arange(3), h * w))
        assert np.array_equal(tt["fpn_levels"][l].cpu().numpy(), np.full(n, l))
        exp_loc = np.tile(np.stack([xs[koff:koff + h * w], ys[koff:koff + h * w]], 1), (3, 1))
        assert np.array_equal(tt["locations"][l].cpu().numpy(), exp_loc)
        off += n
        koff += h * w


# ------------------------------------------------------------------------------------------------------- losses
def upload_targets(tg_np, n, shapes):
    from dafne_amd.modeling.dafne.dafne_outputs import Targets
    tg = Targets(n, shapes, tn.STRIDES[:len(shapes)], dev())
    tg.labels.copy_(torch.from_numpy(tg_np["labels"].astype(np.int32)))
    tg.target_inds.copy_(torch.from_numpy(tg_np["target_inds"].astype(np.int32)))
    tg.corners.copy_(torch.from_numpy(tg_np["corners"]))
    tg.ltrb.copy_(torch.from_numpy(tg_np["ltrb"]))
    tg.abcd.copy_(torch.from_numpy(tg_np["abcd"]))
    return tg


def cooked_levels(preds, n, shapes, Lc):
    from dafne_amd import postprocess as pp
    logits, corners, center, ctr = preds
    lv = []
    parts = [tn.split_levels(a if a.ndim == 2 else a[:, None], n, shapes) for a in (logits, corners, center, ctr)]
    for l in range(len(shapes)):
        t = [torch.from_numpy(np.ascontiguousarray(p[l])).to(dev()) for p in parts]
        lv.append(pp.LevelInput(t[0], t[1], t[2] if Lc["has_center_reg"] else None, t[3] if Lc["ctr_mode"] != "none" else None,
                                tn.STRIDES[l], 1.0))
    return lv


def run_loss_case(tg_np, preds, n, shapes, Lc, tag, runs=1):
    outs = make_outputs(Lc=Lc)
    outs.strides = list(tn.STRIDES[:len(shapes)])
    tg = upload_targets(tg_np, n, shapes)
    levels = cooked_levels(preds, n, shapes, Lc)
    exp = tn.losses(preds[0], preds[1], preds[2], preds[3], tg_np, Lc)
    rows = []
    for _ in range(runs):
        extras, losses = outs.dafne_losses_packed(levels, tg, cooked=True, want_ctr_targets=True)
        rows.append((extras["values_f64"].clone(), extras["ctr_targets"].clone()))
    torch.cuda.synchronize()
    row = rows[0][0].cpu().numpy()
    want = np.array([exp["cls"], exp["corners"], exp["center"], exp["ctr"]])
    rel = np.abs(row[:4] - want) / np.maximum(np.abs(want), 1e-300)
    rel[want == 0] = np.abs(row[:4])[want == 0]
    print(tag, "kernel", row, "relative difference", rel)
    assert row[4] == exp["num_pos"], (tag, row[4], exp["num_pos"])
    assert np.all(rel <= 1e-9), (tag, row, want, rel)
    assert abs(row[5] - exp["loss_denorm"]) <= 1e-9 * exp["loss_denorm"], (tag, row[5], exp["loss_denorm"])
    # the loss dict: the reference's keys, fp32 roundings of the row
    assert sorted(losses) == sorted(["loss/cls", "loss/corners"] + (["loss/center"] if Lc["has_center_reg"] else [])
                                    + (["loss/ctr"] if Lc["ctr_mode"] != "none" else []))
    assert losses["loss/cls"].dtype == torch.float32 and losses["loss/cls"].dim() == 0 and losses["loss/cls"].is_cuda
    assert float(losses["loss/cls"]) == float(np.float32(row[0]))
    assert sorted(k for k in extras if k in ("loss_denorm", "num_pos")) == ["loss_denorm", "num_pos"]
    # centerness targets at the positives: the fp32 rounding of the restatement's
    pos = tg_np["labels"] != Lc["num_classes"]
    ct = rows[0][1].cpu().numpy()
    assert np.array_equal(bits(ct[pos]), bits(exp["ctr_targets"].astype(np.float32))) and not ct[~pos].any()
    for r, c in rows[1:]:
        assert torch.equal(r.view(torch.int64), rows[0][0].view(torch.int64)) and torch.equal(c.view(torch.int32), rows[0][1].view(torch.int32))


@pytest.fixture(scope="module")
def case_b():
    gts, shapes = tn.case_a()
    tg = tn.assign(gts, shapes, tn.assign_config("released"))
    return tg, tn.case_b_predictions(tg, seed=21), shapes


@pytest.mark.parametrize("name", [n for n, _ in tn.loss_configs()])
def test_losses_case_b(case_b, name):
    tg, preds, shapes = case_b
    run_loss_case(tg, preds, 3, shapes, dict(tn.loss_configs())[name], name)


def test_losses_no_positives():
    _, shapes = tn.case_a()
    empty = [tn.gt_of(np.zeros((0, 8), np.float32), np.zeros(0, np.int64))] * 3
    tg0 = tn.assign(empty, shapes, tn.assign_config("released"))
    run_loss_case(tg0, tn.case_b_predictions(tg0, seed=22), 3, shapes, tn.LOSS_RELEASED, "nopos")


@pytest.mark.parametrize("kind", ["zero_ctr", "nan_ctr"])
@pytest.mark.parametrize("mode", ["oriented", "plain"])
def test_losses_handmade_centerness(kind, mode):
    th = tn.handmade_targets(kind)
    run_loss_case(th, tn.case_b_predictions(th, seed=23), 1, [(8, 8)], dict(tn.LOSS_RELEASED, ctr_mode=mode), (kind, mode))


def test_losses_run_to_run(case_b):
    tg, preds, shapes = case_b
    run_loss_case(tg, preds, 3, shapes, tn.LOSS_RELEASED, "run-to-run", runs=3)


# ------------------------------------------------------------------------------------------------ whole model
def test_validation_losses_whole_model():
    """R50 with random weights at 2 x 3 x 256 x 320 and made-up boxes: validation_losses equals losses(*head.forward(...)) on
    the same features and the restatement on the head outputs read back; detections are the same bits before and after."""
    import os
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.data.targets import make_gt_instances
    from dafne_amd.registry import build_model
    from oracle import model as om
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_cfg(os.path.join(root, "configs", "dota-1.0_r50.yaml"))
    m = build_model(cfg)
    m.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=5))
    m.to(dev())
    m.invalidate()
    rng = np.random.default_rng(9)
    g = torch.Generator().manual_seed(2)
    ims = [torch.randint(0, 256, (3, 256, 320), generator=g, dtype=torch.uint8) for _ in range(2)]
    quads = [tn.random_quads(12, rng, 256, 320), tn.random_quads(3, rng, 256, 320, lo=60.0, hi=250.0)]
    classes = [rng.integers(0, 15, 12), rng.integers(0, 15, 3)]
    inputs = [{"image": ims[i], "height": 256, "width": 320, "instances": make_gt_instances(quads[i], classes[i], (256, 320))}
              for i in range(2)]

    def detections():
        out = m(inputs)
        torch.cuda.synchronize()
        return [(o["instances"].pred_corners.clone(), o["instances"].scores.clone(), o["instances"].pred_classes.clone()) for o in out]
    before = detections()
    vl = m.validation_losses(inputs)
    torch.cuda.synchronize()
    after = detections()
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert sorted(vl) == ["loss/center", "loss/cls", "loss/corners", "loss/ctr", "loss/total"]
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in vl.values())
    assert float(vl["loss/total"]) == float(vl["loss/cls"] + vl["loss/corners"] + vl["loss/center"] + vl["loss/ctr"])
    last = m._last_validation
    row = last["extras"]["values_f64"].cpu().numpy()
    assert row[4] > 0, "no positive location: the made-up boxes are useless"
    # (a) the reference-signature path on the same features
    pg = m.proposal_generator
    feats = [a.nchw_float() for a in last["plan"].features]
    logits, regs, centers, ltrb, ctrs, _, _ = pg.dafne_head(None, feats)
    extras, ls = pg.dafne_outputs.losses(logits, regs, centers, ltrb, ctrs, None, [x["instances"] for x in inputs])
    torch.cuda.synchronize()
    assert torch.equal(extras["values_f64"], last["extras"]["values_f64"]), (extras["values_f64"], row)
    for k in ls:
        assert torch.equal(ls[k], vl[k])
    # (b) the restatement on the head outputs read back
    d = cfg.MODEL.DAFNE
    gts = [tn.gt_of(quads[i], classes[i]) for i in range(2)]
    shapes = [tuple(t.shape[2:]) for t in logits]
    T = tn.assign_config("released", num_classes=d.NUM_CLASSES, center_sample=d.CENTER_SAMPLE, center_sample_only=d.CENTER_SAMPLE_ONLY,
                         combine=d.COMBINE_CENTER_SAMPLE, radius=d.POS_RADIUS, in_box_check=d.ENABLE_IN_BOX_CHECK,
                         size_filter=d.ENABLE_LEVEL_SIZE_FILTERING, stride_norm=d.ENABLE_FPN_STRIDE_NORM)
    tg = tn.assign(gts, shapes, T)
    check_assignment(last["targets"], tg, "model")
    Lc = dict(tn.LOSS_RELEASED, alpha=d.LOSS_ALPHA, gamma=d.LOSS_GAMMA, beta=d.LOSS_SMOOTH_L1_BETA, logspace=d.ENABLE_LOSS_LOG,
              modulation=d.ENABLE_LOSS_MODULATION, ctr_mode=d.CENTERNESS, ctr_alpha=float(d.CENTERNESS_ALPHA),
              sort_corners=d.SORT_CORNERS, has_center_reg=True, lambda_norm=d.LOSS_LAMBDA_NORM,
              lambdas=dict(cls=d.LOSS_LAMBDA.CLS, corners=d.LOSS_LAMBDA.CORNERS, center=d.LOSS_LAMBDA.CENTER, ctr=d.LOSS_LAMBDA.CTR))

    def flat(ts, ch):
        return np.concatenate([t.permute(0, 2, 3, 1).reshape(-1, ch).cpu().numpy() for t in ts])
    exp = tn.losses(flat(logits, d.NUM_CLASSES), flat(regs, 8), flat(centers, 2), flat(ctrs, 1)[:, 0], tg, Lc)
    want = np.array([exp["cls"], exp["corners"], exp["center"], exp["ctr"]])
    rel = np.abs(row[:4] - want) / np.abs(want)
    print("whole model: kernel", row, "restatement", want, "relative difference", rel)
    assert row[4] == exp["num_pos"] and np.all(rel <= 1e-9), (row, want, rel)
