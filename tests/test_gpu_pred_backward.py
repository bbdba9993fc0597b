"""GPU: dafne_head_uncook_backward_hip and OneStageDetector.backward_prediction_layers against the fp64 restatement of
tests/_pred_backward_np.py (which builds on tests/_targets_np.py and tests/_targets_grad_np.py).

Setup of the model tests: R50 from configs/dota-1.0_r50.yaml with random weights, 2 images of 64 x 96 with a few made-up boxes.
Loop test: K = 3 plain SGD steps (no momentum) at learning rate 0.01 on the one batch; the restatement's drop of the total loss for the
same initial weights, batch and tower maps is printed by the test and the GPU loop must reach at least half of it.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _pred_backward_np as R
import _targets_grad_np as tg_np
import _targets_np as tn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_K, LOOP_LR = 3, 0.01


def dev():
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ uncook kernel
@pytest.mark.parametrize("c2c,has_ctr", [(True, True), (True, False), (False, True), (False, False)],
                         ids=["c2c_ctr", "c2c_noctr", "direct_ctr", "direct_noctr"])
def test_uncook_kernel(c2c, has_ctr):
    from dafne_amd.modeling.dafne.pred_backward import uncook_backward
    rng = np.random.default_rng(3 + 2 * c2c + has_ctr)
    n, shapes = 2, [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1), (17, 31)]      # the last level: more than one workgroup
    pred_c = 9 if has_ctr else 8
    scales = [0.7, 1.0, 1.3, 2.1, 0.9, 1.1]

    def arr(h, w, c, s=1.0):
        return (rng.normal(0, s, (n, h, w, c)) * np.exp(rng.uniform(-6, 2, (n, h, w, c)))).astype(np.float32)
    g_reg = [arr(h, w, 8) for h, w in shapes]
    g_creg = [arr(h, w, 2) for h, w in shapes] if c2c else None
    g_ctr = [arr(h, w, 1)[..., 0] for h, w in shapes] if has_ctr else None
    dc = [arr(h, w, pred_c, 3.0) for h, w in shapes]
    center = [arr(h, w, 2, 3.0) for h, w in shapes] if c2c else None

    def up(ts):
        return None if ts is None else [torch.from_numpy(np.ascontiguousarray(t)).to(dev()) for t in ts]
    runs = []
    for _ in range(2):
        gd, gc, gs = uncook_backward(up(g_reg), up(g_creg), up(g_ctr), up(dc), pred_c, up(center), scales, pred_c)
        torch.cuda.synchronize()
        runs.append(([t.cpu() for t in gd], [t.cpu() for t in gc] if gc is not None else None, gs.cpu()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert torch.equal(runs[0][2], runs[1][2]), "g_scale differs from run to run"
    gd, gc, gs = runs[0]

    def within_one_ulp(got, want):
        got = got.numpy().astype(np.float64)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got - want) <= ulp).all(), float(np.max(np.abs(got - want) / ulp))
    for l, (h, w) in enumerate(shapes):
        s = float(np.float32(scales[l]))
        wd, wc, ws = R.uncook(g_reg[l], g_creg[l] if c2c else None, dc[l][..., :8], center[l] if c2c else None, s)
        within_one_ulp(gd[l][..., :8], wd)
        if has_ctr:
            assert np.array_equal(gd[l][..., 8].numpy(), g_ctr[l])
        if c2c:
            within_one_ulp(gc[l], wc)
        terms = R.uncook_abs_terms(g_reg[l], g_creg[l] if c2c else None, dc[l][..., :8], center[l] if c2c else None)
        npx = n * h * w
        assert abs(float(gs[l]) - ws) <= npx * 2.0 ** -53 * terms + 1e-300, (l, float(gs[l]), ws)


# ------------------------------------------------------------------------------------------------ whole model
_M = {}


def released_model():
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    if "m" not in _M:
        cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
        m = build_model(cfg)
        m.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=5))
        m.to(dev())
        m.invalidate()
        _M["m"] = (cfg, m, {k: v.detach().clone() for k, v in m.state_dict().items()})
    cfg, m, sd = _M["m"]
    m.load_state_dict(sd)            # (a test may have stepped the parameters)
    m.zero_grad(set_to_none=True)
    return cfg, m


def labelled_batch():
    from dafne_amd.data.targets import make_gt_instances
    rng = np.random.default_rng(9)
    g = torch.Generator().manual_seed(2)
    ims = [torch.randint(0, 256, (3, 64, 96), generator=g, dtype=torch.uint8) for _ in range(2)]
    quads = [tn.random_quads(4, rng, 64, 96, lo=10.0, hi=50.0), tn.random_quads(2, rng, 64, 96, lo=30.0, hi=90.0)]
    classes = [rng.integers(0, 15, 4), rng.integers(0, 15, 2)]
    inputs = [{"image": ims[i], "height": 64, "width": 96, "instances": make_gt_instances(quads[i], classes[i], (64, 96))}
              for i in range(2)]
    return inputs, quads, classes


def configs_of(cfg):
    d = cfg.MODEL.DAFNE
    T = tn.assign_config("released", num_classes=d.NUM_CLASSES, center_sample=d.CENTER_SAMPLE, center_sample_only=d.CENTER_SAMPLE_ONLY,
                         combine=d.COMBINE_CENTER_SAMPLE, radius=d.POS_RADIUS, in_box_check=d.ENABLE_IN_BOX_CHECK,
                         size_filter=d.ENABLE_LEVEL_SIZE_FILTERING, stride_norm=d.ENABLE_FPN_STRIDE_NORM)
    Lc = dict(tn.LOSS_RELEASED, alpha=d.LOSS_ALPHA, gamma=d.LOSS_GAMMA, beta=d.LOSS_SMOOTH_L1_BETA, logspace=d.ENABLE_LOSS_LOG,
              modulation=d.ENABLE_LOSS_MODULATION, ctr_mode=d.CENTERNESS, ctr_alpha=float(d.CENTERNESS_ALPHA),
              sort_corners=d.SORT_CORNERS, has_center_reg=True, lambda_norm=d.LOSS_LAMBDA_NORM,
              lambdas=dict(cls=d.LOSS_LAMBDA.CLS, corners=d.LOSS_LAMBDA.CORNERS, center=d.LOSS_LAMBDA.CENTER, ctr=d.LOSS_LAMBDA.CTR))
    return T, Lc


def tower_maps(hp):
    """The bf16 numbers the three prediction convolutions multiplied, per level [N,H,W,256] fp64: the plan's own tower outputs,
    with GroupNorm + ReLU in gn_apply_kernel's expression where the convolution normalises on load."""
    out = {}
    for key, name in (("cls_logits", "cls"), ("corners_ctrness", "corners"), ("center_pred", "center")):
        if key not in hp.pred_inputs:
            continue
        ins, gn_in = hp.pred_inputs[key]
        maps = []
        for l, a in enumerate(ins):
            x = a.t[:, 1:-1, 1:-1].float().cpu()
            if gn_in is not None:
                st = gn_in[0][l].cpu()                                              # [N, 32, 2]
                mean = st[:, :, 0].repeat_interleave(8, 1)[:, None, None, :]
                rstd = st[:, :, 1].repeat_interleave(8, 1)[:, None, None, :]
                t = (x - mean) * rstd
                y = (t.double() * gn_in[1].cpu().double() + gn_in[2].cpu().double()).float()      # one rounding: the kernel's fma
                x = torch.relu(y.to(torch.bfloat16).float())
            maps.append(x.numpy().astype(np.float64))
        out[name] = maps
    return out


def head_params(m):
    head = m.proposal_generator.dafne_head
    p = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in head.state_dict().items()
         if k.split(".")[0] in ("cls_logits", "corners_pred", "ctrness", "center_pred")}
    p["scales"] = [float(s.scale.detach().cpu()[0]) for s in head.scales]
    return p


def test_backward_prediction_layers_end_to_end():
    cfg, m = released_model()
    inputs, quads, classes = labelled_batch()
    head = m.proposal_generator.dafne_head

    def detections():
        out = m(inputs)
        torch.cuda.synchronize()
        return [(o["instances"].pred_corners.clone(), o["instances"].scores.clone(), o["instances"].pred_classes.clone()) for o in out]
    before = detections()
    want_losses = {k: v.clone() for k, v in m.validation_losses(inputs).items()}
    got = m.backward_prediction_layers(inputs)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want_losses)
    for k in got:
        assert torch.equal(got[k], want_losses[k]), k
    params = m.prediction_parameters()
    assert len(params) == 8 + 5 and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    ids = set(id(p) for p in params)
    assert all(p.grad is None for p in m.parameters() if id(p) not in ids), "a frozen parameter received a gradient"
    first = [p.grad.clone() for p in params]
    last = m._last_pred_backward
    assert float(last["plan"].head.logits[0].abs().sum()) > 0
    # the gradients come from the COOKED loss forward, the returned dict from the raw form: the same fp64 row, bit for bit
    raw_row = m._last_validation["extras"]["values_f64"]
    assert last["plan"] is m._last_validation["plan"]
    assert torch.equal(last["cooked_values_f64"], raw_row), (last["cooked_values_f64"], raw_row)
    assert torch.equal(raw_row.to(torch.float32)[0], got["loss/cls"])
    # ---- the restatement, fed with the plan's own tower maps and the head outputs the plan computed from them
    hp = last["plan"].head
    towers = tower_maps(hp)
    T, Lc = configs_of(cfg)
    shapes = [tuple(t.shape[1:3]) for t in hp.logits]
    tg = tn.assign([tn.gt_of(quads[i], classes[i]) for i in range(2)], shapes, T)
    assert (tg["labels"] != 15).sum() > 0, "no positive location: the made-up boxes are useless"
    f32 = np.float32
    logits = [t.cpu().numpy() for t in hp.logits]
    dc = [t.cpu().numpy() for t in hp.delta_ctr]
    ce = [t.cpu().numpy() for t in hp.center]
    regs, cregs = [], []
    for l in range(5):
        s = f32(hp.scales[l])
        regs.append(((np.tile(ce[l], 4) + dc[l][..., :8]).astype(f32) * s).astype(f32))
        cregs.append((ce[l] * s).astype(f32))

    def flat(ts, c):
        return np.concatenate([t.reshape(-1, c) for t in ts], 0)
    g = tg_np.grads(flat(logits, 15), flat(regs, 8), flat(cregs, 2), flat([t[..., 8:9] for t in dc], 1)[:, 0], tg, Lc)
    off, g_logits, g_cc, g_ce, g_sc, g_sc_abs = 0, [], [], [], [], []
    for l, (h, w) in enumerate(shapes):
        npx = 2 * h * w
        sl = slice(off, off + npx)
        off += npx
        g_logits.append(g["logits"][sl].reshape(2, h, w, 15))
        g_reg, g_creg = g["corners"][sl].reshape(2, h, w, 8), g["center"][sl].reshape(2, h, w, 2)
        gd, gc, gs = R.uncook(g_reg, g_creg, dc[l][..., :8], ce[l], float(f32(hp.scales[l])))
        g_cc.append(np.concatenate([gd, g["ctr"][sl].reshape(2, h, w, 1)], -1))
        g_ce.append(gc)
        g_sc.append(gs)
        g_sc_abs.append(R.uncook_abs_terms(g_reg, g_creg, dc[l][..., :8], ce[l]))
    want = {}
    worst = 0.0

    def check(name, got_t, ref, absum, n):
        nonlocal worst
        err = np.abs(got_t.detach().cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
        bound = R.wgrad_bound(absum, n)
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert (err <= bound).all(), (name, float(np.max(err - bound)))
    dW, db, aW, ab, n = R.wgrad(towers["cls"], g_logits)
    check("cls_logits.weight", head.cls_logits.weight.grad, dW, aW, n)
    check("cls_logits.bias", head.cls_logits.bias.grad, db, ab, n)
    dW, db, aW, ab, n = R.wgrad(towers["corners"], g_cc)
    check("corners_pred.weight", head.corners_pred.weight.grad, dW[:8], aW[:8], n)
    check("corners_pred.bias", head.corners_pred.bias.grad, db[:8], ab[:8], n)
    check("ctrness.weight", head.ctrness.weight.grad, dW[8:9], aW[8:9], n)
    check("ctrness.bias", head.ctrness.bias.grad, db[8:9], ab[8:9], n)
    dW, db, aW, ab, n = R.wgrad(towers["center"], g_ce)
    check("center_pred.weight", head.center_pred.weight.grad, dW, aW, n)
    check("center_pred.bias", head.center_pred.bias.grad, db, ab, n)
    for l in range(5):
        check("scales.%d" % l, head.scales[l].scale.grad, np.array([g_sc[l]]), np.array([g_sc_abs[l]]), n)
    print("backward_prediction_layers: largest err / bound %.4f" % worst)
    # ---- accumulation: a second call doubles .grad exactly; zero_grad() and one call reproduce the first bits
    m.backward_prediction_layers(inputs)
    torch.cuda.synchronize()
    for p, f in zip(params, first):
        assert torch.equal(p.grad, f + f)
    m.zero_grad(set_to_none=True)
    m.backward_prediction_layers(inputs)
    torch.cuda.synchronize()
    for p, f in zip(params, first):
        assert torch.equal(p.grad, f)
    # ---- nothing else moved: THIS model's detections after three calls (no optimiser step) are the bits it gave before the
    # first one (a before / after comparison on one model, not against a second model that never called the method);
    # forward() still refuses train()
    for a, b in zip(before, detections()):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m(inputs)
        with pytest.raises(NotImplementedError):
            m.backward_prediction_layers(inputs)
    finally:
        m.eval()


def test_refusals(monkeypatch):
    import torch.distributed as dist
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from test_gpu_ablation_head import ablation_model
    inputs, _, _ = labelled_batch()
    _, it = ablation_model("iterative", "plain")
    with pytest.raises(NotImplementedError):
        it.backward_prediction_layers(inputs)
    with pytest.raises(NotImplementedError):
        it.prediction_parameters()
    cfg8 = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), ["ENGINE.WEIGHT_DTYPE", "fp8_e4m3"])
    with pytest.raises(NotImplementedError):
        build_model(cfg8).backward_prediction_layers(inputs)
    _, m = released_model()
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError):
        m.backward_prediction_layers(inputs)
    assert all(p.grad is None for p in m.parameters())


def test_finetune_tool_runs_on_a_scene_directory(tmp_path, capsys):
    """tools/finetune_pred.py on two small synthetic scenes with labelTxt: two steps on TrainBatches of changing slab size with
    invalidate() between them, one JSON line of finite losses per step, and a checkpoint that checkpoint.load_weights (what
    tools/eval_net.py --weights calls) loads completely, with moved prediction layers and an untouched trunk."""
    import json
    import sys
    from PIL import Image
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.checkpoint import load_weights, save_checkpoint
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    cfg, m = released_model()
    start = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    save_checkpoint(m, str(tmp_path / "start.pth"))
    rng = np.random.default_rng(4)
    sd, ld = tmp_path / "scenes", tmp_path / "labelTxt"
    sd.mkdir()
    ld.mkdir()
    classes = ["plane", "ship", "harbor"]
    for name, (h, w) in (("P0001", (200, 260)), ("P0002", (180, 150))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(sd / (name + ".png"))
        rows = ["imagesource:GoogleEarth", "gsd:0.146"]
        for q in tn.random_quads(10, rng, h, w, lo=16.0, hi=48.0):
            rows.append(" ".join("%.1f" % v for v in q) + " %s 0" % classes[int(rng.integers(0, 3))])
        (ld / (name + ".txt")).write_text("\n".join(rows) + "\n")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import finetune_pred
    finally:
        sys.path.pop(0)
    out = tmp_path / "tuned.pth"
    capsys.readouterr()
    rc = finetune_pred.main(["--config-file", os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), "--weights", str(tmp_path / "start.pth"),
                             "--scene-dir", str(sd), "--scene-labels", str(ld), "--steps", "2", "--batch", "2", "--patch-size", "128",
                             "--overlap", "32", "--lr", "0.01", "--seed", "1", "--out", str(out),
                             "INPUT.MIN_SIZE_TRAIN", "[96, 128, 160]", "INPUT.MAX_SIZE_TRAIN", "192"])
    torch.cuda.synchronize()
    assert rc == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [0, 1]
    for l in lines:
        assert sorted(k for k in l if k.startswith("loss/")) == ["loss/center", "loss/cls", "loss/corners", "loss/ctr", "loss/total"]
        assert all(np.isfinite(l[k]) for k in l if k.startswith("loss/")) and l["loss/total"] > 0
    fresh = build_model(load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")))
    missing, unexpected = load_weights(fresh, str(out))
    assert missing == [] and unexpected == []
    tuned = fresh.state_dict()
    pred = ("cls_logits.", "corners_pred.", "ctrness.", "center_pred.", "scales.")
    moved = [k for k in tuned if not torch.equal(tuned[k].cpu(), start[k])]
    assert moved and all(any(("dafne_head." + p) in k for p in pred) for k in moved), moved[:5]
    assert any("cls_logits.weight" in k for k in moved)


@pytest.mark.parametrize("strategy,centerness", [("direct", "none"), ("offset", "plain")])
def test_ablation_heads_get_gradients(strategy, centerness):
    """The direct / offset heads (no center_pred; without centerness an 8-channel prediction): finite gradients on exactly
    prediction_parameters(), the losses of validation_losses."""
    from test_gpu_ablation_head import ablation_model
    _, m = ablation_model(strategy, centerness)
    inputs, _, _ = labelled_batch()
    m.zero_grad(set_to_none=True)
    want = {k: v.clone() for k, v in m.validation_losses(inputs).items()}
    got = m.backward_prediction_layers(inputs)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k])
    params = m.prediction_parameters()
    assert len(params) == (4 if centerness == "none" else 6) + 5
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert any(float(p.grad.abs().sum()) > 0 for p in params)
    m.zero_grad(set_to_none=True)


def test_sgd_loop_lowers_the_loss():
    cfg, m = released_model()
    inputs, quads, classes = labelled_batch()
    p0 = head_params(m)
    opt = torch.optim.SGD(m.prediction_parameters(), lr=LOOP_LR)
    totals = []
    for _ in range(LOOP_K):
        opt.zero_grad(set_to_none=True)
        totals.append(m.backward_prediction_layers(inputs)["loss/total"])
        if "towers" not in _M:
            hp = m._last_pred_backward["plan"].head
            _M["towers"] = (tower_maps(hp), [tuple(t.shape[1:3]) for t in hp.logits])      # frozen: the same at every step
        opt.step()
        m.invalidate()
    totals.append(m.validation_losses(inputs)["loss/total"])
    torch.cuda.synchronize()
    totals = [float(t) for t in totals]
    towers, shapes = _M["towers"]
    T, Lc = configs_of(cfg)
    tg = tn.assign([tn.gt_of(quads[i], classes[i]) for i in range(2)], shapes, T)
    ref, _ = R.sgd_loop(p0, towers, tg, Lc, LOOP_LR, LOOP_K)
    print("sgd loop K=%d lr=%g: restatement %s, engine %s" % (LOOP_K, LOOP_LR, ["%.6f" % v for v in ref], ["%.6f" % v for v in totals]))
    ref_drop, drop = ref[0] - ref[-1], totals[0] - totals[-1]
    assert ref_drop > 0, "the restatement's own loop does not lower the loss: K / learning rate are badly chosen"
    assert drop >= 0.5 * ref_drop, (drop, ref_drop)
    m.zero_grad(set_to_none=True)
