"""GPU: OneStageDetector.backward_head_tail / tail_parameters (modeling/dafne/tail_backward.py) on a small seeded model: the
released head (R50 from configs/dota-1.0_r50.yaml, random weights, 2 images of 64 x 96 with a few made-up boxes) and the ablation
heads.  The tower gradients are held against the fp64 restatement of tests/_tail_backward_np.py under the bound derived in
tests/test_gpu_pred_dgrad.py, on maps, statistics, weights and gradients read back from the plan.
"""
import os

import numpy as np
import pytest
import torch

import _tail_backward_np as R
import _targets_np as tn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOWERS = (("cls_tower", "cls_logits"), ("corners_tower", "corners_ctrness"))
LOOP_K, LOOP_LR = 3, 0.01
_M = {}


def dev():
    return torch.device("cuda", 0)


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
    return [{"image": ims[i], "height": 64, "width": 96, "instances": make_gt_instances(quads[i], classes[i], (64, 96))}
            for i in range(2)]


def unpacked(w, cout):
    """engine.pack_conv's bf16 [Cout_pad, 256/64, 3, 3, 64] -> OIHW fp64 [cout, 256, 3, 3]."""
    return w.float().cpu().reshape(-1, 4, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(-1, 256, 3, 3)[:cout].numpy().astype(np.float64)


def restatement_of(hp, key, gouts):
    """The restatement on what the plan's prediction call `key` read: raw tower maps, their statistics, the GroupNorm affine, the
    packed weight; the mask is where the bf16 number the forward multiplied (gn_apply_kernel's expression) is > 0."""
    ins, gn_in = hp.pred_inputs[key]
    call = hp.pred_calls[key]
    cout = int(call.prm.Cout)
    gamma, beta = gn_in[1].cpu(), gn_in[2].cpu()
    xs, stats, masks = [], [], []
    for l, a in enumerate(ins):
        x = a.t[:, 1:-1, 1:-1].float().cpu()
        st = gn_in[0][l].cpu()                                              # [N, 32, 2]
        mean = st[:, :, 0].repeat_interleave(8, 1)[:, None, None, :]
        rstd = st[:, :, 1].repeat_interleave(8, 1)[:, None, None, :]
        y = (((x - mean) * rstd).double() * gamma.double() + beta.double()).float()      # one rounding: the kernel's fma
        masks.append((y.to(torch.bfloat16).float() > 0).numpy())
        xs.append(x.numpy())
        stats.append(st.numpy())
    return R.tail_backward(xs, stats, gamma.numpy(), beta.numpy(), unpacked(call.keep[0], cout),
                           [g[..., :cout].cpu().numpy() for g in gouts], masks)


def n_tiles(hp, n):
    return sum(n * ((t.shape[1] + 3) // 4) * ((t.shape[2] + 31) // 32) for t in hp.logits)


def test_backward_head_tail_end_to_end():
    cfg, m = released_model()
    inputs = labelled_batch()
    head = m.proposal_generator.dafne_head
    want_losses = {k: v.clone() for k, v in m.validation_losses(inputs).items()}
    m.backward_prediction_layers(inputs)
    torch.cuda.synchronize()
    pred = m.prediction_parameters()
    pred_grads = [p.grad.clone() for p in pred]
    m.zero_grad(set_to_none=True)
    got = m.backward_head_tail(inputs)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want_losses)
    for k in got:
        assert torch.equal(got[k], want_losses[k]), k
    params = m.tail_parameters()
    assert len(params) == 8 + 5 + 6 and [id(p) for p in params[:13]] == [id(p) for p in pred]
    for p, g in zip(pred, pred_grads):
        assert torch.equal(p.grad, g), "a prediction-layer gradient differs from backward_prediction_layers"
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    ids = set(id(p) for p in params)
    names = {id(p): k for k, p in m.named_parameters()}
    with_grad = [names[id(p)] for p in m.parameters() if p.grad is not None and id(p) not in ids]
    assert not with_grad, "frozen parameters received a gradient: %s" % with_grad[:4]
    assert all(p.grad is None for k, p in m.named_parameters() if "center_tower" in k or k.startswith("backbone."))
    # ---- the tower gradients against the restatement, on what the plan's calls read
    last = m._last_head_tail
    assert last["plan"] is m._last_validation["plan"] and sorted(last["gx"]) == ["cls_tower", "corners_tower"]
    hp = last["plan"].head
    tiles = n_tiles(hp, 2)
    worst = 0.0

    def check(name, got_t, ref, bound):
        nonlocal worst
        err = np.abs(got_t.detach().cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert (err <= bound).all(), (name, float(np.max(err - bound)))
    for tower, key in TOWERS:
        ref = restatement_of(hp, key, last["g"][tower])
        assert any(float(np.abs(g).max()) > 0 for g in ref["gx"]), "%s: the gradient is all zero, the batch is useless" % tower
        for l, t in enumerate(last["gx"][tower]):
            assert tuple(t.shape) == tuple(hp.logits[l].shape[:3]) + (256,)
            check("%s gx[%d]" % (tower, l), t, ref["gx"][l], R.bound_gx(ref["gx_abs"][l]))
        mods = getattr(head, tower)
        check(tower + ".10.weight", mods[10].weight.grad, ref["dgamma"], R.bound_sum(ref["dgamma_abs"], tiles))
        check(tower + ".10.bias", mods[10].bias.grad, ref["dbeta"], R.bound_sum(ref["dbeta_abs"], tiles))
        check(tower + ".9.bias", mods[9].bias.grad, ref["dbias"], R.bound_sum(ref["dbias_abs"], tiles))
    print("backward_head_tail: largest err / bound %.4f" % worst)
    # ---- accumulation: a second call doubles .grad exactly; zero_grad() and one call reproduce the first bits
    first = [p.grad.clone() for p in params]
    m.backward_head_tail(inputs)
    torch.cuda.synchronize()
    for p, f in zip(params, first):
        assert torch.equal(p.grad, f + f)
    m.zero_grad(set_to_none=True)
    m.backward_head_tail(inputs)
    torch.cuda.synchronize()
    for p, f in zip(params, first):
        assert torch.equal(p.grad, f)
    m.zero_grad(set_to_none=True)
    m.invalidate()
    assert m._last_head_tail is None


def test_sgd_loop_over_tail_parameters_lowers_the_loss():
    cfg, m = released_model()
    inputs = labelled_batch()
    opt = torch.optim.SGD(m.tail_parameters(), lr=LOOP_LR)
    tail = m.tail_parameters()[13:]
    start = [p.detach().clone() for p in tail]
    totals = []
    for _ in range(LOOP_K):
        opt.zero_grad(set_to_none=True)
        totals.append(m.backward_head_tail(inputs)["loss/total"])
        opt.step()
        m.invalidate()
    totals.append(m.validation_losses(inputs)["loss/total"])
    torch.cuda.synchronize()
    totals = [float(t) for t in totals]
    print("sgd loop over tail_parameters K=%d lr=%g: %s" % (LOOP_K, LOOP_LR, ["%.6f" % v for v in totals]))
    assert totals[-1] < totals[0], totals
    assert all(not torch.equal(p.detach(), s) for p, s in zip(tail, start)), "a tower parameter did not move"
    m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("strategy,centerness", [("direct", "none"), ("offset", "plain")])
def test_ablation_heads_get_tower_gradients(strategy, centerness):
    from test_gpu_ablation_head import ablation_model
    _, m = ablation_model(strategy, centerness)
    inputs = labelled_batch()
    m.zero_grad(set_to_none=True)
    want = {k: v.clone() for k, v in m.validation_losses(inputs).items()}
    got = m.backward_head_tail(inputs)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k])
    params = m.tail_parameters()
    assert len(params) == (4 if centerness == "none" else 6) + 5 + 6
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert all(float(p.grad.abs().sum()) > 0 for p in params[-6:])
    ids = set(id(p) for p in params)
    assert all(p.grad is None for p in m.parameters() if id(p) not in ids)
    m.zero_grad(set_to_none=True)


def test_refusals(monkeypatch):
    import torch.distributed as dist
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    from test_gpu_ablation_head import ablation_model
    inputs = labelled_batch()
    _, it = ablation_model("iterative", "plain")
    with pytest.raises(NotImplementedError):
        it.backward_head_tail(inputs)
    with pytest.raises(NotImplementedError):
        it.tail_parameters()
    cfg8 = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), ["ENGINE.WEIGHT_DTYPE", "fp8_e4m3"])
    with pytest.raises(NotImplementedError):
        build_model(cfg8).backward_head_tail(inputs)
    # the engine switch that keeps the raw map: off -> the prediction calls read an already normalised map
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
    monkeypatch.setenv("DAFNE_FUSE_GN_PRED", "0")
    plain = build_model(cfg)
    plain.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=5))
    plain.to(dev())
    plain.invalidate()
    with pytest.raises(NotImplementedError, match="fuse_gn_pred"):
        plain.backward_head_tail(inputs)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in plain.parameters())
    monkeypatch.delenv("DAFNE_FUSE_GN_PRED")
    _, m = released_model()
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError):
        m.backward_head_tail(inputs)
    assert all(p.grad is None for p in m.parameters())


def test_finetune_tool_with_tail_runs_on_a_scene_directory(tmp_path, capsys):
    """tools/finetune_pred.py --tail on two small synthetic scenes with labelTxt: two steps, one JSON line of finite losses per
    step, and a checkpoint that checkpoint.load_weights loads completely, in which the prediction layers AND the last GroupNorm /
    bias of cls_tower and corners_tower moved and nothing else did."""
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
                             "--overlap", "32", "--lr", "0.01", "--seed", "1", "--tail", "--out", str(out),
                             "INPUT.MIN_SIZE_TRAIN", "[96, 128, 160]", "INPUT.MAX_SIZE_TRAIN", "192"])
    torch.cuda.synchronize()
    assert rc == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [0, 1]
    for l in lines:
        assert all(np.isfinite(l[k]) for k in l if k.startswith("loss/")) and l["loss/total"] > 0
    fresh = build_model(load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")))
    missing, unexpected = load_weights(fresh, str(out))
    assert missing == [] and unexpected == []
    tuned = fresh.state_dict()
    allowed = ["cls_logits.", "corners_pred.", "ctrness.", "center_pred.", "scales."] + \
              ["%s.%s" % (t, k) for t in ("cls_tower", "corners_tower") for k in ("9.bias", "10.weight", "10.bias")]
    moved = [k for k in tuned if not torch.equal(tuned[k].cpu(), start[k])]
    assert moved and all(any(("dafne_head." + p) in k for p in allowed) for k in moved), moved[:5]
    for t in ("cls_tower", "corners_tower"):
        for k in ("9.bias", "10.weight", "10.bias"):
            assert any(k2.endswith("dafne_head.%s.%s" % (t, k)) for k2 in moved), (t, k)
