"""GPU: OneStageDetector.backward_towers / tower_parameters (modeling/dafne/tower_backward.py) on the fixtures of
tests/test_gpu_tail_backward.py: the released head (R50, seed 5, 2 images of 64 x 96 with a few made-up boxes) and the ablation
heads.  Per tower and layer the gradients are held against the fp64 restatement of tests/_tower_backward_np.py under its derived
bounds, evaluated on the maps, statistics, weights and incoming gradient read back from the plan and from _last_towers: each layer
is judged on what it actually read, so errors do not chain.
"""
import os

import numpy as np
import pytest
import torch

import _targets_np as tn
import _tower_backward_np as R
from test_gpu_tail_backward import ROOT, dev, labelled_batch, released_model, unpacked

pytestmark = pytest.mark.gpu
TOWERS = ("cls_tower", "corners_tower")
LOOP_K, LOOP_LR = 3, 0.003


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def layer_inputs(hp, name, i):
    """What tower layer i read -> (raw maps per level [N,H,W,256] fp32 numpy, stats per level or None, gamma, beta)."""
    ins, gn_in = hp.tower_inputs[(name, i)]
    xs = [a.t[:, 1:-1, 1:-1].float().cpu().numpy() for a in ins]
    if gn_in is None:
        return xs, None, None, None
    return xs, [gn_in[0][l].cpu().numpy() for l in range(len(ins))], gn_in[1].cpu().numpy(), gn_in[2].cpu().numpy()


def test_backward_towers_end_to_end():
    cfg, m = released_model()
    inputs = labelled_batch()
    head = m.proposal_generator.dafne_head
    want_losses = {k: v.clone() for k, v in m.backward_head_tail(inputs).items()}
    torch.cuda.synchronize()
    tail = m.tail_parameters()
    tail_grads = [p.grad.clone() for p in tail]
    m.zero_grad(set_to_none=True)
    got = m.backward_towers(inputs)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want_losses)
    for k in got:
        assert torch.equal(got[k], want_losses[k]), k
    params = m.tower_parameters()
    assert len(params) == 45 and len(tail) == 19 and all(a is b for a, b in zip(params[:19], tail))
    assert len(set(id(p) for p in params)) == 45
    for p, g in zip(tail, tail_grads):
        assert torch.equal(p.grad, g), "a gradient of tail_parameters differs from backward_head_tail"
    names = {id(p): k for k, p in m.named_parameters()}
    # every listed parameter gets a finite gradient, and a non-zero one -- but for a per-level scale whose level holds no positive
    # location on this small batch: that gradient is exactly zero in backward_head_tail too (the bits above), by the loss's definition
    for k, p in enumerate(params):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), names[id(p)]
        assert float(p.grad.abs().sum()) > 0 or (k < 19 and ".scales." in names[id(p)]), names[id(p)]
    assert sum(float(p.grad.abs().sum()) > 0 for p in params if ".scales." in names[id(p)]) >= 1
    # the documented order of the 13 tensors per tower
    for t, name in enumerate(TOWERS):
        want = ["9.weight"] + [k for i in (2, 1, 0) for k in ("%d.weight" % (3 * i + 1), "%d.bias" % (3 * i + 1), "%d.bias" % (3 * i),
                                                              "%d.weight" % (3 * i))]
        gotn = [names[id(p)].split("dafne_head.")[1] for p in params[19 + 13 * t:19 + 13 * (t + 1)]]
        assert gotn == ["%s.%s" % (name, k) for k in want], gotn
    ids = set(id(p) for p in params)
    with_grad = [names[id(p)] for p in m.parameters() if p.grad is not None and id(p) not in ids]
    assert not with_grad, "frozen parameters received a gradient: %s" % with_grad[:4]
    assert all(p.grad is None for k, p in m.named_parameters() if "center_tower" in k or k.startswith("backbone."))

    # ---- every layer against the restatement, on what it read
    last = m._last_towers
    assert last["plan"] is m._last_validation["plan"] and last["plan"] is m._last_head_tail["plan"]
    hp = last["plan"].head
    assert sorted(hp.tower_calls) == sorted((n_, i) for n_ in ("center_tower",) + TOWERS for i in range(4))
    # corners_tower.0 normalises center_tower.9's raw map on load; cls_tower.0 reads the FPN maps as they are
    assert hp.tower_inputs[("corners_tower", 0)][1] is not None and hp.tower_inputs[("cls_tower", 0)][1] is None
    shapes = [tuple(t.shape[1:3]) for t in hp.logits]
    lane_px = R.lane_pixels(shapes, 2, cus())
    worst = {"wgrad": 0.0, "dgrad": 0.0}

    def check(kind, name, got_t, ref, bound):
        err = np.abs(got_t.detach().cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
        with np.errstate(all="ignore"):
            worst[kind] = max(worst[kind], float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert (err <= bound).all(), (name, float(np.max(err - bound)))
    for name in TOWERS:
        mods = getattr(head, name)
        for i in (3, 2, 1, 0):
            g = [t.cpu().numpy() for t in last["g"][(name, i)]]
            assert any(float(np.abs(x).max()) > 0 for x in g), "%s layer %d: the gradient is all zero" % (name, i)
            xs, stats, gamma, beta = layer_inputs(hp, name, i)
            xa = xs if stats is None else [R.applied(x, st, gamma, beta) for x, st in zip(xs, stats)]
            dW, _, aW, _, npx = R.wgrad(xa, g)
            check("wgrad", "%s.%d.weight" % (name, 3 * i), mods[3 * i].weight.grad, dW, R.wgrad_bound(aW, npx))
            if i == 0:
                continue
            call = hp.tower_calls[(name, i)]
            ref = R.layer_backward(xs, stats, gamma, beta, unpacked(call.keep[0], 256), g, [a > 0 for a in xa])
            for l, t in enumerate(last["g"][(name, i - 1)]):
                assert tuple(t.shape) == (2,) + shapes[l] + (256,)
                check("dgrad", "%s layer %d gx[%d]" % (name, i, l), t, ref["gx"][l], R.bound_gx(ref["gx_abs"][l]))
            check("dgrad", "%s.%d.weight" % (name, 3 * i - 2), mods[3 * i - 2].weight.grad, ref["dgamma"], R.bound_sum(ref["dgamma_abs"], lane_px))
            check("dgrad", "%s.%d.bias" % (name, 3 * i - 2), mods[3 * i - 2].bias.grad, ref["dbeta"], R.bound_sum(ref["dbeta_abs"], lane_px))
            check("dgrad", "%s.%d.bias" % (name, 3 * i - 3), mods[3 * i - 3].bias.grad, ref["dbias"], R.bound_sum(ref["dbias_abs"], lane_px))
    print("backward_towers: largest err / bound: weight gradient %.4f, data gradient %.4f" % (worst["wgrad"], worst["dgrad"]))

    # ---- accumulation: a second call doubles .grad exactly; zero_grad() and one call reproduce the first bits
    first = [p.grad.clone() for p in params]
    m.backward_towers(inputs)
    torch.cuda.synchronize()
    for p, f in zip(params, first):
        assert torch.equal(p.grad, f + f)
    m.zero_grad(set_to_none=True)
    m.backward_towers(inputs)
    torch.cuda.synchronize()
    for p, f in zip(params, first):
        assert torch.equal(p.grad, f)
    m.zero_grad(set_to_none=True)
    m.invalidate()
    assert m._last_towers is None


def test_sgd_loop_over_tower_parameters_lowers_the_loss():
    cfg, m = released_model()
    inputs = labelled_batch()
    opt = torch.optim.SGD(m.tower_parameters(), lr=LOOP_LR)
    towers = m.tower_parameters()[19:]
    start = [p.detach().clone() for p in towers]
    totals = []
    for _ in range(LOOP_K):
        opt.zero_grad(set_to_none=True)
        totals.append(m.backward_towers(inputs)["loss/total"])
        opt.step()
        m.invalidate()
    totals.append(m.validation_losses(inputs)["loss/total"])
    torch.cuda.synchronize()
    totals = [float(t) for t in totals]
    print("sgd loop over tower_parameters K=%d lr=%g: %s" % (LOOP_K, LOOP_LR, ["%.6f" % v for v in totals]))
    assert totals[-1] < totals[0], totals
    assert all(not torch.equal(p.detach(), s) for p, s in zip(towers, start)), "a tower parameter did not move"
    m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("strategy,centerness", [("direct", "none"), ("offset", "plain")])
def test_ablation_heads_get_all_tower_gradients(strategy, centerness):
    from test_gpu_ablation_head import ablation_model
    _, m = ablation_model(strategy, centerness)
    inputs = labelled_batch()
    m.zero_grad(set_to_none=True)
    want = {k: v.clone() for k, v in m.validation_losses(inputs).items()}
    got = m.backward_towers(inputs)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k])
    params = m.tower_parameters()
    assert len(params) == (4 if centerness == "none" else 6) + 5 + 6 + 26
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert all(float(p.grad.abs().sum()) > 0 for p in params[-26:])
    ids = set(id(p) for p in params)
    assert all(p.grad is None for p in m.parameters() if id(p) not in ids)
    m.zero_grad(set_to_none=True)
    m.invalidate()


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
        it.backward_towers(inputs)
    with pytest.raises(NotImplementedError):
        it.tower_parameters()
    cfg8 = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), ["ENGINE.WEIGHT_DTYPE", "fp8_e4m3"])
    with pytest.raises(NotImplementedError):
        build_model(cfg8).backward_towers(inputs)
    # the engine switches that keep the raw maps: off -> a layer reads an already normalised map
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
    for env, match in (("DAFNE_FUSE_GN", "fuse_gn "), ("DAFNE_FUSE_GN_PRED", "fuse_gn_pred")):
        monkeypatch.setenv(env, "0")
        plain = build_model(cfg)
        plain.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=5))
        plain.to(dev())
        plain.invalidate()
        with pytest.raises(NotImplementedError, match=match):
            plain.backward_towers(inputs)
        torch.cuda.synchronize()
        assert all(p.grad is None for p in plain.parameters())
        monkeypatch.delenv(env)
    _, m = released_model()
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError):
        m.backward_towers(inputs)
    assert all(p.grad is None for p in m.parameters())


def test_finetune_tool_with_towers_runs_on_a_scene_directory(tmp_path, capsys):
    """tools/finetune_pred.py --towers on two small synthetic scenes with labelTxt: two steps, one JSON line of finite losses per
    step, and a checkpoint that checkpoint.load_weights loads completely, in which the prediction layers and cls_tower /
    corners_tower moved and nothing else did."""
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
                             "--overlap", "32", "--lr", "0.003", "--seed", "1", "--towers", "--out", str(out),
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
    allowed = ["cls_logits.", "corners_pred.", "ctrness.", "center_pred.", "scales.", "cls_tower.", "corners_tower."]
    moved = [k for k in tuned if not torch.equal(tuned[k].cpu(), start[k])]
    assert moved and all(any(("dafne_head." + p) in k for p in allowed) for k in moved), moved[:5]
    for t in TOWERS:
        for i in range(4):
            for k in ("%d.weight" % (3 * i), "%d.bias" % (3 * i), "%d.weight" % (3 * i + 1), "%d.bias" % (3 * i + 1)):
                assert any(k2.endswith("dafne_head.%s.%s" % (t, k)) for k2 in moved), (t, k)
