"""CPU: the fp64 restatement of the prediction layers' backward (tests/_pred_backward_np.py) against torch autograd, the row split
of the fused corners_ctrness gradient, the library's refusals without a device, and the restatement's own fine-tune loop.

Loop: K = 6 SGD steps at learning rate 0.02 on synthetic non-negative bf16 tower maps (2 images of 64 x 96, the released head at
std 0.01 weights); the test prints the drop of the total loss and asserts it is positive and many times the step-to-step noise of
bf16 weight rounding (the drop of the same loop with fp64 weights differs from it by less than a tenth).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _pred_backward_np as R
import _targets_np as tn

HEADS = [("center-to-corner", True), ("center-to-corner", False), ("direct", True), ("direct", False), ("offset", True),
         ("offset", False)]


def synthetic(strategy, has_ctr, seed=0, n=2, shapes=((5, 7), (3, 4), (1, 2))):
    rng = np.random.default_rng(seed)
    C = 16
    towers = {k: [R.bf16_round(np.abs(rng.normal(0, 1, (n, h, w, C))).astype(np.float32)).astype(np.float64) for h, w in shapes]
              for k in ("cls", "corners", "center")}
    params = {"cls_logits.weight": rng.normal(0, 0.1, (15, C, 3, 3)), "cls_logits.bias": rng.normal(0, 0.1, 15),
              "corners_pred.weight": rng.normal(0, 0.1, (8, C, 3, 3)), "corners_pred.bias": rng.normal(0, 0.1, 8),
              "scales": [1.0 + 0.1 * l for l in range(len(shapes))]}
    if has_ctr:
        params.update({"ctrness.weight": rng.normal(0, 0.1, (1, C, 3, 3)), "ctrness.bias": rng.normal(0, 0.1, 1)})
    if strategy == "center-to-corner":
        params.update({"center_pred.weight": rng.normal(0, 0.1, (2, C, 3, 3)), "center_pred.bias": rng.normal(0, 0.1, 2)})
    if strategy == "offset":
        params["base_corners"] = np.array([-2.0, 2.0, 2.0, 2.0, 2.0, -2.0, -2.0, -2.0])
    return params, towers


@pytest.mark.parametrize("strategy,has_ctr", HEADS)
def test_restatement_equals_autograd(strategy, has_ctr):
    """conv -> cook -> an arbitrary smooth scalar of the finished outputs: the restatement's uncook + weight gradient equals torch
    autograd in fp64 through F.conv2d and the cooking expressions to 1e-12 relative."""
    c2c = strategy == "center-to-corner"
    params, towers = synthetic(strategy, has_ctr, seed=len(strategy) + has_ctr)
    rng = np.random.default_rng(5)
    keys = [k for k in params if k not in ("scales", "base_corners")]
    tp = {k: torch.tensor(R.bf16_round(np.asarray(params[k], np.float32)).astype(np.float64) if k.endswith("weight")
                          else np.asarray(params[k], np.float32).astype(np.float64), requires_grad=True) for k in keys}
    ts = [torch.tensor(float(np.float32(s)), dtype=torch.float64, requires_grad=True) for s in params["scales"]]

    def conv(x, w, b):
        return F.conv2d(torch.tensor(x).permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)
    total = 0.0
    ups = []
    for l in range(len(ts)):
        logits = conv(towers["cls"][l], tp["cls_logits.weight"], tp["cls_logits.bias"])
        bias = tp["corners_pred.bias"] + (torch.tensor(params["base_corners"]) if strategy == "offset" else 0.0)
        delta = conv(towers["corners"][l], tp["corners_pred.weight"], bias)
        shp = tuple(logits.shape[:3])
        u = {"logits": rng.normal(0, 1, shp + (15,)), "reg": rng.normal(0, 1, shp + (8,)), "creg": rng.normal(0, 1, shp + (2,)),
             "ctr": rng.normal(0, 1, shp + (1,))}
        ups.append(u)
        if c2c:
            center = conv(towers["center"][l], tp["center_pred.weight"], tp["center_pred.bias"])
            reg, creg = (center.repeat(1, 1, 1, 4) + delta) * ts[l], center * ts[l]
            total = total + (creg * torch.tensor(u["creg"])).sum()
        else:
            reg = delta * ts[l]
        total = total + (logits * torch.tensor(u["logits"])).sum() + (reg * torch.tensor(u["reg"])).sum()
        if has_ctr:
            ctr = conv(towers["corners"][l], tp["ctrness.weight"], tp["ctrness.bias"])
            total = total + (ctr * torch.tensor(u["ctr"])).sum()
    total.backward()
    # the restatement: the same upstream gradients through uncook and wgrad
    lv = R.forward_head(params, towers, strategy, has_ctr)
    g_cc, g_ce, g_sc = [], [], []
    for l, o in enumerate(lv):
        gd, gc, gs = R.uncook(ups[l]["reg"], ups[l]["creg"] if c2c else None, o["delta"], o["center"], o["scale"])
        g_cc.append(np.concatenate([gd, ups[l]["ctr"]], -1) if has_ctr else gd)
        g_ce.append(gc)
        g_sc.append(gs)
    got = {}
    dW, db, _, _, _ = R.wgrad(towers["cls"], [u["logits"] for u in ups])
    got["cls_logits.weight"], got["cls_logits.bias"] = dW, db
    dW, db, _, _, _ = R.wgrad(towers["corners"], g_cc)
    got.update(R.split_fused(dW, db, has_ctr))
    if c2c:
        dW, db, _, _, _ = R.wgrad(towers["center"], g_ce)
        got["center_pred.weight"], got["center_pred.bias"] = dW, db
    assert sorted(got) == sorted(keys)

    def close(a, b, what):
        scale = max(np.abs(b).max(), 1e-300)
        assert np.abs(a - b).max() <= 1e-12 * scale, (what, np.abs(a - b).max() / scale)
    for k in keys:
        close(got[k], tp[k].grad.numpy(), k)
    for l in range(len(ts)):
        close(np.array(g_sc[l]), ts[l].grad.numpy(), "scale %d" % l)


def test_fused_rows_map_to_the_state_dict_keys():
    from dafne_amd.modeling.dafne.pred_backward import split_corners_ctrness
    dw, db = torch.arange(9 * 256 * 9, dtype=torch.float32).reshape(9, 256, 3, 3), torch.arange(9, dtype=torch.float32)
    for strategy in ("center-to-corner", "direct", "offset"):
        s = split_corners_ctrness(dw, db, (strategy, True))
        assert sorted(s) == ["corners_pred.bias", "corners_pred.weight", "ctrness.bias", "ctrness.weight"]
        assert torch.equal(s["corners_pred.weight"], dw[:8]) and torch.equal(s["ctrness.weight"], dw[8:9])
        assert torch.equal(s["corners_pred.bias"], db[:8]) and torch.equal(s["ctrness.bias"], db[8:9])
        s = split_corners_ctrness(dw[:8], db[:8], (strategy, False))
        assert sorted(s) == ["corners_pred.bias", "corners_pred.weight"]
        with pytest.raises(ValueError):
            split_corners_ctrness(dw, db, (strategy, False))
    with pytest.raises(NotImplementedError):
        split_corners_ctrness(dw, db, ("iterative", True))
    # the same order as the restatement's and as pack_head_weights' concatenation (corners_pred rows, then ctrness)
    r = R.split_fused(dw.numpy(), db.numpy(), True)
    assert np.array_equal(r["ctrness.weight"], dw[8:9].numpy())


def test_abi_and_refusals_without_a_device():
    from dafne_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.dafne_abi_version() >= 154
    seg = (_lib.ConvSeg * 1)(_lib.ConvSeg(8, None, None, 2, 3, 2, 3))
    ptrs = (ctypes.c_void_p * 1)(8)

    def prm(**kw):
        p = _lib.ConvParams(1, 1, 256, 9, 3, 3, 1, 1, 8, None, None, None, None, None, None, None, None, 0.0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(p, ps=9, g=ptrs):
        return L.dafne_pred_wgrad_hip(ctypes.byref(p), seg, g, ps, ctypes.c_void_p(8), ctypes.c_void_p(8), ctypes.c_void_p(8), 1 << 30,
                                      None)
    assert call(prm(Cin=128)) == 4 and call(prm(Cout=17)) == 4 and call(prm(Cout=0)) == 4
    assert call(prm(KH=1, KW=1, pad=0)) == 4 and call(prm(stride=2)) == 4
    assert call(prm(), ps=8) == 1 and call(prm(n_segs=6)) == 1 and call(prm(), g=None) == 1
    assert call(prm(flags=8 | 32)) == 1                                    # GN input without statistics
    assert b"pred_wgrad" in L.dafne_last_error()
    assert L.dafne_pred_wgrad_workspace_bytes(ctypes.byref(prm(Cin=128)), seg) == 0
    lv = (_lib.UncookLevel * 1)(_lib.UncookLevel(8, None, None, 8, None, 8, None, 8, 2, 1, 8, 2, 8, 2, 2, 3, 1.0))
    assert L.dafne_head_uncook_backward_workspace_bytes(lv, 1, 2) == 8       # 12 pixels: one workgroup's partial
    assert L.dafne_head_uncook_backward_hip(lv, 1, 2, None, ctypes.c_void_p(8), 8, None) == 1
    lv[0].g_delta_ps = 7
    assert L.dafne_head_uncook_backward_hip(lv, 1, 2, ctypes.c_void_p(8), ctypes.c_void_p(8), 8, None) == 1
    lv[0].g_delta_ps = 8
    lv[0].d_center = 8                                                       # a center without its gradients
    assert L.dafne_head_uncook_backward_hip(lv, 1, 2, ctypes.c_void_p(8), ctypes.c_void_p(8), 8, None) == 1
    assert L.dafne_head_uncook_backward_hip(lv, 9, 2, ctypes.c_void_p(8), ctypes.c_void_p(8), 8, None) == 1


def loop_case():
    """2 images of 64 x 96, the released configuration, synthetic non-negative bf16 tower maps with 32 channels."""
    rng = np.random.default_rng(17)
    h, w = 64, 96
    gts = [tn.gt_of(tn.random_quads(4, rng, h, w, lo=10.0, hi=50.0), rng.integers(0, 15, 4)),
           tn.gt_of(tn.random_quads(2, rng, h, w, lo=30.0, hi=90.0), rng.integers(0, 15, 2))]
    shapes = tn.level_shapes(h, w)
    tg = tn.assign(gts, shapes, tn.assign_config("released"))
    C = 32
    towers = {k: [R.bf16_round(np.abs(rng.normal(0, 1, (2, a, b, C))).astype(np.float32)).astype(np.float64) for a, b in shapes]
              for k in ("cls", "corners", "center")}
    params = {"cls_logits.weight": rng.normal(0, 0.01, (15, C, 3, 3)), "cls_logits.bias": np.full(15, -4.59512),
              "corners_pred.weight": rng.normal(0, 0.01, (8, C, 3, 3)), "corners_pred.bias": np.zeros(8),
              "ctrness.weight": rng.normal(0, 0.01, (1, C, 3, 3)), "ctrness.bias": np.zeros(1),
              "center_pred.weight": rng.normal(0, 0.01, (2, C, 3, 3)), "center_pred.bias": np.zeros(2),
              "scales": [1.0] * 5}
    return params, towers, tg


def test_restatement_loop_lowers_the_loss(monkeypatch):
    params, towers, tg = loop_case()
    assert (tg["labels"] != 15).sum() > 0
    K, lr = 6, 0.02
    totals, _ = R.sgd_loop(params, towers, tg, tn.LOSS_RELEASED, lr, K)
    monkeypatch.setattr(R, "bf16_round", lambda x: np.asarray(x, dtype=np.float32))      # the same loop without bf16 weights
    exact, _ = R.sgd_loop(params, towers, tg, tn.LOSS_RELEASED, lr, K)
    drop, drop_exact = totals[0] - totals[-1], exact[0] - exact[-1]
    print("restatement loop K=%d lr=%g: total %s, drop %.6f (fp32 weights: %.6f)" % (K, lr, ["%.6f" % t for t in totals], drop,
                                                                                       drop_exact))
    assert drop > 0 and all(b < a for a, b in zip(totals, totals[1:]))
    assert abs(drop - drop_exact) < 0.1 * drop, "the drop is not several times the noise of bf16 weight rounding"
