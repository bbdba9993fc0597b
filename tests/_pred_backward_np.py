"""fp64 restatement (numpy / CPU torch) of the backward of the head's prediction layers, independent of the HIP kernels:

    bf16_round            fp32 -> bf16 round-to-nearest-even, as torch rounds (pack_head_weights / pack_conv)
    wgrad                 weight and bias gradient of a 3x3 / stride 1 / pad 1 convolution over several levels, with the
                          sum of |g x| per element that the kernel's error bound is stated in
    cook / uncook         the finished regressions of DAFNeHead.forward (dafne.py:394-411) and the chain rule back through them
    finetune_step / loop  one complete fine-tune step on given tower maps: round the weights to bf16, 3x3 conv, cook,
                          tests/_targets_np.py values, tests/_targets_grad_np.py gradients, uncook, weight gradient, SGD

Layouts: maps X [N, H, W, C] (un-haloed; the convolution pads with zeros), gradients g [N, H, W, Cout], weights OIHW
[Cout, C, 3, 3] as in the state dict.
"""
import numpy as np


def bf16_round(x):
    """fp32 array -> the nearest bf16 (ties to even), returned as fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def conv3x3(X, w, b):
    """X [N,H,W,C] f64, w [Cout,C,3,3], b [Cout] -> [N,H,W,Cout] f64 (zero padding 1)."""
    N, H, W, C = X.shape
    Xp = np.zeros((N, H + 2, W + 2, C), dtype=np.float64)
    Xp[:, 1:-1, 1:-1] = X
    out = np.zeros((N, H, W, w.shape[0]), dtype=np.float64) + np.asarray(b, dtype=np.float64)
    for kh in range(3):
        for kw in range(3):
            out += np.einsum("nyxc,oc->nyxo", Xp[:, kh:kh + H, kw:kw + W], np.asarray(w[:, :, kh, kw], dtype=np.float64))
    return out


def wgrad(Xs, gs):
    """Xs, gs: per level [N,H,W,C] / [N,H,W,Cout] -> (dW [Cout,C,3,3], db [Cout], absW, absb, n): absW / absb are the sums of
    |g x| (|g| for the bias) behind every element, n the number of summed pixels."""
    C, Co = Xs[0].shape[3], gs[0].shape[3]
    dW = np.zeros((Co, C, 3, 3)); aW = np.zeros((Co, C, 3, 3)); db = np.zeros(Co); ab = np.zeros(Co)
    n = 0
    for X, g in zip(Xs, gs):
        X = np.asarray(X, dtype=np.float64); g = np.asarray(g, dtype=np.float64)
        N, H, W, _ = X.shape
        n += N * H * W
        Xp = np.zeros((N, H + 2, W + 2, C), dtype=np.float64)
        Xp[:, 1:-1, 1:-1] = X
        for kh in range(3):
            for kw in range(3):
                P = Xp[:, kh:kh + H, kw:kw + W].reshape(-1, C)
                dW[:, :, kh, kw] += g.reshape(-1, Co).T @ P
                aW[:, :, kh, kw] += np.abs(g).reshape(-1, Co).T @ np.abs(P)
        db += g.sum((0, 1, 2))
        ab += np.abs(g).sum((0, 1, 2))
    return dW, db, aW, ab, n


def wgrad_bound(absum, n):
    """The kernel's bound: g as a hi + lo bf16 pair (2^-16 covers the split and the final rounding), fp32 accumulation over n
    pixels."""
    return (2.0 ** -16 + n * 2.0 ** -24) * absum


# ---------------------------------------------------------------------------------------------- cook / uncook
def cook(delta, center, scale):
    """delta [..., 8], center [..., 2] or None -> (reg [..., 8], center_reg [..., 2] or None): dafne.py:394-411."""
    if center is None:
        return delta * scale, None
    return (np.tile(center, 4) + delta) * scale, center * scale


def uncook(g_reg, g_center_reg, delta, center, scale):
    """Gradients of the finished tensors -> (g_delta, g_center or None, g_scale): g_delta = s g_reg; g_center = s (sum over the
    four corners of g_reg + g_center_reg); g_scale = sum g_reg (center.repeat + delta) + sum g_center_reg center."""
    g_reg = np.asarray(g_reg, dtype=np.float64); delta = np.asarray(delta, dtype=np.float64)
    g_delta = g_reg * scale
    if center is None:
        return g_delta, None, float((g_reg * delta).sum())
    center = np.asarray(center, dtype=np.float64); g_center_reg = np.asarray(g_center_reg, dtype=np.float64)
    g_center = scale * (g_reg.reshape(g_reg.shape[:-1] + (4, 2)).sum(-2) + g_center_reg)
    g_scale = float((g_reg * (np.tile(center, 4) + delta)).sum() + (g_center_reg * center).sum())
    return g_delta, g_center, g_scale


def uncook_abs_terms(g_reg, g_center_reg, delta, center):
    """sum of |terms| of g_scale (its error bound is stated in it)."""
    g_reg = np.asarray(g_reg, dtype=np.float64); delta = np.asarray(delta, dtype=np.float64)
    if center is None:
        return float(np.abs(g_reg * delta).sum())
    center = np.asarray(center, dtype=np.float64); g_center_reg = np.asarray(g_center_reg, dtype=np.float64)
    return float(np.abs(g_reg * (np.tile(center, 4) + delta)).sum() + np.abs(g_center_reg * center).sum())


# ---------------------------------------------------------------------------------------------- the fine-tune step
def split_fused(dw, db, has_ctr):
    """rows of the fused corners_ctrness gradient -> state-dict keys (engine.pack_head_weights' order)."""
    out = {"corners_pred.weight": dw[:8], "corners_pred.bias": db[:8]}
    if has_ctr:
        out["ctrness.weight"] = dw[8:9]
        out["ctrness.bias"] = db[8:9]
    return out


def forward_head(params, towers, strategy, has_ctr):
    """params: {"cls_logits.weight": ..., "scales": [5]}, fp64 master values; towers: {"cls": [X per level], "corners": [...],
    "center": [...]} -> per-level dict of raw and finished outputs.  The weights are rounded to bf16 as pack_head_weights
    rounds them, the biases stay fp32 (the offset head's base_corners joins the bias)."""
    def w16(k):
        return bf16_round(np.asarray(params[k], dtype=np.float32)).astype(np.float64)

    def b32(k):
        return np.asarray(params[k], dtype=np.float32).astype(np.float64)
    c2c = strategy == "center-to-corner"
    out = []
    for l in range(len(towers["cls"])):
        logits = conv3x3(towers["cls"][l], w16("cls_logits.weight"), b32("cls_logits.bias"))
        bias = b32("corners_pred.bias")
        if strategy == "offset":
            bias = bias + np.asarray(params["base_corners"], dtype=np.float64).reshape(8)
        delta = conv3x3(towers["corners"][l], w16("corners_pred.weight"), bias)
        ctr = conv3x3(towers["corners"][l], w16("ctrness.weight"), b32("ctrness.bias")) if has_ctr else None
        center = conv3x3(towers["center"][l], w16("center_pred.weight"), b32("center_pred.bias")) if c2c else None
        s = float(np.float32(params["scales"][l]))
        reg, creg = cook(delta, center, s)
        out.append({"logits": logits, "delta": delta, "center": center, "ctr": ctr, "reg": reg, "center_reg": creg, "scale": s})
    return out


def finetune_step(params, towers, tg, Lc, strategy="center-to-corner", has_ctr=True):
    """-> (losses dict from tests/_targets_np.losses, grads {key: fp64 gradient}) for one batch.  tg: tests/_targets_np.assign's
    targets, Lc: its loss configuration."""
    import _targets_grad_np as G
    import _targets_np as T
    c2c = strategy == "center-to-corner"
    lv = forward_head(params, towers, strategy, has_ctr)

    def flat(key, c):
        return np.concatenate([o[key].reshape(-1, c) for o in lv], 0)
    nc = lv[0]["logits"].shape[-1]
    logits, reg = flat("logits", nc), flat("reg", 8)
    creg = flat("center_reg", 2) if c2c else None
    ctr = flat("ctr", 1).reshape(-1) if has_ctr else None
    vals = T.losses(logits, reg, creg, ctr, tg, Lc)
    g = G.grads(logits, reg, creg, ctr, tg, Lc)
    grads, off = {}, 0
    g_logits, g_cc, g_ce, g_scales = [], [], [], []
    for o in lv:
        n_px = o["logits"].shape[0] * o["logits"].shape[1] * o["logits"].shape[2]
        sl = slice(off, off + n_px)
        off += n_px
        shp = o["logits"].shape[:3]
        g_logits.append(np.asarray(g["logits"][sl]).reshape(shp + (nc,)))
        g_reg = np.asarray(g["corners"][sl]).reshape(shp + (8,))
        g_creg = np.asarray(g["center"][sl]).reshape(shp + (2,)) if c2c else None
        gd, gc, gs = uncook(g_reg, g_creg, o["delta"], o["center"], o["scale"])
        if has_ctr:
            gd = np.concatenate([gd, np.asarray(g["ctr"][sl]).reshape(shp + (1,))], -1)
        g_cc.append(gd)
        g_ce.append(gc)
        g_scales.append(gs)
    dW, db, _, _, _ = wgrad(towers["cls"], g_logits)
    grads["cls_logits.weight"], grads["cls_logits.bias"] = dW, db
    dW, db, _, _, _ = wgrad(towers["corners"], g_cc)
    grads.update(split_fused(dW, db, has_ctr))
    if c2c:
        dW, db, _, _, _ = wgrad(towers["center"], g_ce)
        grads["center_pred.weight"], grads["center_pred.bias"] = dW, db
    for l, gs in enumerate(g_scales):
        grads["scales.%d.scale" % l] = np.array([gs])
    return vals, grads, {"g_logits": g_logits, "g_cc": g_cc, "g_center": g_ce, "levels": lv}


def sgd_loop(params, towers, tg, Lc, lr, steps, momentum=0.0, strategy="center-to-corner", has_ctr=True):
    """`steps` plain SGD steps (torch.optim.SGD's update: buf = momentum buf + grad, p -= lr buf) on fp64 master parameters
    -> the total loss before every step and after the last."""
    params = {k: (list(v) if k == "scales" else np.array(v, dtype=np.float64)) for k, v in params.items()}
    bufs, totals = {}, []

    def total(vals):
        return float(vals["cls"] + vals["corners"] + vals["center"] + vals["ctr"])
    for _ in range(steps):
        vals, grads, _ = finetune_step(params, towers, tg, Lc, strategy, has_ctr)
        totals.append(total(vals))
        for k, g in grads.items():
            buf = bufs.get(k)
            buf = g.copy() if buf is None else momentum * buf + g
            bufs[k] = buf
            if k.startswith("scales."):
                params["scales"][int(k.split(".")[1])] -= lr * float(buf[0])
            else:
                params[k] = params[k] - lr * buf
    vals, _, _ = finetune_step(params, towers, tg, Lc, strategy, has_ctr)
    totals.append(total(vals))
    return totals, params
