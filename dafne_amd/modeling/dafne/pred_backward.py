"""Backward of the head's prediction layers (DESIGN row F11): the weight / bias gradients of cls_logits, corners_pred,
ctrness and center_pred (dafne.py:318-344) and the gradients of the five per-level scales, from the loss gradients with
respect to the finished head outputs (loss_function.py / dafne_losses_backward_hip).

    pred_wgrad(call, gouts, ps)            one dafne_pred_wgrad_hip launch pair on a forward prediction call's own description
    split_corners_ctrness(dw, db, mode)    rows of the fused corners_ctrness gradient -> state-dict keys
    uncook_backward(...)                   dafne_head_uncook_backward_hip: finished regressions -> raw delta / center / scales
    backward_prediction_layers(model, b)   what OneStageDetector.backward_prediction_layers runs

The last GroupNorm and bias of the complete towers are tail_backward.py's (DESIGN row F12), their convolutions and other GroupNorms
tower_backward.py's (DESIGN row F13); center_tower, the FPN and the backbone have no backward: they stay frozen.
"""
import ctypes

import torch

from ... import _lib

PRED_LAYERS = ("cls_logits", "corners_pred", "ctrness", "center_pred")


def pred_wgrad(call, gouts, ps=None, stream=None):
    """call: the forward prediction launch (engine.ConvCall: its prm / segs describe the input maps, the GroupNorm on load
    included).  gouts: per segment an fp32 device tensor [N, H, W, >= Cout] whose last dimension is contiguous and whose pixel
    stride is `ps` floats (default: the tensor's own; a view of the leading channels of a wider buffer works).
    -> (dW [Cout, 256, 3, 3], db [Cout]) fp32, OIHW as in the state dict; every element written, equal bits from run to run."""
    L = _lib.load()
    prm, segs = call.prm, call.segs
    n_segs, cout = int(prm.n_segs), int(prm.Cout)
    if len(gouts) != n_segs:
        raise ValueError("pred_wgrad: %d gradients for %d segments" % (len(gouts), n_segs))
    dev = gouts[0].device
    if dev.type != "cuda":
        raise _lib.DafneHipError("pred_wgrad: the MI355X engine has no CPU path (got CPU tensors)")
    for s, g in enumerate(gouts):
        if g.dtype != torch.float32 or g.dim() != 4 or g.stride(3) != 1:
            raise ValueError("pred_wgrad: gradient %d must be fp32 [N, H, W, C] with contiguous channels" % s)
        p = g.stride(2)
        if ps is None:
            ps = p
        if p != ps or g.stride(1) != ps * g.shape[2] or g.stride(0) != ps * g.shape[2] * g.shape[1]:
            raise ValueError("pred_wgrad: gradient %d is not a dense [N, H, W] grid of pixel stride %d" % (s, ps))
        if (g.shape[0], g.shape[1], g.shape[2]) != (prm.n_images, segs[s].Hout, segs[s].Wout) or g.shape[3] < cout:
            raise ValueError("pred_wgrad: gradient %d has shape %s" % (s, tuple(g.shape)))
    ptrs = (ctypes.c_void_p * n_segs)(*[g.data_ptr() for g in gouts])
    with torch.cuda.device(dev):
        nbytes = L.dafne_pred_wgrad_workspace_bytes(ctypes.byref(prm), segs)
        if nbytes == 0:
            # the launch below names the refusal
            nbytes = 16
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dw = torch.empty(cout, 256, 3, 3, dtype=torch.float32, device=dev)
        db = torch.empty(cout, dtype=torch.float32, device=dev)
        _lib.check(L.dafne_pred_wgrad_hip(ctypes.byref(prm), segs, ptrs, int(ps), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes,
                                          stream if stream is not None else _lib.current_stream()), "dafne_pred_wgrad_hip")
    return dw, db


def split_corners_ctrness(dw, db, head_mode):
    """The gradient of the fused corners_ctrness launch -> {state-dict key under dafne_head: gradient}: rows 0..7 are
    corners_pred, row 8 (with centerness) is ctrness (engine.pack_head_weights).  The offset head's base_corners is folded into
    the forward BIAS only, so db[:8] is corners_pred.bias's gradient unchanged.  The iterative head (rows = the tower parts of
    c0..c3_pred) has no backward here."""
    strategy, has_ctr = head_mode
    if strategy == "iterative":
        raise NotImplementedError("the prediction-layer backward does not cover CORNER_PREDICTION iterative (corner chain)")
    want = 9 if has_ctr else 8
    if dw.shape[0] != want or db.shape[0] != want:
        raise ValueError("corners_ctrness gradient with %d rows, the head has %d" % (dw.shape[0], want))
    out = {"corners_pred.weight": dw[:8], "corners_pred.bias": db[:8]}
    if has_ctr:
        out["ctrness.weight"] = dw[8:9]
        out["ctrness.bias"] = db[8:9]
    return out


def uncook_backward(g_reg, g_center_reg, g_ctrness, delta, delta_ps, center, scales, pred_c):
    """dafne_head_uncook_backward_hip over the levels.  g_reg [N,H,W,8], g_center_reg [N,H,W,2] or None, g_ctrness [N,H,W] or
    None: the loss gradients with respect to the finished tensors; delta (pixel stride delta_ps) / center: the raw outputs of
    the prediction convolutions; scales: the five floats the forward multiplied by.
    -> (g_delta per level [N,H,W,pred_c] with the centerness gradient in channel 8, g_center per level or None,
    g_scale [n_levels] fp64 on the device)."""
    L = _lib.load()
    n_levels = len(g_reg)
    dev = g_reg[0].device
    if dev.type != "cuda":
        raise _lib.DafneHipError("uncook_backward: the MI355X engine has no CPU path (got CPU tensors)")
    c2c, has_ctr = center is not None, g_ctrness is not None
    if pred_c != (9 if has_ctr else 8):
        raise ValueError("uncook_backward: %d prediction channels %s centerness" % (pred_c, "with" if has_ctr else "without"))
    n = int(g_reg[0].shape[0])
    lv = (_lib.UncookLevel * n_levels)()
    g_delta, g_center = [], ([] if c2c else None)
    with torch.cuda.device(dev):
        for l in range(n_levels):
            _, h, w, _ = g_reg[l].shape
            gd = torch.empty(n, h, w, pred_c, dtype=torch.float32, device=dev)
            gc = torch.empty(n, h, w, 2, dtype=torch.float32, device=dev) if c2c else None
            g_delta.append(gd)
            if c2c:
                g_center.append(gc)
            for t in (g_reg[l], delta[l]) + ((g_center_reg[l], center[l]) if c2c else ()) + ((g_ctrness[l],) if has_ctr else ()):
                if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                    raise ValueError("uncook_backward: contiguous fp32 device tensors only")
            lv[l] = _lib.UncookLevel(_lib.ptr(g_reg[l]), _lib.ptr(g_center_reg[l]) if c2c else None,
                                     _lib.ptr(g_ctrness[l]) if has_ctr else None, _lib.ptr(delta[l]),
                                     _lib.ptr(center[l]) if c2c else None, _lib.ptr(gd), _lib.ptr(gc),
                                     8, 2, 1, int(delta_ps), 2, pred_c, 2, h, w, float(scales[l]))
        nbytes = L.dafne_head_uncook_backward_workspace_bytes(lv, n_levels, n)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        g_scale = torch.empty(n_levels, dtype=torch.float64, device=dev)
        _lib.check(L.dafne_head_uncook_backward_hip(lv, n_levels, n, _lib.ptr(g_scale), _lib.ptr(ws), nbytes, _lib.current_stream()),
                   "dafne_head_uncook_backward_hip")
    return g_delta, g_center, g_scale


def prediction_parameters(model):
    """The parameters backward_prediction_layers gives a .grad, in a fixed order, for the optimiser: cls_logits.{weight,bias},
    corners_pred.*, ctrness.* (with centerness), center_pred.* (center-to-corner), scales.{0..4}.scale."""
    head = model.proposal_generator.dafne_head
    strategy, has_ctr = head.head_mode
    if strategy == "iterative":
        raise NotImplementedError("the prediction-layer backward does not cover CORNER_PREDICTION iterative (corner chain)")
    mods = [head.cls_logits, head.corners_pred] + ([head.ctrness] if has_ctr else []) + \
           ([head.center_pred] if strategy == "center-to-corner" else [])
    out = []
    for m in mods:
        out += [m.weight, m.bias]
    return out + [s.scale for s in head.scales]


def _accumulate(p, g):
    """autograd's rule: .grad is created when None, added to otherwise."""
    g = g.detach().reshape(p.shape).to(dtype=p.dtype, device=p.device)
    if p.grad is None:
        p.grad = g.clone()
    else:
        p.grad.add_(g)


def backward_prediction_layers(model, batch, _tail=None, _slot="train"):
    """OneStageDetector.backward_prediction_layers: validation_losses' forward on a plan slot of its own, then target
    assignment (the forward's), the cooked loss forward + backward, the uncook kernel and three weight-gradient calls;
    accumulates into .grad of prediction_parameters(model) and returns validation_losses' dict (the same launches: the same
    bits).  Nothing is read back to the host.
    _tail (tail_backward.backward_head_tail): called as _tail(plan, None, None) once the plan is known and before any .grad is
    touched (it may refuse the plan), and as _tail(plan, g_logits, g_delta) after the last launch here, with the per-level loss
    gradients with respect to the raw outputs of cls_logits and corners_pred (+ ctrness).
    _slot: the plan slot the forward runs on ("towers", tower_backward.backward_towers: that plan keeps the tower maps)."""
    import torch.distributed as dist
    from ... import postprocess as pp
    from .loss_function import _backward_call
    head = model.proposal_generator.dafne_head
    strategy, has_ctr = head.head_mode
    if strategy == "iterative":
        raise NotImplementedError("backward_prediction_layers does not cover CORNER_PREDICTION iterative: the corner chain "
                                  "has no backward")
    if model.cfg.ENGINE.WEIGHT_DTYPE == "fp8_e4m3":
        raise NotImplementedError("backward_prediction_layers needs bf16 compute weights (ENGINE.WEIGHT_DTYPE fp8_e4m3 serves "
                                  "a quantised model; fine-tune the bf16 one)")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("backward_prediction_layers is single-process: no gradient all-reduce (DDP is out of scope)")
    losses = model.validation_losses(batch, _slot=_slot)
    last = model._last_validation
    plan, tg = last["plan"], last["targets"]
    hp = plan.head
    if _tail is not None:
        _tail(plan, None, None)
    outs = model.proposal_generator.dafne_outputs
    strides = model.proposal_generator.fpn_strides
    c2c = hp.center is not None
    pred_c = hp.delta_ctr[0].shape[-1]
    dev = hp.logits[0].device
    with torch.cuda.device(dev):
        # the finished regressions, in DAFNeHead.forward's fp32 expressions (the raw form of the loss kernel rounds alike)
        cooked = []
        for l, s in enumerate(strides):
            sc, dc = hp.scales[l], hp.delta_ctr[l]
            if c2c:
                reg = ((hp.center[l].repeat(1, 1, 1, 4) + dc[..., :8]) * sc).contiguous()
                creg = (hp.center[l] * sc).contiguous()
            else:
                reg, creg = (dc[..., :8] * sc).contiguous(), None
            ctr = dc.view(-1)[8:] if has_ctr else None
            cooked.append(pp.LevelInput(hp.logits[l], reg, creg, ctr, s, 1.0, ctrness_ps=pred_c))
        call = {}
        cooked_extras, _ = outs.dafne_losses_packed(cooked, tg, cooked=True, _call=call)
        grads = []
        for lv in cooked:
            n, h, w = lv.N, lv.H, lv.W
            grads.append((torch.empty_like(lv.logits), torch.empty(n, h, w, 8, dtype=torch.float32, device=dev),
                          torch.empty(n, h, w, 2, dtype=torch.float32, device=dev) if c2c else None,
                          torch.empty(n, h, w, dtype=torch.float32, device=dev) if has_ctr else None))
        _backward_call(call, cooked, tg, torch.ones(4, dtype=torch.float64, device=dev), grads)
        g_delta, g_center, g_scale = uncook_backward(
            [g[1] for g in grads], [g[2] for g in grads] if c2c else None, [g[3] for g in grads] if has_ctr else None,
            hp.delta_ctr, pred_c, hp.center, hp.scales, pred_c)
        dw, db = pred_wgrad(hp.pred_calls["cls_logits"], [g[0] for g in grads])
        _accumulate(head.cls_logits.weight, dw)
        _accumulate(head.cls_logits.bias, db)
        dw, db = pred_wgrad(hp.pred_calls["corners_ctrness"], g_delta)
        for key, g in split_corners_ctrness(dw, db, (strategy, has_ctr)).items():
            mod, name = key.split(".")
            _accumulate(getattr(getattr(head, mod), name), g)
        if c2c:
            dw, db = pred_wgrad(hp.pred_calls["center_pred"], g_center)
            _accumulate(head.center_pred.weight, dw)
            _accumulate(head.center_pred.bias, db)
        gs32 = g_scale.to(torch.float32)
        for l, sp in enumerate(head.scales):
            _accumulate(sp.scale, gs32[l:l + 1])
        if _tail is not None:
            _tail(plan, [g[0] for g in grads], g_delta)
    # (tests: the plan the gradients were computed on and the cooked loss forward's fp64 row, which must equal the returned
    # raw-form values bit for bit; nothing else is kept alive, and invalidate() drops it)
    model._last_pred_backward = {"plan": plan, "cooked_values_f64": cooked_extras["values_f64"]}
    return losses
