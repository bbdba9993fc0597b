"""DAFNeOutputs.losses() with gradients: a torch.autograd.Function whose forward is the device path losses() always took
(assign_targets + dafne_losses_packed(cooked=True): the same launches, the same bits) and whose backward is one
dafne_losses_backward_hip call -- the derivative of the four loss terms (dafne_outputs.py:620-731, smooth_l1.py) with respect
to the head outputs that feed them, with the reference's autograd conventions (include/dafne_amd.h).

What is differentiated: logits <- loss/cls, corner regression <- loss/corners, center regression <- loss/center, centerness
logits <- loss/ctr.  The targets are constants.  Once differentiable; one process (dafne_losses_packed refuses a process
group with more than one rank).  Nothing is read back to the host between forward and backward: the backward re-adds the
forward's partial sums on the device.
"""
import contextlib
import ctypes

import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from ... import postprocess as pp


def _groups(outs, heads, n_levels):
    """The flat head tensors as (logits, corners, center or None, ctr or None), each a list over the levels."""
    it = [list(heads[i:i + n_levels]) for i in range(0, len(heads), n_levels)]
    logits, corners = it[0], it[1]
    k = 2
    center = ctr = None
    if outs.has_center_reg:
        center, k = it[k], k + 1
    if outs.has_centerness:
        ctr = it[k]
    return logits, corners, center, ctr


def _backward_call(call, levels, tg, grad4, grads):
    """One dafne_losses_backward_hip call.  grads: per level (logits, corners, center, ctr) NHWC fp32 buffers or None."""
    L = _lib.load()
    prm, descs = call["prm"], call["descs"]
    dev = levels[0].logits.device
    gd = (_lib.LevelGrad * len(levels))()
    for i, (gl, gc, ge, gt) in enumerate(grads):
        gd[i] = _lib.LevelGrad(_lib.ptr(gl), _lib.ptr(gc), _lib.ptr(ge), _lib.ptr(gt),
                               gl.shape[3] if gl is not None else 0, 8, 2, 1)
    with torch.cuda.device(dev):
        nbytes = L.dafne_losses_backward_workspace_bytes(ctypes.byref(prm), descs)
        if nbytes == 0:
            raise _lib.DafneHipError("dafne_losses_backward_workspace_bytes: bad parameters / level table")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_losses_backward_hip(
            ctypes.byref(prm), descs, _lib.ptr(tg.labels), _lib.ptr(tg.corners), _lib.ptr(tg.ltrb), _lib.ptr(tg.abcd),
            _lib.ptr(call["ws"]), call["ws_bytes"], _lib.ptr(grad4), gd, _lib.ptr(ws), nbytes, _lib.current_stream()),
            "dafne_losses_backward_hip")


class DafneLossFunction(torch.autograd.Function):
    """apply(outs, gt_instances, holder, n_levels, *heads) -> (loss/cls, loss/corners, loss/center, loss/ctr) as 0-dim fp32
    tensors (a term the configuration lacks: 0).  heads: the NCHW logits of every level, then the corner regressions, then the
    center regressions (center-to-corner only), then the centerness logits (with centerness only).  holder: a dict that
    receives losses()'s extras."""

    @staticmethod
    def forward(ctx, outs, gt_instances, holder, n_levels, *heads):
        logits, corners, center, ctr = _groups(outs, heads, n_levels)

        def nhwc(t):
            return t.detach().float().permute(0, 2, 3, 1).contiguous()
        levels = []
        for l, s in enumerate(outs.strides):
            levels.append(pp.LevelInput(nhwc(logits[l]), nhwc(corners[l]), nhwc(center[l]) if center is not None else None,
                                        nhwc(ctr[l]) if ctr is not None else None, s, 1.0))
        tg = outs.assign_targets([(lv.H, lv.W) for lv in levels], gt_instances, levels[0].logits.device)
        call = {}
        extras, _ = outs.dafne_losses_packed(levels, tg, cooked=True, _call=call)
        holder["extras"] = extras
        ctx.levels, ctx.tg, ctx.call = levels, tg, call
        ctx.n_levels, ctx.has = n_levels, (center is not None, ctr is not None)
        ctx.dtypes = [t.dtype for t in heads]
        r32 = extras["values_f64"].to(torch.float32)       # the conversion dafne_losses_packed makes: the same bits
        return r32[0], r32[1], r32[2], r32[3]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_corners, g_center, g_ctr):
        levels, tg, call, n_levels = ctx.levels, ctx.tg, ctx.call, ctx.n_levels
        needs = ctx.needs_input_grad[4:]
        has_center, has_ctr = ctx.has
        want = [any(needs[i:i + n_levels]) for i in range(0, len(needs), n_levels)]
        want_logits, want_corners = want[0], want[1]
        want_center = has_center and want[2]
        want_ctr = has_ctr and want[2 + int(has_center)]
        dev = levels[0].logits.device
        with torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext():
            grad4 = torch.stack([g.reshape(()) for g in (g_cls, g_corners, g_center, g_ctr)]).to(torch.float64)
            if dev.type == "cuda":      # the saved buffers may have been made on another stream than the one backward runs on
                cur = torch.cuda.current_stream()
                saved = [tg.labels, tg.corners, tg.ltrb, tg.abcd, call["ws"]]
                for lv in levels:
                    saved += [t for t in (lv.logits, lv.delta, lv.center, lv.ctrness) if t is not None]
                for t in saved:
                    t.record_stream(cur)
            grads = []
            for lv in levels:
                grads.append((torch.empty_like(lv.logits) if want_logits else None,
                              torch.empty_like(lv.delta) if want_corners else None,
                              torch.empty_like(lv.center) if want_center else None,
                              torch.empty_like(lv.ctrness) if want_ctr else None))
            if want_logits or want_corners or want_center or want_ctr:
                _backward_call(call, levels, tg, grad4, grads)
        out = []
        for k in range(len(needs) // n_levels):
            col = k if k < 2 else (2 if (k == 2 and has_center) else 3)
            for l in range(n_levels):
                i = k * n_levels + l
                g = grads[l][col]
                out.append(g.permute(0, 3, 1, 2).to(ctx.dtypes[i]) if (needs[i] and g is not None) else None)
        return (None, None, None, None) + tuple(out)


def losses_with_grad(outs, logits_pred, corners_reg_pred, center_reg_pred, ctrness_pred, gt_instances):
    """DAFNeOutputs.losses()'s (extras, losses) with a grad_fn on the losses."""
    n_levels = len(outs.strides)
    heads = list(logits_pred)[:n_levels] + list(corners_reg_pred)[:n_levels]
    if outs.has_center_reg:
        heads += list(center_reg_pred)[:n_levels]
    if outs.has_centerness:
        heads += list(ctrness_pred)[:n_levels]
    if len(heads) % n_levels or any(not isinstance(t, torch.Tensor) for t in heads):
        raise ValueError("losses: every head output needs one tensor per level (%d levels)" % n_levels)
    holder = {}
    l_cls, l_corners, l_center, l_ctr = DafneLossFunction.apply(outs, gt_instances, holder, n_levels, *heads)
    losses = {"loss/cls": l_cls, "loss/corners": l_corners}
    if outs.has_center_reg:
        losses["loss/center"] = l_center
    if outs.has_centerness:
        losses["loss/ctr"] = l_ctr
    return holder["extras"], losses
