"""Backward of the complete head towers (DESIGN row F13): from the gradient at the raw output of <tower>.9, where tail_backward.py
ends, down through the four 3x3 256 -> 256 convolutions and three GroupNorms of cls_tower and corners_tower.

    tower_wgrad(call, gouts)              one dafne_tower_wgrad_hip call on a forward tower launch's own description
    tower_dgrad_gn(call, weight, gouts)   one dafne_tower_dgrad_gn_hip call on the same description
    tower_parameters(model)               tail_parameters + per complete tower .9.weight, then for i = 2, 1, 0
                                          .{3i+1}.weight, .{3i+1}.bias, .{3i}.bias, .{3i}.weight
    backward_towers(model, batch)         what OneStageDetector.backward_towers runs

Tower layer i (0..3) is convolution <tower>.{3i} followed by GroupNorm <tower>.{3i+1}; the forward applies that GroupNorm and the
ReLU while layer i + 1 loads its input (GN_INPUT), so the launch of layer i + 1 describes everything its backward reads: the raw
output of layer i, its statistics and the affine.  No data gradient leaves layer 0: center_tower (whose last map corners_tower.0
reads in the released head), the FPN and the backbone stay frozen.
"""
import ctypes

import torch

from ... import _lib
from .pred_backward import _accumulate
from .tail_backward import F_GNIN, backward_head_tail, complete_towers, tail_parameters

C = 256


def _check_gouts(what, prm, segs, gouts):
    if len(gouts) != int(prm.n_segs):
        raise ValueError("%s: %d gradients for %d segments" % (what, len(gouts), int(prm.n_segs)))
    dev = gouts[0].device
    if dev.type != "cuda":
        raise _lib.DafneHipError("%s: the MI355X engine has no CPU path (got CPU tensors)" % what)
    for s, g in enumerate(gouts):
        if g.dtype != torch.float32 or g.dim() != 4 or g.device != dev or not g.is_contiguous():
            raise ValueError("%s: gradient %d must be a dense fp32 [N, H, W, 256] tensor on %s" % (what, s, dev))
        if tuple(g.shape) != (prm.n_images, segs[s].Hout, segs[s].Wout, C):
            raise ValueError("%s: gradient %d has shape %s" % (what, s, tuple(g.shape)))
    return dev


def tower_wgrad(call, gouts, stream=None):
    """call: the forward launch of a tower convolution (engine.ConvCall, 256 -> 256: its prm / segs describe the input maps, the
    GroupNorm on load included).  gouts: per segment a dense fp32 device tensor [N, H, W, 256], the gradient at the convolution's
    raw output.  -> dW [256, 256, 3, 3] fp32, OIHW as in the state dict; every element written, equal bits from run to run."""
    L = _lib.load()
    prm, segs = call.prm, call.segs
    dev = _check_gouts("tower_wgrad", prm, segs, gouts)
    ptrs = (ctypes.c_void_p * len(gouts))(*[g.data_ptr() for g in gouts])
    with torch.cuda.device(dev):
        nbytes = L.dafne_tower_wgrad_workspace_bytes(ctypes.byref(prm), segs)
        if nbytes == 0:
            # the launch below names the refusal
            nbytes = 16
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dw = torch.empty(C, C, 3, 3, dtype=torch.float32, device=dev)
        _lib.check(L.dafne_tower_wgrad_hip(ctypes.byref(prm), segs, ptrs, _lib.ptr(dw), _lib.ptr(ws), nbytes,
                                           stream if stream is not None else _lib.current_stream()), "dafne_tower_wgrad_hip")
    return dw


def tower_dgrad_gn(call, weight, gouts, stream=None):
    """call: as for tower_wgrad, with GN_INPUT (its prm / segs hold the raw maps of the layer before, their statistics and the
    GroupNorm affine).  weight: the packed bf16 weight that launch multiplied (engine.pack_conv; call.keep[0]).  gouts: as for
    tower_wgrad.  -> (gx: per segment fp32 [N, H, W, 256], dgamma [256], dbeta [256], dbias [256]): the gradients with respect to
    the raw map, the GroupNorm weight / bias and the bias of the convolution that wrote the map.  Every element written, equal bits
    from run to run."""
    L = _lib.load()
    prm, segs = call.prm, call.segs
    dev = _check_gouts("tower_dgrad_gn", prm, segs, gouts)
    if weight.dtype != torch.bfloat16 or weight.device != dev or not weight.is_contiguous() or weight.numel() < C * 2304:
        raise ValueError("tower_dgrad_gn: weight must be the packed bf16 weight of the call on %s (>= %d elements)" % (dev, C * 2304))
    gptrs = (ctypes.c_void_p * len(gouts))(*[g.data_ptr() for g in gouts])
    with torch.cuda.device(dev):
        nbytes = L.dafne_tower_dgrad_gn_workspace_bytes(ctypes.byref(prm), segs)
        if nbytes == 0:
            # the launch below names the refusal
            nbytes = 16
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        gx = [torch.empty_like(g) for g in gouts]
        xptrs = (ctypes.c_void_p * len(gx))(*[t.data_ptr() for t in gx])
        dgamma, dbeta, dbias = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(3))
        _lib.check(L.dafne_tower_dgrad_gn_hip(ctypes.byref(prm), segs, _lib.ptr(weight), gptrs, xptrs, _lib.ptr(dgamma), _lib.ptr(dbeta),
                                              _lib.ptr(dbias), _lib.ptr(ws), nbytes,
                                              stream if stream is not None else _lib.current_stream()), "dafne_tower_dgrad_gn_hip")
    return gx, dgamma, dbeta, dbias


def tower_parameters(model):
    """tail_parameters(model), then for every complete tower (cls_tower, corners_tower): <tower>.9.weight, and for i = 2, 1, 0
    <tower>.{3i+1}.weight, <tower>.{3i+1}.bias, <tower>.{3i}.bias, <tower>.{3i}.weight -- the order backward_towers reaches them in.
    13 tensors per tower: 19 + 26 = 45 for the released head."""
    head = model.proposal_generator.dafne_head
    out = tail_parameters(model)
    for name in complete_towers(model):
        tower = getattr(head, name)
        out.append(tower[9].weight)
        for i in (2, 1, 0):
            out += [tower[3 * i + 1].weight, tower[3 * i + 1].bias, tower[3 * i].bias, tower[3 * i].weight]
    return out


def backward_towers(model, batch):
    """OneStageDetector.backward_towers: backward_head_tail on the plan slot "towers" (the same launches: the same bits for the
    losses and every gradient of tail_parameters), then per complete tower, for layer i = 3 down to 0, tower_wgrad on the layer's
    gradient and, if i > 0, tower_dgrad_gn for the gradient at the raw output of layer i - 1, with that GroupNorm's affine
    gradient and that convolution's bias gradient.  Accumulates into .grad of tower_parameters(model) and returns the loss dict.
    Keeps model._last_towers = {"plan", "g": {(tower, i): the per-level gradients at the raw output of layer i}} (tests)."""
    towers = complete_towers(model)          # (refuses the iterative head; fp8 and more than one rank: backward_head_tail)

    def check(plan):
        hp = plan.head
        for name in towers:
            for i in range(4):
                call = hp.tower_calls.get((name, i))
                if call is None:
                    raise RuntimeError("backward_towers: the plan does not record %s layer %d" % (name, i))
                if call.fp8 is not None:
                    raise NotImplementedError("backward_towers needs bf16 compute weights (%s.%d runs on fp8 weights)" % (name, 3 * i))
                if i > 0 and not (int(call.prm.flags) & F_GNIN):
                    raise NotImplementedError("backward_towers needs tower layers that normalise on load: with the engine switch fuse_gn "
                                              "(DAFNE_FUSE_GN) off the raw output of %s.%d no longer exists" % (name, 3 * (i - 1)))

    losses = backward_head_tail(model, batch, _slot="towers", _towers=check)
    last = model._last_head_tail
    plan = last["plan"]
    head = model.proposal_generator.dafne_head
    record = {}
    for name in towers:
        tower = getattr(head, name)
        g = last["gx"][name]
        for i in (3, 2, 1, 0):
            call = plan.head.tower_calls[(name, i)]
            record[(name, i)] = g
            _accumulate(tower[3 * i].weight, tower_wgrad(call, g))
            if i > 0:
                g, dgamma, dbeta, dbias = tower_dgrad_gn(call, call.keep[0], g)
                _accumulate(tower[3 * i - 2].weight, dgamma)
                _accumulate(tower[3 * i - 2].bias, dbeta)
                _accumulate(tower[3 * i - 3].bias, dbias)
    model._last_towers = {"plan": plan, "g": record}
    return losses
