"""Backward of the head's tail (DESIGN row F12): from the loss gradients at the raw outputs of the prediction convolutions back
through those convolutions (data gradient), the ReLU and the last GroupNorm of a tower, to the raw output of the tower's last
convolution (dafne_pred_dgrad_gn_hip, csrc/conv_pred_dgrad.hip).

    pred_dgrad_gn(call, weight, gouts, ps)   one dafne_pred_dgrad_gn_hip call on a forward prediction call's own description
    tail_parameters(model)                   prediction_parameters + <tower>.9.bias, <tower>.10.{weight,bias} of the complete towers
    backward_head_tail(model, batch)         what OneStageDetector.backward_head_tail runs

The tensor it ends at, gx, is what a 256 -> 256 weight- or data-gradient kernel of tower convolution .9 takes as its output
gradient: tower_backward.py (DESIGN row F13) goes on from there; here that convolution's weight and everything before it stay frozen.
"""
import ctypes

import torch

from ... import _lib
from .pred_backward import _accumulate, backward_prediction_layers, prediction_parameters

F_GNIN = 32     # DAFNE_CONV_GN_INPUT

# tower -> the prediction call that reads it.  A tower is COMPLETE when that call is its last layer's only reader
_TOWER_CALL = (("cls_tower", "cls_logits"), ("corners_tower", "corners_ctrness"))


def pred_dgrad_gn(call, weight, gouts, ps=None, stream=None):
    """call: the forward prediction launch (engine.ConvCall; flags F_F32 | F_GNIN: its prm / segs hold the raw tower maps, their
    statistics and the GroupNorm affine).  weight: the packed bf16 weight that launch multiplied (engine.pack_conv).  gouts: as
    for pred_wgrad -- per segment an fp32 device tensor [N, H, W, >= Cout] of pixel stride `ps`.
    -> (gx: per segment fp32 [N, H, W, 256], dgamma [256], dbeta [256], dbias [256]): the gradients with respect to the raw
    tower map, the GroupNorm weight / bias and the bias of the convolution that wrote the map.  Every element written, equal
    bits from run to run."""
    L = _lib.load()
    prm, segs = call.prm, call.segs
    n_segs, cout = int(prm.n_segs), int(prm.Cout)
    if len(gouts) != n_segs:
        raise ValueError("pred_dgrad_gn: %d gradients for %d segments" % (len(gouts), n_segs))
    dev = gouts[0].device
    if dev.type != "cuda":
        raise _lib.DafneHipError("pred_dgrad_gn: the MI355X engine has no CPU path (got CPU tensors)")
    if weight.dtype != torch.bfloat16 or weight.device != dev or not weight.is_contiguous() or weight.numel() < cout * 2304:
        raise ValueError("pred_dgrad_gn: weight must be the packed bf16 weight of the call on %s (>= %d elements)" % (dev, cout * 2304))
    for s, g in enumerate(gouts):
        if g.dtype != torch.float32 or g.dim() != 4 or g.stride(3) != 1:
            raise ValueError("pred_dgrad_gn: gradient %d must be fp32 [N, H, W, C] with contiguous channels" % s)
        p = g.stride(2)
        if ps is None:
            ps = p
        if p != ps or g.stride(1) != ps * g.shape[2] or g.stride(0) != ps * g.shape[2] * g.shape[1]:
            raise ValueError("pred_dgrad_gn: gradient %d is not a dense [N, H, W] grid of pixel stride %d" % (s, ps))
        if (g.shape[0], g.shape[1], g.shape[2]) != (prm.n_images, segs[s].Hout, segs[s].Wout) or g.shape[3] < cout:
            raise ValueError("pred_dgrad_gn: gradient %d has shape %s" % (s, tuple(g.shape)))
    gptrs = (ctypes.c_void_p * n_segs)(*[g.data_ptr() for g in gouts])
    with torch.cuda.device(dev):
        nbytes = L.dafne_pred_dgrad_gn_workspace_bytes(ctypes.byref(prm), segs)
        if nbytes == 0:
            # the launch below names the refusal
            nbytes = 16
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        gx = [torch.empty(g.shape[0], g.shape[1], g.shape[2], 256, dtype=torch.float32, device=dev) for g in gouts]
        xptrs = (ctypes.c_void_p * n_segs)(*[t.data_ptr() for t in gx])
        dgamma, dbeta, dbias = (torch.empty(256, dtype=torch.float32, device=dev) for _ in range(3))
        _lib.check(L.dafne_pred_dgrad_gn_hip(ctypes.byref(prm), segs, _lib.ptr(weight), gptrs, int(ps), xptrs, _lib.ptr(dgamma),
                                             _lib.ptr(dbeta), _lib.ptr(dbias), _lib.ptr(ws), nbytes,
                                             stream if stream is not None else _lib.current_stream()), "dafne_pred_dgrad_gn_hip")
    return gx, dgamma, dbeta, dbias


def complete_towers(model):
    """The towers whose last layer feeds one prediction call and nothing else: cls_tower and corners_tower.  The
    center-to-corner head's center_tower is NOT among them: its last layer also feeds corners_tower.0, so the gradient that
    arrives through center_pred alone is incomplete until the tower backward exists."""
    head = model.proposal_generator.dafne_head
    if head.head_mode[0] == "iterative":
        raise NotImplementedError("the head-tail backward does not cover CORNER_PREDICTION iterative (corner chain)")
    return [name for name, _ in _TOWER_CALL]


def tail_parameters(model):
    """prediction_parameters(model), then for every complete tower (cls_tower, corners_tower) <tower>.9.bias, <tower>.10.weight
    and <tower>.10.bias: what backward_head_tail gives a .grad, in a fixed order, for the optimiser.  center_tower (center-to-
    corner head) is excluded: its last layer also feeds corners_tower.0, so its gradient is incomplete until the tower backward
    exists."""
    head = model.proposal_generator.dafne_head
    out = prediction_parameters(model)
    for name in complete_towers(model):
        tower = getattr(head, name)
        out += [tower[9].bias, tower[10].weight, tower[10].bias]
    return out


def backward_head_tail(model, batch, _slot="train", _towers=None):
    """OneStageDetector.backward_head_tail: backward_prediction_layers (the same launches: the same bits for the losses and the
    prediction layers' gradients), then one pred_dgrad_gn call per complete tower on the loss gradients at the raw logits and at
    the raw corners (+ centerness) outputs; accumulates into .grad of tail_parameters(model) and returns the loss dict.  Keeps
    model._last_head_tail = {"plan", "gx": {tower: per-level list}, "g": {tower: the per-level gradients the call read}} (tests,
    and the next slice of the tower backward).
    _slot / _towers (tower_backward.backward_towers): the plan slot, and a callback _towers(plan) that runs once the plan is known,
    before any .grad is touched, and may refuse it."""
    import torch.distributed as dist
    head = model.proposal_generator.dafne_head
    if head.head_mode[0] == "iterative":
        raise NotImplementedError("backward_head_tail does not cover CORNER_PREDICTION iterative: the corner chain has no backward")
    if model.cfg.ENGINE.WEIGHT_DTYPE == "fp8_e4m3":
        raise NotImplementedError("backward_head_tail needs bf16 compute weights (ENGINE.WEIGHT_DTYPE fp8_e4m3 serves a quantised "
                                  "model; fine-tune the bf16 one)")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("backward_head_tail is single-process: no gradient all-reduce (DDP is out of scope)")
    towers = complete_towers(model)
    record = {}

    def tail(plan, g_logits, g_delta):
        calls = plan.head.pred_calls
        if g_logits is None:
            if _towers is not None:
                _towers(plan)
            for name, key in _TOWER_CALL:
                if not (int(calls[key].prm.flags) & F_GNIN):
                    raise NotImplementedError("backward_head_tail needs prediction calls that normalise on load: with the engine switch "
                                              "fuse_gn_pred (DAFNE_FUSE_GN_PRED) off the raw output of %s.9 no longer exists" % name)
            return
        gx, gout = {}, {}
        for (name, key), g in zip(_TOWER_CALL, (g_logits, g_delta)):
            if name not in towers:
                continue
            call = calls[key]
            gout[name] = g
            gx[name], dgamma, dbeta, dbias = pred_dgrad_gn(call, call.keep[0], g)
            tower = getattr(head, name)
            _accumulate(tower[9].bias, dbias)
            _accumulate(tower[10].weight, dgamma)
            _accumulate(tower[10].bias, dbeta)
        record.update(plan=plan, gx=gx, g=gout)

    losses = backward_prediction_layers(model, batch, _tail=tail, _slot=_slot)
    model._last_head_tail = record
    return losses
