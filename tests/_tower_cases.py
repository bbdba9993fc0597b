"""Shared inputs of tests/test_gpu_tower_wgrad.py and tests/test_gpu_tower_dgrad.py: raw 256-channel tower maps with their
GroupNorm statistics (finalised and applied by dafne_groupnorm_relu_nhwc_bf16_hip on the device), gradients over many orders of
magnitude, bf16-representable 256 -> 256 weights, and the forward tower call's description of its input.  Every case is made once."""
import ctypes
import types

import numpy as np
import torch

import _tower_backward_np as R

BF = torch.bfloat16
C = 256
F_GN, F_GNIN, F_GNFIN, F_EXCL = 16, 32, 64, 128
TH, TW = R.TH, R.TW

PYRAMID = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
# "many": 2 x 261 + 2 x 4 = 530 tiles at N = 2 on 2 x 1041 + 2 x 165 = 2412 pixels: more tiles than the data-gradient launch has
# workgroups (one per CU) or the weight-gradient launch pixel splits (CUs / 16): workgroups walk several tiles
LEVEL_SETS = {"1x1": [(1, 1)], "2x3": [(2, 3)], "tile+1": [(TH + 1, TW + 1)], "pyramid": PYRAMID, "many": [(1041, 1), (5, 33)]}


def dev():
    return torch.device("cuda", 0)


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def haloed(x):
    """[N,H,W,C] fp32 -> the engine's haloed bf16 map [N,H+2,W+2,C] on the device."""
    n, h, w, c = x.shape
    t = torch.zeros(n, h + 2, w + 2, c, dtype=BF, device=dev())
    t[:, 1:-1, 1:-1] = x.to(dev()).to(BF)
    return t


def gn_maps(raws, n, gamma, beta):
    """Raw tower maps -> (statistics on the device, the maps dafne_groupnorm_relu_nhwc_bf16_hip writes from them)."""
    from dafne_amd import _lib
    L = _lib.load()
    part = []
    for m in raws:
        x = m[:, 1:-1, 1:-1].float().reshape(n, -1, C // 8, 8)
        part.append(torch.stack((x.sum((1, 3)), (x * x).sum((1, 3))), -1))          # [n, 32, 2]
    partial = torch.cat(part, 0).contiguous()
    stats = torch.zeros(len(raws), n, C // 8, 2, dtype=torch.float32, device=dev())
    applied = [m.clone() for m in raws]
    gsegs = (_lib.GnSeg * len(raws))()
    for k, m in enumerate(applied):
        gsegs[k] = _lib.GnSeg(m.data_ptr(), m.shape[1] - 2, m.shape[2] - 2, k * n, 1)
    _lib.check(L.dafne_groupnorm_relu_nhwc_bf16_hip(gsegs, len(raws), n, C, _lib.ptr(partial), _lib.ptr(stats), _lib.ptr(gamma),
                                                    _lib.ptr(beta), ctypes.c_float(1e-5), _lib.current_stream()))
    torch.cuda.synchronize()
    return stats, applied


def make_call(maps, n, gn_in=None, flags=F_GN | F_GNFIN | F_EXCL):
    """The forward tower call's description of its input: dafne_conv_params + dafne_conv_seg[] (engine.ConvCall's fields)."""
    from dafne_amd import _lib
    gi = [t.data_ptr() for t in gn_in] if gn_in is not None else [None, None, None]
    prm = _lib.ConvParams(n, len(maps), C, C, 3, 3, 1, 1, flags | (F_GNIN if gn_in is not None else 0), None, None, None,
                          gi[0], gi[1], gi[2], None, None, 0.0)
    segs = (_lib.ConvSeg * len(maps))()
    for i, m in enumerate(maps):
        h, w = m.shape[1] - 2, m.shape[2] - 2
        segs[i] = _lib.ConvSeg(m.data_ptr(), None, None, h, w, h, w)
    return types.SimpleNamespace(prm=prm, segs=segs, keep=(maps, gn_in), fp8=None)


def packed(W):
    """OIHW fp32 (bf16-representable) -> the packed bf16 weight the forward multiplies (engine.pack_conv)."""
    from dafne_amd import engine
    return engine.pack_conv(W, None, dev())[0]


_CASES = {}


def case(n, name, tag="", beta_shift=0.0):
    """-> dict: raws / applied (haloed device maps), gn_in (stats, gamma, beta on the device), gs (fp32 [n,h,w,256] per level, host),
    gdev (the same on the device), W (OIHW fp32, bf16-representable), and the host copies the restatement reads: xs (raw, un-haloed),
    xa (applied, un-haloed), stats, gamma, beta, masks.  gamma of both signs; beta_shift moves every beta (a large positive one
    makes relu(beta) > 0 where the halo must stay zero)."""
    key = (n, name, tag)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * n + 13 * len(name) + len(tag))
        shapes = LEVEL_SETS[name]
        raws = [haloed(torch.from_numpy(rng.normal(0.3, 1.0, (n, h, w, C)).astype(np.float32))) for h, w in shapes]
        g = torch.Generator().manual_seed(n + 17)
        gamma = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()
        beta = torch.randn(C, generator=g) * 0.3 + beta_shift
        gamma, beta = gamma.to(dev()).contiguous(), beta.to(dev()).contiguous()
        stats, applied = gn_maps(raws, n, gamma, beta)
        # focal-loss-like gradients: many orders of magnitude, both signs
        gs = [(rng.normal(0, 1, (n, h, w, C)) * np.exp(rng.uniform(-14, 2, (n, h, w, C)))).astype(np.float32) for h, w in shapes]
        W = torch.from_numpy(rng.normal(0, 0.03, (C, C, 3, 3)).astype(np.float32)).to(BF).float()
        _CASES[key] = dict(
            shapes=shapes, raws=raws, applied=applied, gn_in=(stats, gamma, beta), gs=gs,
            gdev=[torch.from_numpy(x).to(dev()).contiguous() for x in gs], W=W,
            xs=[m[:, 1:-1, 1:-1].float().cpu().numpy() for m in raws], xa=[m[:, 1:-1, 1:-1].float().cpu().numpy() for m in applied],
            stats=[s for s in stats.cpu().numpy()], gamma=gamma.cpu().numpy(), beta=beta.cpu().numpy(),
            masks=[(m[:, 1:-1, 1:-1].float() > 0).cpu().numpy() for m in applied])
    return _CASES[key]


_REFS = {}


def wgrad_reference(n, name, tag, gnin):
    """(dW fp64, sum |g x|, pixels) of a case, computed once: X is the applied map (GN_INPUT) or the stored map itself."""
    key = ("w", n, name, tag, gnin)
    if key not in _REFS:
        c = _CASES[(n, name, tag)]
        dW, _, aW, _, npx = R.wgrad(c["xa"] if gnin else c["xs"], c["gs"])
        _REFS[key] = (dW, aW, npx)
    return _REFS[key]


def dgrad_reference(n, name, tag):
    key = ("d", n, name, tag)
    if key not in _REFS:
        c = _CASES[(n, name, tag)]
        _REFS[key] = R.layer_backward(c["xs"], c["stats"], c["gamma"], c["beta"], c["W"].numpy(), c["gs"], c["masks"])
    return _REFS[key]
