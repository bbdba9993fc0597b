"""GPU: dafne_pred_dgrad_gn_hip (csrc/conv_pred_dgrad.hip) -- the data gradient of the head's prediction convolutions carried back
through the ReLU and the last GroupNorm of a tower -- against the fp64 restatement of tests/_tail_backward_np.py, with the ReLU
mask taken from the map dafne_groupnorm_relu_nhwc_bf16_hip writes on the device.

Bound, every element; it follows from the arithmetic and is not a measured number (u = 2^-24):
  * ga: g enters as a hi + lo bf16 pair (|g - hi - lo| <= 2^-16 |g|), the weights are exact bf16, the products are exact in the fp32
    accumulator, which takes <= 320 of them (ten MFMAs of K = 32): |err ga| <= (2^-16 + 320 u) A, A = sum |g| |W|;
  * after it a pixel's value passes fewer than 64 fp32 roundings: xhat (2), gz gamma (1), the tile's group sums (32 additions in a
    lane, 5 across lanes; the tiles are added in fp64), s / m (1), xhat s2 / m, two subtractions and rstd (5).  So
        |err gx| <= C rstd (A |gamma| [mask] + S1 / m + |xhat| S2 / m),   C = 2^-16 + 384 u,
    S1 = sum_group A |gamma| [mask], S2 = sum_group A |gamma| |xhat| [mask]: the cancellation in gx is bounded on the sum of its three
    terms' magnitudes;
  * dgamma, dbeta, dbias add, per lane, 8 values per tile over at most `tiles` tiles in fp32, then 4 across lanes, then fp64:
        |err| <= (C + (8 tiles + 4) u) sum of the magnitudes  (A |xhat| [mask], A [mask], the gx magnitudes above).
The largest err / bound of every case is printed (profiles/NOTES_head_tail.md records it).
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import _tail_backward_np as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C = 256
F_F32, F_GNIN = 8, 32
TH, TW = 4, 32                                  # the kernel's tile of pixels

PYRAMID = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
# "many": 2 x 261 + 2 x 4 = 530 tiles at N = 2, more than the 2 x 256 workgroups of a launch: workgroups walk a second tile
LEVEL_SETS = {"1x1": [(1, 1)], "2x3": [(2, 3)], "tile+1": [(TH + 1, TW + 1)], "pyramid": PYRAMID, "many": [(1041, 1), (5, 33)]}
COUTS = (1, 2, 9, 15, 16)


def dev():
    return torch.device("cuda", 0)


def n_tiles(shapes, n):
    return sum(n * ((h + TH - 1) // TH) * ((w + TW - 1) // TW) for h, w in shapes)


def haloed(x):
    """[N,H,W,C] fp32 (bf16-representable) -> the engine's haloed bf16 map [N,H+2,W+2,C] on the device."""
    n, h, w, c = x.shape
    t = torch.zeros(n, h + 2, w + 2, c, dtype=BF, device=dev())
    t[:, 1:-1, 1:-1] = x.to(dev()).to(BF)
    return t


def make_call(maps, n, cout, gn_in=None, flags=F_F32):
    """The forward prediction call's description of its input: dafne_conv_params + dafne_conv_seg[] (engine.ConvCall's fields)."""
    from dafne_amd import _lib
    gi = [t.data_ptr() for t in gn_in] if gn_in is not None else [None, None, None]
    prm = _lib.ConvParams(n, len(maps), C, cout, 3, 3, 1, 1, flags | (F_GNIN if gn_in is not None else 0), None, None, None,
                          gi[0], gi[1], gi[2], None, None, 0.0)
    segs = (_lib.ConvSeg * len(maps))()
    for i, m in enumerate(maps):
        h, w = m.shape[1] - 2, m.shape[2] - 2
        segs[i] = _lib.ConvSeg(m.data_ptr(), None, None, h, w, h, w)
    return types.SimpleNamespace(prm=prm, segs=segs, keep=(maps, gn_in))


def gn_maps(raws, n, gamma, beta):
    """Raw tower maps -> (statistics on the device, the maps dafne_groupnorm_relu_nhwc_bf16_hip writes from them).  The partial
    sums (one tile per image) are formed on the host; the kernel finalises mean / rstd and applies them in place on a copy."""
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


def strided(g, cout, ps):
    """g [N,H,W,16] fp32 -> a device view [N,H,W,cout] with pixel stride ps, the gap filled with NaN."""
    n, h, w, _ = g.shape
    buf = torch.full((n, h, w, ps), float("nan"), dtype=torch.float32, device=dev())
    buf[..., :cout] = g[..., :cout].to(dev())
    return buf[..., :cout]


def packed(W):
    """OIHW fp32 (bf16-representable) -> the packed bf16 weight the forward multiplies (engine.pack_conv)."""
    from dafne_amd import engine
    return engine.pack_conv(W, None, dev())[0]


_CASES = {}


def case(n, name, gamma=None, beta=None, tag=""):
    """Raw maps, statistics, affine, the applied maps' masks, gradients (16 channels: a Cout-channel call reads the leading ones)
    and weights (16 rows), made once."""
    key = (n, name, tag)
    if key not in _CASES:
        rng = np.random.default_rng(100 * n + 7 * len(name) + 3)
        shapes = LEVEL_SETS[name]
        raws = [haloed(torch.from_numpy(rng.normal(0.3, 1.0, (n, h, w, C)).astype(np.float32))) for h, w in shapes]
        g = torch.Generator().manual_seed(n)
        gamma = ((torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).float()) if gamma is None else gamma
        beta = torch.randn(C, generator=g) * 0.3 if beta is None else beta
        gamma, beta = gamma.to(dev()).contiguous(), beta.to(dev()).contiguous()
        stats, applied = gn_maps(raws, n, gamma, beta)
        # focal-loss-like gradients: many orders of magnitude, both signs
        gs = [(rng.normal(0, 1, (n, h, w, 16)) * np.exp(rng.uniform(-14, 2, (n, h, w, 16)))).astype(np.float32) for h, w in shapes]
        W = torch.from_numpy(rng.normal(0, 0.05, (16, C, 3, 3)).astype(np.float32)).to(BF).float()
        ref_in = dict(xs=[m[:, 1:-1, 1:-1].float().cpu().numpy() for m in raws], stats=[s for s in stats.cpu().numpy()],
                      gamma=gamma.cpu().numpy(), beta=beta.cpu().numpy(),
                      masks=[(m[:, 1:-1, 1:-1].float() > 0).cpu().numpy() for m in applied])
        _CASES[key] = (raws, (stats, gamma, beta), [torch.from_numpy(x) for x in gs], W, ref_in)
    return _CASES[key]


def reference(ref_in, W, gs, cout):
    return R.tail_backward(ref_in["xs"], ref_in["stats"], ref_in["gamma"], ref_in["beta"], W[:cout].numpy(),
                           [g[..., :cout].numpy() for g in gs], ref_in["masks"])


def check_against(ref, got, tiles, what):
    """-> the largest err / bound; asserts every element."""
    gx, dgamma, dbeta, dbias = got
    worst = 0.0

    def one(name, g, r, b):
        nonlocal worst
        g = g.cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all(), (what, name)
        e = np.abs(g - r)
        with np.errstate(all="ignore"):
            ratio = float(np.nanmax(np.where(b > 0, e / b, 0.0)))
        worst = max(worst, ratio)
        assert (e <= b).all(), "%s %s: max err / bound %.3g, %d elements beyond" % (what, name, ratio, int((e > b).sum()))
    for l, t in enumerate(gx):
        one("gx[%d]" % l, t, ref["gx"][l], R.bound_gx(ref["gx_abs"][l]))
    one("dgamma", dgamma, ref["dgamma"], R.bound_sum(ref["dgamma_abs"], tiles))
    one("dbeta", dbeta, ref["dbeta"], R.bound_sum(ref["dbeta_abs"], tiles))
    one("dbias", dbias, ref["dbias"], R.bound_sum(ref["dbias_abs"], tiles))
    return worst


@pytest.mark.parametrize("name", [k for k in LEVEL_SETS if k != "many"])
@pytest.mark.parametrize("n", [1, 2])
def test_against_fp64(n, name):
    from dafne_amd.modeling.dafne.tail_backward import pred_dgrad_gn
    raws, gn_in, gs, W, ref_in = case(n, name)
    tiles = n_tiles(LEVEL_SETS[name], n)
    worst = 0.0
    for cout in COUTS:
        ref = reference(ref_in, W, gs, cout)
        wp = packed(W[:cout])
        for ps in (cout, cout + 1):
            call = make_call(raws, n, cout, gn_in=gn_in)
            got = pred_dgrad_gn(call, wp, [strided(g, cout, ps) for g in gs], ps)
            torch.cuda.synchronize()
            worst = max(worst, check_against(ref, got, tiles, "Cout %d ps %d" % (cout, ps)))
    print("pred_dgrad_gn n=%d %s: largest err / bound %.4f" % (n, name, worst))


def test_workgroups_that_walk_several_tiles():
    """More tiles (530) than a launch has workgroups (two per CU): a workgroup accumulates dgamma / dbeta / dbias over its second
    tile, across an image or level change with fresh statistics, and restages its LDS ring behind the first tile's reads."""
    from dafne_amd import _lib
    from dafne_amd.modeling.dafne.tail_backward import pred_dgrad_gn
    n = 2
    raws, gn_in, gs, W, ref_in = case(n, "many")
    shapes = LEVEL_SETS["many"]
    tiles = n_tiles(shapes, n)
    call16 = make_call(raws, n, 16, gn_in=gn_in)
    nbytes = _lib.load().dafne_pred_dgrad_gn_workspace_bytes(ctypes.byref(call16.prm), call16.segs)
    # the workspace: 768 floats per workgroup, 64 per tile, 64 per (level, image)
    groups, rest = divmod(nbytes // 4 - 64 * tiles - 64 * len(shapes) * n, 768)
    assert rest == 0 and 0 < groups < tiles, "every workgroup has one tile on this device (%d workgroups, %d tiles): the case does " \
                                             "not walk" % (groups, tiles)
    for cout in (16, 9):
        ref = reference(ref_in, W, gs, cout)
        res = []
        for _ in range(2):
            got = pred_dgrad_gn(make_call(raws, n, cout, gn_in=gn_in), packed(W[:cout]), [strided(g, cout, cout) for g in gs], cout)
            torch.cuda.synchronize()
            res.append(got)
        for a, b in zip(res[0][0] + list(res[0][1:]), res[1][0] + list(res[1][1:])):
            assert torch.equal(a, b), "two runs differ"
        worst = check_against(ref, res[0], tiles, "many Cout %d" % cout)
        print("pred_dgrad_gn many Cout %d (%d workgroups, %d tiles): largest err / bound %.4f" % (cout, groups, tiles, worst))


def test_zero_gradient_gives_zero():
    from dafne_amd.modeling.dafne.tail_backward import pred_dgrad_gn
    n, cout = 2, 9
    raws, gn_in, gs, W, _ = case(n, "pyramid")
    zeros = [torch.zeros(n, h, w, cout, dtype=torch.float32, device=dev()) for h, w in PYRAMID]
    gx, dgamma, dbeta, dbias = pred_dgrad_gn(make_call(raws, n, cout, gn_in=gn_in), packed(W[:cout]), zeros)
    torch.cuda.synchronize()
    for t in gx + [dgamma, dbeta, dbias]:
        assert bool((t == 0).all())


def test_dead_channels_get_no_affine_gradient():
    """beta so negative that the forward's a == 0 everywhere: the mask is empty, dgamma and dbeta of the channel are exactly 0."""
    from dafne_amd.modeling.dafne.tail_backward import pred_dgrad_gn
    n, cout = 2, 16
    dead = torch.zeros(C, dtype=torch.bool)
    dead[[0, 5, 8, 63, 64, 130, 255]] = True
    g = torch.Generator().manual_seed(5)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.where(dead, torch.full((C,), -1000.0), torch.randn(C, generator=g) * 0.3)
    raws, gn_in, gs, W, ref_in = case(n, "pyramid", gamma=gamma, beta=beta, tag="dead")
    assert all(not mk[..., dead.numpy()].any() for mk in ref_in["masks"])
    gx, dgamma, dbeta, dbias = pred_dgrad_gn(make_call(raws, n, cout, gn_in=gn_in), packed(W), [x.to(dev()) for x in gs])
    torch.cuda.synchronize()
    assert bool((dgamma.cpu()[dead] == 0).all()) and bool((dbeta.cpu()[dead] == 0).all())
    assert bool((dgamma.cpu()[~dead] != 0).any()) and bool((dbeta.cpu()[~dead] != 0).all())
    worst = check_against(reference(ref_in, W, gs, cout), (gx, dgamma, dbeta, dbias), n_tiles(PYRAMID, n), "dead channels")
    print("pred_dgrad_gn dead channels: largest err / bound %.4f" % worst)


def test_one_hot_gradient_counts_the_taps_inside_the_image():
    """All weights 1, gamma 1, beta large (every a > 0), g = 1 at one (level, image, y, x, co): ga is 1 at the in-image neighbours
    of the pixel, so dbeta[c] is their number, exactly: 4 at a corner, 6 on an edge, 9 inside."""
    from dafne_amd.modeling.dafne.tail_backward import pred_dgrad_gn
    n, cout = 2, 9
    raws, gn_in, _, _, ref_in = case(n, "pyramid", gamma=torch.ones(C), beta=torch.full((C,), 100.0), tag="ones")
    assert all(mk.all() for mk in ref_in["masks"])
    wp = packed(torch.ones(cout, C, 3, 3))
    spots = [(0, 0, 0, 0, 0, 4), (0, 1, 0, 19, 3, 4), (0, 0, 11, 0, 8, 4), (0, 1, 11, 19, 1, 4), (0, 1, 5, 7, 4, 9),     # level, image, y, x, co, taps
             (0, 0, 0, 7, 2, 6), (0, 1, 6, 19, 5, 6), (2, 0, 2, 4, 2, 4), (2, 1, 1, 2, 6, 9), (4, 1, 0, 1, 5, 2), (1, 1, 3, 9, 7, 6)]
    for lv, im, y, x, co, want in spots:
        gs = [torch.zeros(n, h, w, cout, dtype=torch.float32, device=dev()) for h, w in PYRAMID]
        gs[lv][im, y, x, co] = 1.0
        _, _, dbeta, _ = pred_dgrad_gn(make_call(raws, n, cout, gn_in=gn_in), wp, gs)
        torch.cuda.synchronize()
        assert bool((dbeta == float(want)).all()), (lv, im, y, x, co, want, dbeta[:4].tolist())


def raw_call(call, weight, gouts, ps, gx, dgamma, dbeta, dbias, ws, ws_bytes):
    """The library call itself -> its return code."""
    from dafne_amd import _lib
    L = _lib.load()

    def table(ts):
        return None if ts is None else (ctypes.c_void_p * max(1, len(ts)))(*[None if t is None else t.data_ptr() for t in ts])
    rc = L.dafne_pred_dgrad_gn_hip(ctypes.byref(call.prm), call.segs, _lib.ptr(weight), table(gouts), ps, table(gx), _lib.ptr(dgamma),
                                   _lib.ptr(dbeta), _lib.ptr(dbias), _lib.ptr(ws), ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def test_runs_are_identical_and_every_element_is_written():
    """Two runs give equal bits; outputs pre-filled with NaN come back finite."""
    from dafne_amd import _lib
    n, cout = 2, 16
    raws, gn_in, gs, W, _ = case(n, "pyramid")
    gv = [g.to(dev()).contiguous() for g in gs]
    wp = packed(W)
    res = []
    for _ in range(2):
        call = make_call(raws, n, cout, gn_in=gn_in)
        nbytes = _lib.load().dafne_pred_dgrad_gn_workspace_bytes(ctypes.byref(call.prm), call.segs)
        assert nbytes > 0
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev())
        gx = [torch.full((n, h, w, C), float("nan"), dtype=torch.float32, device=dev()) for h, w in PYRAMID]
        vec = [torch.full((C,), float("nan"), dtype=torch.float32, device=dev()) for _ in range(3)]
        _lib.check(raw_call(call, wp, gv, 16, gx, vec[0], vec[1], vec[2], ws, nbytes), "dafne_pred_dgrad_gn_hip")
        for t in gx + vec:
            assert bool(torch.isfinite(t).all())
        res.append([t.cpu() for t in gx + vec])
    for a, b in zip(*res):
        assert torch.equal(a, b), "two runs differ"


def test_refusals_leave_the_outputs_untouched():
    from dafne_amd import _lib
    L = _lib.load()
    n, cout = 1, 9
    m = haloed(torch.zeros(n, 2, 3, C))
    gn_in = (torch.zeros(1, n, 32, 2, device=dev()), torch.ones(C, device=dev()), torch.zeros(C, device=dev()))
    g = torch.zeros(n, 2, 3, cout, dtype=torch.float32, device=dev())
    wp = packed(torch.zeros(16, C, 3, 3))
    gx = torch.full((n, 2, 3, C), 7.0, dtype=torch.float32, device=dev())
    dg, db, dc = (torch.full((C,), 7.0, dtype=torch.float32, device=dev()) for _ in range(3))
    INVALID, WORKSPACE, UNSUPPORTED = 1, 2, 4

    def edited(gn=gn_in, **kw):
        c = make_call([m], n, cout, gn_in=gn)
        for k, v in kw.items():
            setattr(c.prm, k, v)
        return c
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    full = dict(weight=wp, gouts=[g], ps=cout, gx=[gx], dgamma=dg, dbeta=db, dbias=dc, ws=ws, ws_bytes=ws.numel())
    cases = [
        ("Cin", edited(Cin=128), {}, UNSUPPORTED),
        ("Cout 0", edited(Cout=0), {}, UNSUPPORTED),
        ("Cout 17", edited(Cout=17), dict(ps=17), UNSUPPORTED),
        ("1x1", edited(KH=1, KW=1, pad=0), {}, UNSUPPORTED),
        ("stride 2", edited(stride=2), {}, UNSUPPORTED),
        ("pad 0", edited(pad=0), {}, UNSUPPORTED),
        ("ps < Cout", edited(), dict(ps=cout - 1), INVALID),
        ("null gradient", edited(), dict(gouts=[None]), INVALID),
        ("null gradient table", edited(), dict(gouts=None), INVALID),
        ("null gx", edited(), dict(gx=[None]), INVALID),
        ("null gx table", edited(), dict(gx=None), INVALID),
        ("null weight", edited(), dict(weight=None), INVALID),
        ("null dgamma", edited(), dict(dgamma=None), INVALID),
        ("null dbeta", edited(), dict(dbeta=None), INVALID),
        ("null dbias", edited(), dict(dbias=None), INVALID),
        ("null workspace", edited(), dict(ws=None), INVALID),
        ("small workspace", edited(), dict(ws_bytes=16), WORKSPACE),
        ("six segments", edited(n_segs=6), dict(gouts=[g] * 6, gx=[gx] * 6), INVALID),
        ("no segments", edited(n_segs=0), {}, INVALID),
        ("no GroupNorm on load", edited(gn=None), {}, INVALID),
        ("GN input without statistics", edited(gn=None, flags=F_F32 | F_GNIN), {}, INVALID),
        ("unknown flag", edited(flags=F_F32 | F_GNIN | 1), {}, INVALID),
    ]
    for what, call, kw, want in cases:
        rc = raw_call(call, **dict(full, **kw))
        assert rc == want, (what, rc, L.dafne_last_error())
        assert L.dafne_last_error(), what
    c = edited()
    c.segs[0].d_in = None
    assert raw_call(c, **full) == INVALID
    # the forward call's 32-bit offset limit: 2^32 bytes of haloed input (nothing is launched, the map is never read)
    big = edited()
    big.prm.n_images = 8
    big.segs[0].Hin = big.segs[0].Hout = 1022
    big.segs[0].Win = big.segs[0].Wout = 1022
    assert raw_call(big, **full) == UNSUPPORTED
    assert L.dafne_pred_dgrad_gn_workspace_bytes(ctypes.byref(big.prm), big.segs) == 0
    assert L.dafne_pred_dgrad_gn_workspace_bytes(ctypes.byref(edited(gn=None).prm), edited(gn=None).segs) == 0
    torch.cuda.synchronize()
    for t in (gx, dg, db, dc):
        assert bool((t == 7.0).all())
    # ... and the accepted call on the same buffers writes all of them
    _lib.check(raw_call(edited(), **full), "dafne_pred_dgrad_gn_hip")
    for t in (gx, dg, db, dc):
        assert bool((t == 0.0).all())
