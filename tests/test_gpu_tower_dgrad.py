"""GPU: dafne_tower_dgrad_gn_hip (csrc/conv_tower_dgrad.hip) -- the data gradient of a 256 -> 256 tower convolution carried back
through the ReLU and the GroupNorm before it -- alone, against the fp64 restatement of tests/_tower_backward_np.py, with the ReLU
mask taken from the map dafne_groupnorm_relu_nhwc_bf16_hip writes on the device.

Bounds, every element (derived in tests/_tower_backward_np.py, not measured; u = 2^-24):
    |err gx| <= C rstd (A |gamma| [mask] + S1 / m + |xhat| S2 / m),        C = 2^-16 + (4608 + 46) u
    |err dgamma, dbeta, dbias| <= (C + (lane_px + 4) u) sum of the magnitudes
The largest err / bound of every case is printed (profiles/NOTES_tower_backward.md records it).
"""
import ctypes

import numpy as np
import pytest
import torch

import _tower_backward_np as R
import _tower_cases as T

pytestmark = pytest.mark.gpu
C = T.C


def check_against(ref, got, lane_px, what):
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
    one("dgamma", dgamma, ref["dgamma"], R.bound_sum(ref["dgamma_abs"], lane_px))
    one("dbeta", dbeta, ref["dbeta"], R.bound_sum(ref["dbeta_abs"], lane_px))
    one("dbias", dbias, ref["dbias"], R.bound_sum(ref["dbias_abs"], lane_px))
    return worst


def run(c, n):
    from dafne_amd.modeling.dafne.tower_backward import tower_dgrad_gn
    got = tower_dgrad_gn(T.make_call(c["raws"], n, gn_in=c["gn_in"]), T.packed(c["W"]), c["gdev"])
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", [k for k in T.LEVEL_SETS if k != "many"])
@pytest.mark.parametrize("n", [1, 2])
def test_against_fp64(n, name):
    c = T.case(n, name)
    ref = T.dgrad_reference(n, name, "")
    assert any(float(np.abs(g).max()) > 0 for g in ref["gx"])
    worst = check_against(ref, run(c, n), R.lane_pixels(c["shapes"], n, T.cus()), "%s n=%d" % (name, n))
    print("tower_dgrad_gn n=%d %s: largest err / bound %.4f" % (n, name, worst))


def test_large_positive_beta():
    """beta = +5 everywhere: nearly every a > 0; a ring of g treated as relu(beta)-like non-zero values would show at the borders."""
    n = 2
    c = T.case(n, "pyramid", tag="beta+5", beta_shift=5.0)
    assert all(m.mean() > 0.95 for m in c["masks"])
    worst = check_against(T.dgrad_reference(n, "pyramid", "beta+5"), run(c, n), R.lane_pixels(c["shapes"], n, T.cus()), "beta + 5")
    print("tower_dgrad_gn large beta: largest err / bound %.4f" % worst)


def test_workgroups_that_walk_several_tiles():
    """530 tiles, more than the launch has workgroups (one per CU): a workgroup accumulates dgamma / dbeta over its second tile, across
    an image or level change with fresh statistics, and restages its LDS ring and weight buffers behind the first tile's reads."""
    from dafne_amd import _lib
    n = 2
    c = T.case(n, "many")
    shapes = T.LEVEL_SETS["many"]
    tiles = R.n_tiles(shapes, n)
    pixels = sum(n * h * w for h, w in shapes)
    call = T.make_call(c["raws"], n, gn_in=c["gn_in"])
    nbytes = _lib.load().dafne_tower_dgrad_gn_workspace_bytes(ctypes.byref(call.prm), call.segs)
    # the workspace: the transposed weight, 512 floats per pass-1 workgroup, 64 per tile, 64 per (level, image), 256 per pass-2 workgroup
    g2 = min((pixels + 3) // 4, 8 * T.cus())
    groups, rest = divmod((nbytes - 1179648) // 4 - 64 * tiles - 64 * len(shapes) * n - 256 * g2, 512)
    assert rest == 0 and 0 < groups < tiles, "every workgroup has one tile on this device (%d workgroups, %d tiles)" % (groups, tiles)
    a, b = run(c, n), run(c, n)
    for x, y in zip(a[0] + list(a[1:]), b[0] + list(b[1:])):
        assert torch.equal(x, y), "two runs differ"
    worst = check_against(T.dgrad_reference(n, "many", ""), a, R.lane_pixels(shapes, n, T.cus()), "many")
    print("tower_dgrad_gn many (%d workgroups, %d tiles): largest err / bound %.4f" % (groups, tiles, worst))


def test_zero_gradient_gives_zero():
    from dafne_amd.modeling.dafne.tower_backward import tower_dgrad_gn
    n = 2
    c = T.case(n, "pyramid")
    gx, dgamma, dbeta, dbias = tower_dgrad_gn(T.make_call(c["raws"], n, gn_in=c["gn_in"]), T.packed(c["W"]),
                                              [torch.zeros_like(g) for g in c["gdev"]])
    torch.cuda.synchronize()
    for t in gx + [dgamma, dbeta, dbias]:
        assert bool((t == 0).all())


def test_one_hot_gradient_counts_the_taps_inside_the_image():
    """All weights 1, gamma 1, beta large (every a > 0), g = 1 at one (level, image, y, x, co): ga is 1 at the in-image neighbours
    of the pixel, so dbeta[c] is their number, exactly: 4 at a corner, 6 on an edge, 9 inside."""
    from dafne_amd.modeling.dafne.tower_backward import tower_dgrad_gn
    n = 2
    c = T.case(n, "pyramid")
    gn_in = (c["gn_in"][0], torch.ones(C, device=T.dev()), torch.full((C,), 100.0, device=T.dev()))
    wp = T.packed(torch.ones(C, C, 3, 3))
    spots = [(0, 0, 0, 0, 0, 4), (0, 1, 11, 19, 255, 4), (0, 1, 5, 7, 64, 9), (0, 0, 0, 7, 130, 6), (2, 1, 1, 2, 63, 9), (4, 1, 0, 1, 200, 2)]
    for lv, im, y, x, co, want in spots:                                     # level, image, y, x, co, taps
        gs = [torch.zeros(n, h, w, C, dtype=torch.float32, device=T.dev()) for h, w in T.PYRAMID]
        gs[lv][im, y, x, co] = 1.0
        _, _, dbeta, _ = tower_dgrad_gn(T.make_call(c["raws"], n, gn_in=gn_in), wp, gs)
        torch.cuda.synchronize()
        assert bool((dbeta == float(want)).all()), (lv, im, y, x, co, want, dbeta[:4].tolist())


def raw_call(call, weight, gouts, gx, dgamma, dbeta, dbias, ws, ws_bytes):
    """The library call itself -> its return code."""
    from dafne_amd import _lib
    L = _lib.load()

    def table(ts):
        return None if ts is None else (ctypes.c_void_p * max(1, len(ts)))(*[None if t is None else t.data_ptr() for t in ts])
    rc = L.dafne_tower_dgrad_gn_hip(ctypes.byref(call.prm), call.segs, _lib.ptr(weight), table(gouts), table(gx), _lib.ptr(dgamma),
                                    _lib.ptr(dbeta), _lib.ptr(dbias), _lib.ptr(ws), ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def test_runs_are_identical_and_every_element_is_written():
    """Two runs give equal bits; outputs and workspace pre-filled with NaN come back finite."""
    from dafne_amd import _lib
    n = 2
    c = T.case(n, "pyramid")
    wp = T.packed(c["W"])
    res = []
    for _ in range(2):
        call = T.make_call(c["raws"], n, gn_in=c["gn_in"])
        nbytes = _lib.load().dafne_tower_dgrad_gn_workspace_bytes(ctypes.byref(call.prm), call.segs)
        assert nbytes > 0
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=T.dev())
        gx = [torch.full((n, h, w, C), float("nan"), dtype=torch.float32, device=T.dev()) for h, w in T.PYRAMID]
        vec = [torch.full((C,), float("nan"), dtype=torch.float32, device=T.dev()) for _ in range(3)]
        _lib.check(raw_call(call, wp, c["gdev"], gx, vec[0], vec[1], vec[2], ws, nbytes), "dafne_tower_dgrad_gn_hip")
        for t in gx + vec:
            assert bool(torch.isfinite(t).all())
        res.append([t.cpu() for t in gx + vec])
    for a, b in zip(*res):
        assert torch.equal(a, b), "two runs differ"


def test_refusals_leave_the_outputs_untouched():
    from dafne_amd import _lib
    L = _lib.load()
    n = 1
    m = T.haloed(torch.zeros(n, 2, 3, C))
    gn_in = (torch.zeros(1, n, 32, 2, device=T.dev()), torch.ones(C, device=T.dev()), torch.zeros(C, device=T.dev()))
    g = torch.zeros(n, 2, 3, C, dtype=torch.float32, device=T.dev())
    wp = T.packed(torch.zeros(C, C, 3, 3))
    gx = torch.full((n, 2, 3, C), 7.0, dtype=torch.float32, device=T.dev())
    dg, db, dc = (torch.full((C,), 7.0, dtype=torch.float32, device=T.dev()) for _ in range(3))
    INVALID, WORKSPACE, UNSUPPORTED = 1, 2, 4

    def edited(gn=gn_in, **kw):
        c = T.make_call([m], n, gn_in=gn)
        for k, v in kw.items():
            setattr(c.prm, k, v)
        return c
    ws = torch.empty(4 << 20, dtype=torch.uint8, device=T.dev())
    assert 0 < L.dafne_tower_dgrad_gn_workspace_bytes(ctypes.byref(edited().prm), edited().segs) <= ws.numel()
    full = dict(weight=wp, gouts=[g], gx=[gx], dgamma=dg, dbeta=db, dbias=dc, ws=ws, ws_bytes=ws.numel())
    cases = [
        ("Cin", edited(Cin=128), {}, UNSUPPORTED),
        ("Cout 16", edited(Cout=16), {}, UNSUPPORTED),
        ("1x1", edited(KH=1, KW=1, pad=0), {}, UNSUPPORTED),
        ("stride 2", edited(stride=2), {}, UNSUPPORTED),
        ("pad 0", edited(pad=0), {}, UNSUPPORTED),
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
        ("GN input without statistics", edited(gn=None, flags=T.F_GN | T.F_GNIN), {}, INVALID),
        ("fp32 output flag", edited(flags=T.F_GNIN | 8), {}, INVALID),
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
    assert L.dafne_tower_dgrad_gn_workspace_bytes(ctypes.byref(big.prm), big.segs) == 0
    assert L.dafne_tower_dgrad_gn_workspace_bytes(ctypes.byref(edited(gn=None).prm), edited(gn=None).segs) == 0
    wide = edited()
    wide.segs[0].Hin = wide.segs[0].Hout = 1025
    wide.segs[0].Win = wide.segs[0].Wout = 1024
    assert raw_call(wide, **full) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (gx, dg, db, dc):
        assert bool((t == 7.0).all())
    # ... and the accepted call on the same buffers writes all of them
    _lib.check(raw_call(edited(), **full), "dafne_tower_dgrad_gn_hip")
    for t in (gx, dg, db, dc):
        assert bool((t == 0.0).all())
