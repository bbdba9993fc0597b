"""GPU: dafne_pred_wgrad_hip (csrc/conv_pred_wgrad.hip) -- the weight / bias gradient of the head's prediction convolutions --
against the fp64 restatement of tests/_pred_backward_np.py.

Bound, every element: |err| <= (2^-16 + n 2^-24) sum |g x|, n = the number of summed pixels.  It follows from the arithmetic and
is not a measured number: g enters as a hi + lo bf16 pair (|g - hi - lo| <= 2^-16 |g|), the products with the bf16 map are exact in
the fp32 accumulator, n fp32 additions round 2^-24 each, the partials are added in fp64 and rounded to fp32 once (2^-24).
The largest err / bound this file observed is printed by every case (profiles/NOTES_pred_backward.md records it).
"""
import ctypes
import types

import numpy as np
import pytest
import torch

import _pred_backward_np as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C = 256
F_F32, F_GNIN = 8, 32

PYRAMID = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
# "many": 2 x (33 x 5) + 2 x 2 = 334 tiles at N = 2, more than the 256 workgroups of a launch: workgroups walk a second tile
LEVEL_SETS = {"1x1": [(1, 1)], "2x3": [(2, 3)], "tile+1": [(5, 33)], "pyramid": PYRAMID, "many": [(132, 132), (7, 9)]}
COUTS = (1, 2, 9, 15, 16)


def dev():
    return torch.device("cuda", 0)


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


def raw_call(call, gouts, ps, dw, db, ws=None, ws_bytes=None):
    """The library call itself -> its return code (the refusal tests look at it)."""
    from dafne_amd import _lib
    L = _lib.load()
    ptrs = (ctypes.c_void_p * max(1, len(gouts)))(*[None if g is None else g.data_ptr() for g in gouts]) if gouts is not None else None
    if ws is None:
        nbytes = L.dafne_pred_wgrad_workspace_bytes(ctypes.byref(call.prm), call.segs) or 1 << 20
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
        ws_bytes = nbytes if ws_bytes is None else ws_bytes
    rc = L.dafne_pred_wgrad_hip(ctypes.byref(call.prm), call.segs, ptrs, ps, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), ws_bytes,
                                _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def gn_maps(raws, n, seed):
    """Raw tower maps -> (statistics, gamma, beta, the maps dafne_groupnorm_relu_nhwc_bf16_hip writes from them).  The partial
    sums (one tile per image) are formed on the host; the kernel finalises mean / rstd and applies them in place on a copy."""
    from dafne_amd import _lib
    L = _lib.load()
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev())
    beta = (torch.randn(C, generator=g) * 0.3).to(dev())
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
    return (stats, gamma, beta), applied


def strided(g, cout, ps):
    """g [N,H,W,16] fp32 -> a device view [N,H,W,cout] with pixel stride ps, the gap filled with NaN."""
    n, h, w, _ = g.shape
    buf = torch.full((n, h, w, ps), float("nan"), dtype=torch.float32, device=dev())
    buf[..., :cout] = g[..., :cout].to(dev())
    return buf[..., :cout]


_CASES = {}


def case(n, name, gn):
    """Maps, gradients (16 channels: a Cout-channel call reads the leading ones) and the fp64 reference, made once."""
    key = (n, name, gn)
    if key not in _CASES:
        rng = np.random.default_rng(100 * n + 7 * len(name) + int(gn))
        shapes = LEVEL_SETS[name]
        raws = [haloed(torch.from_numpy(rng.normal(0.3, 1.0, (n, h, w, C)).astype(np.float32))) for h, w in shapes]
        gn_in, maps = (None, raws)
        if gn:
            gn_in, maps = gn_maps(raws, n, seed=n)
        # focal-loss-like gradients: many orders of magnitude, both signs
        gs = [(rng.normal(0, 1, (n, h, w, 16)) * np.exp(rng.uniform(-14, 2, (n, h, w, 16)))).astype(np.float32) for h, w in shapes]
        Xs = [m[:, 1:-1, 1:-1].float().cpu().numpy().astype(np.float64) for m in maps]
        ref = R.wgrad(Xs, gs)
        _CASES[key] = (raws, gn_in, maps, [torch.from_numpy(g) for g in gs], ref)
    return _CASES[key]


@pytest.mark.parametrize("gn", [False, True], ids=["plain", "gn"])
@pytest.mark.parametrize("name", [k for k in LEVEL_SETS if k != "many"])
@pytest.mark.parametrize("n", [1, 2])
def test_against_fp64(n, name, gn):
    from dafne_amd.modeling.dafne.pred_backward import pred_wgrad
    raws, gn_in, maps, gs, (dW, db, aW, ab, npx) = case(n, name, gn)
    worst = 0.0
    for cout in COUTS:
        for ps in (cout, cout + 1):
            call = make_call(raws if gn else maps, n, cout, gn_in=gn_in)
            gv = [strided(g, cout, ps) for g in gs]
            got_w, got_b = pred_wgrad(call, gv, ps)
            torch.cuda.synchronize()
            gw, gb = got_w.cpu().numpy().astype(np.float64), got_b.cpu().numpy().astype(np.float64)
            assert np.isfinite(gw).all() and np.isfinite(gb).all()
            ew, eb = np.abs(gw - dW[:cout]), np.abs(gb - db[:cout])
            bw, bb = R.wgrad_bound(aW[:cout], npx), R.wgrad_bound(ab[:cout], npx)
            with np.errstate(all="ignore"):
                ratio = max(np.nanmax(np.where(bw > 0, ew / bw, 0.0)), np.nanmax(np.where(bb > 0, eb / bb, 0.0)))
            worst = max(worst, float(ratio))
            assert (ew <= bw).all(), "dW: Cout %d ps %d: max err/bound %.3g" % (cout, ps, ratio)
            assert (eb <= bb).all(), "db: Cout %d ps %d: max err/bound %.3g" % (cout, ps, ratio)
    print("pred_wgrad n=%d %s %s: largest err / bound %.4f" % (n, name, "gn" if gn else "plain", worst))


@pytest.mark.parametrize("gn", [False, True], ids=["plain", "gn"])
def test_one_hot_gradient_copies_the_map_exactly(gn):
    """g = 1 at one (n, y, x, co): dW[co, :, kh, kw] is X[n, y+kh-1, x+kw-1, :] exactly, exactly 0 for a tap outside the image
    (GN input: a normalised halo would show up here as relu(beta)), every other row exactly 0."""
    from dafne_amd.modeling.dafne.pred_backward import pred_wgrad
    n, name, cout = 2, "pyramid", 9
    raws, gn_in, maps, _, _ = case(n, name, gn)
    shapes = LEVEL_SETS[name]
    spots = [(0, 0, 0, 0, 0), (0, 1, 0, 19, 3), (0, 0, 11, 0, 8), (0, 1, 11, 19, 1), (0, 1, 5, 7, 4),      # level, image, y, x, co
             (2, 0, 2, 4, 2), (4, 1, 0, 1, 5), (1, 1, 3, 9, 7)]
    for lv, im, y, x, co in spots:
        gs = [torch.zeros(n, h, w, cout, dtype=torch.float32, device=dev()) for h, w in shapes]
        gs[lv][im, y, x, co] = 1.0
        call = make_call(raws if gn else maps, n, cout, gn_in=gn_in)
        dw, db = pred_wgrad(call, gs)
        torch.cuda.synchronize()
        dw, db = dw.cpu(), db.cpu()
        X = maps[lv][im].float().cpu()                          # haloed: tap (kh, kw) of pixel (y, x) is X[y + kh, x + kw]
        want = torch.zeros(cout, C, 3, 3)
        for kh in range(3):
            for kw in range(3):
                want[co, :, kh, kw] = X[y + kh, x + kw]
        assert torch.equal(dw, want), (lv, im, y, x, co, (dw - want).abs().max())
        wb = torch.zeros(cout)
        wb[co] = 1.0
        assert torch.equal(db, wb)
        h, w = shapes[lv]
        for kh in range(3):
            for kw in range(3):
                if not (0 <= y + kh - 1 < h and 0 <= x + kw - 1 < w):
                    assert float(dw[co, :, kh, kw].abs().max()) == 0.0


@pytest.mark.parametrize("gn", [False, True], ids=["plain", "gn"])
def test_workgroups_that_walk_several_tiles(gn):
    """More tiles (334) than a launch has workgroups (one per CU): a workgroup accumulates over its second tile, across an image
    or level change with fresh statistics, and rewrites its LDS patch behind the first tile's reads.  Against the fp64 restatement
    under the same bound, two runs with equal bits, and one-hot gradients in tiles 329 (the last of level 0) and 333 (the last of
    level 1), which are a workgroup's second tile whenever the device has fewer than 329 CUs."""
    import ctypes
    from dafne_amd import _lib
    from dafne_amd.modeling.dafne.pred_backward import pred_wgrad
    n = 2
    raws, gn_in, maps, gs, (dW, db, aW, ab, npx) = case(n, "many", gn)
    call16 = make_call(raws if gn else maps, n, 16, gn_in=gn_in)
    nbytes = _lib.load().dafne_pred_wgrad_workspace_bytes(ctypes.byref(call16.prm), call16.segs)
    groups = nbytes // ((16 * 2304 + 16) * 4)
    assert 0 < groups < 334, "every workgroup has one tile on this device (%d workgroups): the case does not walk" % groups
    for cout in (16, 9):
        call = make_call(raws if gn else maps, n, cout, gn_in=gn_in)
        gv = [strided(g, cout, cout) for g in gs]
        res = []
        for _ in range(2):
            got_w, got_b = pred_wgrad(call, gv, cout)
            torch.cuda.synchronize()
            res.append((got_w.cpu(), got_b.cpu()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "two runs differ"
        gw, gb = res[0][0].numpy().astype(np.float64), res[0][1].numpy().astype(np.float64)
        ew, eb = np.abs(gw - dW[:cout]), np.abs(gb - db[:cout])
        bw, bb = R.wgrad_bound(aW[:cout], npx), R.wgrad_bound(ab[:cout], npx)
        assert (ew <= bw).all() and (eb <= bb).all(), (cout, float((ew / np.maximum(bw, 1e-300)).max()))
        print("pred_wgrad many %s Cout %d (%d workgroups): largest err / bound %.4f"
              % ("gn" if gn else "plain", cout, groups, float((ew / np.maximum(bw, 1e-300)).max())))
    shapes = LEVEL_SETS["many"]
    cout = 9
    for lv, im, y, x, co in [(0, 1, 131, 131, 4), (1, 1, 6, 8, 8), (0, 1, 64, 40, 0)]:
        g1 = [torch.zeros(n, h, w, cout, dtype=torch.float32, device=dev()) for h, w in shapes]
        g1[lv][im, y, x, co] = 1.0
        dw, _ = pred_wgrad(make_call(raws if gn else maps, n, cout, gn_in=gn_in), g1)
        torch.cuda.synchronize()
        X = maps[lv][im].float().cpu()
        want = torch.zeros(cout, C, 3, 3)
        for kh in range(3):
            for kw in range(3):
                want[co, :, kh, kw] = X[y + kh, x + kw]
        assert torch.equal(dw.cpu(), want), (lv, im, y, x, co)


def test_gn_on_load_equals_the_applied_map_and_runs_are_identical():
    """GroupNorm on load == the plain call on the map dafne_groupnorm_relu_nhwc_bf16_hip writes from the same raw map and
    statistics, bit for bit; two runs give equal bits; outputs pre-filled with NaN come back finite."""
    from dafne_amd import _lib
    n, cout = 2, 16
    raws, gn_in, maps, gs, _ = case(n, "pyramid", True)
    gv = [g.to(dev()).contiguous() for g in gs]
    res = []
    for call in (make_call(raws, n, cout, gn_in=gn_in), make_call(maps, n, cout), make_call(raws, n, cout, gn_in=gn_in)):
        dw = torch.full((cout, C, 3, 3), float("nan"), dtype=torch.float32, device=dev())
        db = torch.full((cout,), float("nan"), dtype=torch.float32, device=dev())
        rc = raw_call(call, gv, 16, dw, db)
        _lib.check(rc, "dafne_pred_wgrad_hip")
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        res.append((dw.cpu(), db.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), "GN on load differs from the applied map"
    assert torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[2][1]), "two runs differ"


def test_refusals_leave_the_outputs_untouched():
    from dafne_amd import _lib
    n, cout = 1, 9
    m = haloed(torch.zeros(n, 2, 3, C))
    g = torch.zeros(n, 2, 3, cout, dtype=torch.float32, device=dev())
    dw = torch.full((cout, C, 3, 3), 7.0, dtype=torch.float32, device=dev())
    db = torch.full((cout,), 7.0, dtype=torch.float32, device=dev())
    INVALID, WORKSPACE, UNSUPPORTED = 1, 2, 4

    def edited(**kw):
        c = make_call([m], n, cout)
        for k, v in kw.items():
            setattr(c.prm, k, v)
        return c
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    cases = [
        ("Cin", edited(Cin=128), [g], cout, dw, db, UNSUPPORTED),
        ("Cout 0", edited(Cout=0), [g], cout, dw, db, UNSUPPORTED),
        ("Cout 17", edited(Cout=17), [g], 17, dw, db, UNSUPPORTED),
        ("1x1", edited(KH=1, KW=1, pad=0), [g], cout, dw, db, UNSUPPORTED),
        ("stride 2", edited(stride=2), [g], cout, dw, db, UNSUPPORTED),
        ("pad 0", edited(pad=0), [g], cout, dw, db, UNSUPPORTED),
        ("ps < Cout", edited(), [g], cout - 1, dw, db, INVALID),
        ("null gradient", edited(), [None], cout, dw, db, INVALID),
        ("null gradient table", edited(), None, cout, dw, db, INVALID),
        ("null dW", edited(), [g], cout, None, db, INVALID),
        ("null db", edited(), [g], cout, dw, None, INVALID),
        ("six segments", edited(n_segs=6), [g] * 6, cout, dw, db, INVALID),
        ("no segments", edited(n_segs=0), [g], cout, dw, db, INVALID),
        ("GN input without statistics", edited(flags=F_F32 | F_GNIN), [g], cout, dw, db, INVALID),
        ("unknown flag", edited(flags=F_F32 | 1), [g], cout, dw, db, INVALID),
    ]
    for what, call, gouts, ps, a, b, want in cases:
        rc = raw_call(call, gouts, ps, a, b, ws=ws, ws_bytes=ws.numel())
        assert rc == want, (what, rc, _lib.load().dafne_last_error())
        assert _lib.load().dafne_last_error(), what
    # null input map, null workspace, small workspace
    c = make_call([m], n, cout)
    c.segs[0].d_in = None
    assert raw_call(c, [g], cout, dw, db, ws=ws, ws_bytes=ws.numel()) == INVALID
    L = _lib.load()
    c = make_call([m], n, cout)
    ptrs = (ctypes.c_void_p * 1)(g.data_ptr())
    assert L.dafne_pred_wgrad_hip(ctypes.byref(c.prm), c.segs, ptrs, cout, _lib.ptr(dw), _lib.ptr(db), None, 1 << 20,
                                  _lib.current_stream()) == INVALID
    assert L.dafne_pred_wgrad_hip(ctypes.byref(c.prm), c.segs, ptrs, cout, _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), 16,
                                  _lib.current_stream()) == WORKSPACE
    # the forward call's 32-bit offset limit: 2^32 bytes of haloed input (nothing is launched, the map is never read)
    big = make_call([m], n, cout)
    big.prm.n_images = 8
    big.segs[0].Hin = big.segs[0].Hout = 1022
    big.segs[0].Win = big.segs[0].Wout = 1022
    assert raw_call(big, [g], cout, dw, db, ws=ws, ws_bytes=ws.numel()) == UNSUPPORTED
    assert L.dafne_pred_wgrad_workspace_bytes(ctypes.byref(big.prm), big.segs) == 0
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((db == 7.0).all())
