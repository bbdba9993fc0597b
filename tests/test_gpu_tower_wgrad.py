"""GPU: dafne_tower_wgrad_hip (csrc/conv_tower_wgrad.hip) -- the weight gradient of a 256 -> 256 tower convolution -- alone, against
the fp64 restatement of tests/_tower_backward_np.py.  X of the restatement is the map dafne_groupnorm_relu_nhwc_bf16_hip writes on
the device (GN_INPUT) or the stored map itself (plain: cls_tower.0 reads FPN maps).

Bound, every element (derived in tests/_tower_backward_np.py, not measured): |err| <= (2^-16 + n 2^-24) sum |g x| over the n summed
pixels.  The largest err / bound of every case is printed (profiles/NOTES_tower_backward.md records it).
"""
import ctypes

import numpy as np
import pytest
import torch

import _tower_backward_np as R
import _tower_cases as T

pytestmark = pytest.mark.gpu
C = T.C


def check_against(dw, ref, what):
    """-> the largest err / bound; asserts every element."""
    dW, aW, npx = ref
    got = dw.cpu().numpy().astype(np.float64)
    assert got.shape == (C, C, 3, 3) and np.isfinite(got).all(), what
    bound = R.wgrad_bound(aW, npx)
    err = np.abs(got - dW)
    with np.errstate(all="ignore"):
        ratio = float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
    assert (err <= bound).all(), "%s: max err / bound %.3g, %d elements beyond" % (what, ratio, int((err > bound).sum()))
    return ratio


def run(c, n, gnin):
    from dafne_amd.modeling.dafne.tower_backward import tower_wgrad
    call = T.make_call(c["raws"], n, gn_in=c["gn_in"] if gnin else None)
    dw = tower_wgrad(call, c["gdev"])
    torch.cuda.synchronize()
    return dw


@pytest.mark.parametrize("gnin", [True, False], ids=["gn_input", "plain"])
@pytest.mark.parametrize("name", [k for k in T.LEVEL_SETS if k != "many"])
@pytest.mark.parametrize("n", [1, 2])
def test_against_fp64(n, name, gnin):
    c = T.case(n, name)
    worst = check_against(run(c, n, gnin), T.wgrad_reference(n, name, "", gnin), "%s n=%d gnin=%s" % (name, n, gnin))
    print("tower_wgrad n=%d %s %s: largest err / bound %.4f" % (n, name, "GN_INPUT" if gnin else "plain", worst))


def test_large_positive_beta_keeps_the_halo_zero():
    """beta = +5 everywhere: relu(beta) > 0, so a halo normalised like a pixel would add g * relu(beta) to every border tap."""
    n = 2
    c = T.case(n, "pyramid", tag="beta+5", beta_shift=5.0)
    assert all(m.mean() > 0.95 for m in c["masks"])
    worst = check_against(run(c, n, True), T.wgrad_reference(n, "pyramid", "beta+5", True), "beta + 5")
    print("tower_wgrad large beta: largest err / bound %.4f" % worst)


@pytest.mark.parametrize("gnin", [True, False], ids=["gn_input", "plain"])
def test_workgroups_that_walk_several_tiles(gnin):
    """530 tiles, more than the launch has pixel splits: a workgroup accumulates over its second tile, across an image or level
    change with fresh statistics, and restages its LDS patch behind the first tile's reads.  Two runs give equal bits."""
    from dafne_amd import _lib
    n = 2
    c = T.case(n, "many")
    tiles = R.n_tiles(T.LEVEL_SETS["many"], n)
    call = T.make_call(c["raws"], n, gn_in=c["gn_in"])
    nbytes = _lib.load().dafne_tower_wgrad_workspace_bytes(ctypes.byref(call.prm), call.segs)
    splits, rest = divmod(nbytes, C * 2304 * 4)
    assert rest == 0 and 0 < splits < tiles, "every split has one tile on this device (%d splits, %d tiles)" % (splits, tiles)
    a, b = run(c, n, gnin), run(c, n, gnin)
    assert torch.equal(a, b), "two runs differ"
    worst = check_against(a, T.wgrad_reference(n, "many", "", gnin), "many")
    print("tower_wgrad many %s (%d splits, %d tiles): largest err / bound %.4f" % ("GN_INPUT" if gnin else "plain", splits, tiles, worst))


def raw_call(call, gouts, dw, ws, ws_bytes):
    """The library call itself -> its return code."""
    from dafne_amd import _lib
    L = _lib.load()
    table = None if gouts is None else (ctypes.c_void_p * max(1, len(gouts)))(*[None if t is None else t.data_ptr() for t in gouts])
    rc = L.dafne_tower_wgrad_hip(ctypes.byref(call.prm), call.segs, table, _lib.ptr(dw), _lib.ptr(ws), ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc


def test_runs_are_identical_and_every_element_is_written():
    """Outputs and workspace pre-filled with NaN come back finite; two runs give equal bits."""
    from dafne_amd import _lib
    n = 2
    c = T.case(n, "pyramid")
    res = []
    for _ in range(2):
        call = T.make_call(c["raws"], n, gn_in=c["gn_in"])
        nbytes = _lib.load().dafne_tower_wgrad_workspace_bytes(ctypes.byref(call.prm), call.segs)
        assert nbytes > 0
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=T.dev())
        dw = torch.full((C, C, 3, 3), float("nan"), dtype=torch.float32, device=T.dev())
        _lib.check(raw_call(call, c["gdev"], dw, ws, nbytes), "dafne_tower_wgrad_hip")
        assert bool(torch.isfinite(dw).all())
        res.append(dw.cpu())
    assert torch.equal(res[0], res[1]), "two runs differ"


def test_zero_gradient_gives_zero():
    n = 1
    c = T.case(n, "tile+1")
    call = T.make_call(c["raws"], n, gn_in=c["gn_in"])
    from dafne_amd.modeling.dafne.tower_backward import tower_wgrad
    dw = tower_wgrad(call, [torch.zeros_like(g) for g in c["gdev"]])
    torch.cuda.synchronize()
    assert bool((dw == 0).all())


def test_refusals_leave_the_output_untouched():
    from dafne_amd import _lib
    L = _lib.load()
    n = 1
    m = T.haloed(torch.zeros(n, 2, 3, C))
    gn_in = (torch.zeros(1, n, 32, 2, device=T.dev()), torch.ones(C, device=T.dev()), torch.zeros(C, device=T.dev()))
    g = torch.zeros(n, 2, 3, C, dtype=torch.float32, device=T.dev())
    dw = torch.full((C, C, 3, 3), 7.0, dtype=torch.float32, device=T.dev())
    INVALID, WORKSPACE, UNSUPPORTED = 1, 2, 4

    def edited(gn=gn_in, **kw):
        c = T.make_call([m], n, gn_in=gn)
        for k, v in kw.items():
            setattr(c.prm, k, v)
        return c
    ws = torch.empty(L.dafne_tower_wgrad_workspace_bytes(ctypes.byref(edited().prm), edited().segs), dtype=torch.uint8, device=T.dev())
    assert ws.numel() == C * 2304 * 4              # six pixels: one tile, one split
    full = dict(gouts=[g], dw=dw, ws=ws, ws_bytes=ws.numel())
    cases = [
        ("Cin", edited(Cin=128), {}, UNSUPPORTED),
        ("Cout 16", edited(Cout=16), {}, UNSUPPORTED),
        ("Cout 512", edited(Cout=512), {}, UNSUPPORTED),
        ("1x1", edited(KH=1, KW=1, pad=0), {}, UNSUPPORTED),
        ("stride 2", edited(stride=2), {}, UNSUPPORTED),
        ("pad 0", edited(pad=0), {}, UNSUPPORTED),
        ("null gradient", edited(), dict(gouts=[None]), INVALID),
        ("null gradient table", edited(), dict(gouts=None), INVALID),
        ("null dW", edited(), dict(dw=None), INVALID),
        ("null workspace", edited(), dict(ws=None), INVALID),
        ("small workspace", edited(), dict(ws_bytes=16), WORKSPACE),
        ("six segments", edited(n_segs=6), dict(gouts=[g] * 6), INVALID),
        ("no segments", edited(n_segs=0), {}, INVALID),
        ("GN input without statistics", edited(gn=None, flags=T.F_GN | T.F_GNIN), {}, INVALID),
        ("fp32 output flag", edited(flags=T.F_GNIN | 8), {}, INVALID),
        ("ReLU flag", edited(flags=T.F_GNIN | 1), {}, INVALID),
    ]
    for what, call, kw, want in cases:
        rc = raw_call(call, **dict(full, **kw))
        assert rc == want, (what, rc, L.dafne_last_error())
        assert L.dafne_last_error(), what
    c = edited()
    c.segs[0].d_in = None
    assert raw_call(c, **full) == INVALID
    assert L.dafne_tower_wgrad_hip(None, None, None, None, None, 0, None) == INVALID
    # the forward call's 32-bit offset limit: 2^32 bytes of haloed input (nothing is launched, the map is never read)
    big = edited()
    big.prm.n_images = 8
    big.segs[0].Hin = big.segs[0].Hout = 1022
    big.segs[0].Win = big.segs[0].Wout = 1022
    assert raw_call(big, **full) == UNSUPPORTED
    assert L.dafne_tower_wgrad_workspace_bytes(ctypes.byref(big.prm), big.segs) == 0
    # 2^20 pixels per image
    wide = edited()
    wide.segs[0].Hin = wide.segs[0].Hout = 1025
    wide.segs[0].Win = wide.segs[0].Wout = 1024
    assert raw_call(wide, **full) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all())
    # ... and the accepted call on the same buffers writes all of it
    _lib.check(raw_call(edited(), **full), "dafne_tower_wgrad_hip")
    assert bool((dw == 0.0).all())
