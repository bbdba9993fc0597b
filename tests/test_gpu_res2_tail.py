"""GPU: the last res2 block computed only where res3 reads it (conv_blk_narrow_s2.hip), res3.0's two 1x1 layers on the
compact map, ReLU-on-load for P7 (conv_wr, DAFNE_CONV_RELU_INPUT) -- every one BIT FOR BIT against what it replaces, and
the whole model with the two plan switches off against on."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    return torch.device("cuda", 0)


def bfr(x):
    return x.to(BF).float()


def same_bits(a, b):
    """torch.equal on the bit patterns (NaN == NaN when the payloads agree)."""
    if a.dtype == BF:
        a, b = a.view(torch.int16), b.view(torch.int16)
    elif a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel against its sibling
@pytest.mark.parametrize("N,H,W", [(1, 8, 32), (2, 64, 64), (3, 13, 21), (1, 1, 1), (1, 40, 410), (2, 256, 256), (5, 72, 104)])
def test_block_narrow_s2_equals_the_even_pixels_of_the_full_block(N, H, W):
    """dafne_bottleneck_block_narrow_s2_hip against dafne_bottleneck_block_narrow_hip (no head, identity shortcut) on the
    same seeded inputs: the compact map's interior is the even-pixel subsample of the full map, torch.equal; its halo is
    zero; a second launch gives the same bits; the small cases also against torch within the bf16 tolerance of
    test_bottleneck_block_narrow_equals_the_separate_launches.  Odd H / W (Ho = (H+1)/2), ragged 2 x 32 tiles in both
    directions, one tile (1 x 1) up to 16 tiles per workgroup (2 x 128 x 128 output pixels)."""
    from dafne_amd import engine, _lib
    L = _lib.load()
    d = dev()
    g = torch.Generator().manual_seed(7000 + H * W)
    u = bfr(torch.relu(torch.randn(N, 64, H, W, generator=g)))
    w2 = bfr(torch.randn(64, 64, 3, 3, generator=g) / 24.0)
    b2 = torch.randn(64, generator=g) * 0.2
    w3 = bfr(torch.randn(256, 64, 1, 1, generator=g) / 8.0)
    b3 = torch.randn(256, generator=g) * 0.2
    x = bfr(torch.relu(torch.randn(N, 256, H, W, generator=g)))
    st = _lib.current_stream()
    ua, xa = engine.Act.from_nchw(u.to(d)), engine.Act.from_nchw(x.to(d))
    w2p, b2p = engine.pack_conv(w2, b2, d)
    w3p, b3p = engine.pack_conv(w3, b3, d)
    wf = engine.pack_blk_narrow(w2p, w3p, None, None)
    # the full block
    scratch = torch.empty(L.dafne_bottleneck_block_narrow_scratch_bytes(), dtype=torch.uint8, device=d)
    y_full = engine.Act(N, H, W, 256, d)
    _lib.check(L.dafne_bottleneck_block_narrow_hip(_lib.ptr(ua.t), _lib.ptr(xa.t), _lib.ptr(wf), _lib.ptr(b2p), _lib.ptr(b3p), None, None,
                                                   N, H, W, _lib.ptr(y_full.t), None, _lib.ptr(scratch), scratch.numel(), st), "blk_narrow")
    # the stride-2 form
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    scratch2 = torch.empty(L.dafne_bottleneck_block_narrow_s2_scratch_bytes(), dtype=torch.uint8, device=d)
    y_s2 = engine.Act(N, Ho, Wo, 256, d)

    def launch():
        _lib.check(L.dafne_bottleneck_block_narrow_s2_hip(_lib.ptr(ua.t), _lib.ptr(xa.t), _lib.ptr(wf), _lib.ptr(b2p), _lib.ptr(b3p), N, H, W,
                                                          _lib.ptr(y_s2.t), _lib.ptr(scratch2), scratch2.numel(), st), "blk_narrow_s2")
        torch.cuda.synchronize()
    launch()
    first = y_s2.t.clone()
    want = y_full.t[:, 1:H + 1:2, 1:W + 1:2]
    assert tuple(want.shape) == (N, Ho, Wo, 256)
    assert float(want.float().abs().max()) > 0
    assert torch.equal(first[:, 1:-1, 1:-1], want)
    halo = first.clone()
    halo[:, 1:-1, 1:-1] = 0
    assert float(halo.float().abs().max()) == 0
    launch()
    assert torch.equal(y_s2.t, first)
    if N * H * W <= 3 * 64 * 64:
        t_ref = bfr(F.relu(F.conv2d(u, w2, b2, padding=1)))
        y_ref = bfr(F.relu(F.conv2d(t_ref, w3, b3) + x))[:, :, ::2, ::2]
        got = y_s2.nchw_float().cpu()
        assert float((got - y_ref).abs().max()) < 0.03 * float(y_ref.abs().max())
    # too small a dump area is refused
    assert L.dafne_bottleneck_block_narrow_s2_hip(_lib.ptr(ua.t), _lib.ptr(xa.t), _lib.ptr(wf), _lib.ptr(b2p), _lib.ptr(b3p), N, H, W,
                                                  _lib.ptr(y_s2.t), _lib.ptr(scratch2), scratch2.numel() - 1, st) != 0


# ------------------------------------------------------------------------------------------------------------------
# 2. res3.0's two 1x1 layers: stride 1 on the compact map == stride 2 on the full map
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("cout,flags_relu", [(128, True), (512, False)])        # res3.0.conv1 (+ ReLU), res3.0.shortcut
def test_res3_block0_1x1_layers_on_the_compact_map(n, cout, flags_relu, shared):
    """The plan's shapes (res2 map 256 x 256 of a 1024^2 image, 256 channels): engine.ConvCall with stride 1 on the
    even-pixel map runs the same kernel with the same tiles as stride 2 on the full map and writes the same bits."""
    from dafne_amd import engine, _lib
    d = dev()
    g = torch.Generator().manual_seed(8100 + n + cout)
    H = W = 256
    x = bfr(torch.relu(torch.randn(n, 256, H, W, generator=g)))
    w = bfr(torch.randn(cout, 256, 1, 1, generator=g) / 16.0)
    b = torch.randn(cout, generator=g) * 0.2
    full = engine.Act.from_nchw(x.to(d))
    compact = engine.Act.from_nchw(x[:, :, ::2, ::2].contiguous().to(d))
    wp, bp = engine.pack_conv(w, b, d)
    fl = engine.F_RELU if flags_relu else 0
    o2, o1 = engine.Act(n, H // 2, W // 2, cout, d), engine.Act(n, H // 2, W // 2, cout, d)
    c2 = engine.ConvCall(wp, bp, 256, cout, 1, 2, 0, fl, [(full.t, o2.t, None, H, W, H // 2, W // 2)], n, shared_gpu=shared)
    c1 = engine.ConvCall(wp, bp, 256, cout, 1, 1, 0, fl, [(compact.t, o1.t, None, H // 2, W // 2, H // 2, W // 2)], n, shared_gpu=shared)
    assert c1.kernel_name() == c2.kernel_name() and c1.num_tiles() == c2.num_tiles() and c1.tile_pixels() == c2.tile_pixels()
    c2(_lib.current_stream())
    c1(_lib.current_stream())
    torch.cuda.synchronize()
    assert float(o2.t.float().abs().max()) > 0
    assert torch.equal(o1.t, o2.t)


# ------------------------------------------------------------------------------------------------------------------
# 3. P7: ReLU of the input on load
def _p7_pair(a, n, h, w, seed):
    """-> (conv_wr with RELU_INPUT on `a`, relu_copy + plain conv_wr) for P7's layer (3x3, stride 2, pad 1, 256 -> 256)."""
    from dafne_amd import engine, _lib
    L = _lib.load()
    d = dev()
    g = torch.Generator().manual_seed(seed)
    wt = bfr(torch.randn(256, 256, 3, 3, generator=g) / 48.0)
    b = torch.randn(256, generator=g) * 0.1
    wp, bp = engine.pack_conv(wt, b, d)
    wfrag = engine.pack_conv_frag(wp)
    ho, wo = engine.conv_out_hw(h, w, 3, 2, 1)
    st = _lib.current_stream()
    ws = engine.WrWorkspace(d)
    rect = engine.Act(n, h, w, 256, d)
    _lib.check(L.dafne_relu_copy_bf16_hip(_lib.ptr(a.t), _lib.ptr(rect.t), a.t.numel(), st), "relu_copy")
    o_ref, o_new = engine.Act(n, ho, wo, 256, d), engine.Act(n, ho, wo, 256, d)
    c_ref = engine.ConvCall(wp, bp, 256, 256, 3, 2, 1, 0, [(rect.t, o_ref.t, None, h, w, ho, wo)], n)
    c_new = engine.ConvCall(wp, bp, 256, 256, 3, 2, 1, engine.F_RELU_INPUT, [(a.t, o_new.t, None, h, w, ho, wo)], n)
    assert L.dafne_conv2d_wr_ok(ctypes.byref(c_ref.prm), c_ref.segs) == 1 and L.dafne_conv2d_wr_ok(ctypes.byref(c_new.prm), c_new.segs) == 1
    calls = [engine.WrCall(c_ref, wfrag, ws), engine.WrCall(c_new, wfrag, ws)]
    assert calls[0].splits == calls[1].splits
    for c in calls:
        c(st)
    torch.cuda.synchronize()
    return o_new, o_ref, rect, c_new


def test_conv_wr_relu_input_equals_relu_copy_then_conv():
    """dafne_conv2d_wr_hip with DAFNE_CONV_RELU_INPUT on (a) a map holding all 65 536 bf16 bit patterns (-0, the negative NaNs
    and -inf give 0; +inf and the positive NaNs stay) and (b) a seeded random map equals dafne_relu_copy_bf16_hip followed by
    the plain call, bit for bit; the input is left as it was; dafne_conv2d_nhwc_bf16_hip still refuses the flag."""
    from dafne_amd import engine, _lib
    d = dev()
    # (a) bits = pixel * 256 + channel on a 16 x 16 map
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).reshape(1, 16, 16, 256)
    a = engine.Act(1, 16, 16, 256, d)
    a.t[:, 1:-1, 1:-1, :] = bits.to(d)
    before = a.t.clone()
    o_new, o_ref, rect, _ = _p7_pair(a, 1, 16, 16, 11)
    ri = rect.t[:, 1:-1, 1:-1, :].reshape(-1).view(torch.int16).cpu().to(torch.int32) & 0xffff
    want = torch.arange(65536, dtype=torch.int32)
    want[want >= 0x8000] = 0
    assert torch.equal(ri, want)                                    # the reference side is what the issue defines
    assert same_bits(a.t, before)
    assert same_bits(o_new.t, o_ref.t)
    finite = torch.isfinite(o_ref.t.float())
    assert float(finite.float().mean()) > 0.5 and float(o_ref.t.float()[finite].abs().max()) > 0
    # (b) a random map with both signs, three images
    g = torch.Generator().manual_seed(12)
    x = bfr(torch.randn(3, 256, 20, 12, generator=g))
    a = engine.Act.from_nchw(x.to(d))
    o_new, o_ref, rect, c_new = _p7_pair(a, 3, 20, 12, 13)
    assert float(o_ref.t.float().abs().max()) > 0
    assert torch.equal(o_new.t, o_ref.t)
    ref = bfr(F.conv2d(F.relu(x), *_p7_weights(13), stride=2, padding=1))
    got = o_new.nchw_float().cpu()
    tol = 2 * 2.0 ** -8 * ref.abs().clamp_min(2.0 ** -6) + 1e-3     # tests/test_gpu_conv.py close_bf16 (split-K: fp32 grouping)
    assert not bool(((got - ref).abs() > tol).any())
    # the generic entry does not know the flag
    with pytest.raises(_lib.DafneHipError):
        c_new(_lib.current_stream())
    torch.cuda.synchronize()


def _p7_weights(seed):
    g = torch.Generator().manual_seed(seed)
    wt = bfr(torch.randn(256, 256, 3, 3, generator=g) / 48.0)
    b = torch.randn(256, generator=g) * 0.1
    return wt, b


# ------------------------------------------------------------------------------------------------------------------
# 4. the whole model, switches off against on
def _head_tensors(head):
    out = []
    for name in ("logits", "delta_ctr", "center", "corners"):
        v = getattr(head, name, None)
        if v is not None:
            out += [(name, l, t.clone()) for l, t in enumerate(v)]
    return out


def _same_rows(got, exp, tag):
    (r, c), (rw, cw) = got, exp
    assert torch.equal(c, cw), (tag, c.tolist(), cw.tolist())
    for i in range(c.shape[0]):                 # (rows past an image's count are not part of the result)
        assert torch.equal(r[i, :int(cw[i])], rw[i, :int(cw[i])]), (tag, i)


def _run_model(depth, on, shapes, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    for k in ("DAFNE_RES2_TAIL_S2", "DAFNE_P7_RELU_IN"):
        monkeypatch.setenv(k, "1" if on else "0")
    d = dev()
    cfg, model, sd = bench.build_model(depth, d, seed=0)
    res = {}
    for (n, h, w, splits) in shapes:
        g = torch.Generator().manual_seed(100 + n + h)
        batch = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8).to(d)
        rows, counts = model.detect_packed(batch)
        torch.cuda.synchronize()
        plan = model.plan(n, h, w)
        r = {"serial": (rows.clone(), counts.clone()), "feats": [a.t.clone() for a in plan.features], "head": _head_tensors(plan.head),
             "names": [c.kernel_name() for c in plan.calls]}
        got = []
        for _ in range(3):
            o = model.detect_packed(batch, pipelined=True, splits=splits, defer=True)
            if o is not None:
                got.append(o)
        got.append(model.flush_deferred())
        torch.cuda.synchronize()
        assert len(got) == 3
        r["deferred"] = [(a.clone(), b.clone()) for a, b in got]
        st = model._pipe[(n, h, w, splits)]
        r["sub_names"] = [[c.kernel_name() for c in p.calls] for p in st["plans"][0]]
        res[(n, h, w)] = r
    return res


@pytest.mark.parametrize("depth", [50, 101])
def test_whole_model_same_bits_with_the_switches_off_and_on(depth, monkeypatch):
    """R50 / R101 with bench.build_model's seeded weights, a fresh model per setting, DAFNE_RES2_TAIL_S2 / DAFNE_P7_RELU_IN 0
    against 1, at 1024^2 batch 3 and 256 x 320 batch 4: the five FPN maps, every head output and (rows, counts) of
    detect_packed -- serial, and pipelined + deferred over three steps -- are torch.equal.  With the switches on a plan's
    launch list holds no relu_copy and exactly one conv_blk_narrow_s2 (and no full last res2 block); off: today's list."""
    shapes = [(3, 1024, 1024, 3), (4, 256, 320, 2)]
    off = _run_model(depth, False, shapes, monkeypatch)
    on = _run_model(depth, True, shapes, monkeypatch)
    for key in off:
        a, b = off[key], on[key]
        for names in [b["names"]] + b["sub_names"]:
            assert names.count("relu_copy") == 0 and names.count("conv_blk_narrow_s2") == 1 and names.count("conv_blk_narrow_last") == 0, key
        for names in [a["names"]] + a["sub_names"]:
            assert names.count("relu_copy") == 1 and names.count("conv_blk_narrow_s2") == 0 and names.count("conv_blk_narrow_last") == 1, key
        assert len(b["names"]) == len(a["names"]) - 1
        for l, (fa, fb) in enumerate(zip(a["feats"], b["feats"])):
            assert float(fa.float().abs().max()) > 0
            assert torch.equal(fa, fb), (key, "FPN map", l)
        assert len(a["head"]) == len(b["head"]) >= 10
        for (na, la, ta), (nb, lb, tb) in zip(a["head"], b["head"]):
            assert (na, la) == (nb, lb) and same_bits(ta, tb), (key, na, la)
        if key[1] == 1024:
            assert int(a["serial"][1].sum()) > 0
        _same_rows(a["serial"], b["serial"], (key, "serial"))
        for i, (ra, rb) in enumerate(zip(a["deferred"], b["deferred"])):
            _same_rows(ra, rb, (key, "deferred", i))
