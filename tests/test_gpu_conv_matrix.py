"""GPU: every case of tests/_conv_cases.py through engine.ConvCall, on the kernel the case was written for, against the same
convolution in fp64 on the CPU (one double matmul per tap over the shifted map; nothing of the library under test).

Two data regimes:
  exact     x in [-2, 2], w in {-1, 0, 1} (one in eight zero), bias and residual in [-8, 8]: integers, bf16-representable.  Every
            product and partial sum is an integer below 2^24 (asserted per case in tests/test_conv_dispatch_cpu.py), so fp32
            accumulation is exact in any order on any MFMA shape: fp32 outputs must EQUAL the reference, bf16 outputs its
            round-to-nearest-even bf16.  A missing tap, a pixel read from the wrong place or a stale operand shows as an integer.
  gaussian  as tests/test_gpu_conv.py: bf16-rounded normal data, close_bf16 (2 bf16 ulps) on bf16 outputs, 2e-3 * max|ref| on
            fp32 outputs.
Outputs start as NaN in the interior, every launch runs twice into the same buffers, every segment and every image is compared
and the one-pixel halo of every bf16 output must still be zero."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from _conv_cases import B_MAX, CASES, LIMIT_CASES, R_MAX, X_MAX, out_hw
from test_gpu_conv import close_bf16, dev

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ints(shape, lim, g):
    return torch.randint(-lim, lim + 1, shape, generator=g, dtype=torch.int8).float()


def _weights_exact(cout, cin, k, g):
    r = torch.randint(0, 8, (cout, cin, k, k), generator=g, dtype=torch.int8)
    return torch.where(r == 0, 0.0, torch.where(r % 2 == 1, 1.0, -1.0))             # one in eight is zero


def make_data(case, regime):
    """-> xs [N,H,W,Cin] per segment, w [Cout,Cin,k,k], bias [Cout] or None, rs [N,h,w,Cout] per segment or None (the residual,
    or the half-size map of the top-down add); fp32 tensors on the CPU holding bf16-representable values (the bias: any fp32)."""
    g = torch.Generator().manual_seed(zlib.crc32((case.name + regime).encode()))
    kk = case.cin * case.k * case.k
    res_sizes = None
    if "RES" in case.flags or "UP" in case.flags:
        res_sizes = [out_hw(h, w, case.k, case.stride) for h, w in case.sizes]
        if "UP" in case.flags:
            res_sizes = [(h // 2, w // 2) for h, w in res_sizes]
    if regime == "exact":
        xs = [_ints((case.n, h, w, case.cin), X_MAX, g) for h, w in case.sizes]
        w = _weights_exact(case.cout, case.cin, case.k, g)
        b = _ints((case.cout,), B_MAX, g) if case.bias else None
        rs = [_ints((case.n, h, w_, case.cout), R_MAX, g) for h, w_ in res_sizes] if res_sizes else None
    else:
        xs = [torch.randn(case.n, h, w, case.cin, generator=g).to(BF).float() for h, w in case.sizes]
        w = (torch.randn(case.cout, case.cin, case.k, case.k, generator=g) / kk ** 0.5).to(BF).float()
        b = torch.randn(case.cout, generator=g) * 0.1 if case.bias else None
        rs = [torch.randn(case.n, h, w_, case.cout, generator=g).to(BF).float() for h, w_ in res_sizes] if res_sizes else None
    return xs, w, b, rs


def ref_conv_image(x, w, b, k, stride):
    """fp64 convolution of ONE image x [H,W,Cin] (zero padding k // 2) -> [Ho,Wo,Cout] double: one double matmul per tap over the
    shifted (strided) map, in bands of rows (a 2^20-pixel map in double is large)."""
    h, wd_, cin = x.shape
    cout, p = w.shape[0], k // 2
    ho, wo = out_hw(h, wd_, k, stride)
    xp = F.pad(x, (0, 0, p, p, p, p))
    wt = w.double().permute(2, 3, 1, 0).contiguous()                   # [k, k, Cin, Cout]
    y = torch.empty(ho, wo, cout, dtype=torch.float64)
    band = max(1, (1 << 16) // wo)
    for r0 in range(0, ho, band):
        r1 = min(ho, r0 + band)
        acc = torch.zeros((r1 - r0) * wo, cout, dtype=torch.float64)
        for kh in range(k):
            for kw in range(k):
                sl = xp[r0 * stride + kh:(r1 - 1) * stride + kh + 1:stride, kw:(wo - 1) * stride + kw + 1:stride]
                acc += sl.reshape(-1, cin).double() @ wt[kh, kw]
        y[r0:r1] = acc.reshape(r1 - r0, wo, cout)
    if b is not None:
        y += b.double()
    return y


def reference(case, xs, w, b, rs):
    """-> per segment (y raw [N,Ho,Wo,Cout] double: bias included, before the epilogue; out: after residual / top-down add / ReLU)."""
    res = []
    for s, x in enumerate(xs):
        y = torch.stack([ref_conv_image(x[n], w, b, case.k, case.stride) for n in range(case.n)])
        o = y
        if "RES" in case.flags:
            o = o + rs[s].double()
        if "UP" in case.flags:
            o = o + rs[s].double().repeat_interleave(2, 1).repeat_interleave(2, 2)
        if "RELU" in case.flags:
            o = o.clamp_min(0)
        res.append((y, o))
    return res


def to_act(x, d):
    from dafne_amd import engine
    n, h, w, c = x.shape
    a = engine.Act(n, h, w, c, d)
    a.t[:, 1:-1, 1:-1, :] = x.to(BF).to(d)
    return a


class Launch:
    """The device side of a case: buffers, the ConvCall, two launches."""

    def __init__(self, case, xs, w, b, rs):
        from dafne_amd import engine, _lib
        d = dev()
        self.case, self.f32 = case, "F32" in case.flags
        self.ins = [to_act(x, d) for x in xs]
        self.res = [to_act(r, d) for r in rs] if rs is not None else None
        wp, bp = engine.pack_conv(w, b, d)
        flags = 0
        for name, bit in (("RELU", engine.F_RELU), ("RES", engine.F_RES), ("UP", engine.F_UP), ("F32", engine.F_F32), ("GN", engine.F_GN)):
            if name in case.flags:
                flags |= bit
        self.outs, segs = [], []
        for s, a in enumerate(self.ins):
            ho, wo = out_hw(a.h, a.w, case.k, case.stride)
            if self.f32:
                o = torch.full((case.n, ho, wo, case.cout), float("nan"), dtype=torch.float32, device=d)
                ot = o
            else:
                o = engine.Act(case.n, ho, wo, case.cout, d)
                o.t[:, 1:-1, 1:-1, :] = float("nan")
                ot = o.t
            self.outs.append(o)
            segs.append((a.t, ot, self.res[s].t if self.res is not None else None, a.h, a.w, ho, wo))
        self.partial = None
        bias = bp if case.bias else None
        if "GN" in case.flags:
            nt = engine.ConvCall(wp, bias, case.cin, case.cout, case.k, case.stride, case.k // 2, flags & ~engine.F_GN, segs, case.n).num_tiles()
            self.partial = torch.full((nt, case.cout // 8, 2), float("nan"), dtype=torch.float32, device=d)
        self.call = engine.ConvCall(wp, bias, case.cin, case.cout, case.k, case.stride, case.k // 2, flags, segs, case.n,
                                    gn_partial=self.partial)
        assert self.call.kernel_name() == case.kernel
        st = _lib.current_stream()
        self.call(st)
        self.call(st)                   # twice into the same buffers: nothing is left behind, nothing is read back
        torch.cuda.synchronize()

    def interior(self, s):
        return self.outs[s] if self.f32 else self.outs[s].t[:, 1:-1, 1:-1, :]

    def check_halo(self):
        if self.f32:
            return
        for o in self.outs:
            t = o.t
            for edge in (t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1]):
                assert bool((edge == 0).all()), "halo of a bf16 output written"


def assert_same(got, ref, what):
    if torch.equal(got, ref):
        return
    bad = got != ref                    # (NaN != anything: an unwritten output counts)
    idx = bad.nonzero()[:8].cpu().tolist()
    first = [(i, float(got[tuple(i)]), float(ref[tuple(i)])) for i in idx]
    raise AssertionError("%s: %d of %d values differ; first (n, h, w, c), got, reference: %s" % (what, int(bad.sum()), bad.numel(), first))


def check_outputs(L, refs, regime):
    case, d = L.case, dev()
    L.check_halo()
    for s, (y, o) in enumerate(refs):
        got = L.interior(s)
        what = "%s segment %d (%s)" % (case.name, s, regime)
        assert bool(torch.isfinite(got).all()), what + ": output not written everywhere"
        if regime == "exact":
            assert float(o.abs().max()) < 2 ** 24
            ref = o.float().to(d)                                   # integers below 2^24: exact in fp32
            assert_same(got, ref if L.f32 else ref.to(BF), what)    # .to(bf16) rounds to nearest even, as f2bf / v_cvt_pk_bf16_f32
        elif L.f32:
            err = float((got.double().cpu() - o).abs().max())
            assert err < 2e-3 * float(o.abs().max()), (what, err)
        else:
            close_bf16(got.float().cpu(), o.float().to(BF).float())
    if L.partial is not None:
        tpi = L.call.tiles_per_image()
        part = L.partial.double().cpu()
        assert bool(torch.isfinite(part).all()), "GroupNorm partial sums not written for every tile"
        t0 = 0
        for s, (y, _) in enumerate(refs):
            n, g = case.n, case.cout // 8
            ps = part[t0:t0 + tpi[s] * n].reshape(n, tpi[s], g, 2).sum(1)          # the tiles of an image, summed in fp64
            t0 += tpi[s] * n
            grp = y.reshape(n, -1, g, 8)
            s1, s2 = grp.sum((1, 3)), (grp * grp).sum((1, 3))
            if regime == "exact":
                assert float(grp.abs().sum((1, 3)).max()) < 2 ** 24             # then every tile's fp32 sum of integers is exact
                assert torch.equal(ps[..., 0], s1), (case.name, s, float((ps[..., 0] - s1).abs().max()))
            else:
                assert torch.allclose(ps[..., 0], s1, rtol=1e-4, atol=1e-1)
            assert torch.allclose(ps[..., 1], s2, rtol=1e-4, atol=1e-1)
        assert t0 == L.call.num_tiles()


@pytest.mark.parametrize("regime", ["exact", "gaussian"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_conv_case_equals_fp64_reference(case, regime, monkeypatch):
    xs, w, b, rs = make_data(case, regime)
    refs = reference(case, xs, w, b, rs)
    if case.kernel == "conv_igemm<2,2,2,2>":
        # the 4-stage operand ring and the double buffer: same K order, identical bits (DAFNE_CONV_RING is read per call)
        runs = []
        for ring in ("1", "0"):
            monkeypatch.setenv("DAFNE_CONV_RING", ring)
            runs.append(Launch(case, xs, w, b, rs))
        for s in range(len(xs)):
            assert torch.equal(runs[0].interior(s), runs[1].interior(s)), "ring and two-stage loop differ"
        if runs[0].partial is not None:
            assert torch.equal(runs[0].partial, runs[1].partial)
        for L in runs:
            check_outputs(L, refs, regime)
    else:
        check_outputs(Launch(case, xs, w, b, rs), refs, regime)


@pytest.mark.parametrize("cin,cout,k,size,n,n_bad", LIMIT_CASES)
def test_largest_batch_below_the_32bit_offset_limit(cin, cout, k, size, n, n_bad):
    """The largest batch the library accepts for 32-bit input offsets (just below 2^32 bytes of haloed input): exact data made on
    the device, images 0, N / 2 and N - 1 against the fp64 reference.  An offset that wrapped would read an early image's pixels
    for a late one.  (Three fixed images, not all: the host copy of ~4 GB maps is what this avoids.)"""
    from dafne_amd import engine, _lib
    d = dev()
    h, wd_ = size
    g = torch.Generator().manual_seed(cin + cout + n)
    w = _weights_exact(cout, cin, k, g)
    b = _ints((cout,), B_MAX, g)
    gd = torch.Generator(device=d).manual_seed(n)
    a = engine.Act(n, h, wd_, cin, d)
    assert a.t.numel() * 2 <= 0xffffffff < (a.t.numel() // n) * (n + 1) * 2
    for i in range(n):
        a.t[i, 1:-1, 1:-1, :] = torch.randint(-X_MAX, X_MAX + 1, (h, wd_, cin), generator=gd, dtype=torch.int8, device=d).to(BF)
    o = engine.Act(n, h, wd_, cout, d)
    o.t[:, 1:-1, 1:-1, :] = float("nan")
    wp, bp = engine.pack_conv(w, b, d)
    call = engine.ConvCall(wp, bp, cin, cout, k, 1, k // 2, 0, [(a.t, o.t, None, h, wd_, h, wd_)], n)
    assert call.kernel_name() == ("conv_ws" if k == 1 else "conv_igemm<1,4,2,2>")
    call(_lib.current_stream())
    torch.cuda.synchronize()
    try:
        assert bool(torch.isfinite(o.t).all())
        for edge in (o.t[:, 0], o.t[:, -1], o.t[:, :, 0], o.t[:, :, -1]):
            assert bool((edge == 0).all())
        for i in (0, n // 2, n - 1):
            x = a.t[i, 1:-1, 1:-1, :].float().cpu()
            ref = ref_conv_image(x, w, b, k, 1)
            assert float(ref.abs().max()) < 2 ** 24
            assert_same(o.t[i, 1:-1, 1:-1, :], ref.float().to(d).to(BF), "image %d of %d" % (i, n))
    finally:
        del a, o, call
        torch.cuda.empty_cache()
