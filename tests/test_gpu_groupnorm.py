"""GPU: the GroupNorm chain of the head towers, kernel by kernel, against an fp64 reference on the CPU (one double matmul per tap:
ref_conv_image of tests/test_gpu_conv_matrix.py; nothing of the library under test).  The cases, their data and the references
live in tests/test_groupnorm_cases_cpu.py, which also proves without a device that every case lands on the kernel it names and
that the data is exact: integer maps, weights in {-1, 0, 1}, integer biases, max|y| <= 256 and sum|y|, sum y^2 < 2^24 per image and
group -- every partial sum of every tile and every sum over tiles is an exact integer in fp32 in any order.

  A  producers    partial buffer NaN with 64 guard rows, two launches: every row below num_tiles() finite, the guard rows still
                  NaN; per (segment, image, group) the fp64 sum of the image's tile rows EQUALS the reference's sum y and sum y^2;
                  the raw bf16 map equals the reference, the halo is zero.  Every producer that takes F_GNFIN runs in both forms
                  (the fused form publishes its partials through another store path).
  B  finalisation (mean, rstd) through dafne_groupnorm_finalize_hip and through F_GNFIN (counters zero before the first launch, statistics
                  NaN before each of two launches: after each the counters are all 0 and the statistics finite): fused and separate bit-identical;
                  mean within one fp32 ulp of float32(sum y / cnt); |rstd / rstd64 - 1| <= 2^-22 E[y^2] / (var64 + eps) + 2^-21
                  (derived in test_groupnorm_cases_cpu.rstd_bound); the zero-variance group: mean = bias exactly, rstd within
                  2^-21 of eps^-1/2.
  C  consumers    F_GNIN with statistics written by the test (integer mean, rstd in {1/8, 1/4, 1/2}, different for every (segment,
                  image, group); dyadic gamma, beta): every operand is exact in fp32 in both forms of the expression, the only
                  rounding is the operand's to bf16, the convolution sums multiples of 2^-5: bf16 outputs EQUAL the reference
                  rounded to bf16, fp32 outputs the reference.  Outputs start as NaN, two launches, halos checked.
  D  the pass     dafne_groupnorm_relu_nhwc_bf16_hip on the data of C, five segments with a 1 x 1 level in one launch, partial sums
                  chosen so that the finalisation yields exactly the injected statistics (eps = 1): output equals
                  bf16(relu(..)) of the reference, the halo (filled with a sentinel) is untouched.

Coverage per kernel:
  conv_igemm<2,2,2,2>, <4,2,2,4>, <1,4,2,2>, <1,4,1,2>   A, B (separate finalisation; 32, 32, 8 and 4 groups)
  conv3x3_patch          A, B (separate and gn_fused_finalize: tower levels, 45 tiles per image, large mean on its GN_INPUT
                         instance; Cout 512 and 112 tiles per image: separate only), C
  conv3x3_rp m32 / m16   A, B (separate and gn_fused_finalize; single and pair launch), C (single and pair launch); A, B and C
                         also with 261 tiles, two per workgroup of the persistent grid (rp-multi, on-rp-multi)
  conv3x3_patch_fp8      A, B (separate and gn_fused_finalize); its consumer side is tests/test_gpu_fp8.py's
  conv3x3_slab, conv3x3_pred16                           C
  gn_finalize_kernel     B: second group round (64 groups), 4-deep loop (112 tiles), 1 x 1 level, zero variance, large mean; D
  gn_fused_finalize      B on conv3x3_patch, conv3x3_rp (single, pair) and conv3x3_patch_fp8
  gn_apply_kernel        D
The only tolerances are 0, one fp32 ulp and the derived rstd bound."""
import ctypes
import types

import numpy as np
import pytest
import torch

from test_groupnorm_cases_cpu import (BF, C_BY_NAME, CONSUMERS, EPS, MULTI_TILE, PRODUCERS, RP, _halves, check_mean_rstd, consumer_reference,
                                      group_sums, producer_reference, takes_fused_finalize, zero_group)
import test_gpu_conv
from test_gpu_conv import _gsegs, _rp_call, dev, rp16  # noqa: F401  (rp16: the fixture that selects _rp_call's MFMA form)
from test_gpu_conv_matrix import assert_same, to_act
from test_gpu_fp8 import run_fp8

pytestmark = pytest.mark.gpu
GUARD = 64
NAN = float("nan")

_RUNS = {}        # (case, fused, m16) -> run_producer's result on the CPU: A and B look at the same two launches


def _check_form(case, m16):
    """_rp_call builds the MFMA form the rp16 fixture selected: `m16` must be that form (and False off the resident-patch kernel)."""
    assert bool(m16) == bool(test_gpu_conv._RP16), "m16 does not match the rp16 fixture"
    assert case.entry in ("rp", "pair") or not m16


def _more_tiles_than_cus(case, tiles, d):
    """a workgroup of the persistent grid takes more than one tile in exactly the cases that say so"""
    assert (tiles > torch.cuda.get_device_properties(d).multi_processor_count) == (case.name in MULTI_TILE), (case.name, tiles)


def _nan_act(n, h, w, c, d):
    from dafne_amd import engine
    a = engine.Act(n, h, w, c, d)
    a.t[:, 1:-1, 1:-1, :] = NAN
    return a


def _halo_is(t, value, what):
    for edge in (t[:, 0], t[:, -1], t[:, :, 0], t[:, :, -1]):
        assert bool((edge == value).all()), what + ": halo written"


def _finalize(partial, sizes, tpis, n, c, d, eps=EPS):
    """dafne_groupnorm_finalize_hip over all levels -> stats [levels, N, C/8, 2] on the CPU (the buffer starts as NaN)."""
    from dafne_amd import _lib
    stats = torch.full((len(sizes), n, c // 8, 2), NAN, dtype=torch.float32, device=d)
    maps = [types.SimpleNamespace(t=partial, h=h, w=w) for h, w in sizes]       # (the finalisation never touches the map)
    _lib.check(_lib.load().dafne_groupnorm_finalize_hip(_gsegs(maps, tpis, n), len(sizes), n, c, _lib.ptr(partial), _lib.ptr(stats),
                                                        ctypes.c_float(eps), _lib.current_stream()), "finalize")
    torch.cuda.synchronize()
    return stats.cpu()


def run_producer(case, fused, m16=False):
    """Two launches of a producer case into NaN buffers -> per half a namespace: raw (haloed bf16 maps on the CPU, or None where
    run_fp8 checked the halo itself), interior (fp32 [N,H,W,C] per level), partial (CPU), nt, tpis, sep (statistics of the separate
    finalisation of these partials), log (after each launch: counters, fused statistics).  Run once per (case, form)."""
    _check_form(case, m16)
    key = (case.name, fused, bool(m16))
    if key in _RUNS:
        return _RUNS[key]
    from dafne_amd import engine, _lib
    d, st = dev(), _lib.current_stream()
    n, g = case.n, case.cout // 8
    halves = []
    for half in _halves(case):
        xs, w, b, ys = producer_reference(case, half)
        H = types.SimpleNamespace(log=[], raw=None)
        H.stats = torch.full((len(xs), n, g, 2), NAN, dtype=torch.float32, device=d)
        H.counters = torch.zeros(len(xs), n, dtype=torch.int32, device=d)
        gn_fin = (H.stats, H.counters, EPS) if fused else None

        def after(_call, H=H):
            H.log.append((H.counters.cpu().clone(), H.stats.cpu().clone()))
            H.stats.fill_(NAN)          # every launch has to write them again

        if case.entry == "fp8":
            outs, H.partial_dev, H.call = run_fp8([x.permute(0, 3, 1, 2).contiguous() for x in xs], w, b, 1.0, gn_stats=True,
                                                  gn_fin=gn_fin, guard_rows=GUARD, launches=2, after_launch=after)
            H.interior = [o.permute(0, 2, 3, 1).contiguous() for o in outs]
            H.after = None
        else:
            H.ins = [to_act(x, d) for x in xs]
            H.outs = [_nan_act(n, h, w_, case.cout, d) for h, w_ in case.sizes]
            wp, bp = engine.pack_conv(w, b, d)
            segs = [(i.t, o.t, None, i.h, i.w, i.h, i.w) for i, o in zip(H.ins, H.outs)]
            kw, flags = {}, engine.F_GN | (engine.F_GNFIN if fused else 0)
            if case.gnin:              # identity statistics: the operand is relu(x)
                ident = torch.zeros(len(xs), n, case.cin // 8, 2, device=d)
                ident[..., 1] = 1.0
                kw["gn_in"] = (ident, torch.ones(case.cin, device=d), torch.zeros(case.cin, device=d))
                flags |= engine.F_GNIN
            if case.entry == "generic":
                mk = lambda fl, **k: engine.ConvCall(wp, bp, case.cin, case.cout, case.k, 1, case.k // 2, fl, segs, n, **k)
            else:
                mk = lambda fl, **k: _rp_call(wp, bp, case.cout, fl, segs, n, d, **k)
            nt = mk(flags & ~(engine.F_GN | engine.F_GNFIN), **kw).num_tiles()
            H.partial_dev = torch.full((nt + GUARD, g, 2), NAN, dtype=torch.float32, device=d)
            H.call = mk(flags, gn_partial=H.partial_dev, gn_fin=gn_fin, **kw)
            assert H.call.num_tiles() == nt
            H.after = after
        assert H.call.kernel_name() == case.kernel
        H.nt, H.tpis = H.call.num_tiles(), H.call.tiles_per_image()
        assert sum(t * n for t in H.tpis) == H.nt
        halves.append(H)
    if case.entry in ("rp", "pair"):
        _more_tiles_than_cus(case, sum(H.nt for H in halves), d)
    if case.entry != "fp8":
        launch = engine.ConvPairCall(halves[0].call, halves[1].call) if case.entry == "pair" else halves[0].call
        for _ in range(2):              # twice into the same buffers: nothing is left behind, nothing is read back
            launch(st)
            torch.cuda.synchronize()
            for H in halves:
                H.after(None)
    for H in halves:
        H.partial = H.partial_dev.cpu()
        if case.entry != "fp8":
            H.raw = [o.t.cpu() for o in H.outs]
            H.interior = [r[:, 1:-1, 1:-1, :].float() for r in H.raw]
        H.sep = _finalize(H.partial_dev, case.sizes, H.tpis, n, case.cout, d)
        H.ins = H.outs = H.call = H.partial_dev = None
    _RUNS[key] = halves
    return halves


def check_producer(case, fused, m16=False):
    """A"""
    g = case.cout // 8
    for half, H in zip(_halves(case), run_producer(case, fused, m16)):
        xs, w, b, ys = producer_reference(case, half)
        what = "%s half %d%s" % (case.name, half, " fused finalisation" if fused else "")
        assert H.partial.shape[0] == H.nt + GUARD
        assert bool(torch.isfinite(H.partial[:H.nt]).all()), what + ": partial sums not written for every tile"
        assert bool(torch.isnan(H.partial[H.nt:]).all()), what + ": partial rows beyond num_tiles() written"
        t0 = 0
        for s, y in enumerate(ys):
            tpi = H.tpis[s]
            rows = H.partial[t0:t0 + tpi * case.n].double().reshape(case.n, tpi, g, 2).sum(1)      # the tiles of an image, in fp64
            t0 += tpi * case.n
            s1, s2, _ = group_sums(y)
            assert_same(rows[..., 0], s1, "%s level %d: sum y per (image, group)" % (what, s))
            assert_same(rows[..., 1], s2, "%s level %d: sum y^2 per (image, group)" % (what, s))
            assert_same(H.interior[s], y.float().to(BF).float(), "%s level %d: raw map" % (what, s))
            assert torch.equal(y.float().to(BF).double(), y)                   # (|y| <= 256: the bf16 map stores y itself)
            if H.raw is not None:
                _halo_is(H.raw[s], 0, "%s level %d" % (what, s))
        assert t0 == H.nt


def check_statistics(case, m16=False):
    """B"""
    fused_ok = takes_fused_finalize(case)
    plain = run_producer(case, False, m16)
    fused = run_producer(case, True, m16) if fused_ok else [None] * len(plain)
    for half, P, Fz in zip(_halves(case), plain, fused):
        xs, w, b, ys = producer_reference(case, half)
        z, zb = zero_group(case, half), float(b[8 * zero_group(case, half)])
        what = "%s half %d" % (case.name, half)
        variants = [("separate", P.sep)]
        if Fz is not None:
            assert len(Fz.log) == 2
            for k, (counters, stats) in enumerate(Fz.log):
                assert int(counters.abs().max()) == 0, "%s: arrival counters not reset by launch %d" % (what, k)
                assert bool(torch.isfinite(stats).all()), "%s: statistics not written by launch %d" % (what, k)
            assert torch.equal(Fz.log[0][1], Fz.log[1][1]), what + ": the second launch finalised other statistics"
            # the fused finalisation reduces in gn_finalize_kernel's order: bit-identical, on its own partials and the plain form's
            assert torch.equal(Fz.partial[:Fz.nt], P.partial[:P.nt]), what + ": partial sums of the two forms differ"
            assert_same(Fz.log[1][1], Fz.sep, what + ": fused against separate finalisation")
            assert_same(Fz.log[1][1], P.sep, what + ": fused against separate finalisation of the plain launch")
            variants.append(("fused", Fz.log[1][1]))
        for name, stats in variants:
            assert bool(torch.isfinite(stats).all()), (what, name)
            for s, y in enumerate(ys):
                mean, rstd = stats[s, :, :, 0].numpy(), stats[s, :, :, 1].numpy()
                check_mean_rstd(mean, rstd, y, "%s level %d %s" % (what, s, name))
                assert (mean[:, z] == np.float32(zb)).all(), (what, s, name, "zero-variance group: mean", mean[:, z], zb)
                rel = np.abs(rstd[:, z].astype(np.float64) * EPS ** 0.5 - 1.0)
                assert (rel <= 2.0 ** -21).all(), (what, s, name, "zero-variance group: rstd", float(rel.max()))


GENERIC = [c for c in PRODUCERS if c.entry in ("generic", "fp8")]
RESIDENT = [c for c in PRODUCERS if c.entry in ("rp", "pair")]


def _forms(cases):
    out = []
    for c in cases:
        out.append(pytest.param(c, False, id=c.name))
        if takes_fused_finalize(c):
            out.append(pytest.param(c, True, id=c.name + "-gnfin"))
    return out


@pytest.mark.parametrize("case,fused", _forms(GENERIC))
def test_producer_partial_sums_equal_fp64_reference(case, fused):
    check_producer(case, fused)


@pytest.mark.parametrize("case,fused", _forms(RESIDENT))
def test_resident_patch_producer_partial_sums_equal_fp64_reference(case, fused, rp16):
    """Both MFMA forms: with exact data the 16x16x32 form must give equal sums and an equal map as well."""
    check_producer(case, fused, rp16)


@pytest.mark.parametrize("case", GENERIC, ids=[c.name for c in GENERIC])
def test_finalised_statistics_against_fp64(case):
    check_statistics(case)


@pytest.mark.parametrize("case", RESIDENT, ids=[c.name for c in RESIDENT])
def test_resident_patch_finalised_statistics_against_fp64(case, rp16):
    check_statistics(case, rp16)


# ------------------------------------------------------------------------------------------------------------ C
def check_consumer(case, m16=False):
    from dafne_amd import engine, _lib
    _check_form(case, m16)
    d, st = dev(), _lib.current_stream()
    n = case.n
    halves = []
    for half in _halves(case):
        xs, stats, gamma, beta, w, b, ops, ys = consumer_reference(case, half)
        H = types.SimpleNamespace(ys=ys)
        H.ins = [to_act(x, d) for x in xs]
        if case.f32:
            H.outs = [torch.full((n, h, w_, case.cout), NAN, dtype=torch.float32, device=d) for h, w_ in case.sizes]
            outs_t = H.outs
        else:
            H.outs = [_nan_act(n, h, w_, case.cout, d) for h, w_ in case.sizes]
            outs_t = [o.t for o in H.outs]
        wp, bp = engine.pack_conv(w, b, d)
        segs = [(i.t, o, None, i.h, i.w, i.h, i.w) for i, o in zip(H.ins, outs_t)]
        gn_in = (stats.to(d).contiguous(), gamma.to(d).contiguous(), beta.to(d).contiguous())
        flags = engine.F_GNIN | (engine.F_F32 if case.f32 else 0)
        if case.entry == "generic":
            H.call = engine.ConvCall(wp, bp, case.cin, case.cout, 3, 1, 1, flags, segs, n, gn_in=gn_in)
        else:
            H.call = _rp_call(wp, bp, case.cout, flags, segs, n, d, gn_in=gn_in)
        assert H.call.kernel_name() == case.kernel
        halves.append(H)
    _more_tiles_than_cus(case, halves[0].call.num_tiles(), d)
    launch = engine.ConvPairCall(halves[0].call, halves[1].call) if case.entry == "pair" else halves[0].call
    launch(st)
    launch(st)                          # twice into the same buffers
    torch.cuda.synchronize()
    for half, H in zip(_halves(case), halves):
        for s, y in enumerate(H.ys):
            what = "%s half %d level %d" % (case.name, half, s)
            ref = y.float()
            assert torch.equal(ref.double(), y)                                 # multiples of 2^-5 below 2^24 quanta
            if case.f32:
                assert_same(H.outs[s], ref.to(d), what)
            else:
                assert_same(H.outs[s].t[:, 1:-1, 1:-1, :], ref.to(BF).to(d), what)
                _halo_is(H.outs[s].t, 0, what)


ON_LOAD = [c for c in CONSUMERS if c.kernel != RP]
ON_LOAD_RP = [c for c in CONSUMERS if c.kernel == RP]


@pytest.mark.parametrize("case", ON_LOAD, ids=[c.name for c in ON_LOAD])
def test_groupnorm_on_load_equals_fp64_reference(case):
    check_consumer(case)


@pytest.mark.parametrize("case", ON_LOAD_RP, ids=[c.name for c in ON_LOAD_RP])
def test_resident_patch_groupnorm_on_load_equals_fp64_reference(case, rp16):
    check_consumer(case, rp16)


# ------------------------------------------------------------------------------------------------------------ D
def test_separate_pass_equals_fp64_reference():
    """dafne_groupnorm_relu_nhwc_bf16_hip (gn_finalize_kernel + gn_apply_kernel) on the maps, statistics and affine parameters of
    the on-load cases, five segments in one launch (seg_start of gn_apply_kernel), the last a 1 x 1 level.  The partial sums are
    made up so that the finalisation yields the injected statistics exactly: with eps = 1, var = rstd^-2 - 1 in {3, 15, 63},
    a = mean cnt and b = (var + mean^2) cnt are integers below 2^24 spread over the image's tiles; b / cnt, mean^2, the
    difference and var + eps in {4, 16, 64} are exact, rsqrtf of a power of four is the power of two."""
    from dafne_amd import engine, _lib
    case = C_BY_NAME["on-patch"]
    xs, stats, gamma, beta, w, b, ops, ys = consumer_reference(case)
    d, n, c = dev(), case.n, case.cin
    g = c // 8
    tpis = [5, 3, 2, 1, 1]
    assert len(xs) == 5 and case.sizes[-1] == (1, 1)
    partial = torch.zeros(sum(tpis) * n, g, 2, dtype=torch.float64)
    t0 = 0
    for s, (h, w_) in enumerate(case.sizes):
        cnt = h * w_ * 8
        mean, rstd = stats[s, :, :, 0].double(), stats[s, :, :, 1].double()
        a = mean * cnt
        bsum = (1.0 / (rstd * rstd) - 1.0 + mean * mean) * cnt
        assert float(a.abs().max()) < 2 ** 24 and float(bsum.max()) < 2 ** 24 and torch.equal(bsum, bsum.round())
        a1, b1 = (a / 3).round(), (bsum / 2).floor()
        for i in range(n):
            first, other, last = t0 + i * tpis[s], t0 + i * tpis[s] + i % tpis[s], t0 + (i + 1) * tpis[s] - 1
            partial[first, :, 0] += a1[i]
            partial[other, :, 0] += a[i] - a1[i]
            partial[first, :, 1] += b1[i]
            partial[last, :, 1] += bsum[i] - b1[i]
        t0 += tpis[s] * n
    assert torch.equal(partial.float().double(), partial)
    partial = partial.float().to(d)
    maps = [to_act(x, d) for x in xs]
    for m in maps:                       # a sentinel in the halo: untouched means neither normalised nor cleared
        m.t[:, 0], m.t[:, -1], m.t[:, :, 0], m.t[:, :, -1] = 3.0, 3.0, 3.0, 3.0
    out_stats = torch.full((5, n, g, 2), NAN, dtype=torch.float32, device=d)
    gd, bd = gamma.to(d).contiguous(), beta.to(d).contiguous()
    _lib.check(_lib.load().dafne_groupnorm_relu_nhwc_bf16_hip(_gsegs(maps, tpis, n), 5, n, c, _lib.ptr(partial), _lib.ptr(out_stats),
                                                              _lib.ptr(gd), _lib.ptr(bd), ctypes.c_float(1.0), _lib.current_stream()), "gn")
    torch.cuda.synchronize()
    assert_same(out_stats.cpu(), stats, "finalised statistics against the injected ones (level, image, group, mean / rstd)")
    for s, (m, op) in enumerate(zip(maps, ops)):
        assert_same(m.t[:, 1:-1, 1:-1, :], op.float().to(BF).to(d), "level %d" % s)       # op: bf16(relu(..)) of the fp64 expression
        _halo_is(m.t, 3.0, "level %d" % s)
