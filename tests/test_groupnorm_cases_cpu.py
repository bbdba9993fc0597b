"""The case table of the GroupNorm chain (producers of per-tile partial sums, finalisation, on-load consumers, the separate pass),
its data and its fp64 references -- shared with tests/test_gpu_groupnorm.py -- and, without a device, the preconditions the GPU
tests rest on:
  * every case lands on the kernel it names (the probing calls of tests/test_conv_dispatch_cpu.py; dafne_conv3x3_c256_ok and
    dafne_conv2d_fp8w_num_tiles for the resident-patch and fp8 entry points);
  * the exact-data bounds: all maps, weights and biases are integers, max|y| <= 256 (the raw bf16 map stores y itself) and, per
    image and group, sum|y| < 2^24 and sum y^2 < 2^24 -- every partial sum of every tile and every later sum over tiles is then
    an exact integer in fp32 in any order, so the device's sums must EQUAL the reference's;
  * the derived bound on rstd holds for an fp32 emulation of the kernels' formula (the reference alone stays within it);
  * the consumers' injected statistics and affine parameters make every operand a short dyadic number (exact in fp32 in both
    forms of the expression) and every output a sum of multiples of 2^-5 below 2^24 quanta.

Producer data: x in [-X, X], w in {-1, 0, 1} with one non-zero in `dens`, bias = boff + an integer in [blo, bhi]; one group per
case has all-zero weights and one common bias (variance exactly 0).  Consumer data: x in [-12, 12]; statistics written by the
test -- mean an integer in [-6, 1], rstd in {1/8, 1/4, 1/2}, both different for every (segment, image, group); gamma in {0.5,
0.75, 1, 1.25, 1.5, 2}, beta a multiple of 1/16 in [-1, 4], per channel (beta - mean rstd gamma > 0 for most channels: a padding
pixel that got normalised instead of staying zero changes every border output)."""
import collections
import ctypes
import functools
import os
import zlib

import numpy as np
import pytest
import torch

from _conv_cases import IG0, IG1, IG2, IG3, PATCH, PRED16, SLAB
from test_gpu_conv_matrix import _ints, ref_conv_image

BF = torch.bfloat16
EPS = float(np.float32(1e-5))            # the kernels take eps as a float
RP, FP8 = "conv3x3_rp", "conv3x3_patch_fp8"
F_F32, F_GN, F_GNIN, F_GNFIN = 8, 16, 32, 64
MI355X_CUS = 256                         # the persistent kernels launch at most one workgroup per CU

PCase = collections.namedtuple("PCase", "name entry cin cout k sizes n x dens blo bhi boff gnin kernel data why")


def _p(name, entry, cin, cout, k, sizes, n, x, dens, brange, kernel, why, boff=0, gnin=False, data=None):
    return PCase(name, entry, cin, cout, k, list(sizes), n, x, dens, brange[0], brange[1], boff, gnin, kernel, data or name, why)


TOWER = [(40, 72), (17, 33), (8, 8), (1, 1)]
# 9 tiles of 8 x 32 per image on 410 pixels: at N = 29, 261 tiles -- more than CUs, so the persistent kernels give a workgroup two
# tiles (131 workgroups; tile t and tile t + 131 lie in different images, mostly in different segments) -- at the cost of
# ~12 000 reference pixels
RAGGED = [(9, 33), (1, 33), (8, 8), (3, 5), (1, 1)]
N_MULTI = 29
# entry: "generic" dafne_conv2d_nhwc_bf16_hip, "rp" dafne_conv3x3_c256_hip (both MFMA forms), "pair" dafne_conv3x3_c256_pair_hip,
# "fp8" dafne_conv2d_nhwc_fp8w_hip.  The generic entry point sends a layer to conv3x3_patch only from 200 tiles of 8 x 32 per
# nominal batch of 8 on (or with GN_INPUT): the patch cases are the smallest level sets that get there.
PRODUCERS = [
    _p("igemm2222", "generic", 256, 256, 3, [(10, 14)], 2, 2, 16, (-8, 8), IG2, "two ragged 128-pixel tiles per image"),
    _p("igemm4224", "generic", 320, 256, 1, [(113, 143)], 2, 1, 8, (-4, 4), IG3,
       "64 tiles of 256 pixels per image (512 per nominal batch: the fewest the dispatch sends there), ragged last tile, odd sizes"),
    _p("igemm1422", "generic", 128, 64, 3, [(13, 21)], 2, 2, 16, (-8, 8), IG1, "8 groups: group < Cout / 8 masking"),
    _p("igemm1412", "generic", 128, 32, 3, [(13, 21)], 2, 2, 16, (-8, 8), IG0, "4 groups"),
    _p("patch-levels", "generic", 256, 256, 3, [(44, 72), (17, 33), (8, 8), (1, 1)], 2, 2, 16, (-8, 8), PATCH,
       "ragged 8 x 32 tiles both ways, tile0 across segments, a one-pixel level (44 rows, not 40: 26 tiles per image, 208 >= 200)"),
    _p("patch-512", "generic", 64, 512, 3, [(40, 72), (3, 5)], 2, 2, 8, (-8, 8), PATCH,
       "64 groups: two channel tiles write one partial row; second group round of gn_finalize_kernel"),
    _p("patch-112tiles", "generic", 64, 256, 3, [(128, 200)], 1, 1, 8, (-2, 2), PATCH,
       "112 tiles per image: the 4-deep loop of gn_finalize_kernel (taken above 96)"),
    _p("patch-45tiles", "generic", 256, 256, 3, [(72, 136)], 1, 1, 32, (-2, 2), PATCH,
       "45 tiles per image: a slice of the finalisation sums more than one tile"),
    _p("patch-largemean", "generic", 256, 256, 3, [(8, 8), (3, 5)], 2, 1, 64, (-4, 4), PATCH,
       "|mean| >= 8 std: var = E[y^2] - mean^2 cancels; small levels reach the patch kernel through its GN_INPUT form (identity "
       "statistics: the operand is relu(x))", boff=48, gnin=True),
    _p("rp-levels", "rp", 256, 256, 3, TOWER, 3, 2, 16, (-8, 8), RP, "the tower levels: one tile per workgroup"),
    _p("rp-multi", "rp", 256, 256, 3, RAGGED, N_MULTI, 2, 16, (-8, 8), RP,
       "261 tiles: two per workgroup -- the per-tile partial row and the F_GNFIN ticket across a workgroup's tiles, which lie in "
       "different (segment, image) pairs"),
    _p("rp-45tiles", "rp", 256, 256, 3, [(72, 136)], 1, 1, 32, (-2, 2), RP, "45 tiles per image", data="patch-45tiles"),
    _p("rp-largemean", "rp", 256, 256, 3, [(8, 8), (3, 5)], 3, 1, 64, (-4, 4), RP, "|mean| >= 8 std", boff=48),
    _p("rp-pair", "pair", 256, 256, 3, TOWER, 3, 2, 16, (-8, 8), RP, "two layers in one launch: each half's partials and statistics in its own buffers"),
    _p("fp8-levels", "fp8", 256, 256, 3, TOWER, 3, 2, 16, (-8, 8), FP8,
       "in_qscale 1: integers up to 2 and weights +-1 are e4m3 values, the outputs are the same integers", data="rp-levels"),
]
P_BY_NAME = {c.name: c for c in PRODUCERS}
TPI_FLOOR = {"patch-112tiles": 97, "patch-45tiles": 33, "rp-45tiles": 33}       # tiles per image the case is there for
MULTI_TILE = ("rp-multi", "on-rp-multi", "on-pred16")       # more tiles than CUs: a workgroup of the persistent grid takes two
LARGE_MEAN = ("patch-largemean", "rp-largemean")

CCase = collections.namedtuple("CCase", "name entry cin cout sizes n dens f32 kernel data why")
LEVELS5 = [(40, 72), (17, 33), (8, 8), (3, 5), (1, 1)]
LEVELS4 = LEVELS5[1:]
CONSUMERS = [
    CCase("on-patch", "generic", 256, 256, LEVELS5, 3, 8, False, PATCH, "on-patch", "GN_INPUT of conv3x3_patch (kernel id 6)"),
    CCase("on-rp", "rp", 256, 256, LEVELS5, 3, 8, False, RP, "on-patch", "scale / shift form a x + b, one tile per workgroup"),
    CCase("on-rp-multi", "rp", 256, 256, RAGGED, N_MULTI, 8, False, RP, "on-rp-multi",
          "261 tiles: two per workgroup, which changes (segment, image) between them -- the double-buffered statistics table and the "
          "prefetch of the next tile's statistics and patch"),
    CCase("on-rp-pair", "pair", 256, 256, LEVELS5, 3, 8, False, RP, "on-patch", "each half reads its own statistics"),
    CCase("on-slab128", "generic", 128, 32, LEVELS4, 3, 8, True, SLAB, "on-slab128", "two slabs, the whole 32-channel tile"),
    CCase("on-slab64", "generic", 64, 7, LEVELS4, 3, 8, True, SLAB, "on-slab64", "one slab, masked channels"),
    CCase("on-pred16", "generic", 256, 15, [(88, 256)] + LEVELS4, 3, 8, True, PRED16, "on-pred16",
          "291 tiles on 256 CUs: two per workgroup of the persistent grid"),
]
C_BY_NAME = {c.name: c for c in CONSUMERS}
GAMMAS = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0)
QUANTUM = 2.0 ** -5                      # (int / 8) * (int / 4) + int / 16: every operand is a multiple of 2^-5


# ------------------------------------------------------------------------------------------------------------ producers
def zero_group(case, half=0):
    return zlib.crc32(("zero %s/%d" % (case.data, half)).encode()) % (case.cout // 8)


def producer_data(case, half=0):
    """-> xs [N,H,W,Cin] per level, w [Cout,Cin,k,k], bias [Cout]: fp32 tensors on the CPU holding integers."""
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%d" % (case.data, half)).encode()))
    xs = [_ints((case.n, h, w, case.cin), case.x, g) for h, w in case.sizes]
    r = torch.randint(0, 2 * case.dens, (case.cout, case.cin, case.k, case.k), generator=g)
    w = torch.where(r == 0, 1.0, torch.where(r == 1, -1.0, 0.0))
    b = case.boff + torch.randint(case.blo, case.bhi + 1, (case.cout,), generator=g).float()
    z = zero_group(case, half)
    w[8 * z:8 * z + 8] = 0
    b[8 * z:8 * z + 8] = b[8 * z]
    return xs, w, b


@functools.lru_cache(maxsize=None)
def _producer_reference(data, half):
    case = next(c for c in PRODUCERS if c.data == data)
    xs, w, b = producer_data(case, half)
    ys = []
    for x in xs:
        ys.append(torch.stack([ref_conv_image(x[n].clamp_min(0) if case.gnin else x[n], w, b, case.k, 1) for n in range(case.n)]))
    return xs, w, b, ys


def producer_reference(case, half=0):
    """-> xs, w, bias, ys: ys [N,H,W,Cout] double per level, the fp64 convolution with bias before any rounding.  Computed once
    per data set; nobody writes to it."""
    return _producer_reference(case.data, half)


def group_sums(y):
    """y [N,H,W,C] double -> sum y, sum y^2, sum |y| per (image, group): [N, C/8] double each."""
    n, c = y.shape[0], y.shape[-1]
    grp = y.reshape(n, -1, c // 8, 8)
    return grp.sum((1, 3)), (grp * grp).sum((1, 3)), grp.abs().sum((1, 3))


def rstd_bound(e2, var):
    """The bound on |rstd / rstd64 - 1| per group.  With exact partial sums a = sum y and b = sum y^2 are exact in the kernel, so
    var = b / cnt - mean^2 carries at most the roundings of b / cnt, mean^2 (mean itself rounded) and the subtraction:
    |d var| <= 5 * 2^-24 * E[y^2] < 2^-21 E[y^2]; rstd = (var + eps)^-1/2 moves by half of that relatively to var + eps; 2^-21
    covers rsqrtf and the final rounding."""
    return 2.0 ** -22 * e2 / (var + EPS) + 2.0 ** -21


def stats64(y):
    """-> mean, rstd, bound (rstd_bound) per (image, group), double, from the fp64 map."""
    s1, s2, _ = group_sums(y)
    cnt = float(y.shape[1] * y.shape[2] * 8)
    mean, e2 = s1 / cnt, s2 / cnt
    var = e2 - mean * mean
    return mean, 1.0 / torch.sqrt(var + EPS), rstd_bound(e2, var)


def stats32_emulated(y):
    """gn_finalize_kernel's formula step by step in fp32 (numpy: every operation rounded once) from the exact sums."""
    s1, s2, _ = group_sums(y)
    a, b = s1.numpy().astype(np.float32), s2.numpy().astype(np.float32)
    assert np.array_equal(a.astype(np.float64), s1.numpy()) and np.array_equal(b.astype(np.float64), s2.numpy())
    cnt = np.float32(y.shape[1] * y.shape[2] * 8)
    mean = a / cnt
    var = np.maximum(b / cnt - mean * mean, np.float32(0))
    rstd = (np.float32(1) / np.sqrt((var + np.float32(EPS)).astype(np.float64))).astype(np.float32)
    return mean, rstd


def check_mean_rstd(mean, rstd, y, what):
    """mean, rstd [N, G] (fp32 values in numpy / torch) against the fp64 reference of the map y: mean within one fp32 ulp of
    float32(sum y / cnt), rstd within rstd_bound."""
    m64, r64, bound = stats64(y)
    mean, rstd = np.asarray(mean, dtype=np.float64), np.asarray(rstd, dtype=np.float64)
    assert np.isfinite(mean).all() and np.isfinite(rstd).all(), what
    m32 = m64.numpy().astype(np.float32)
    dm = np.abs(mean - m32.astype(np.float64))
    assert (dm <= np.spacing(np.abs(m32)).astype(np.float64)).all(), (what, "mean", float(dm.max()))
    rel = np.abs(rstd / r64.numpy() - 1.0)
    assert (rel <= bound.numpy()).all(), (what, "rstd", float((rel / bound.numpy()).max()))
    return float((rel / bound.numpy()).max())


# ------------------------------------------------------------------------------------------------------------ consumers
def consumer_data(case, half=0):
    """-> xs [N,H,W,Cin] per level (integers), stats [levels,N,Cin/8,2] (mean, rstd), gamma, beta [Cin], w [Cout,Cin,3,3], bias."""
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%d" % (case.data, half)).encode()))
    xs = [_ints((case.n, h, w, case.cin), 12, g) for h, w in case.sizes]
    shape = (len(case.sizes), case.n, case.cin // 8)
    stats = torch.stack([torch.randint(-6, 2, shape, generator=g).float(),
                         torch.exp2(-torch.randint(1, 4, shape, generator=g).float())], -1)
    gamma = torch.tensor(GAMMAS)[torch.randint(0, len(GAMMAS), (case.cin,), generator=g)]
    beta = torch.randint(-16, 65, (case.cin,), generator=g).float() / 16
    r = torch.randint(0, 2 * case.dens, (case.cout, case.cin, 3, 3), generator=g)
    w = torch.where(r == 0, 1.0, torch.where(r == 1, -1.0, 0.0))
    b = torch.randint(-8, 9, (case.cout,), generator=g).float()
    return xs, stats, gamma, beta, w, b


def normalised(x, stats_s, gamma, beta):
    """relu((x - mean) rstd gamma + beta) of one level in fp64: x [N,H,W,C], stats_s [N,C/8,2] -> [N,H,W,C] double (exact)."""
    n, h, w, c = x.shape
    mean = stats_s[..., 0].double().repeat_interleave(8, 1).reshape(n, 1, 1, c)
    rstd = stats_s[..., 1].double().repeat_interleave(8, 1).reshape(n, 1, 1, c)
    return ((x.double() - mean) * rstd * gamma.double() + beta.double()).clamp_min(0)


@functools.lru_cache(maxsize=None)
def _consumer_reference(data, half):
    case = next(c for c in CONSUMERS if c.data == data)
    xs, stats, gamma, beta, w, b = consumer_data(case, half)
    ops, ys = [], []
    for s, x in enumerate(xs):
        op = normalised(x, stats[s], gamma, beta)
        assert torch.equal(op.float().double(), op)                 # exact in fp32: .to(bf16) below is the only rounding
        op = op.float().to(BF).double()
        ops.append(op)
        ys.append(torch.stack([ref_conv_image(op[n], w, b, 3, 1) for n in range(case.n)]))
    return xs, stats, gamma, beta, w, b, ops, ys


def consumer_reference(case, half=0):
    """-> xs, stats, gamma, beta, w, bias, ops, ys: ops the bf16-rounded operand per level (double), ys its fp64 convolution."""
    return _consumer_reference(case.data, half)


# ------------------------------------------------------------------------------------------------------------ probing
def probe_entry(entry, cin, cout, k, sizes, n, bits):
    """(kernel name or None, tiles, message) of a launch through one of the entry points, from the library alone (dummy
    pointers: nothing is dereferenced on the host)."""
    from dafne_amd import _lib
    from dafne_amd.engine import ConvCall
    L = _lib.load()
    dummy = 0x1000
    on = lambda bit: dummy if bits & bit else None
    prm = _lib.ConvParams(n, len(sizes), cin, cout, k, k, 1, k // 2, bits, dummy, dummy, on(F_GN), on(F_GNIN), on(F_GNIN), on(F_GNIN),
                          on(F_GNFIN), on(F_GNFIN), EPS if bits & F_GNFIN else 0.0)
    segs = (_lib.ConvSeg * len(sizes))()
    for i, (h, w) in enumerate(sizes):
        segs[i] = _lib.ConvSeg(dummy, dummy, None, h, w, h, w)
    if entry == "generic":
        kid = L.dafne_conv2d_kernel_id(ctypes.byref(prm), segs)
        msg = L.dafne_last_error().decode(errors="replace") if kid < 0 else ""
        return (ConvCall.KERNEL_NAMES[kid] if kid >= 0 else None), L.dafne_conv2d_num_tiles(ctypes.byref(prm), segs), msg
    if entry == "fp8":
        tiles = L.dafne_conv2d_fp8w_num_tiles(ctypes.byref(prm), segs)
        msg = L.dafne_last_error().decode(errors="replace") if tiles < 0 else ""
        return (FP8 if tiles > 0 else None), tiles, msg
    ok = L.dafne_conv3x3_c256_ok(ctypes.byref(prm), segs)
    msg = L.dafne_last_error().decode(errors="replace") if not ok else ""
    return (RP if ok else None), L.dafne_conv3x3_c256_num_tiles(ctypes.byref(prm), segs), msg


def takes_fused_finalize(case):
    """F_GNFIN: the 3x3 patch kernels (bf16, resident-patch, fp8) with Cout == 256."""
    return case.kernel in (PATCH, RP, FP8) and case.cout == 256


@pytest.fixture(scope="module")
def built():
    from dafne_amd import build
    assert not [k for k in os.environ if k.startswith(("DAFNE_CONV_", "DAFNE_WS_"))], "this module tests the default dispatch"
    return build.build()


@pytest.mark.parametrize("case", PRODUCERS, ids=[c.name for c in PRODUCERS])
def test_producer_case_runs_on_the_kernel_it_names(built, case):
    assert case.why and len(set(c.name for c in PRODUCERS)) == len(PRODUCERS)
    bits = F_GN | (F_GNIN if case.gnin else 0)
    name, tiles, msg = probe_entry(case.entry, case.cin, case.cout, case.k, case.sizes, case.n, bits)
    assert name == case.kernel, (case.name, "now runs on", name, msg)
    assert tiles > 0
    if case.name in TPI_FLOOR:
        assert tiles // case.n >= TPI_FLOOR[case.name]
    if case.kernel == RP:                # persistent: one workgroup per CU at most
        assert (tiles * len(_halves(case)) > MI355X_CUS) == (case.name in MULTI_TILE)
    if takes_fused_finalize(case):
        name, tiles_f, msg = probe_entry(case.entry, case.cin, case.cout, case.k, case.sizes, case.n, bits | F_GNFIN)
        assert name == case.kernel and tiles_f == tiles, msg


def test_fused_finalize_is_refused_off_the_256_channel_patch_kernels(built):
    """GN_FINALIZE reduces 32 groups: Cout = 512 on the patch kernels and every other kernel refuse the flag."""
    for name in ("patch-512", "igemm2222", "igemm1422"):
        case = P_BY_NAME[name]
        assert not takes_fused_finalize(case)
        kernel, tiles, msg = probe_entry(case.entry, case.cin, case.cout, case.k, case.sizes, case.n, F_GN | F_GNFIN)
        assert kernel is None and tiles == -1 and "GN_FINALIZE needs" in msg, (name, msg)
    for entry in ("rp", "fp8"):
        kernel, _, msg = probe_entry(entry, 256, 512, 3, TOWER, 3, F_GN | F_GNFIN)
        assert kernel is None and "GN_FINALIZE needs" in msg, (entry, msg)
        assert probe_entry(entry, 256, 512, 3, TOWER, 3, F_GN)[0] is not None


@pytest.mark.parametrize("case", CONSUMERS, ids=[c.name for c in CONSUMERS])
def test_consumer_case_runs_on_the_kernel_it_names(built, case):
    assert case.why
    bits = F_GNIN | (F_F32 if case.f32 else 0)
    name, tiles, msg = probe_entry(case.entry, case.cin, case.cout, 3, case.sizes, case.n, bits)
    assert name == case.kernel, (case.name, "now runs on", name, msg)
    assert tiles == sum(case.n * ((h + 7) // 8) * ((w + 31) // 32) for h, w in case.sizes)
    assert case.kernel != PRED16 or case.name in MULTI_TILE
    if case.kernel in (RP, PRED16):      # persistent: one workgroup per CU at most
        assert (tiles * len(_halves(case)) > MI355X_CUS) == (case.name in MULTI_TILE)


def _halves(case):
    return (0, 1) if case.entry == "pair" else (0,)


@pytest.mark.parametrize("case", PRODUCERS, ids=[c.name for c in PRODUCERS])
def test_producer_data_is_exact_and_the_rstd_bound_holds_for_fp32(case):
    for half in _halves(case):
        xs, w, b, ys = producer_reference(case, half)
        g = case.cout // 8
        z = zero_group(case, half)
        assert float(w[8 * z:8 * z + 8].abs().max()) == 0 and len(set(b[8 * z:8 * z + 8].tolist())) == 1
        assert len(set(tuple(r) for r in b.reshape(g, 8).tolist())) > 1               # the bias differs between groups
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and torch.equal(b, b.round())
        for x, y in zip(xs, ys):
            assert float(x.abs().max()) <= case.x <= 2 and torch.equal(x, x.round())
            s1, s2, sa = group_sums(y)
            assert torch.equal(y, y.round()) and float(y.abs().max()) <= 256, (case.name, float(y.abs().max()))
            assert float(sa.max()) < 2 ** 24 and float(s2.max()) < 2 ** 24, (case.name, float(sa.max()), float(s2.max()))
            mean, rstd = stats32_emulated(y)
            worst = check_mean_rstd(mean, rstd, y, case.name)
            assert worst <= 1.0
            m64, r64, _ = stats64(y)
            assert float(m64[:, z].sub(float(b[8 * z])).abs().max()) == 0             # the zero-variance group: mean = bias,
            assert np.array_equal(mean[:, z], np.full(case.n, float(b[8 * z]), np.float32))
            assert float((r64[:, z] * EPS ** 0.5 - 1).abs().max()) < 1e-12            # rstd = eps^-1/2
            if case.name in LARGE_MEAN:
                var = (1.0 / (r64 * r64) - EPS).clamp_min(0)
                big = m64.abs() >= 8 * var.sqrt()
                assert float(big.float().mean()) > 0.9, (case.name, float(big.float().mean()))


def test_rstd_bound_is_the_derived_one():
    """The bound is 2^-22 E[y^2] / (var + eps) + 2^-21, nothing measured: fixed points."""
    assert rstd_bound(torch.tensor(1.0, dtype=torch.float64), torch.tensor(1.0, dtype=torch.float64)).item() == 2.0 ** -22 / (1.0 + EPS) + 2.0 ** -21
    assert rstd_bound(torch.tensor(0.0, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)).item() == 2.0 ** -21
    assert abs(rstd_bound(torch.tensor(3200.0, dtype=torch.float64), torch.tensor(25.0, dtype=torch.float64)).item() / (2.0 ** -22 * 128 + 2.0 ** -21) - 1) < 1e-6


@pytest.mark.parametrize("case", CONSUMERS, ids=[c.name for c in CONSUMERS])
def test_consumer_data_is_exact(case):
    for half in _halves(case):
        xs, stats, gamma, beta, w, b, ops, ys = consumer_reference(case, half)
        mean, rstd = stats[..., 0], stats[..., 1]
        assert torch.equal(mean, mean.round()) and set(rstd.unique().tolist()) == {0.125, 0.25, 0.5}
        assert set(gamma.tolist()) <= set(GAMMAS) and torch.equal(beta * 16, (beta * 16).round()) and float(beta.abs().max()) <= 4
        assert torch.equal(b, b.round())
        # statistics differ between any two (segment, image) pairs and between neighbouring groups: a read from the wrong
        # place changes the operand
        flat = stats.reshape(-1, case.cin // 8, 2)
        for i in range(flat.shape[0]):
            for j in range(i):
                assert not torch.equal(flat[i], flat[j])
        assert float((flat[:, 1:] != flat[:, :-1]).any(-1).float().mean()) > 0.8
        # what a zero-padding pixel would become if it were normalised: positive in most channels of every (segment, image)
        pad = beta.reshape(1, 1, -1) - (mean * rstd).repeat_interleave(8, 2) * gamma.reshape(1, 1, -1)
        assert float((pad > 0).float().mean()) > 0.75 and bool(((pad > 0).float().mean(-1) > 0.5).all())
        wsum = float(w.abs().sum((1, 2, 3)).max())
        for x, op, y in zip(xs, ops, ys):
            assert float(x.abs().max()) <= 256 and torch.equal(x, x.round())
            q = op / QUANTUM
            assert torch.equal(q, q.round())
            assert wsum * float(q.max()) < 2 ** 24                  # sum |w| |operand| / quantum of any output
            assert float(y.abs().max()) / QUANTUM < 2 ** 24
