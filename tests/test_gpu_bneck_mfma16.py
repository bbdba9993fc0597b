"""GPU: conv_bneck_kernel's 16x16x32 form (dafne_bottleneck_body16_hip, weights engine.pack_bneck16) against the 32x32x16 form
(dafne_bottleneck_body_hip, bit-identical to the separate launches: tests/test_gpu_conv.py) and against torch.

The new form sums the same products in another order (32 k per instruction), so an output may land one bf16 ulp away.  The three
GEMM sites are looked at ONE AT A TIME: identity weights pass values through exactly in either instruction's order, so with

    random W2, W3 = [I; 0; 0; 0], zero shortcut, zero bias3      Y[:, :256] IS T          (phase A, the 3x3)
    centre-tap-identity W2, random W3, a selecting W1'           T = relu(U) exactly; Y    (G1 + the epilogue), Z = picked rows of Y
    identity W2 and W3, random W1'                               Y exact; Z                (G2a / G2b)

a difference can come from the one random matrix only.  Criterion and cap: test_gpu_conv._same_conv_output, the ones the towers'
16x16x32 form is held to (at most one bf16 ulp, on fewer than 2 per mille of the outputs), applied to the exposed outputs' interior.
Shapes: the smallest at which the kernel can go wrong -- one full tile, a ragged one in both directions, several tiles of two images --
at both tile heights, with and without the next block's head, and in place (Y over X).
Reference block: detectron2 BottleneckBlock [recalled], res4 of build_dafne_resnet_fpn_backbone."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import _same_conv_output, bfr, close_bf16, dev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 32), (1, 5, 33), (2, 6, 64)]       # one full tile | ragged in both directions | several tiles, two images
CAP = 2e-3                                          # _same_conv_output's cap on the share of outputs that differ


def _eye_w2():
    w = torch.zeros(256, 256, 3, 3)
    w[torch.arange(256), torch.arange(256), 1, 1] = 1.0
    return w


def _eye_w3():
    w = torch.zeros(1024, 256, 1, 1)
    w[torch.arange(256), torch.arange(256)] = 1.0
    return w


SEL = 4 * torch.arange(256) + 1                     # the selecting W1': Z channel o = Y channel 4 o + 1


def _sel_w1():
    w = torch.zeros(256, 1024, 1, 1)
    w[torch.arange(256), SEL] = 1.0
    return w


_CASES = {}


def _case(kind, N, H, W):
    """Seeded CPU operands of one case (shared by the tests that need them, never modified): u, x, (w2, b2), (w3, b3), (w1, b1)."""
    key = (kind, N, H, W)
    if key not in _CASES:
        g = torch.Generator().manual_seed(4100 + 7 * H * W + len(kind))
        u = bfr(torch.randn(N, 256, H, W, generator=g))
        x = bfr(torch.randn(N, 1024, H, W, generator=g))
        w2 = bfr(torch.randn(256, 256, 3, 3, generator=g) / 48.0)
        b2 = torch.randn(256, generator=g) * 0.2
        w3 = bfr(torch.randn(1024, 256, 1, 1, generator=g) / 16.0)
        b3 = torch.randn(1024, generator=g) * 0.2
        w1 = bfr(torch.randn(256, 1024, 1, 1, generator=g) / 32.0)
        b1 = torch.randn(256, generator=g) * 0.2
        z256, z1024 = torch.zeros(256), torch.zeros(1024)
        if kind == "T":
            x, w3, b3, w1, b1 = torch.zeros_like(x), _eye_w3(), z1024, _sel_w1(), z256
        elif kind == "Y":
            w2, b2, w1, b1 = _eye_w2(), z256, _sel_w1(), z256
        elif kind == "Z":
            w2, b2, w3, b3 = _eye_w2(), z256, _eye_w3(), z1024
        else:
            assert kind == "all"
        _CASES[key] = (u, x, (w2, b2), (w3, b3), (w1, b1))
    return _CASES[key]


def _dominated_share(inp, w, b, res, pad):
    """CPU: the share of the outputs of relu(conv(inp, w) + b + res) that are positive and cancellation-dominated.  The partial sums
    of an output are of the size R = sqrt(sum of its squared terms) (a random walk), and each of the <= K / 16 fp32 accumulator
    roundings of either form moves the result by at most 2^-24 of a partial sum: the two forms end about 2^-24 sqrt(K / 16) R <=
    2^-20.4 R apart (K <= 2304).  An output v >= 2^-12 R has a bf16 spacing of at least 2^-21 R, and the chance that the two fp32
    values straddle a rounding boundary falls as 1 / v from there; below it a difference is likelier than not."""
    v = F.conv2d(inp, w, b, padding=pad)
    r2 = F.conv2d(inp * inp, w * w, b * b, padding=pad)
    if res is not None:
        v, r2 = v + res, r2 + res * res
    dom = (v > 0) & (v < 2.0 ** -12 * r2.sqrt())
    return float(dom.float().mean())


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_seeded_inputs_keep_the_reference_clear_of_cancellation(N, H, W):
    """The cap on the share of differing outputs is a condition on the inputs as well: the exposed GEMM of every single-GEMM case has
    so few cancellation-dominated outputs that they could use up a quarter of the cap at most (a Gaussian output has about
    0.4 * 2^-12 = 1e-4 of its mass there; CPU arithmetic only, marked gpu with its module)."""
    u, x, (w2, b2), _, _ = _case("T", N, H, W)
    assert _dominated_share(u, w2, b2, None, 1) < CAP / 4
    u, x, _, (w3, b3), _ = _case("Y", N, H, W)
    assert _dominated_share(F.relu(u), w3, b3, x, 0) < CAP / 4
    u, x, _, _, (w1, b1) = _case("Z", N, H, W)
    t = torch.zeros_like(x)
    t[:, :256] = F.relu(u)
    assert _dominated_share(bfr(F.relu(t + x)), w1, b1, None, 0) < CAP / 4


class _Run:
    """Device operands of one case and the two entry points on them."""

    def __init__(self, kind, N, H, W):
        from dafne_amd import engine, _lib
        self.engine, self._lib, self.L = engine, _lib, _lib.load()
        self.N, self.H, self.W = N, H, W
        d = dev()
        u, x, (w2, b2), (w3, b3), (w1, b1) = _case(kind, N, H, W)
        self.ua, self.xa = engine.Act.from_nchw(u.to(d)), engine.Act.from_nchw(x.to(d))
        self.w2p, self.b2p = engine.pack_conv(w2, b2, d)
        self.w3p, self.b3p = engine.pack_conv(w3, b3, d)
        self.w1p, self.b1p = engine.pack_conv(w1, b1, d)
        self.wf32 = engine.pack_bneck(self.w2p, self.w3p, self.w1p)
        self.wf16 = engine.pack_bneck16(self.w2p, self.w3p, self.w1p)
        self.wf16_nohead = engine.pack_bneck16(self.w2p, self.w3p, torch.zeros_like(self.w1p))
        assert self.wf16.shape == self.wf32.shape and not torch.equal(self.wf16, self.wf32)
        self.nscr = self.L.dafne_bottleneck_body_scratch_bytes()
        self.scr = torch.empty(self.nscr, dtype=torch.uint8, device=d)

    def outputs(self):
        d = dev()
        return self.engine.Act(self.N, self.H, self.W, 1024, d), self.engine.Act(self.N, self.H, self.W, 256, d)

    def call(self, m16, y_t, z_t, wf=None, res_t=None, stream=None):
        _lib = self._lib
        fn = self.L.dafne_bottleneck_body16_hip if m16 else self.L.dafne_bottleneck_body_hip
        wf = wf if wf is not None else (self.wf16 if m16 else self.wf32)
        head = z_t is not None
        _lib.check(fn(_lib.ptr(self.ua.t), _lib.ptr(res_t if res_t is not None else self.xa.t), _lib.ptr(wf), _lib.ptr(self.b2p),
                      _lib.ptr(self.b3p), _lib.ptr(self.b1p) if head else None, self.N, self.H, self.W, _lib.ptr(y_t),
                      _lib.ptr(z_t) if head else None, _lib.ptr(self.scr), self.nscr, stream if stream is not None else _lib.current_stream()),
                   "bneck16" if m16 else "bneck")


def _interior(t):
    return t[:, 1:-1, 1:-1]


def _halo_is_zero(t):
    return (float(t[:, 0].abs().max()) == 0 and float(t[:, -1].abs().max()) == 0 and float(t[:, :, 0].abs().max()) == 0
            and float(t[:, :, -1].abs().max()) == 0)


def _all_forms(r):
    """The 16x16x32 entry with the head (twice: the second launch finds LDS dirty), without it and in place: the three agree bit for
    bit, write nothing else -> (y16, z16, y32, z32)."""
    y32, z32 = r.outputs()
    r.call(False, y32.t, z32.t)
    y16, z16 = r.outputs()
    for _ in range(2):
        r.call(True, y16.t, z16.t)
    torch.cuda.synchronize()
    assert _halo_is_zero(y16.t) and _halo_is_zero(z16.t)
    # no head: d_next NULL, a zero conv1' section
    y_nh, z_nh = r.outputs()
    z_nh.t.fill_(5.0)
    r.call(True, y_nh.t, None, wf=r.wf16_nohead)
    torch.cuda.synchronize()
    assert torch.equal(y_nh.t, y16.t) and bool((z_nh.t == 5.0).all())
    # in place: Y over X
    x_ip = r.xa.t.clone()
    _, z_ip = r.outputs()
    r.call(True, x_ip, z_ip.t, res_t=x_ip)
    torch.cuda.synchronize()
    assert torch.equal(x_ip, y16.t) and torch.equal(z_ip.t, z16.t)
    return y16, z16, y32, z32


@pytest.fixture(params=[4, 2], ids=["th4", "th2"])
def th(request, monkeypatch):
    monkeypatch.setenv("DAFNE_BNECK_TH", str(request.param))
    return request.param


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_phase_a_alone(N, H, W, th):
    """Random W2 behind identity W3 and a zero shortcut: Y's first 256 channels are T."""
    y16, z16, y32, z32 = _all_forms(_Run("T", N, H, W))
    _same_conv_output(_interior(y16.t)[..., :256], _interior(y32.t)[..., :256], True)
    assert float(y16.t[..., 256:].abs().max()) == 0 and float(_interior(y16.t)[..., :256].abs().max()) > 0
    assert torch.equal(z16.t, y16.t[..., SEL.to(dev())])


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_conv3_and_shortcut_alone(N, H, W, th):
    """T = relu(U) exactly, random W3 and shortcut: Y; the selecting W1' shows the Y chunks that conv1' reads from LDS."""
    y16, z16, y32, z32 = _all_forms(_Run("Y", N, H, W))
    _same_conv_output(_interior(y16.t), _interior(y32.t), True)
    assert float(y16.t.abs().max()) > 0
    assert torch.equal(z16.t, y16.t[..., SEL.to(dev())])


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_next_conv1_alone(N, H, W, th):
    """Identity W2 and W3: Y = relu(T + X) in both forms bit for bit; random W1': Z."""
    y16, z16, y32, z32 = _all_forms(_Run("Z", N, H, W))
    assert torch.equal(y16.t, y32.t)
    _same_conv_output(_interior(z16.t), _interior(z32.t), True)
    assert float(z16.t.abs().max()) > 0


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_all_random_vs_torch(N, H, W, th):
    """All three matrices random: Y and Z against torch fp32, within test_gpu_conv.close_bf16's bound.  That bound is one layer's
    (fp32 summation order + the bf16 rounding of its output), so Z's reference is torch's conv1' on the Y the kernel stored, as
    test_bottleneck_body_fused_equals_three_convs takes Y's from the stored T: on torch's own Y, the 1-ulp roundings of a few dozen of
    an output's 1024 inputs add up to a third ulp-sized term (first form of this test: 4 of 196 608 Z values 2^-7 off at 2 x 6 x 64).
    T never leaves the chip: Y's reference runs on torch's T, two layers in one bound, which holds."""
    y16, z16, y32, z32 = _all_forms(_Run("all", N, H, W))
    u, x, (w2, b2), (w3, b3), (w1, b1) = _case("all", N, H, W)
    t_ref = bfr(F.relu(F.conv2d(u, w2, b2, padding=1)))
    y_ref = bfr(F.relu(F.conv2d(t_ref, w3, b3) + x))
    y_got = y16.nchw_float().cpu()
    z_ref = bfr(F.relu(F.conv2d(y_got, w1, b1)))
    close_bf16(y_got, y_ref)
    close_bf16(z16.nchw_float().cpu(), z_ref)


def test_run_to_run_identity_beside_memory_traffic(th):
    """50 launches of the 2 x 6 x 64 case beside 256-MB device copies on two other streams (the disturbance of
    tests/test_gpu_reproducible.py::test_bottleneck_beside_memory_traffic: the waves of a workgroup drift apart by whole steps):
    the bits of the idle GPU every time."""
    r = _Run("all", 2, 6, 64)
    d = dev()
    ms = torch.cuda.Stream(device=d, priority=-1)
    side = [torch.cuda.Stream(device=d, priority=-1) for _ in range(2)]
    big = [torch.empty(64 << 20, dtype=torch.float32, device=d) for _ in range(4)]
    y, z = r.outputs()

    def run():
        r.call(True, y.t, z.t, stream=ctypes.c_void_p(ms.cuda_stream))
        with torch.cuda.stream(ms):
            return y.t.clone(), z.t.clone()
    torch.cuda.synchronize()
    ref = run()
    torch.cuda.synchronize()
    bad = n = 0
    for _ in range(10):
        for k, s in enumerate(side):
            with torch.cuda.stream(s):
                for _ in range(3):
                    big[2 * k].copy_(big[2 * k + 1])
        pend = [run() for _ in range(5)]
        torch.cuda.synchronize()
        for yy, zz in pend:
            n += 1
            bad += 0 if (torch.equal(yy, ref[0]) and torch.equal(zz, ref[1])) else 1
    assert n == 50 and bad == 0, "%d of %d launches of conv_bneck's 16x16x32 form (tile height %d) differ from the idle result" % (bad, n, th)


def test_model_runs_one_form_at_any_batch_size_and_layout(monkeypatch):
    """R101 at 64 x 64: every res4 block of every plan runs the 16x16x32 entry (EngineOptions.rp_mfma16, fixed when the weights are
    packed), an image gets the same detections alone and in a batch of 3, and serial == pipelined."""
    for name in ("DAFNE_RP_MFMA16", "DAFNE_BNECK_TH", "DAFNE_FUSE_BNECK", "DAFNE_FUSE_B2B", "DAFNE_FUSE_BNECK_LAST"):
        monkeypatch.delenv(name, raising=False)
    from test_gpu_model import build
    cfg, m, P = build("dota-1.0_r101.yaml", seed=31)
    g = torch.Generator().manual_seed(8)
    b3 = torch.randint(0, 256, (3, 3, 64, 64), generator=g, dtype=torch.uint8).to(dev())
    r3, c3 = m.detect_packed(b3)
    torch.cuda.synchronize()
    r3, c3 = r3.clone(), c3.clone()
    for i in range(3):
        r1, c1 = m.detect_packed(b3[i:i + 1].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(c1, c3[i:i + 1]) and torch.equal(r1[0, :int(c1[0])], r3[i, :int(c3[i])]), i
    rp, cp = m.detect_packed(b3, pipelined=True, splits=2)
    torch.cuda.synchronize()
    assert torch.equal(cp, c3) and all(torch.equal(rp[i, :int(c3[i])], r3[i, :int(c3[i])]) for i in range(3))
    for n in (1, 3):
        body = [c for c in m.plan(n, 64, 64).calls if c.kernel_name() in ("conv_bneck", "conv_bneck_last")]
        assert len(body) == 23 and all(c.fn.__name__ == "dafne_bottleneck_body16_hip" for c in body), n
