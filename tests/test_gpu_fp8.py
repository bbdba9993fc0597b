"""GPU parity of the fp8 (OCP e4m3) convolution path -- BASELINE config 5, dafne_conv2d_nhwc_fp8w_hip.

The reference has no fp8 path, so the definition lives here and in oracle/model.py (fp8=True): weights are e4m3 with
one power-of-two scale per output channel, the activation is multiplied by in_qscale, clamped to +-448 and rounded to
e4m3 (round to nearest even = torch.float8_e4m3fn), the products are accumulated in fp32.  An e4m3 x e4m3 product has
8 significant bits, so products are exact in fp32 and a torch fp32 convolution of the dequantised operands differs
from the kernel only by fp32 summation order and the final bf16 rounding: tolerance 2 bf16 ulps, as for the bf16 kernels.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import bfr, close_bf16, dev

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn


def q8(x, qscale=1.0):
    return (x * qscale).clamp(-448.0, 448.0).to(F8).float()


def run_fp8(xs, w, b, in_qscale, flags=0, gn_in=None, gn_stats=False, kernel=None,
            gn_fin=None, guard_rows=None, launches=1, after_launch=None):
    """xs: list of [N,C,H,W] float maps (levels sharing the weights).  Returns (outputs NCHW float on the CPU, partial, call).
    kernel: the kernel the call must land on (conv3x3_patch_fp8, the only fp8 kernel since round 6).
    gn_fin: (stats, counters, eps) -> flag F_GNFIN (the last tile of every image finalises the statistics of the output).
    guard_rows: the strict form of tests/test_gpu_groupnorm.py -- the partial buffer has num_tiles() + guard_rows rows and starts as
    NaN, like the interior of the outputs.  launches: how often the call runs into the same buffers; after_launch(call) runs
    after each of them (synchronised)."""
    from dafne_amd import engine, _lib
    d = dev()
    n, cin = xs[0].shape[:2]
    cout = w.shape[0]
    ins = [engine.Act.from_nchw(x.to(d)) for x in xs]
    outs = [engine.Act(n, x.shape[2], x.shape[3], cout, d) for x in xs]
    if guard_rows is not None:
        for o in outs:
            o.t[:, 1:-1, 1:-1, :] = float("nan")
    wq, wscale = engine.pack_conv_fp8(w, d)
    bias = b.float().to(d).contiguous()
    segs = [(i.t, o.t, None, i.h, i.w, i.h, i.w) for i, o in zip(ins, outs)]
    oscale = (wscale / in_qscale).contiguous()
    if gn_in is not None:
        flags |= engine.F_GNIN
    probe = engine.ConvCall(wq, bias, cin, cout, 3, 1, 1, flags, segs, n, gn_in=gn_in, fp8=(oscale, in_qscale))
    partial = None
    if gn_stats:
        if guard_rows is None:
            partial = torch.zeros(4096, cout // 8, 2, dtype=torch.float32, device=d)
        else:
            partial = torch.full((probe.num_tiles() + guard_rows, cout // 8, 2), float("nan"), dtype=torch.float32, device=d)
        flags |= engine.F_GN | (engine.F_GNFIN if gn_fin is not None else 0)
        probe = engine.ConvCall(wq, bias, cin, cout, 3, 1, 1, flags, segs, n,
                                gn_partial=partial, gn_in=gn_in, fp8=(oscale, in_qscale), gn_fin=gn_fin)
    assert probe.kernel_name() == (kernel or "conv3x3_patch_fp8")
    for _ in range(launches):
        probe(_lib.current_stream())
        torch.cuda.synchronize()
        if after_launch is not None:
            after_launch(probe)
    for o in outs:      # the halo must still be zero
        assert float(o.t[:, 0].abs().max()) == 0 and float(o.t[:, -1].abs().max()) == 0
        assert float(o.t[:, :, 0].abs().max()) == 0 and float(o.t[:, :, -1].abs().max()) == 0
    return [o.nchw_float().cpu() for o in outs], partial, probe


def test_e4m3_weight_quantiser_is_exact_in_bf16():
    from dafne_amd import engine
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 64, 3, 3, generator=g) * torch.logspace(-4, 1, 64)[:, None, None, None]
    w[7] = 0
    q, s, deq = engine.quantize_weight_e4m3(w)
    assert q.dtype == F8 and torch.equal(deq.to(torch.bfloat16).float(), deq)
    assert torch.equal(torch.exp2(torch.round(torch.log2(s))), s)               # powers of two
    assert float((q.float().abs().amax(dim=(1, 2, 3)))[torch.arange(64) != 7].min()) >= 224.0     # the range is used
    assert float((deq - w).abs().max() / w.abs().max()) < 2.0 ** -4


@pytest.fixture(params=["patch_fp8"])
def c256_kernel(request):
    """The kernel of the fp8 layers with 256 input channels: conv3x3_patch_fp8 (ENGINE.FP8_CONV3X3_KERNEL "patch").  Rounds 3-5 had a
    second one (conv3x3_rp8: faster alone, slower in the timed layout; removed in round 6), hence the fixture."""
    return "conv3x3_" + request.param


@pytest.fixture(params=["cfg_patch"])
def fp8_kernel_cfg(request):
    """The kernel choice as a model property: cfg.ENGINE.FP8_CONV3X3_KERNEL."""
    return {"cfg_patch": "patch"}[request.param]


@pytest.mark.parametrize("H,W,N,cout,relu,qs", [
    (64, 64, 5, 256, False, 1.0),            # FPN-output-like
    (40, 100, 3, 256, True, 4.0),            # ragged in both directions
    (33, 47, 3, 512, True, 0.5),             # two channel tiles, ragged rows and columns
    (3, 5, 7, 256, False, 16.0),             # a single ragged tile per image
    (128, 128, 2, 256, True, 2.0),           # more tiles than workgroups of the persistent grid: several rounds per workgroup
])
def test_fp8_c256_kernels_vs_torch(H, W, N, cout, relu, qs, c256_kernel):
    from dafne_amd import engine
    g = torch.Generator().manual_seed(cout + H + W)
    x = bfr(torch.randn(N, 256, H, W, generator=g) * 3.0)
    x[0, :, 0, 0] = 1000.0                    # saturates at 448 / qs
    x[0, :, -1, -1] = -1000.0
    w = torch.randn(cout, 256, 3, 3, generator=g) / (256 * 9) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    _, wscale, wdeq = engine.quantize_weight_e4m3(w)
    ref = F.conv2d(q8(x, qs), wdeq / qs, b, padding=1)
    if relu:
        ref = F.relu(ref)
    (got,), _, _ = run_fp8([x], w, b, qs, flags=engine.F_RELU if relu else 0, kernel=c256_kernel)
    close_bf16(got, bfr(ref))


@pytest.mark.parametrize("cin,cout,H,W,N,relu,qs", [
    (64, 256, 40, 100, 3, True, 4.0),        # one slab, ragged in both directions
    (128, 512, 33, 47, 3, True, 0.5),        # two channel tiles, two slabs, ragged rows and columns
    (320, 256, 24, 64, 6, False, 16.0),      # five slabs
    (512, 256, 9, 31, 2, True, 2.0),         # eight slabs, a single ragged tile per image
])
def test_fp8_patch_kernel_vs_torch(cin, cout, H, W, N, relu, qs):
    from dafne_amd import engine
    g = torch.Generator().manual_seed(cin + cout + H + W)
    x = bfr(torch.randn(N, cin, H, W, generator=g) * 3.0)
    x[0, :, 0, 0] = 1000.0                    # saturates at 448 / qs
    x[0, :, -1, -1] = -1000.0
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    _, wscale, wdeq = engine.quantize_weight_e4m3(w)
    ref = F.conv2d(q8(x, qs), wdeq / qs, b, padding=1)
    if relu:
        ref = F.relu(ref)
    (got,), _, _ = run_fp8([x], w, b, qs, flags=engine.F_RELU if relu else 0)
    close_bf16(got, bfr(ref))


def test_fp8_gn_input_chain_over_levels(c256_kernel):
    """Tower layer pair over three levels: layer 1 (bf16 patch kernel) emits the raw map + GroupNorm partial sums, the
    statistics are finalised, layer 2 is the fp8 kernel with GN_INPUT: GroupNorm + ReLU + e4m3 rounding while the patch
    is loaded, GroupNorm statistics of its own output.  The reference applies the same expression to the device's raw
    map and statistics."""
    from dafne_amd import engine, _lib
    d = dev()
    L = _lib.load()
    g = torch.Generator().manual_seed(78)
    C, N = 256, 4
    sizes = [(48, 104), (16, 32), (8, 8)]       # 24 + 2 + 1 tiles per image (the patch kernel takes >= 200 per nominal batch of 8)
    xs = [bfr(torch.randn(N, C, h, w, generator=g)) for h, w in sizes]
    w1 = bfr(torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5)
    w2 = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(d)
    beta = (0.3 * torch.randn(C, generator=g)).to(d)
    ins = [engine.Act.from_nchw(x.to(d)) for x in xs]
    wp1, bp1 = engine.pack_conv(w1, b1, d)
    st = _lib.current_stream()
    raw = [engine.Act(N, h, w, C, d) for h, w in sizes]
    segs = [(i.t, o.t, None, i.h, i.w, i.h, i.w) for i, o in zip(ins, raw)]
    partial = torch.zeros(4096, C // 8, 2, dtype=torch.float32, device=d)
    c1 = engine.ConvCall(wp1, bp1, C, C, 3, 1, 1, engine.F_GN, segs, N, gn_partial=partial)
    assert c1.kernel_name() == "conv3x3_patch"
    c1(st)
    stats = torch.zeros(len(raw), N, C // 8, 2, dtype=torch.float32, device=d)
    gsegs = (_lib.GnSeg * len(raw))()
    t0 = 0
    for k, (o, tpi) in enumerate(zip(raw, c1.tiles_per_image())):
        gsegs[k] = _lib.GnSeg(o.t.data_ptr(), o.h, o.w, t0, tpi)
        t0 += tpi * N
    _lib.check(L.dafne_groupnorm_finalize_hip(gsegs, len(raw), N, C, _lib.ptr(partial), _lib.ptr(stats),
                                              ctypes.c_float(1e-5), st), "finalize")
    torch.cuda.synchronize()
    raw_maps = [r.nchw_float() for r in raw]           # device tensors, fp32 view of the bf16 maps
    outs, partial2, c2 = run_fp8(raw_maps, w2, b2, 1.0, gn_in=(stats, gamma, beta), gn_stats=True, kernel=c256_kernel)
    _, _, w2deq = engine.quantize_weight_e4m3(w2)
    t0 = 0
    for k, (rm, got) in enumerate(zip(raw_maps, outs)):
        mean = stats[k, :, :, 0].cpu()[:, :, None, None, None]
        rstd = stats[k, :, :, 1].cpu()[:, :, None, None, None]
        n, c, h, w = rm.shape
        xg = rm.cpu().reshape(n, c // 8, 8, h, w)
        y = (xg - mean) * rstd * gamma.cpu().reshape(1, c // 8, 8, 1, 1) + beta.cpu().reshape(1, c // 8, 8, 1, 1)
        y = F.relu(y).reshape(n, c, h, w)
        ref = F.conv2d(q8(y), w2deq, b2, padding=1)
        close_bf16(got, bfr(ref))
        # GroupNorm partial sums of the fp8 layer's own output: per (tile, group) sums over the valid pixels
        tpi = c2.tiles_per_image()[k]
        ps = partial2[t0:t0 + tpi * n].reshape(n, tpi, c // 8, 2).sum(1).cpu()
        t0 += tpi * n
        rg = ref.reshape(n, c // 8, -1)
        assert torch.allclose(ps[..., 0], rg.sum(-1), rtol=2e-3, atol=0.5)
        assert torch.allclose(ps[..., 1], (rg * rg).sum(-1), rtol=2e-3, atol=0.5)


def test_fp8w_rejects_unsupported_shapes():
    from dafne_amd import engine, _lib
    d = dev()
    x = engine.Act(1, 16, 16, 64, d)
    o = engine.Act(1, 16, 16, 128, d)
    w = torch.zeros(128, 64 * 9, dtype=torch.uint8, device=d)
    b = torch.zeros(128, device=d)
    sc = torch.ones(128, device=d)
    c = engine.ConvCall(w, b, 64, 128, 3, 1, 1, 0, [(x.t, o.t, None, 16, 16, 16, 16)], 1, fp8=(sc, 1.0))
    with pytest.raises(_lib.DafneHipError, match="fp8w"):
        c(_lib.current_stream())


# ---------------------------------------------------------------------------------- config 5 model (fp8 weights)
def _build(cfgname, seed, fp8_kernel=None):
    import os
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_cfg(os.path.join(root, "configs", cfgname))
    if fp8_kernel is not None:
        cfg.ENGINE.FP8_CONV3X3_KERNEL = fp8_kernel
    m = build_model(cfg)
    P = om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=seed)
    m.load_state_dict(P)
    m.to(dev())
    m.invalidate()
    return cfg, m, P


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def test_fp8_model_backbone_and_head_vs_oracle():
    """ucas_aod_r101_fp8.yaml (ENGINE.WEIGHT_DTYPE fp8_e4m3) vs oracle/model.py with fp8=True: the backbone runs the
    bf16 kernels on exactly dequantised e4m3 weights (same tolerance as the bf16 model, tests/test_gpu_model.py), the
    head's GroupNorm-fed tower layers run the fp8 MFMA kernel.

    Head tolerance: an e4m3 rounding step is 2^-3 relative, so a pipeline of up to 7 quantise-on-load layers amplifies
    any fp32 summation-order difference far more than the bf16 pipeline does (a perturbation eps flips a rounding with
    probability eps / ulp and then costs a whole ulp).  The bound is therefore MEASURED on the oracle itself: the
    oracle's outputs for the same features with 5 % of the elements moved by one bf16 ulp ("twin").  The engine must be
    no further from the oracle than that twin (or 2.5e-2, the bf16 model's bound, where the twin is closer), and closer
    to the fp8 definition than to the bf16 model (the quantisation is really applied)."""
    from oracle import model as om
    cfg, m, P = _build("ucas_aod_r101_fp8.yaml", seed=3)
    assert cfg.ENGINE.WEIGHT_DTYPE == "fp8_e4m3"
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (2, 3, 128, 160), generator=g, dtype=torch.uint8)
    x, _ = om.preprocess([img[0], img[1]], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD)
    keys = ("p3", "p4", "p5", "p6", "p7")
    with torch.no_grad():
        f_q = om.backbone_forward(P, x, 101, emulate_bf16=True, fp8=True)
        f_b = om.backbone_forward(P, x, 101, emulate_bf16=True)
        fq = [f_q[k] for k in keys]
        h_q = om.head_forward(P, fq, emulate_bf16=True, fp8=True)
        h_b = om.head_forward(P, fq, emulate_bf16=True)
        gt = torch.Generator().manual_seed(1)
        twin = [(f * (1 + (torch.rand(f.shape, generator=gt) < 0.05).float() * 2.0 ** -8)).to(torch.bfloat16).float() for f in fq]
        h_t = om.head_forward(P, twin, emulate_bf16=True, fp8=True)
    feats = m.backbone(x.to(dev()))
    for k in keys:
        e_q, e_b = _rel(feats[k].cpu(), f_q[k]), _rel(feats[k].cpu(), f_b[k])
        assert e_q < 2.5e-2 and e_b > 2 * e_q, (k, e_q, e_b)
    head = m.proposal_generator.dafne_head
    logits, regs, centers, _, ctrs, _, _ = head(None, [f.to(dev()) for f in fq])
    for l in range(5):
        for i, (name, got) in enumerate((("logits", logits[l]), ("reg", regs[l]), ("center", centers[l]), ("ctr", ctrs[l]))):
            e_q, e_b, e_t = _rel(got.cpu(), h_q[i][l]), _rel(got.cpu(), h_b[i][l]), _rel(h_t[i][l], h_q[i][l])
            assert e_q < max(2.5e-2, e_t), (name, l, e_q, e_t)
            assert e_b > e_q, (name, l, e_q, e_b)


def test_fp8_model_uses_the_fp8_kernel_and_runs_end_to_end(c256_kernel):
    """Config 5 end to end at a small size.  Without activation calibration the ten GroupNorm-fed tower layers go to
    the fp8 3x3 kernels; after calibrate_fp8 pinned the plain-input layers' scales so do the 23 + 3 res4 / res5 3x3 layers,
    the 3 FPN output convolutions and the 2 FPN-fed tower layers: 41.  Calibration is EXPLICIT by default: an fp8 model
    without scales raises instead of quantising by whatever batch comes first; scales can be installed and persisted with
    the weights.  Detections are well formed."""
    import numpy as np
    cfg, m, P = _build("ucas_aod_r101_fp8.yaml", seed=17)
    g = torch.Generator().manual_seed(3)
    h, w = 256, 320
    img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
    assert cfg.ENGINE.FP8_ACT_CALIBRATION == "explicit"
    with pytest.raises(RuntimeError, match="calibrate_fp8"):
        m([{"image": img, "height": h, "width": w}])
    cfg.ENGINE.FP8_ACT_CALIBRATION = "off"
    m([{"image": img, "height": h, "width": w}])
    assert m.fp8_act_scales() is None
    names = [c.kernel_name() for c in m.plan(1, h, w).calls if hasattr(c, "kernel_name")]
    assert names.count(c256_kernel) == 10, names              # layers 1..3 of three towers + corners_tower.0: 256 input channels
    cfg.ENGINE.FP8_ACT_CALIBRATION = "explicit"
    m.calibrate_fp8(img.unsqueeze(0).to(dev()))
    out = m([{"image": img, "height": h, "width": w}])[0]["instances"]
    scales = m.fp8_act_scales()
    # the scales travel with the weights: save -> a fresh model -> load gives the same model, no calibration
    import os
    import tempfile
    from dafne_amd.checkpoint import load_weights, save_checkpoint
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "fp8.pth")
        save_checkpoint(m, path)
        cfg2, m2, _ = _build("ucas_aod_r101_fp8.yaml", seed=99)
        load_weights(m2, path)
    assert m2.fp8_act_scales() == scales
    out2 = m2([{"image": img, "height": h, "width": w}])[0]["instances"]
    assert torch.equal(out2.pred_corners, out.pred_corners) and torch.equal(out2.scores, out.scores)
    assert len(scales) == 31 and all(v > 0 and np.log2(v) == np.round(np.log2(v)) for v in scales.values()), scales
    plan = m.plan(1, h, w)
    names = [c.kernel_name() for c in plan.calls if hasattr(c, "kernel_name")]
    # 26 + 3 + 12, the same set of layers at every image size; the 38 256-input ones (res4, FPN outputs, towers) on the model's
    # FP8_CONV3X3_KERNEL, the three 512-input res5 layers always on the generic fp8 patch kernel
    assert names.count("conv3x3_patch_fp8") == 41, names
    assert "amax_probe" not in names
    assert 0 < len(out) <= cfg.MODEL.DAFNE.POST_NMS_TOPK_TEST + 8
    s = out.scores.cpu().numpy()
    assert np.all(np.diff(s) <= 0) and s.min() > 0 and s.max() <= 1
    assert torch.isfinite(out.pred_corners).all() and int(out.pred_classes.max()) < 2


def test_fp8_model_pipelined_equals_serial(fp8_kernel_cfg):
    """The fp8 model through the pipelined path (sub-batches on concurrent streams, post-process on the side stream)
    gives the detections of the serial path (same kernels on the same sub-batch composition: splits=1) -- with NO environment
    pin: the kernel of the 256-input fp8 layers is a property of the model (cfg.ENGINE.FP8_CONV3X3_KERNEL, both values), so
    the plan that has the GPU to itself and the pipelined step's sub-batch plans use the same one (round 3 chose per plan:
    two roundings of the same sums, 2 bf16 ulps apart)."""
    cfg, m, P = _build("ucas_aod_r101_fp8.yaml", seed=13, fp8_kernel=fp8_kernel_cfg)
    want = {"patch": "conv3x3_patch_fp8"}[fp8_kernel_cfg]
    g = torch.Generator().manual_seed(6)
    batches = [torch.randint(0, 256, (3, 3, 128, 160), generator=g, dtype=torch.uint8).to(dev()) for _ in range(3)]
    m.calibrate_fp8(batches[0])
    serial = [m.detect_packed(b) for b in batches]
    torch.cuda.synchronize()
    serial = [(r.clone(), c.clone()) for r, c in serial]
    piped = [m.detect_packed(b, pipelined=True, splits=1) for b in batches]
    torch.cuda.synchronize()
    for plan in [m.plan(3, 128, 160)] + [p for ps in m._pipe[(3, 128, 160, 1)]["plans"] for p in ps]:
        names = [c.kernel_name() for c in plan.calls if hasattr(c, "kernel_name")]
        assert names.count(want) >= 38, (plan.shared_gpu, names)
    for (r0, c0), (r1, c1) in zip(serial, piped):
        assert torch.equal(c0, c1)
        for i in range(3):
            k = int(c0[i])
            assert torch.equal(r0[i, :k], r1[i, :k])


def test_fp8_calibrated_model_vs_oracle():
    """The calibrated fp8 model end to end (detect_packed on two 192x256 images): the engine's activation scales are
    powers of two that keep 2 x the calibration amax inside e4m3's range, and with THE SAME scales the oracle's fp8
    definition (oracle/model.py act_q8: those layers' inputs rounded to e4m3) is reproduced -- FPN features within the
    bound measured on the oracle itself (its own outputs when 5 % of the stem input is moved by one bf16 ulp: every e4m3
    rounding downstream amplifies such a perturbation), head outputs likewise."""
    from oracle import model as om
    cfg, m, P = _build("ucas_aod_r101_fp8.yaml", seed=23)
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (2, 3, 192, 256), generator=g, dtype=torch.uint8)
    m.calibrate_fp8(img.to(dev()))
    m.detect_packed(img.to(dev()))
    torch.cuda.synchronize()
    aq = m.fp8_act_scales()
    assert set(k for k in aq if k.startswith("res4")) == set("res4.%d.conv2" % b for b in range(23))
    assert {"fpn_output3", "fpn_output4", "fpn_output5", "cls_tower.0", "center_tower.0", "res5.0.conv2"} <= set(aq)
    plan = m.plan(2, 192, 256)
    x, _ = om.preprocess([img[0], img[1]], cfg.MODEL.PIXEL_MEAN, cfg.MODEL.PIXEL_STD)
    keys = ("p3", "p4", "p5", "p6", "p7")
    with torch.no_grad():
        f_q = om.backbone_forward(P, x, 101, emulate_bf16=True, fp8=True, act_q8=aq)
        f_w = om.backbone_forward(P, x, 101, emulate_bf16=True, fp8=True)                  # weights-only fp8
        gt = torch.Generator().manual_seed(1)
        xt = (x * (1 + (torch.rand(x.shape, generator=gt) < 0.05).float() * 2.0 ** -8))
        f_t = om.backbone_forward(P, xt, 101, emulate_bf16=True, fp8=True, act_q8=aq)      # the oracle's own twin
    eng = [a.nchw_float().cpu() for a in plan.features]
    for k, e in zip(keys, eng):
        e_q, e_w, e_t = _rel(e, f_q[k]), _rel(e, f_w[k]), _rel(f_t[k], f_q[k])
        assert e_q < max(2.5e-2, 1.5 * e_t), (k, e_q, e_t)
        # (no "closer to the calibrated definition than to the weights-only one" assertion here: through 26 e4m3-rounded
        # layers the twin's own distance, 6-9 %, is as large as the distance between the two definitions, e_w; that the
        # kernel applies in_qscale / oscale as defined is pinned per layer to 2 bf16 ulps by test_fp8_patch_kernel_vs_torch)
        assert e_w > 0
    with torch.no_grad():
        h_q = om.head_forward(P, eng, emulate_bf16=True, fp8=True, act_q8=aq)
        twin = [(f * (1 + (torch.rand(f.shape, generator=gt) < 0.05).float() * 2.0 ** -8)).to(torch.bfloat16).float() for f in eng]
        h_t = om.head_forward(P, twin, emulate_bf16=True, fp8=True, act_q8=aq)
    hp = plan.head
    for l in range(5):
        lg = hp.logits[l].permute(0, 3, 1, 2).cpu()
        dc = hp.delta_ctr[l].permute(0, 3, 1, 2).cpu()
        ce = hp.center[l].permute(0, 3, 1, 2).cpu()
        sc = float(hp.scales[l])
        got = (lg, (ce.repeat(1, 4, 1, 1) + dc[:, :8]) * sc, ce * sc, dc[:, 8:9])
        for j, name in enumerate(("logits", "reg", "center", "ctr")):
            e_q, e_t = _rel(got[j], h_q[j][l]), _rel(h_t[j][l], h_q[j][l])
            assert e_q < max(2.5e-2, 1.5 * e_t), (name, l, e_q, e_t)
