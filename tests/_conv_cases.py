"""The case table of the generic convolution entry point (dafne_conv2d_nhwc_bf16_hip, csrc/conv.hip), shared by
tests/test_conv_dispatch_cpu.py (which kernel does the library pick -- no device needed) and tests/test_gpu_conv_matrix.py
(does that kernel compute the convolution).  Every case names the kernel it was written for (`kernel`, one of
engine.ConvCall.KERNEL_NAMES) and the edge it is there for (`why`): a dispatch rule that moves a case to another kernel fails the
CPU test instead of silently leaving the kernel untested.

flags: "RELU", "RES" (residual add), "UP" (top-down add: 2x nearest upsample of a half-size map), "F32" (fp32 output without
halo, masked channel store), "GN" (GroupNorm partial sums of the output).  sizes: the input maps (H, W), one launch segment each;
padding is k // 2, the output size follows from the stride."""
import collections
import ctypes

Case = collections.namedtuple("Case", "name cin cout k stride sizes n flags bias kernel why")

IG0, IG1, IG2, IG3 = "conv_igemm<1,4,1,2>", "conv_igemm<1,4,2,2>", "conv_igemm<2,2,2,2>", "conv_igemm<4,2,2,4>"
STREAM, WS, PATCH, SLAB, PRED16 = "conv_stream", "conv_ws", "conv3x3_patch", "conv3x3_slab", "conv3x3_pred16"

# Exact-data regime of the GPU test: |x| <= X_MAX, |w| <= W_MAX, |bias|, |residual| <= B_MAX, R_MAX, all integers.  Every
# partial sum of a case is then an integer of magnitude <= K * X_MAX * W_MAX + B_MAX + R_MAX, exact in fp32 while below 2^24.
X_MAX, W_MAX, B_MAX, R_MAX = 2, 1, 8, 8


def exact_bound(c):
    return c.k * c.k * c.cin * X_MAX * W_MAX + (B_MAX if c.bias else 0) + (R_MAX if ("RES" in c.flags or "UP" in c.flags) else 0)


def _c(cin, cout, k, stride, sizes, n, flags, kernel, why, bias=True):
    if isinstance(sizes, tuple):
        sizes = [sizes]
    fl = tuple(flags.split()) if flags else ()
    name = "%s-%dto%d-k%ds%d-%s-n%d%s%s" % (kernel.replace("conv_", "").replace("conv3x3_", ""), cin, cout, k, stride,
                                           "+".join("%dx%d" % s for s in sizes), n, "".join("-" + f for f in fl),
                                           "" if bias else "-nobias")
    return Case(name, cin, cout, k, stride, list(sizes), n, fl, bias, kernel, why)


CASES = [
    # ---- conv_igemm<1,4,1,2>: Cout <= 32
    _c(64, 8, 1, 1, (13, 21), 2, "F32", IG0, "masked fp32 store with Cout < 8 of a 32-channel tile, ragged last tile"),
    _c(128, 32, 3, 1, (13, 21), 2, "", IG0, "bf16 output at Cout = 32 (the whole tile width)"),
    _c(64, 20, 3, 2, (17, 23), 3, "F32", IG0, "3x3 stride 2 on odd sizes, Cout not a multiple of 8"),
    # ---- conv_igemm<1,4,2,2>: 32 < Cout < 128
    _c(128, 64, 3, 2, (17, 23), 3, "RELU", IG1, "3x3 stride 2 on odd sizes"),
    _c(64, 40, 1, 1, (9, 31), 2, "F32", IG1, "Cout_pad (64) != Cout (40): masked store, zero-padded weight rows"),
    _c(64, 64, 1, 1, (1025, 1023), 1, "", IG1, "divmod_small at 2^20 - 1 pixels with an odd width"),
    _c(64, 64, 1, 1, (16, 16), 2, "", IG1, "plain 1x1 (was in test_conv_vs_torch)"),
    _c(64, 64, 3, 1, (16, 16), 1, "", IG1, "plain 3x3, one tile (was in test_conv_vs_torch)"),
    # ---- conv_igemm<2,2,2,2>: the 128 x 128 tile, ring and double-buffer form
    _c(128, 128, 3, 1, [(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)], 2, "RELU", IG2, "five segments in one launch"),
    _c(512, 256, 1, 1, (32, 48), 2, "UP", IG2, "top-down add (half-size map, nearest upsample) in the epilogue"),
    _c(256, 256, 3, 1, (10, 14), 2, "GN", IG2, "GroupNorm partial sums, two ragged tiles per image"),
    _c(192, 200, 3, 1, (11, 19), 2, "F32", IG2, "fp32 output, two N tiles of which the second is masked (200 = 128 + 72)"),
    _c(128, 128, 3, 1, (9, 13), 2, "", IG2, "odd sizes, ragged (was in test_conv_vs_torch)"),
    _c(256, 256, 3, 1, (16, 16), 1, "", IG2, "one image, two tiles (was in test_conv_vs_torch)"),
    _c(256, 256, 3, 2, (16, 16), 1, "", IG2, "P6 / P7 shape: 3x3 stride 2 (was in test_conv_vs_torch and the ring test)"),
    _c(1024, 256, 1, 1, (8, 8), 1, "", IG2, "K = 16 steps, half a tile (was in test_conv_vs_torch)"),
    _c(1024, 256, 1, 1, (24, 24), 2, "RELU", IG2, "Cin > 512 keeps a 1x1 off conv_stream: 32 half-K stages (was in the streaming test)"),
    _c(512, 512, 3, 1, (32, 32), 3, "RELU", IG2, "res5 conv2 of a 3-image sub-batch: 72 K steps (was in the ring test)"),
    _c(2048, 512, 1, 1, (32, 32), 8, "RELU", IG2, "res5 conv1 at batch 8: 256 tiles (was in the ring test)"),
    _c(256, 256, 3, 2, (32, 32), 2, "", IG2, "P6: 3x3 stride 2, 8 tiles (was in the ring test)"),
    _c(1024, 512, 1, 2, (64, 64), 3, "RELU", IG2, "1x1 stride 2 (was in the ring test)"),
    _c(1024, 128, 1, 1, (24, 40), 2, "RELU RES", IG2, "residual epilogue, ragged last tile, K = 16 steps (was in the ring test)"),
    _c(128, 128, 3, 1, (20, 20), 1, "RELU", IG2, "18 K steps, 4 tiles (was in the ring test)"),
    # ---- conv_igemm<4,2,2,4>: the 256 x 256 tile of eight waves
    _c(256, 256, 3, 2, (257, 255), 8, "RELU", IG3, "3x3 stride 2 on the 256 tile, odd sizes"),
    _c(128, 512, 3, 1, (120, 150), 2, "", IG3, "3x3 that the patch kernel refuses (no bias), ragged, two N tiles", bias=False),
    _c(512, 256, 1, 1, (131, 127), 8, "RELU", IG3, "ragged last tile at batch 8"),
    _c(512, 256, 1, 1, (131, 127), 1, "RELU", IG3, "the same kernel for one image: the choice counts kNominalBatch images"),
    _c(512, 512, 1, 1, [(96, 100), (33, 47), (7, 5)], 3, "", IG3, "three segments, two N tiles"),
    _c(512, 256, 1, 1, (131, 127), 2, "F32", IG3, "fp32 epilogue of the eight-wave tile"),
    # ---- conv_stream: persistent streaming 1x1, residual tile fetched one tile ahead
    _c(512, 512, 1, 1, (150, 131), 2, "RES", STREAM, "1 232 tiles > 2 x 512 resident slots: three tiles per workgroup, ragged last tile"),
    _c(512, 128, 1, 1, (97, 113), 3, "RES RELU", STREAM, "258 tiles < slots and T % 8 != 0 (xcd_remap remainder)"),
    _c(384, 256, 1, 2, (65, 51), 2, "RELU", STREAM, "stride 2 on odd sizes"),
    _c(320, 128, 1, 1, [(40, 56), (20, 28), (3, 4)], 2, "", STREAM, "three segments"),
    _c(512, 128, 1, 1, (1024, 1023), 1, "", STREAM, "divmod_small at ~2^20 pixels, 8 184 tiles"),
    _c(512, 2048, 1, 1, (4, 4), 1, "", STREAM, "16 pixels in one 128-pixel tile, 16 N tiles (was in test_conv_vs_torch)"),
    _c(192, 128, 1, 1, (24, 40), 2, "RELU", STREAM, "Cin <= 256 that conv_ws has no instantiation for"),
    # ---- conv_ws: weight-stationary 1x1, Cin 64 / 128 / 256 with and without residual
    _c(64, 128, 1, 2, (33, 45), 3, "RELU", WS, "stride 2, Cin 64 instantiation, no residual"),
    _c(128, 256, 1, 1, [(40, 56), (20, 28), (3, 4)], 2, "RES", WS, "segments + residual prefetch across a segment change, Cin 128"),
    _c(256, 128, 1, 1, (1, 1), 1, "", WS, "one pixel, one tile, Cin 256 without residual"),
    _c(64, 128, 1, 1, (1024, 1023), 1, "", WS, "divmod_small at ~2^20 pixels"),
    _c(128, 128, 1, 1, (37, 29), 2, "RELU", WS, "Cin 128 without residual, ragged"),
    _c(64, 256, 1, 1, (12, 20), 1, "", WS, "ragged last tile of 240 px (was in test_conv_vs_torch)"),
    _c(256, 128, 1, 2, (16, 16), 2, "", WS, "stride-2 1x1 (was in test_conv_vs_torch)"),
    _c(64, 256, 1, 1, (256, 256), 2, "", WS, "1 024 x 2 tiles (was in test_conv_vs_torch as 'the 8-wave tile')"),
    _c(128, 256, 1, 1, (150, 131), 2, "RES RELU", WS, "several tiles per workgroup, ragged, Cin 128 residual (was in the streaming test)"),
    _c(64, 128, 1, 1, (97, 113), 3, "RES", WS, "shortest K, Cin 64 residual (was in the streaming test)"),
    _c(256, 1024, 1, 1, (40, 40), 3, "RES RELU", WS, "res4 conv3 shape: 8 N tiles per pixel tile, Cin 256 residual (was in the streaming test)"),
    _c(64, 256, 1, 1, (150, 131), 2, "RELU", WS, "no residual: staging tile is write-only (was in the streaming test)"),
    # ---- the 3x3 kernels with test functions of their own in tests/test_gpu_conv.py
    _c(256, 256, 3, 1, [(128, 128), (64, 64), (32, 32), (16, 16), (8, 8)], 1, "", PATCH, "five levels at N = 1"),
    _c(64, 512, 3, 1, (120, 150), 2, "", PATCH, "ragged 8 x 32 tiles, two channel tiles (was in test_conv_vs_torch as '8-wave tile')"),
    _c(128, 32, 3, 1, [(13, 21), (5, 7)], 2, "F32", SLAB, "Cout = 32, Cin != 256, two ragged levels"),
    _c(256, 15, 3, 1, (6, 10), 2, "F32", PRED16, "the shape of test_prediction_conv_f32_output"),
]

# 32-bit input offsets: the haloed input of a segment, all images, must stay below 2^32 bytes.  (cin, cout, k, size, N accepted,
# N rejected...)
LIMIT_CASES = [
    (256, 128, 1, (254, 254), 127, (128, 129)),      # 256 x 256 x 512 B = 2^25 B per image
    (64, 64, 3, (1022, 1022), 31, (33,)),            # 1024 x 1024 x 128 B = 2^27 B per image
]

FLAG_BITS = {"RELU": 1, "RES": 2, "UP": 4, "F32": 8, "GN": 16}


def out_hw(h, w, k, stride):
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def probe(cin, cout, k, stride, sizes, n, flags=(), bias=True):
    """(kernel id, tiles, message) of a launch, from the library alone: dafne_conv2d_kernel_id / _num_tiles only read the
    shapes and test the pointers against null, so dummy non-null pointers do and no device is needed."""
    from dafne_amd import _lib
    L = _lib.load()
    bits = 0
    for f in flags:
        bits |= FLAG_BITS[f]
    dummy = 0x1000
    prm = _lib.ConvParams(n, len(sizes), cin, cout, k, k, stride, k // 2, bits, dummy, dummy if bias else None,
                          dummy if "GN" in flags else None, None, None, None, None, None, 0.0)
    segs = (_lib.ConvSeg * len(sizes))()
    for i, (h, w) in enumerate(sizes):
        ho, wo = out_hw(h, w, k, stride)
        segs[i] = _lib.ConvSeg(dummy, dummy, dummy if ("RES" in flags or "UP" in flags) else None, h, w, ho, wo)
    kid = L.dafne_conv2d_kernel_id(ctypes.byref(prm), segs)
    msg = L.dafne_last_error().decode(errors="replace") if kid < 0 else ""
    tiles = L.dafne_conv2d_num_tiles(ctypes.byref(prm), segs)
    return kid, tiles, msg
