"""fp64 restatement (numpy) of the backward of one tower layer of the head -- conv3x3(256 -> 256, stride 1, pad 1) reading
GroupNorm(32) + ReLU applied on load -- and the error bounds of the two kernels behind it (csrc/conv_tower_wgrad.hip,
csrc/conv_tower_dgrad.hip).  The arithmetic is the siblings', which are generic in Cout:

    wgrad            _pred_backward_np.wgrad (weight gradient with the sum of |g x| behind every element)
    layer_backward   _tail_backward_np.tail_backward (data gradient through the ReLU mask and the GroupNorm: gx, dgamma, dbeta, dbias,
                     each with the sum of the magnitudes of its terms)
    applied          the bf16 number the forward multiplied: bf16(relu(fma(xhat, gamma, beta))), gn_apply_kernel's expression

Only the bounds are new.  They are DERIVED from the kernels' arithmetic, not measured (u = 2^-24):

  * weight gradient: g enters as a hi + lo bf16 pair (|g - hi - lo| <= 2^-16 |g|), X is exact bf16, the products are exact in the
    fp32 accumulator, a workgroup's accumulator takes at most n pixels, the pixel splits are added in fp64 and rounded once:
        |err dW| <= (2^-16 + n u) sum |g x|                       = _pred_backward_np.wgrad_bound(absum, n), as it stands;
  * data gradient, ga: the hi + lo pair again, exact bf16 weights, and ONE fp32 accumulator per (pixel, channel) that takes all
    2 x 2304 products (hi and lo, K = 9 taps x 256 output channels, 144 MFMAs of K = 32):  |err ga| <= (2^-16 + 4608 u) A;
  * after the accumulator a pixel's value passes r = 46 fp32 roundings in conv_tower_dgrad.hip: xhat (2: the subtraction, the
    product), gz gamma (1), the product inside s2's fused multiply-add chain (1), the tile's group sums (32 additions in a lane --
    8 pixel blocks x 4 channels -- and 5 across lanes; the tiles are added in fp64), s / m (1), and in the second pass xhat s2 / m,
    two subtractions and the product with rstd (4).  gz itself is stored and read back exactly.  So
        |err gx| <= C rstd (A |gamma| [mask] + S1 / m + |xhat| S2 / m),   C = 2^-16 + (4608 + 46) u,
    with the magnitude sums of _tail_backward_np.tail_backward (gx_abs);
  * dgamma, dbeta: a lane of pass 1 adds 8 pixels per tile (4 x 32 pixels) over the tiles its workgroup walks,
    ceil(tiles / workgroups), in fp32, then 4 additions across lanes; dbias: a thread of pass 2 adds, per level, the pixels
    4 (b + k workgroups) + lane, ceil(level pixels / (4 workgroups)) of them, then 3 across threads; the workgroups are added in fp64:
        |err| <= (C + (lane_px + 4) u) sum of the magnitudes,     lane_px = lane_pixels(shapes, n, cus).
"""
import numpy as np

import _pred_backward_np as PB
import _tail_backward_np as TB

U = 2.0 ** -24
R_AFTER = 46
C_PIXEL = 2.0 ** -16 + (4608 + R_AFTER) * U
TH, TW = 4, 32                 # both kernels' tile of pixels

wgrad = PB.wgrad
wgrad_bound = PB.wgrad_bound
layer_backward = TB.tail_backward


def n_tiles(shapes, n):
    return sum(n * ((h + TH - 1) // TH) * ((w + TW - 1) // TW) for h, w in shapes)


def applied(x, st, gamma, beta):
    """x [N,H,W,256] (bf16-representable), st [N,32,2] fp32 -> the fp32 value of the bf16 number the forward multiplied, computed
    with the kernel's roundings: (x - mean) * rstd in fp32, ONE rounding for the fused multiply-add, bf16, ReLU."""
    x = np.asarray(x, dtype=np.float32); st = np.asarray(st, dtype=np.float32)
    mean = np.repeat(st[:, :, 0], 8, axis=1)[:, None, None, :]
    rstd = np.repeat(st[:, :, 1], 8, axis=1)[:, None, None, :]
    xh = ((x - mean).astype(np.float32) * rstd).astype(np.float32)
    y = (xh.astype(np.float64) * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)).astype(np.float32)
    return np.maximum(PB.bf16_round(y), 0.0)


def bound_gx(gx_abs):
    return C_PIXEL * gx_abs


def lane_pixels(shapes, n, cus):
    """The most values one lane adds in fp32 for dgamma / dbeta (pass 1: min(tiles, cus) workgroups) or dbias (pass 2:
    min(ceil(pixels / 4), 8 cus) workgroups)."""
    tiles = n_tiles(shapes, n)
    g1 = min(tiles, cus)
    pixels = sum(n * h * w for h, w in shapes)
    g2 = min((pixels + 3) // 4, 8 * cus)
    p1 = 8 * ((tiles + g1 - 1) // g1)
    p2 = sum((n * h * w + 4 * g2 - 1) // (4 * g2) for h, w in shapes)
    return max(p1, p2)


def bound_sum(absum, lane_px):
    return (C_PIXEL + (lane_px + 4) * U) * absum
