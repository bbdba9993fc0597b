"""fp64 restatement (numpy) of the head-tail backward, independent of the HIP kernels: from the gradient g at the raw output of
a prediction convolution (3x3 / stride 1 / pad 1, 256 -> Cout) back through the convolution, the ReLU and the GroupNorm (32 groups
of 8 channels) that the forward applies on load, to the raw tower map x.  Per (level, image, group), m = 8 H W:

    xhat = (x - mean) rstd
    ga[y, x, ci] = sum over (co, kh, kw) of g[y - kh + 1, x - kw + 1, co] W[co, ci, kh, kw]       (taps outside the image: 0)
    gz = ga [mask]               dgamma[c] = sum gz xhat         dbeta[c] = sum gz
    gxhat = gz gamma[c]          s1 = sum_group gxhat            s2 = sum_group gxhat xhat
    gx = rstd (gxhat - s1 / m - xhat s2 / m)                     dbias[c] = sum gx

The ReLU mask is PASSED IN (the forward's own: where the bf16 number it multiplied is > 0); the bf16 roundings of the forward are
straight-through and the statistics are taken as the statistics of x.  Layouts: x [N, H, W, 256], g [N, H, W, Cout], stats
[N, 32, 2] (mean, rstd), W OIHW [Cout, 256, 3, 3], per level.  Next to every result comes the sum of the MAGNITUDES of the terms
behind it (what the kernel's error bound is stated in).
"""
import numpy as np

G = 32


def dgrad(g, W):
    """-> (ga, A): ga as above, A = the same sum over |g| |W|."""
    g = np.asarray(g, dtype=np.float64); W = np.asarray(W, dtype=np.float64)
    N, H, Wd, Co = g.shape
    C = W.shape[1]
    gp = np.zeros((N, H + 2, Wd + 2, Co))
    gp[:, 1:-1, 1:-1] = g
    ga = np.zeros((N, H, Wd, C)); A = np.zeros((N, H, Wd, C))
    for kh in range(3):
        for kw in range(3):
            src = gp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + Wd]          # g[y - kh + 1, x - kw + 1]
            ga += src @ W[:, :, kh, kw]
            A += np.abs(src) @ np.abs(W[:, :, kh, kw])
    return ga, A


def tail_backward(xs, stats, gamma, beta, W, gs, masks):
    """Per-level lists xs, stats, gs, masks (bool [N, H, W, 256]) -> dict:
    gx (list), dgamma, dbeta, dbias [256]; and the magnitude sums gx_abs (list; WITHOUT the bound's constant), dgamma_abs,
    dbeta_abs, dbias_abs.  beta enters through the mask only (kept in the signature for the reader)."""
    gamma = np.asarray(gamma, dtype=np.float64)
    C = gamma.shape[0]
    out = {"gx": [], "gx_abs": [], "dgamma": np.zeros(C), "dbeta": np.zeros(C), "dbias": np.zeros(C),
           "dgamma_abs": np.zeros(C), "dbeta_abs": np.zeros(C), "dbias_abs": np.zeros(C)}
    for x, st, g, mask in zip(xs, stats, gs, masks):
        x = np.asarray(x, dtype=np.float64); st = np.asarray(st, dtype=np.float64)
        N, H, Wd, _ = x.shape
        m = 8.0 * H * Wd
        mean = np.repeat(st[:, :, 0], 8, axis=1)[:, None, None, :]
        rstd = np.repeat(st[:, :, 1], 8, axis=1)[:, None, None, :]
        xhat = (x - mean) * rstd
        ga, A = dgrad(g, W)
        mk = np.asarray(mask, dtype=bool)
        gz, Az = ga * mk, A * mk
        out["dgamma"] += (gz * xhat).sum((0, 1, 2)); out["dgamma_abs"] += (Az * np.abs(xhat)).sum((0, 1, 2))
        out["dbeta"] += gz.sum((0, 1, 2)); out["dbeta_abs"] += Az.sum((0, 1, 2))
        gxhat, Ax = gz * gamma, Az * np.abs(gamma)

        def gsum(v):
            """sum over the pixels and the 8 channels of a group, broadcast back to [N, 1, 1, C]"""
            s = v.reshape(N, H * Wd, G, 8).sum((1, 3))
            return np.repeat(s, 8, axis=1)[:, None, None, :]
        s1, s2 = gsum(gxhat), gsum(gxhat * xhat)
        S1, S2 = gsum(Ax), gsum(Ax * np.abs(xhat))
        gx = rstd * (gxhat - s1 / m - xhat * s2 / m)
        gx_abs = np.abs(rstd) * (Ax + S1 / m + np.abs(xhat) * S2 / m)
        out["gx"].append(gx); out["gx_abs"].append(gx_abs)
        out["dbias"] += gx.sum((0, 1, 2)); out["dbias_abs"] += gx_abs.sum((0, 1, 2))
    return out


U = 2.0 ** -24
# a pixel's chain: the hi + lo split of g (2^-16), <= 320 products in the fp32 accumulator of ten MFMAs, and fewer than 64 fp32
# roundings in everything after it (xhat, the tile's 37-term group sums, s / m, the three-term expression)
C_PIXEL = 2.0 ** -16 + (320 + 64) * U


def bound_gx(gx_abs):
    return C_PIXEL * gx_abs


def bound_sum(absum, tiles):
    """dgamma / dbeta / dbias: a lane adds at most 8 pixels per tile over at most `tiles` tiles in fp32, then four cross-lane
    additions; the partials are added in fp64."""
    return (C_PIXEL + (8 * tiles + 4) * U) * absum
