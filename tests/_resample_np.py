"""Pillow's 8-bit two-pass resampler (libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
ImagingResampleHorizontal_8bpc / Vertical_8bpc) restated in numpy, for the bilinear and the bicubic (a = -0.5) filter.

This is the expectation of the GPU tests of dafne_scene_scaled_tiles_u8_hip; tests/test_scene_scales_cpu.py pins it to
PIL.Image.resize itself, bit for bit, so a wrong expectation cannot hide a wrong kernel.
"""
import numpy as np

PRECISION_BITS = 32 - 8 - 2


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


def coeffs(in_size, out_size, resample):
    """[(xmin, int32 coefficients)] per output index: precompute_coeffs + normalize_coeffs_8bpc for the box (0, in_size)."""
    fn, fsupport = FILTERS[resample]
    scale = float(np.float32(in_size)) / out_size            # the box is a float[4]
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        k = []
        for v in w:
            if ww != 0.0:
                v /= ww
            k.append(int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)))
        out.append((xmin, np.asarray(k, dtype=np.int64)))
    return out


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, new_h, new_w, resample="bicubic"):
    """img [H, W, C] uint8 -> [new_h, new_w, C] uint8 = np.asarray(Image.fromarray(img).resize((new_w, new_h), filter)):
    the horizontal pass into a uint8 intermediate (clipped), then the vertical pass.  A pass whose size does not change is a
    copy in Pillow; its coefficients are the identity, so it is not special-cased here."""
    img = np.asarray(img)
    h, w, c = img.shape
    src = img.astype(np.int64)
    half = 1 << (PRECISION_BITS - 1)
    tmp = np.empty((h, new_w, c), dtype=np.uint8)
    for xx, (xmin, k) in enumerate(coeffs(w, new_w, resample)):
        tmp[:, xx] = _clip8(half + np.tensordot(src[:, xmin:xmin + len(k)], k, axes=([1], [0])))
    t64 = tmp.astype(np.int64)
    out = np.empty((new_h, new_w, c), dtype=np.uint8)
    for yy, (ymin, k) in enumerate(coeffs(h, new_h, resample)):
        out[yy] = _clip8(half + np.tensordot(k, t64[ymin:ymin + len(k)], axes=([0], [0])))
    return out


def crop_zero_pad(img, left, up, patch):
    """The patch x patch window of img [H, W, C] at (left, up), zero past the image (the split's padding=True)."""
    out = np.zeros((patch, patch, img.shape[2]), dtype=img.dtype)
    win = img[up:up + patch, left:left + patch]
    out[:win.shape[0], :win.shape[1]] = win
    return out


def overshoot_image(h, w, seed):
    """Uniform random bytes with rows and columns of alternating 0 / 255 blocks: bicubic overshoot clips at 0 and 255 in both
    passes."""
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    blocks = (((yy // 3) + (xx // 3)) % 2 * 255).astype(np.uint8)
    img[: max(1, h // 2)] = blocks[: max(1, h // 2), :, None]
    return img
