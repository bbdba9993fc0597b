"""The training views (csrc/resize.hip train_views_kernel, csrc/train_views_kernels.h) restated in numpy.

A view = (window of a source, hflip, vflip, (new_h, new_w), rot).  Order of the reference's augmentation list
(tools/plain_train_net.py:229-256): hflip, vflip, resize, rotation.
  pixels       np.rot90(PIL_resize_bilinear(flip(window)), rot) on the H, W axes; the window reads 0 past the source
  coordinates  fp64, one operation at a time, from the fp32 corners at window scale (view_coords), then DAFNeDatasetMapper's
               ground truth (view_gt): area, one rounding to fp32, sort_quadrilateral, hull box, the empty-box filter.
This is the expectation of tests/test_gpu_train_views.py; tests/test_train_views_cpu.py pins the pixel route to PIL.Image.resize
and the coordinate forms to np.rot90.
"""
import numpy as np

from _resample_np import resize as _resize


def crop_window(img_hwc, left, up, win_h, win_w):
    """The win_h x win_w window of img [H, W, C] at (left, up), 0 past the image."""
    out = np.zeros((win_h, win_w, img_hwc.shape[2]), dtype=img_hwc.dtype)
    win = img_hwc[up:up + win_h, left:left + win_w]
    out[:win.shape[0], :win.shape[1]] = win
    return out


def view_pixels(img_hwc, left, up, win_h, win_w, hflip, vflip, new_h, new_w, rot):
    """-> [oh, ow, C] uint8.  The flips come before the resize."""
    w = crop_window(np.asarray(img_hwc), left, up, win_h, win_w)
    if hflip:
        w = w[:, ::-1]
    if vflip:
        w = w[::-1]
    w = np.ascontiguousarray(w)
    r = _resize(w, new_h, new_w, "bilinear")          # new == win: identity coefficients, a copy
    return np.ascontiguousarray(np.rot90(r, rot, axes=(0, 1)))


def out_hw(new_h, new_w, rot):
    return (new_w, new_h) if rot & 1 else (new_h, new_w)


def batch_pixels(views, cap_h, cap_w):
    """views: [(img_hwc, left, up, win_h, win_w, hflip, vflip, new_h, new_w, rot)] -> ([N, 3, cap_h, cap_w] uint8 zero padded,
    valid_hw [N, 2] int32)."""
    out = np.zeros((len(views), 3, cap_h, cap_w), dtype=np.uint8)
    hw = np.zeros((len(views), 2), dtype=np.int32)
    for i, v in enumerate(views):
        p = view_pixels(*v)
        out[i, :, :p.shape[0], :p.shape[1]] = p.transpose(2, 0, 1)
        hw[i] = p.shape[:2]
    return out, hw


def view_coords(corners, win_h, win_w, hflip, vflip, new_h, new_w, rot):
    """corners [n, 8] float32 at window scale -> (x [n, 4], y [n, 4]) float64."""
    c = np.asarray(corners, dtype=np.float32).reshape(-1, 4, 2).astype(np.float64)
    x, y = c[:, :, 0].copy(), c[:, :, 1].copy()
    ww, wh, W, H = np.float64(win_w), np.float64(win_h), np.float64(new_w), np.float64(new_h)
    if hflip:
        x = ww - x
    if vflip:
        y = wh - y
    x = x * (W / ww)
    y = y * (H / wh)
    if rot == 1:
        x, y = y, W - x
    elif rot == 2:
        x, y = W - x, H - y
    elif rot == 3:
        x, y = H - y, x
    return x, y


def view_gt(corners, classes, win_h, win_w, hflip, vflip, new_h, new_w, rot, sort=True):
    """-> dict(corners [k, 8] f32, hbox [k, 4] f32, area [k] f32, classes [k] int32, src [k] int32): the kept rows in input order."""
    from dafne_amd.data.targets import sort_quadrilateral_np
    x, y = view_coords(corners, win_h, win_w, hflip, vflip, new_h, new_w, rot)
    n = x.shape[0]
    s1, s2 = np.zeros(n, np.float64), np.zeros(n, np.float64)
    for i in range(4):
        k = (i + 3) % 4
        s1 = s1 + x[:, i] * y[:, k]
        s2 = s2 + y[:, i] * x[:, k]
    area = (0.5 * np.abs(s1 - s2)).astype(np.float32)
    q = np.stack((x, y), axis=2).reshape(n, 8).astype(np.float32)
    xs, ys = q[:, 0::2], q[:, 1::2]
    if n:
        hbox = np.stack((xs.min(1), ys.min(1), xs.max(1), ys.max(1)), axis=1).astype(np.float32)
    else:
        hbox = np.zeros((0, 4), np.float32)
    if sort:                    # after the box: the sort writes zeros for collinear corners, the rows the filter drops
        q = sort_quadrilateral_np(q)
    keep = ((hbox[:, 2] - hbox[:, 0]) > np.float32(1e-5)) & ((hbox[:, 3] - hbox[:, 1]) > np.float32(1e-5))
    idx = np.nonzero(keep)[0].astype(np.int32)
    return dict(corners=q[idx].reshape(-1, 8), hbox=hbox[idx].reshape(-1, 4), area=area[idx],
                classes=np.asarray(classes, dtype=np.int32).reshape(-1)[idx], src=idx)


def batch_gt(views, corners, classes, offsets, sort=True):
    """views: [(win_h, win_w, hflip, vflip, new_h, new_w, rot)]; corners [G, 8], classes [G], offsets [N + 1] -> the packed
    arrays of dafne_train_gt_hip: corners, hbox, area, classes, offsets [N + 1] int32, src (rows of the input)."""
    parts, off = [], [0]
    for v, p in enumerate(views):
        a, b = int(offsets[v]), int(offsets[v + 1])
        g = view_gt(np.asarray(corners).reshape(-1, 8)[a:b], np.asarray(classes).reshape(-1)[a:b], *p, sort=sort)
        g["src"] = g["src"] + np.int32(a)
        parts.append(g)
        off.append(off[-1] + g["src"].shape[0])
    out = {k: np.concatenate([g[k] for g in parts], axis=0) if parts else None for k in ("corners", "hbox", "area", "classes", "src")}
    out["offsets"] = np.asarray(off, dtype=np.int32)
    return out


def inverse_view(hflip, vflip, rot):
    """Without a resize: the (hflip, vflip, rot) whose view of the view's output gives the window back.  rot90^-rot, then the
    flips undone; a flip pair after a turn by r equals the turn after the flips swapped when r is odd."""
    r = (4 - rot) % 4
    if rot & 1:
        hflip, vflip = vflip, hflip
    return hflip, vflip, r
