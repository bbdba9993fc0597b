#!/usr/bin/env python3
"""tests/golden/scene_labels.npz: the tile label files of the reference's own DOTA split with ground truth,
ImgSplit_multi_process.splitbase.SplitSingle at rate 1 (tools/prepare_dota), for a few small scenes.  The class is made with
__new__ (no worker pool) and writes into temporary directories; stored are the scene label text, the scene size, patch and
overlap, and the name and text of every tile label file it wrote, in its emission order.

cv2 and shapely are not installed where this runs and are stubbed: cv2.imread returns a zero image of the case's shape,
cv2.imwrite does nothing; shapely.geometry is a small convex-polygon `Polygon` written below (area, intersection with the tile
rectangle by Sutherland-Hodgman clipping, exterior.coords, polygon.orient).  So the fixture certifies, against the reference's
code: the tile loop and its rectangle (right = min(left + subsize, w - 1)), parse_dota_poly2's truncation, the half_iou
branches, GetPoly4FromPoly5, choose_best_pointorder_fit_another, polyorig2sub's truncation, the clamp to [1, subsize], the
difficult rule and the text format.  The intersection itself (vertices, their order and start, the areas) is the stub's.

    python tests/golden/make_golden_scene_labels.py        (build container only: imports the reference's split module)
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NAMES = ["plane", "ship", "harbor", "small-vehicle", "bridge"]

# name, h, w, patch, overlap, objects, seed
CASES = [("P0000", 300, 260, 128, 32, 60, 11), ("P0001", 100, 90, 128, 32, 12, 12), ("P0002", 100, 400, 128, 32, 24, 13)]

LOG = []      # (vertices of the intersection, intersection area / object area) of every Polygon.intersection call


# ------------------------------------------------------------------------------------------------ the shapely stub
def _shoelace(pts):
    s = 0.0
    for i in range(len(pts)):
        x0, y0 = pts[i]
        x1, y1 = pts[(i + 1) % len(pts)]
        s = s + (x0 * y1 - x1 * y0)
    return s


def _clip(pts, edge, val):
    def inside(p):
        return (p[0] >= val, p[0] <= val, p[1] >= val, p[1] <= val)[edge]

    def cut(p, c):
        if edge < 2:
            t = (val - p[0]) / (c[0] - p[0])
            return (val, p[1] + t * (c[1] - p[1]))
        t = (val - p[1]) / (c[1] - p[1])
        return (p[0] + t * (c[0] - p[0]), val)
    out = []
    for i in range(len(pts)):
        c, p = pts[i], pts[i - 1]
        if inside(c):
            if not inside(p):
                out.append(cut(p, c))
            out.append(c)
        elif inside(p):
            out.append(cut(p, c))
    return out


class _Ring:
    def __init__(self, pts):
        self.coords = list(pts) + list(pts[:1])        # closed, as shapely's


class Polygon:
    """Convex polygons only."""

    def __init__(self, pts):
        self.pts = [(float(x), float(y)) for x, y in pts]
        self.exterior = _Ring(self.pts)

    @property
    def area(self):
        return abs(_shoelace(self.pts)) * 0.5 if len(self.pts) >= 3 else 0.0

    def intersection(self, rect):
        xs, ys = [p[0] for p in rect.pts], [p[1] for p in rect.pts]
        pts = self.pts
        for edge, val in enumerate((min(xs), max(xs), min(ys), max(ys))):
            pts = _clip(pts, edge, val)
        out = []
        for p in pts:
            if not out or p != out[-1]:
                out.append(p)
        if len(out) > 1 and out[0] == out[-1]:
            out.pop()
        r = Polygon(out)
        LOG.append((len(out), r.area / self.area))
        return r


def _orient(poly, sign=1.0):
    s = _shoelace(poly.pts)
    if len(poly.pts) >= 3 and s * sign < 0:
        ring = poly.exterior.coords[::-1]             # shapely reverses the closed ring: the start vertex stays
        return Polygon(ring[:-1])
    return poly


def _stub_modules(state):
    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda path, *a: np.zeros(state["shape"], dtype=np.uint8)
    cv2.imwrite = lambda path, img: True
    cv2.INTER_CUBIC = 2
    sys.modules["cv2"] = cv2
    shapely = types.ModuleType("shapely")
    geo = types.ModuleType("shapely.geometry")
    polygon = types.ModuleType("shapely.geometry.polygon")
    polygon.orient = _orient
    geo.Polygon = Polygon
    geo.polygon = polygon
    shapely.geometry = geo
    sys.modules["shapely"], sys.modules["shapely.geometry"], sys.modules["shapely.geometry.polygon"] = shapely, geo, polygon


# ------------------------------------------------------------------------------------------------ the scenes
def scene_text(h, w, n, seed):
    """n rotated rectangles (sides 4..90 x 4..40, centres anywhere in the scene), one decimal, every second one reversed."""
    rng = np.random.default_rng(seed)
    lines = ["imagesource:GoogleEarth", "gsd:0.5"]
    for k in range(n):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        a, b = rng.uniform(4, 90) / 2, rng.uniform(4, 40) / 2
        t = rng.uniform(0, np.pi)
        ux, uy = np.cos(t), np.sin(t)
        pts = [(cx + sa * a * ux - sb * b * uy, cy + sa * a * uy + sb * b * ux) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        if k % 2:
            pts = pts[::-1]
        lines.append(" ".join("%.1f %.1f" % p for p in pts) + " %s %d" % (NAMES[int(rng.integers(len(NAMES)))], int(rng.integers(2))))
    return "\n".join(lines) + "\n"


def main():
    assert os.path.isdir(REF), "reference tree not present: fixtures can only be made in the build container"
    state = {"shape": None}
    _stub_modules(state)
    sys.path.insert(0, os.path.join(REF, "tools", "prepare_dota"))
    import ImgSplit_multi_process as sp
    out = {"names": np.array([c[0] for c in CASES]), "cases": np.array([c[1:5] for c in CASES], dtype=np.int64),
           "classnames": np.array(NAMES)}
    marked2 = kept_cut = 0
    for i, (name, h, w, patch, overlap, n, seed) in enumerate(CASES):
        text = scene_text(h, w, n, seed)
        with tempfile.TemporaryDirectory() as td:
            for d in ("src/images", "src/labelTxt", "dst/images", "dst/labelTxt"):
                os.makedirs(os.path.join(td, d))
            with open(os.path.join(td, "src", "labelTxt", name + ".txt"), "w") as f:
                f.write(text)
            s = sp.splitbase.__new__(sp.splitbase)         # (no worker pool: SplitSingle runs in this process)
            s.basepath, s.outpath, s.code = os.path.join(td, "src"), os.path.join(td, "dst"), "utf-8"
            s.gap, s.subsize, s.slide, s.thresh = overlap, patch, patch - overlap, 0.7
            s.imagepath, s.labelpath = os.path.join(td, "src", "images"), os.path.join(td, "src", "labelTxt")
            s.outimagepath, s.outlabelpath = os.path.join(td, "dst", "images"), os.path.join(td, "dst", "labelTxt")
            s.choosebestpoint, s.ext, s.padding = True, ".png", True
            state["shape"] = (h, w, 3)
            order = []
            save = s.savepatches

            def recording(resizeimg, objects, subimgname, left, up, right, down, _save=save, _order=order):
                _order.append(subimgname)
                return _save(resizeimg, objects, subimgname, left, up, right, down)
            s.savepatches = recording
            s.SplitSingle(name, 1, ".png")
            texts = [open(os.path.join(s.outlabelpath, t + ".txt")).read() for t in order]
        for t in texts:
            for line in t.splitlines():
                marked2 += line.endswith(" 2")
        out["scene_%d" % i] = np.array(text)
        out["tiles_%d" % i] = np.array(order)
        out["texts_%d" % i] = np.array(texts)
    n_v = np.array([v for v, _ in LOG])
    ratio = np.array([r for _, r in LOG])
    cut = (ratio > 0) & (ratio < 1)
    seen = {"inside": int((ratio == 1).sum()), "outside": int((ratio <= 0).sum()), "cut4": int((cut & (n_v == 4)).sum()),
            "cut5": int((cut & (n_v == 5)).sum()), "3 vertices": int((cut & (n_v == 3)).sum()), "6+ vertices": int((cut & (n_v > 5)).sum()),
            "kept cut (> thresh)": int((cut & ((n_v == 4) | (n_v == 5)) & (ratio > 0.7)).sum()), "marked 2": int(marked2)}
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    np.savez_compressed(os.path.join(HERE, "scene_labels.npz"), **out)
    print("wrote scene_labels.npz,", len(CASES), "cases,", sum(len(out["tiles_%d" % i]) for i in range(len(CASES))), "tiles")


if __name__ == "__main__":
    main()
