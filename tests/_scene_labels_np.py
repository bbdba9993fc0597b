"""Restatement of the scene-label split (dafne_amd/scene_labels.py, csrc/scene_labels_kernels.h) on the host: the same fp64
operations in the same order, one (tile, object) pair at a time in plain Python floats (IEEE double, no contraction).

What it restates is ImgSplit_multi_process.splitbase.savepatches (tools/prepare_dota, :147-207) for convex quadrilaterals,
with the polygon intersection written out (shapely's is GEOS): Sutherland-Hodgman against the tile rectangle's edges in the
order left, right, up, down.  Every step is numbered as in the kernel's header comment.

  split_pair(box8, difficult, rect, patch, thresh)   -> (code, [8 ints], difficult)
  keep_row(row8, difficult, min_area, min_side)      -> bool, the training filter (DOTA2COCO.py:49, dota.py:226, :247-264)
  split_labels(labels, sizes, ...)                   -> dict of numpy arrays, field for field what split_scene_labels returns
  format_row(row8, name, difficult)                  -> the labelTxt line savepatches writes
"""
import math

import numpy as np

from dafne_amd.data.targets import polygon_area, sort_quadrilateral_np
from dafne_amd.scene import split_origins

NONE, INSIDE, CUT4, CUT5, DROP_LT4, DROP_GT5, NONCONVEX = range(7)
N_CODES = 7


def shoelace(pts):
    """sum over i of (x_i y_(i+1) - x_(i+1) y_i), added in index order."""
    s = 0.0
    n = len(pts)
    for i in range(n):
        x0, y0 = pts[i]
        x1, y1 = pts[(i + 1) % n]
        s = s + (x0 * y1 - x1 * y0)
    return s


def _inside(edge, x, y, val):
    if edge == 0:
        return x >= val
    if edge == 1:
        return x <= val
    if edge == 2:
        return y >= val
    return y <= val


def _isect(edge, val, px, py, cx, cy):
    """The point of p -> c on the edge; the clipped coordinate is the edge's value itself."""
    if edge < 2:
        t = (val - px) / (cx - px)
        return (val, py + t * (cy - py))
    t = (val - py) / (cy - py)
    return (px + t * (cx - px), val)


def clip_edge(pts, edge, val):
    out = []
    n = len(pts)
    for i in range(n):
        cx, cy = pts[i]
        px, py = pts[i - 1]
        cin, pin = _inside(edge, cx, cy, val), _inside(edge, px, py, val)
        if cin:
            if not pin:
                out.append(_isect(edge, val, px, py, cx, cy))
            out.append((cx, cy))
        elif pin:
            out.append(_isect(edge, val, px, py, cx, cy))
    return out


def merge_equal(pts):
    out = []
    for p in pts:
        if not out or not (p[0] == out[-1][0] and p[1] == out[-1][1]):
            out.append(p)
    if len(out) > 1 and out[0][0] == out[-1][0] and out[0][1] == out[-1][1]:
        out.pop()
    return out


def poly4_from_poly5(pts):
    """GetPoly4FromPoly5 (:125-145): the first shortest edge becomes its midpoint."""
    d = []
    for i in range(5):
        a, b = pts[i], pts[(i + 1) % 5]
        dx, dy = a[0] - b[0], a[1] - b[1]
        d.append(math.sqrt(dx * dx + dy * dy))
    pos = 0
    for i in range(1, 5):
        if d[i] < d[pos]:
            pos = i
    out = []
    for c in range(5):
        if c == pos:
            a, b = pts[c], pts[(c + 1) % 5]
            out.append(((a[0] + b[0]) / 2, (a[1] + b[1]) / 2))
        elif c == (pos + 1) % 5:
            continue
        else:
            out.append(pts[c])
    return out


def best_order(pts, dst):
    """choose_best_pointorder_fit_another (:18-35): the first minimum over the four cyclic shifts; the eight squares are added
    as numpy adds eight values: ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7))."""
    best, bd = 0, None
    for k in range(4):
        e = []
        for i in range(4):
            p, q = pts[(i + k) % 4], dst[i]
            ex, ey = p[0] - q[0], p[1] - q[1]
            e.append(ex * ex)
            e.append(ey * ey)
        dist = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))
        if bd is None or dist < bd:
            best, bd = k, dist
    return [pts[(i + best) % 4] for i in range(4)]


def split_pair(box8, difficult, rect, patch, thresh=0.7):
    """One object against one tile.  rect = (left, up, right, down) as SplitSingle forms it.  -> (code, row [8 ints], difficult)."""
    left, up, right, down = [float(v) for v in rect]
    obj = [(float(int(box8[2 * i])), float(int(box8[2 * i + 1]))) for i in range(4)]          # 1. int() truncation on load
    pos = neg = False                                                                         # 2. convexity
    for i in range(4):
        a, b, c = obj[i], obj[(i + 1) % 4], obj[(i + 2) % 4]
        cr = (b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0])
        pos, neg = pos or cr > 0, neg or cr < 0
    zero = [0] * 8
    if pos and neg:
        return NONCONVEX, zero, 0
    area = abs(shoelace(obj)) * 0.5                                                           # 3. area
    if not area > 0:
        return NONE, zero, 0
    if all(left <= x <= right and up <= y <= down for x, y in obj):                           # 4. half_iou == 1
        row = []
        for x, y in obj:
            row += [int(x - left), int(y - up)]
        return INSIDE, row, int(difficult)
    pts = obj                                                                                 # 5. clip
    for edge, val in enumerate((left, right, up, down)):
        pts = clip_edge(pts, edge, val)
    pts = merge_equal(pts)
    if len(pts) < 3:
        return NONE, zero, 0
    s = shoelace(pts)
    half = (abs(s) * 0.5) / area
    if not half > 0:
        return NONE, zero, 0
    if s < 0:                                                                                 # 6. orient(sign=1)
        pts = [pts[0]] + pts[:0:-1]
    if len(pts) < 4:
        return DROP_LT4, zero, 0
    if len(pts) > 5:
        return DROP_GT5, zero, 0
    code = CUT4
    if len(pts) == 5:                                                                         # 7.
        pts = poly4_from_poly5(pts)
        code = CUT5
    pts = best_order(pts, obj)                                                                # 8.
    row = []
    for x, y in pts:                                                                          # 9. int(), 10. clamp
        for v in (int(x - left), int(y - up)):
            row.append(1 if v <= 1 else (patch if v >= patch else v))
    return code, row, int(difficult) if half > thresh else 2                                  # 11.


def keep_row(row8, difficult, min_area, min_side):
    if difficult == 2:
        return False
    pts = [(float(row8[2 * i]), float(row8[2 * i + 1])) for i in range(4)]
    if not abs(shoelace(pts)) * 0.5 > min_area:
        return False
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    if not max(max(xs) - min(xs), max(ys) - min(ys)) >= min_side:
        return False
    for i in range(4):
        for j in range(i + 1, 4):
            if abs(pts[i][0] - pts[j][0]) + abs(pts[i][1] - pts[j][1]) < 1e-2:
                return False
    return True


def format_row(row8, name, difficult):
    """savepatches' line: the values are np.float64 printed with str()."""
    return " ".join(str(np.float64(v)) for v in row8) + " " + name + " " + str(difficult)


def scene_objects(labels):
    """Per scene the indices into labels["boxes"] in label-file order, and each box's class."""
    C = len(labels["classnames"])
    S = len(labels["scene_names"])
    off = np.asarray(labels["offsets"], dtype=np.int64)
    G = int(off[-1])
    bucket = np.repeat(np.arange(S * C), np.diff(off))
    cls = (bucket % C).astype(np.int32)
    scene = bucket // C
    fi = np.asarray(labels["file_index"], dtype=np.int64)
    per_scene = []
    for s in range(S):
        idx = np.nonzero(scene == s)[0]
        per_scene.append(idx[np.argsort(fi[idx], kind="stable")])
    assert sum(len(p) for p in per_scene) == G
    return per_scene, cls


def split_labels(labels, sizes, patch_size=1024, overlap=200, thresh=0.7, min_area=10, min_side=2, ratio=(1, 1), sort=True):
    per_scene, cls = scene_objects(labels)
    boxes = np.asarray(labels["boxes"], dtype=np.float64)
    diff = np.asarray(labels["difficult_value"], dtype=np.int64)
    rx, ry = float(ratio[0]), float(ratio[1])
    origins, tile_scene = [], []
    codes, rows, diffs, kepts = [], [], [], []
    a_off, k_off = [0], [0]
    a_rows, a_cls, a_diff, a_src = [], [], [], []
    k_rows, k_cls, k_src = [], [], []
    for s, (h, w) in enumerate(sizes):
        for left, up in split_origins(h, w, patch_size, overlap):
            rect = (left, up, min(left + patch_size, w - 1), min(up + patch_size, h - 1))
            origins.append((left, up))
            tile_scene.append(s)
            for g in per_scene[s]:
                code, row, d = split_pair(boxes[g], diff[g], rect, patch_size, thresh)
                written = code in (INSIDE, CUT4, CUT5)
                kept = written and keep_row(row, d, min_area, min_side)
                codes.append(code)
                rows.append(row)
                diffs.append(d)
                kepts.append(int(kept))
                if written:
                    a_rows.append(row)
                    a_cls.append(cls[g])
                    a_diff.append(d)
                    a_src.append(g)
                if kept:
                    k_rows.append(row)
                    k_cls.append(cls[g])
                    k_src.append(g)
            a_off.append(len(a_rows))
            k_off.append(len(k_rows))
    kc = np.asarray(k_rows, dtype=np.float64).reshape(-1, 4, 2) * np.array([rx, ry], dtype=np.float64)
    kc = np.ascontiguousarray(kc.reshape(-1, 8).astype(np.float32))
    if sort:
        kc = sort_quadrilateral_np(kc)
    xs, ys = kc[:, 0::2], kc[:, 1::2]
    hbox = np.stack((xs.min(1), ys.min(1), xs.max(1), ys.max(1)), axis=1) if kc.shape[0] else np.zeros((0, 4), np.float32)
    codes = np.asarray(codes, dtype=np.int32)
    stats = np.concatenate([np.bincount(codes, minlength=N_CODES)[:N_CODES], [len(a_rows), len(k_rows)]]).astype(np.int64)
    return {"codes": codes, "rows": np.asarray(rows, dtype=np.int32).reshape(-1, 8), "pair_difficult": np.asarray(diffs, dtype=np.int32),
            "pair_kept": np.asarray(kepts, dtype=np.int32),
            "offsets": np.asarray(a_off, dtype=np.int32), "corners": np.asarray(a_rows, dtype=np.int32).reshape(-1, 8),
            "classes": np.asarray(a_cls, dtype=np.int32), "difficult": np.asarray(a_diff, dtype=np.int32),
            "src": np.asarray(a_src, dtype=np.int64),
            "kept_offsets": np.asarray(k_off, dtype=np.int32), "kept_corners": kc, "kept_hbox": hbox.astype(np.float32),
            "kept_area": polygon_area(kc), "kept_classes": np.asarray(k_cls, dtype=np.int32), "kept_src": np.asarray(k_src, dtype=np.int64),
            "stats": stats, "origins": np.asarray(origins, dtype=np.int64).reshape(-1, 2),
            "tile_scene": np.asarray(tile_scene, dtype=np.int64)}


def tile_texts(res, scene_names, classnames):
    """{tile file stem: text} of the written rows, as write_tile_labels writes them."""
    out = {}
    for t in range(len(res["tile_scene"])):
        a, b = int(res["offsets"][t]), int(res["offsets"][t + 1])
        stem = "%s__1__%d___%d" % (scene_names[int(res["tile_scene"][t])], res["origins"][t][0], res["origins"][t][1])
        out[stem] = "".join(format_row(res["corners"][k], classnames[int(res["classes"][k])], int(res["difficult"][k])) + "\n"
                            for k in range(a, b))
    return out


def random_objects(h, w, n, seed, names, side_a=(4, 90), side_b=(4, 40), box=None):
    """n rotated rectangles with centres in `box` = (x0, y0, x1, y1) (default: the scene), one decimal, every second reversed."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = box if box is not None else (0, 0, w, h)
    out = []
    for k in range(n):
        cx, cy = rng.uniform(x0, x1), rng.uniform(y0, y1)
        a, b = rng.uniform(*side_a) / 2, rng.uniform(*side_b) / 2
        t = rng.uniform(0, np.pi)
        ux, uy = np.cos(t), np.sin(t)
        pts = [(cx + sa * a * ux - sb * b * uy, cy + sa * a * uy + sb * b * ux) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        if k % 2:
            pts = pts[::-1]
        out.append({"name": names[int(rng.integers(len(names)))], "difficult": int(rng.integers(2)),
                    "bbox": [round(float(v), 1) for p in pts for v in p]})
    return out


def labels_from_objects(scenes_objects, scene_names, classnames):
    """load_scene_labels' dict from in-memory objects ([{"name", "difficult", "bbox"}] per scene), without files."""
    import os
    import tempfile
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    with tempfile.TemporaryDirectory() as td:
        for name, objs in zip(scene_names, scenes_objects):
            with open(os.path.join(td, "%s.txt" % name), "w") as f:
                for o in objs:
                    f.write(" ".join(repr(float(v)) for v in o["bbox"]) + " %s %d\n" % (o["name"], o["difficult"]))
        return load_scene_labels(td, scene_names, classnames)
