"""DOTA Task2 (horizontal boxes) in plain numpy, shared by test_task2_cpu.py and the test_gpu_task2_*.py files: the tile
merge's horizontal-box NMS, the oriented-to-horizontal rule, the merge of a tile-level Task2 file, the Task2 rows of the
whole-scene merge and the Task2 match against scene labels.  Nothing here imports dafne_amd.

Restated from the reference's definitions (dafne/utils/ResultMerge_multi_process.py:124-155 py_cpu_nms, :183-223 mergesingle,
dafne/utils/dota_utils.py:122-127 dots4ToRec4, dafne/evaluation/voc_eval.py:158-173), with ONE difference: every sort is
kind="stable", so equal scores have a defined order (argsort(score, stable)[::-1]: among equal scores the later row first).
Without equal scores the reference gives the same lists (tests/golden/task2_merge.npz)."""
import re

import numpy as np

import _scene_eval_np as sev

NMS_THRESH = 0.1


def np_hbb_nms(dets, thresh):
    """dets [M,5] f64 (x1, y1, x2, y2, score) -> kept row indices, descending score."""
    dets = np.asarray(dets, np.float64).reshape(-1, 5)
    x1, y1, x2, y2, scores = (dets[:, k] for k in range(5))
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = scores.argsort(kind="stable")[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        rest = order[1:]
        w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1)
        h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1)
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (areas[i] + areas[rest] - inter)
        order = rest[np.where(ovr <= thresh)[0]]
    return keep


def rec4(b):
    """[N,8] (x0, y0, .., x3, y3) -> [N,4] xmin, ymin, xmax, ymax."""
    b = np.asarray(b, np.float64).reshape(-1, 8)
    return np.stack([b[:, 0::2].min(1), b[:, 1::2].min(1), b[:, 0::2].max(1), b[:, 1::2].max(1)], 1) if len(b) else np.zeros((0, 4))


def task1_to_task2_lines(lines):
    """Tile-level Task1 lines -> tile-level Task2 lines: name and score tokens verbatim, "%.2f" of rec4 of the parsed floats."""
    out = []
    for raw in lines:
        t = raw.strip().split(" ")
        r = rec4(np.array([float(v) for v in t[2:10]]))[0]
        out.append(t[0] + " " + t[1] + " " + " ".join("%.2f" % v for v in r))
    return out


_XY = re.compile(r"__(\d+)___(\d+)")
_RATE = re.compile(r"__([\d+\.]+)__\d+___")


def merge_task2_lines(lines, thresh=NMS_THRESH):
    """One tile-level Task2 file -> the merged file's lines: (coordinate + tile offset) / rate, np_hbb_nms per original image
    (images in order of first appearance), `name str(score) str(x) ..`."""
    boxes = {}
    for raw in lines:
        t = raw.strip().split(" ")
        x, y = (int(v) for v in _XY.findall(t[0])[0])
        rate = float(_RATE.findall(t[0])[0])
        c = [float(v) for v in t[2:]]
        det = [float(c[k] + (x if k % 2 == 0 else y)) / rate for k in range(len(c))] + [float(t[1])]
        boxes.setdefault(t[0].split("__")[0], []).append(det)
    out = []
    for img, dets in boxes.items():
        for i in np_hbb_nms(np.array(dets), thresh):
            out.append(img + " " + str(dets[i][-1]) + " " + " ".join(map(str, dets[i][:-1])))
    return out


def quantise(v, scale):
    return np.rint(np.asarray(v, np.float32).astype(np.float64) * scale) / scale


def merge_hbb_rows_numpy(rows, counts, info, n_scenes, n_classes, skip, score_mode):
    """The Task2 rows of the whole-scene merge: per (scene, class) bucket, tile order then row order; rec4 of the Task1 row's
    quantised, shifted coordinates ("%.2f" as rint(v * 100) / 100, + the tile origin) and the Task1 row's score."""
    k_cap = rows.shape[1]
    buckets = [[] for _ in range(n_scenes * n_classes)]
    srcs = [[] for _ in range(n_scenes * n_classes)]
    for t in range(rows.shape[0]):
        left, up, s = (int(v) for v in info[t])
        for r in range(min(int(counts[t]), k_cap)):
            row = rows[t, r]
            c = int(row[10])
            if (skip >> c) & 1:
                continue
            q = np.empty(8)
            q[0::2] = (quantise(row[0:8:2], 100.0) + left) / 1.0
            q[1::2] = (quantise(row[1:8:2], 100.0) + up) / 1.0
            sc = np.float32(np.float32(row[8] * row[8]) / row[9]) if score_mode else row[8]
            d = np.concatenate([rec4(q)[0], quantise(np.array([sc], np.float32), 10000.0)])
            buckets[s * n_classes + c].append(d)
            srcs[s * n_classes + c].append(t * k_cap + r)
    return buckets, srcs


def np_match_hbb(dets, bucket, gt, offs):
    """dets [N,4], gt [G,4] rectangles -> ovmax [N] f64, jmax [N] int32: inters / uni of hull_candidates' arithmetic
    (voc_eval.py:158-173, +1 on widths, heights and both areas) against EVERY box of the detection's bucket; the maximum and
    its first index; -inf / -1 for an empty or missing bucket."""
    n = dets.shape[0]
    ovmax, jmax = np.full(n, -np.inf), np.full(n, -1, np.int32)
    for d in range(n):
        b = int(bucket[d])
        if not (0 <= b < offs.shape[0] - 1) or offs[b + 1] <= offs[b]:
            continue
        g = gt[offs[b]:offs[b + 1]]
        bx0, by0, bx1, by1 = dets[d]
        iw = np.maximum(np.minimum(g[:, 2], bx1) - np.maximum(g[:, 0], bx0) + 1.0, 0.0)
        ih = np.maximum(np.minimum(g[:, 3], by1) - np.maximum(g[:, 1], by0) + 1.0, 0.0)
        inters = iw * ih
        uni = (bx1 - bx0 + 1.0) * (by1 - by0 + 1.0) + (g[:, 2] - g[:, 0] + 1.0) * (g[:, 3] - g[:, 1] + 1.0) - inters
        ov = inters / uni
        ovmax[d] = np.max(ov)
        jmax[d] = np.argmax(ov)
    return ovmax, jmax


def np_score_hbb(results, labels, n_classes, thr):
    """results: per scene (boxes [K,4] f64, scores [K] f64, labels [K]); labels: packed scene labels whose "boxes" are the
    oriented [G,8] ground truth.  -> per-detection dict + {class: (rec, prec, ap)}, as _scene_eval_np.np_score."""
    C = n_classes
    boxes = np.concatenate([r[0].reshape(-1, 4) for r in results]) if results else np.zeros((0, 4))
    scores = np.concatenate([r[1] for r in results]) if results else np.zeros(0)
    lab = np.concatenate([r[2] for r in results]).astype(np.int64) if results else np.zeros(0, np.int64)
    scene = np.concatenate([np.full(len(r[1]), s, np.int64) for s, r in enumerate(results)]) if results else np.zeros(0, np.int64)
    bucket = (scene * C + lab).astype(np.int32)
    offs = labels["offsets"]
    ovmax, jmax = np_match_hbb(boxes, bucket, rec4(labels["boxes"]), offs)
    rank = np.zeros(lab.shape[0], np.int64)
    order = {}
    for c in range(C):
        idx = np.nonzero(lab == c)[0]
        idx = idx[np.argsort(-scores[idx], kind="stable")]
        rank[idx] = np.arange(idx.size)
        order[c] = idx
    tp, fp = sev.np_mark(rank, ovmax, jmax, bucket, offs, labels["difficult"], thr)
    curves = {c: sev.np_curves(tp[order[c]], fp[order[c]], labels["npos_class"][c]) for c in range(C)}
    return {"ovmax": ovmax, "jmax": jmax, "tp": tp, "fp": fp, "rank": rank, "label": lab, "scene": scene}, curves
