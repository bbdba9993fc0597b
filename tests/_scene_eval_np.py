"""The scene scorer's definition in plain numpy (shared by test_scene_eval_cpu.py and test_gpu_scene_eval.py): voc_eval for
fixed inputs with the greedy marking restated as a rank minimum per ground-truth box.  Nothing here imports dafne_amd; the
polygon IoU comes from the caller (the CPU oracle)."""
import os

import numpy as np


def hull(b):
    return b[..., 0::2].min(-1), b[..., 1::2].min(-1), b[..., 0::2].max(-1), b[..., 1::2].max(-1)


def hull_candidates(bbgt, bb):
    """voc_eval.py:150-178: +1 on widths, heights and both areas."""
    gx0, gy0, gx1, gy1 = hull(bbgt)
    bx0, by0, bx1, by1 = hull(bb)
    iw = np.maximum(np.minimum(gx1, bx1) - np.maximum(gx0, bx0) + 1.0, 0.0)
    ih = np.maximum(np.minimum(gy1, by1) - np.maximum(gy0, by0) + 1.0, 0.0)
    inters = iw * ih
    uni = (bx1 - bx0 + 1.0) * (by1 - by0 + 1.0) + (gx1 - gx0 + 1.0) * (gy1 - gy0 + 1.0) - inters
    return np.where(inters / uni > 0)[0]


def np_match(dets, bucket, gt, offs, iou_pairs):
    """-> ovmax [N] f64, jmax [N] int32 (index inside the bucket; -inf / -1 without candidates)."""
    n = dets.shape[0]
    cand, pg, pd = [], [], []
    for d in range(n):
        b = int(bucket[d])
        idx = np.zeros(0, np.int64)
        if 0 <= b < offs.shape[0] - 1 and offs[b + 1] > offs[b]:
            idx = hull_candidates(gt[offs[b]:offs[b + 1]], dets[d])
        cand.append(idx)
        if idx.size:
            pg.append(gt[offs[b] + idx])
            pd.append(np.repeat(dets[d:d + 1], idx.size, 0))
    ious = iou_pairs(np.concatenate(pg), np.concatenate(pd)) if pg else np.zeros(0)      # ground truth first
    ovmax, jmax = np.full(n, -np.inf), np.full(n, -1, np.int32)
    o = 0
    for d in range(n):
        k = cand[d].size
        if k:
            ov = ious[o:o + k]
            o += k
            ovmax[d] = np.max(ov)
            jmax[d] = cand[d][np.argmax(ov)]
    return ovmax, jmax


def np_mark(rank, ovmax, jmax, bucket, offs, difficult, thr):
    """tp / fp [N] uint8: claimed first = the smallest rank among the detections with this box and ovmax > thr."""
    n = rank.shape[0]
    over = ovmax > thr
    g = np.where(over, offs[np.clip(bucket, 0, offs.shape[0] - 2)].astype(np.int64) + jmax, -1)
    hit = over & ~difficult[np.clip(g, 0, max(difficult.shape[0] - 1, 0))] if difficult.shape[0] else np.zeros(n, bool)
    first = np.full(max(difficult.shape[0], 1), np.iinfo(np.int64).max)
    np.minimum.at(first, g[hit], rank[hit])
    tp = hit & (first[np.clip(g, 0, first.shape[0] - 1)] == rank)
    fp = ~over | (hit & ~tp)
    return tp.astype(np.uint8), fp.astype(np.uint8)


def voc_ap07(rec, prec):
    ap = 0.0
    for t in np.arange(0.0, 1.1, 0.1):
        sel = rec >= t
        p = np.max(prec[sel]) if np.sum(sel) != 0 else 0
        ap = ap + p / 11.0
    return ap


def np_curves(tp, fp, npos):
    fp = np.cumsum(fp.astype(np.float64))
    tp = np.cumsum(tp.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap07(rec, prec)


def np_score(results, labels, n_classes, thr, iou_pairs):
    """results: per scene (corners [K,8] f64, scores [K] f64, labels [K]) numpy.  -> per-detection dict + {class: (rec, prec,
    ap)}; detections in call order, per class sorted by descending score with a stable sort."""
    C = n_classes
    corners = np.concatenate([r[0].reshape(-1, 8) for r in results]) if results else np.zeros((0, 8))
    scores = np.concatenate([r[1] for r in results]) if results else np.zeros(0)
    lab = np.concatenate([r[2] for r in results]).astype(np.int64) if results else np.zeros(0, np.int64)
    scene = np.concatenate([np.full(len(r[1]), s, np.int64) for s, r in enumerate(results)]) if results else np.zeros(0, np.int64)
    bucket = (scene * C + lab).astype(np.int32)
    offs = labels["offsets"]
    ovmax, jmax = np_match(corners, bucket, labels["boxes"], offs, iou_pairs)
    rank = np.zeros(lab.shape[0], np.int64)
    order = {}
    for c in range(C):
        idx = np.nonzero(lab == c)[0]
        idx = idx[np.argsort(-scores[idx], kind="stable")]
        rank[idx] = np.arange(idx.size)
        order[c] = idx
    tp, fp = np_mark(rank, ovmax, jmax, bucket, offs, labels["difficult"], thr)
    curves = {c: np_curves(tp[order[c]], fp[order[c]], labels["npos_class"][c]) for c in range(C)}
    return {"ovmax": ovmax, "jmax": jmax, "tp": tp, "fp": fp, "rank": rank, "label": lab, "scene": scene}, curves


def pack_labels(objs_per_scene, classnames):
    """parse_gt's objects per scene -> the packed arrays load_scene_labels returns, written independently of it."""
    C = len(classnames)
    boxes, diff, offs = [], [], [0]
    npos = np.zeros((len(objs_per_scene), C), np.int64)
    for s, objs in enumerate(objs_per_scene):
        for c, name in enumerate(classnames):
            sel = [o for o in objs if o["name"] == name]
            boxes += [o["bbox"] for o in sel]
            diff += [bool(o["difficult"]) for o in sel]
            npos[s, c] = sum(1 for o in sel if not o["difficult"])
            offs.append(len(boxes))
    return {"boxes": np.array(boxes, np.float64).reshape(-1, 8), "offsets": np.array(offs, np.int32),
            "difficult": np.array(diff, bool).reshape(-1), "npos": npos, "npos_class": npos.sum(0)}


def fixture_case(g, label_dir):
    """tests/golden/scene_eval.npz -> (scene names, class names, threshold, per-scene results); label files written."""
    names = [str(x) for x in g["scene_names"]]
    classes = [str(x) for x in g["classnames"]]
    os.makedirs(label_dir, exist_ok=True)
    for n, t in zip(names, g["label_txt"]):
        with open(os.path.join(label_dir, n + ".txt"), "w") as f:
            f.write(str(t))
    results = [(g["det%d_corners" % s], g["det%d_scores" % s], g["det%d_labels" % s]) for s in range(len(names))]
    return names, classes, float(g["iou_thresh"]), results


def same(a, b):
    """array_equal, nan-aware, on float64 arrays of equal shape."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
