"""Whole-scene detections against the scenes' own DOTA labels, matched on the device.

The DOTA devkit scores the *merged* detections against the labelTxt of the large images, VOC07 AP per class.  With files that
is scene.write_task1_merged -> task1.score_task1 -> voc_eval per class, which parses the text again and walks every detection
twice in Python.  Here the results of detect_scenes / OneStageRCNNWithTTA.detect_scenes go in as they are (device tensors):

  load_scene_labels(label_dir, scene_names, classnames)     the labelTxt files -> packed host arrays, bucket-major
  match_scenes(results, labels, n_classes, iou_thresh)      per detection ovmax / jmax / tp / fp / rank, on the device
  score_scenes(results, labels, classnames, cfg, ...)       rec / prec / ap per class, {"task1": {class: ap, "map": mean}}

What is computed is voc_eval (dafne/evaluation/voc_eval.py:41-224) for fixed inputs, per class c over all scenes of the call:
ground truth = the objects of class c of every scene in file order, npos = the non-difficult ones; detections = the rows with
label c in the order write_task1_merged writes them (scenes in call order, each scene in keep order), sorted by descending
score with a STABLE sort (voc_eval's np.argsort(-confidence) leaves the order of equal scores to numpy's build; the stable
order is one it can give and the one defined here; without equal scores the two agree).  A detection's candidates are the
boxes of its (scene, class) bucket that pass voc_eval's hull test (+1 on widths, heights and both areas); ovmax / jmax =
max / first argmax of iou_poly(ground truth, detection) over them (dafne_scene_match_hip).  jmax does not depend on the
marking's state, so "already claimed" is "a smaller sorted rank with the same jmax and ovmax > thr exists"
(dafne_scene_mark_hip); rec / prec / ap then come from the flags exactly as voc_eval computes them.
"""
import os
from collections import OrderedDict

import numpy as np
import torch

from .. import _lib
from . import dota_evaluation
from .voc_eval import voc_ap


def load_scene_labels(label_dir, scene_names, classnames, parse_gt=dota_evaluation.parse_gt):
    """One `<label_dir>/<scene>.txt` per scene (a missing file raises FileNotFoundError naming it); objects of classes outside
    `classnames` are dropped, as voc_eval never looks at them.  -> {"boxes" [G,8] f64, "offsets" [S*C+1] int32, "difficult"
    [G] bool, "npos" [S,C] int64 (non-difficult boxes per scene and class), "npos_class" [C], "scene_names", "classnames"}:
    boxes sorted bucket-major (bucket = scene * C + class), file order inside a bucket.  Two more keys carry what the bucket
    order loses, for scene_labels.split_scene_labels: "file_index" [G] int32, the object's position among the parsed objects of
    its scene's file (the order ImgSplit walks them in), and "difficult_value" [G] int32, the difficult field as written."""
    classnames = list(classnames)
    index = {c: k for k, c in enumerate(classnames)}
    S, C = len(scene_names), len(classnames)
    boxes, difficult, file_index, counts = [], [], [], np.zeros(S * C, dtype=np.int64)
    npos = np.zeros((S, C), dtype=np.int64)
    for s, name in enumerate(scene_names):
        path = os.path.join(label_dir, "%s.txt" % name)
        if not os.path.isfile(path):
            raise FileNotFoundError("scene labels: no label file for scene %r: %s" % (name, path))
        per_class = [[] for _ in range(C)]
        for pos, o in enumerate(parse_gt(path)):
            k = index.get(o["name"])
            if k is not None:
                per_class[k].append((pos, o))
        for k, objs in enumerate(per_class):
            counts[s * C + k] = len(objs)
            for pos, o in objs:
                boxes.append(o["bbox"])
                difficult.append(o["difficult"])
                file_index.append(pos)
            npos[s, k] = sum(1 for _, o in objs if not bool(o["difficult"]))
    G = len(boxes)
    if G >= 2 ** 31:
        raise ValueError("scene labels: %d boxes overflow the int32 offsets" % G)
    offsets = np.zeros(S * C + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    return {"boxes": np.asarray(boxes, dtype=np.float64).reshape(G, 8), "offsets": offsets,
            "difficult": np.asarray(difficult).astype(bool).reshape(G), "npos": npos, "npos_class": npos.sum(0),
            "scene_names": list(scene_names), "classnames": classnames,
            "file_index": np.asarray(file_index, dtype=np.int32).reshape(G),
            "difficult_value": np.asarray(difficult, dtype=np.int32).reshape(G)}


def rec4(boxes):
    """dota_utils.py:122-127 (dots4ToRec4) on [N,8] rows -> [N,4] xmin, ymin, xmax, ymax: the horizontal ground truth of
    parse_dota_rec (:109-119)."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 8)
    return np.stack([b[:, 0::2].min(1), b[:, 1::2].min(1), b[:, 0::2].max(1), b[:, 1::2].max(1)], axis=1) if b.shape[0] else \
        np.zeros((0, 4), dtype=np.float64)


def match_scenes(results, labels, n_classes, iou_thresh, task="task1"):
    """results: detect_scenes' dicts (corners [K,8] f64, scores [K] f64, labels [K], device tensors), one per scene of
    `labels`, in the same order.  Everything stays on the device; nothing is read back here.  -> dict of device tensors over
    the N detections in call order (scene by scene, each scene in keep order):
      "ovmax" f64, "jmax" int32 (index inside the (scene, class) bucket, -1: no candidate), "tp" / "fp" uint8,
      "rank" int64 (position in its class's stably sorted order), "label" int64 (n_classes: a label outside the classes, in no
      class's list), "scene" int64, "order" int64 (the detections class-major, each class in sorted order: order[k] indexes
      the arrays above) and "class_start" [n_classes + 2] int64 (class c is order[class_start[c]:class_start[c + 1]]).
    task "task2": the results' "task2" entries (boxes [K,4] f64) against rec4 of the labels' boxes, ov = voc_eval's own
    inters / uni on the rectangles over every box of the bucket (dafne_scene_match_hbb_hip); everything else as above."""
    if task not in ("task1", "task2"):
        raise ValueError("match_scenes: task %r is neither \"task1\" nor \"task2\"" % (task,))
    hbb = task == "task2"
    if hbb:
        if any("task2" not in r for r in results):
            raise ValueError("match_scenes: task2 needs the results of detect_scenes(..., tasks=(\"task1\", \"task2\"))")
        results = [{"corners": r["task2"]["boxes"], "scores": r["task2"]["scores"], "labels": r["task2"]["labels"]} for r in results]
    wd = 4 if hbb else 8
    C = int(n_classes)
    S = len(results)
    off = labels["offsets"]
    if off.shape[0] != S * C + 1:
        raise ValueError("match_scenes: labels hold %d buckets, the call has %d scenes x %d classes" % (off.shape[0] - 1, S, C))
    dev = results[0]["corners"].device if S else torch.device("cuda", torch.cuda.current_device())
    L = _lib.load()
    with torch.cuda.device(dev):
        if S:
            corners = torch.cat([r["corners"].reshape(-1, wd) for r in results]).to(device=dev, dtype=torch.float64).contiguous()
            scores = torch.cat([r["scores"].reshape(-1) for r in results]).to(device=dev, dtype=torch.float64)
            lab = torch.cat([r["labels"].reshape(-1) for r in results]).to(device=dev, dtype=torch.int64)
            sizes = torch.tensor([int(r["scores"].numel()) for r in results], dtype=torch.int64)
            scene = torch.repeat_interleave(torch.arange(S, dtype=torch.int64), sizes).to(dev)
        else:
            corners = torch.zeros((0, wd), dtype=torch.float64, device=dev)
            scores = torch.zeros(0, dtype=torch.float64, device=dev)
            lab = scene = torch.zeros(0, dtype=torch.int64, device=dev)
        N = int(corners.shape[0])
        if N >= 2 ** 31:
            raise ValueError("match_scenes: %d detections overflow the int32 ranks" % N)
        inside = (lab >= 0) & (lab < C)
        lab = torch.where(inside, lab, torch.full_like(lab, C))
        bucket = torch.where(inside, scene * C + lab, torch.full_like(lab, -1)).to(torch.int32)
        # descending score, stable; then class-major, stable: every class in its stably sorted order
        by_score = torch.sort(scores, descending=True, stable=True).indices
        order = by_score[torch.sort(lab[by_score], stable=True).indices]
        class_start = torch.searchsorted(lab[order].contiguous(), torch.arange(C + 2, device=dev, dtype=torch.int64))
        pos = torch.empty(N, dtype=torch.int64, device=dev)
        pos[order] = torch.arange(N, device=dev, dtype=torch.int64)
        rank = pos - class_start[lab]
        rank32 = rank.to(torch.int32)

        G = int(labels["boxes"].shape[0])
        gt = torch.from_numpy(np.ascontiguousarray(rec4(labels["boxes"]) if hbb else labels["boxes"], dtype=np.float64)).to(dev)
        offs = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int32)).to(dev)
        diff = torch.from_numpy(np.ascontiguousarray(labels["difficult"]).astype(np.uint8)).to(dev)
        ovmax = torch.empty(N, dtype=torch.float64, device=dev)
        jmax = torch.empty(N, dtype=torch.int32, device=dev)
        tp = torch.empty(N, dtype=torch.uint8, device=dev)
        fp = torch.empty(N, dtype=torch.uint8, device=dev)
        st = _lib.current_stream()
        if hbb:
            _lib.check(L.dafne_scene_match_hbb_hip(_lib.ptr(corners), _lib.ptr(bucket), N, _lib.ptr(gt), _lib.ptr(offs), S * C, G,
                                                   _lib.ptr(ovmax), _lib.ptr(jmax), st), "dafne_scene_match_hbb_hip")
        else:
            _lib.check(L.dafne_scene_match_hip(_lib.ptr(corners), _lib.ptr(bucket), N, _lib.ptr(gt), _lib.ptr(offs), S * C, G,
                                               _lib.ptr(ovmax), _lib.ptr(jmax), st), "dafne_scene_match_hip")
        nbytes = L.dafne_scene_mark_workspace_bytes(G)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(L.dafne_scene_mark_hip(_lib.ptr(rank32), _lib.ptr(ovmax), _lib.ptr(jmax), _lib.ptr(bucket), N, _lib.ptr(offs),
                                          S * C, _lib.ptr(diff), G, float(iou_thresh), _lib.ptr(tp), _lib.ptr(fp), _lib.ptr(ws),
                                          nbytes, st), "dafne_scene_mark_hip")
    return {"ovmax": ovmax, "jmax": jmax, "tp": tp, "fp": fp, "rank": rank, "label": lab, "scene": scene, "order": order,
            "class_start": class_start}


def curves_from_flags(tp, fp, npos):
    """voc_eval.py:207-222 on one class's flags in sorted order: (rec, prec, ap) with the VOC07 11-point metric."""
    fp = np.cumsum(np.asarray(fp, dtype=np.float64))
    tp = np.cumsum(np.asarray(tp, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):        # npos = 0: rec is nan, as voc_eval's is
        rec = tp / float(npos)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, True)


def score_scenes(results, labels, classnames, cfg, output_folder=None, task="task1"):
    """What task1.score_task1 returns for the same detections written with scene.write_task1_merged and the same label
    files -- {"task1": {<class>: ap, ..., "map": mean}}, the same floats -- without the files: match_scenes on the device,
    one host read of the flags, then rec / prec / ap per class with voc_ap (cumulative sums; no per-detection Python).
    Also returned: "rec" / "prec" ({class: array}, voc_eval's), "per_scene" [scenes, classes, 3] int64 = tp, fp, npos of every
    (scene, class), to find the scenes that cost the score, and "match" (match_scenes' device tensors).
    output_folder: results.txt as score_task1 writes it.  scores_overlap.csv is NOT written: it is the plotting input of the
    reference and carries the reference's quirk of indexing the unsorted confidences.
    task="task2": DOTA's horizontal-box task on the results' "task2" entries -> {"task2": {...}}, results_task2.txt (never
    results.txt).  The ground truth is dots4ToRec4 of the label boxes and the overlap is voc_eval's own hull stage
    (voc_eval.py:158-173) -- the DOTA devkit's Task2 evaluation; the same sort, marking kernel and single host read."""
    classnames = list(classnames)
    C, S = len(classnames), len(results)
    m = match_scenes(results, labels, C, cfg.TEST.IOU_TH, task=task)
    order = m["order"]
    host = torch.stack([m["tp"][order].to(torch.int64), m["fp"][order].to(torch.int64), m["scene"][order]])
    host = torch.cat([host.reshape(-1), m["class_start"]]).cpu().numpy()          # the one host read
    N = int(order.shape[0])
    tp, fp, scene = host[:N], host[N:2 * N], host[2 * N:3 * N]
    start = host[3 * N:]
    ap_table = OrderedDict()
    rec, prec = OrderedDict(), OrderedDict()
    per_scene = np.zeros((S, C, 3), dtype=np.int64)
    per_scene[:, :, 2] = labels["npos"]
    mean_ap = 0.0
    for c, name in enumerate(classnames):
        a, b = int(start[c]), int(start[c + 1])
        rec[name], prec[name], ap = curves_from_flags(tp[a:b], fp[a:b], labels["npos_class"][c])
        per_scene[:, c, 0] = np.bincount(scene[a:b], weights=tp[a:b], minlength=S)[:S]
        per_scene[:, c, 1] = np.bincount(scene[a:b], weights=fp[a:b], minlength=S)[:S]
        mean_ap += ap
        ap_table[name] = ap
    ap_table["map"] = mean_ap / len(classnames)
    if output_folder is not None:
        os.makedirs(output_folder, exist_ok=True)
        with open(os.path.join(output_folder, "results_task2.txt" if task == "task2" else "results.txt"), "w") as f:
            for k, v in ap_table.items():
                f.write(f"{k: <18}: {v:2.4f}\n")
    return {"task2" if task == "task2" else "task1": ap_table, "rec": rec, "prec": prec, "per_scene": per_scene, "match": m}
