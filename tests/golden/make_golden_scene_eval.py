#!/usr/bin/env python3
"""Generate tests/golden/scene_eval.npz: the reference's voc_eval and parse_gt, RUN HERE, on scene labels + merged detections.

Synthetic DOTA scenes (labelTxt texts with the two header lines, difficult flags) and merged scene-coordinate detections in the
form scene.write_task1_merged writes them are scored by the reference's own dafne/evaluation/voc_eval.py (loaded as in
make_golden_eval.py: stubs, polyiou over the reference's polyiou.cpp compiled into oracle/_ref) with the reference's own
parse_gt (dafne/evaluation/dota_evaluation.py; the definition is executed from where it lies, as make_golden_datasets.py
does).  Scores are pairwise distinct per class, so the reference's unstable argsort has one answer.  Four classes hold every
outcome of the marking (tp, duplicate fp, low-IoU fp, ignored on a difficult box); one class has detections and no ground
truth, one ground truth and no detections.  The fixture stores the label texts, the detections per scene and rec / prec / ap.

    python tests/golden/make_golden_scene_eval.py          (build container only)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_eval as mge  # noqa: E402
from make_golden_datasets import ref_functions  # noqa: E402

CLASSES = ["plane", "ship", "small-vehicle", "large-vehicle", "harbor", "helicopter"]
FULL = CLASSES[:4]             # every outcome present
NO_GT, NO_DET = "harbor", "helicopter"
SCENES = [("P0003", 2600), ("P0019", 1500), ("P0706", 4000)]
IOU_TH = 0.5


def synth(rng):
    """-> label text per scene, per scene (corners [K,8] f64 at two decimals, labels [K]) in class-major order."""
    texts, dets = [], []
    for name, size in SCENES:
        rows = ["imagesource:GoogleEarth", "gsd:0.146"]
        corners, labels = [], []
        for c, cname in enumerate(CLASSES):
            n = {"plane": 14, "ship": 30, "small-vehicle": 45, "large-vehicle": 20, NO_GT: 0, NO_DET: 6}[cname]
            g = mg.rrects(n, rng, extent=float(size), lo=15.0, hi=60.0 if cname == "small-vehicle" else 160.0).astype(np.float64)
            if cname == "small-vehicle":                 # a parking lot: hulls of neighbours overlap, polygons mostly do not
                g[: n // 2] = mg.rrects(n // 2, rng, extent=260.0, lo=12.0, hi=40.0).astype(np.float64) + 400.0
            g = np.round(g, 1)
            diff = (rng.uniform(size=n) < 0.2).astype(int)
            for k in range(n):
                # 9-field lines (no difficult column) occur in DOTA files: parse_gt reads them as difficult = 0
                tail = " %d" % diff[k] if (diff[k] or k % 5) else ""
                rows.append(" ".join("%.1f" % v for v in g[k]) + " " + cname + tail)
            if cname == NO_DET:
                continue
            d = []
            for k in range(n):
                if rng.uniform() < 0.9:
                    d.append(g[k] + rng.normal(0, 1.2, 8))
                if rng.uniform() < 0.35:
                    d.append(g[k] + rng.normal(0, 1.5, 8))          # duplicate: fp once the box is claimed
                if rng.uniform() < 0.3:
                    d.append(g[k] + np.tile(rng.normal(0, 0.35, 2) * (g[k].max() - g[k].min()), 4))   # shifted: low IoU
            nfp = 5 if cname == NO_GT else max(3, n // 4)
            d += list(mg.rrects(nfp, rng, extent=float(size), lo=15.0, hi=120.0).astype(np.float64))
            corners += d
            labels += [c] * len(d)
        # an object of a class outside the list: voc_eval never asks for it
        rows.append("10.0 10.0 60.0 10.0 60.0 40.0 10.0 40.0 container-crane 0")
        texts.append("\n".join(rows) + "\n")
        dets.append((np.round(np.array(corners, np.float64).reshape(-1, 8), 2), np.array(labels, np.int64)))
    return texts, dets


def main():
    assert os.path.isdir(mg.REF), "reference tree not present: fixtures can only be made in the build container"
    mg.install_stubs()
    mg._mod("polyiou", VectorDouble=mge.VectorDouble, iou_poly=mge.iou_poly)
    mg._mod("shapely")
    mg._mod("shapely.geometry")
    m = mg._mod("dafne.evaluation")
    m.__path__ = [os.path.join(mg.REF, "dafne", "evaluation")]
    if not hasattr(np, "bool"):
        np.bool = bool          # voc_eval.py:98 uses the alias numpy 2 removed
    ve = mg.load_ref("dafne.evaluation.voc_eval")
    parse_gt = ref_functions("dafne/evaluation/dota_evaluation.py", ["parse_gt"], {})["parse_gt"]

    rng = np.random.default_rng(20261016)
    texts, dets = synth(rng)
    names = [n for n, _ in SCENES]
    # scores: 4 decimals, pairwise distinct within a class over all scenes
    per_class = {c: mge.unique_scores(sum(int((l == c).sum()) for _, l in dets), rng) for c in range(len(CLASSES))}
    used = {c: 0 for c in per_class}
    scores = []
    for _, l in dets:
        s = np.zeros(len(l))
        for c in per_class:
            k = int((l == c).sum())
            s[l == c] = per_class[c][used[c]:used[c] + k]
            used[c] += k
        scores.append(s)
    fx = {"classnames": np.array(CLASSES), "scene_names": np.array(names), "iou_thresh": np.float64(IOU_TH),
          "label_txt": np.array(texts)}
    for s, ((corners, labels), sc) in enumerate(zip(dets, scores)):
        fx["det%d_corners" % s], fx["det%d_scores" % s], fx["det%d_labels" % s] = corners, sc, labels
    with tempfile.TemporaryDirectory() as tmp:
        lab = os.path.join(tmp, "labelTxt")
        os.makedirs(lab)
        for n, t in zip(names, texts):
            with open(os.path.join(lab, n + ".txt"), "w") as f:
                f.write(t)
        with open(os.path.join(tmp, "imageset.txt"), "w") as f:
            f.write("\n".join(names))
        total = 0
        for c, cname in enumerate(CLASSES):
            # the lines of scene.write_task1_merged: scenes in call order, each scene's rows in their own order
            nd = 0
            with open(os.path.join(tmp, "Task1_%s.txt" % cname), "w") as f:
                for n, (corners, labels), sc in zip(names, dets, scores):
                    for i in np.nonzero(labels == c)[0]:
                        f.write(n + " " + str(float(sc[i])) + " " + " ".join(map(str, corners[i].tolist())) + "\n")
                        nd += 1
            rec, prec, ap, so = ve.voc_eval(os.path.join(tmp, "Task1_{:s}.txt"), os.path.join(lab, "{:s}.txt"),
                                            os.path.join(tmp, "imageset.txt"), cname, ovthresh=IOU_TH, use_07_metric=True,
                                            parse_gt=parse_gt)
            fx["rec_" + cname], fx["prec_" + cname], fx["ap_" + cname] = np.asarray(rec, np.float64), np.asarray(prec, np.float64), np.float64(ap)
            objs = [o for n in names for o in parse_gt(os.path.join(lab, n + ".txt")) if o["name"] == cname]
            npos = sum(1 for o in objs if not o["difficult"])
            tp = sum(1 for r in so if r[2] == 1)
            dup = sum(1 for r in so if r[2] == 0)
            assert tp > 0 or cname not in FULL, cname
            fp = int(round(tp / prec[-1] - tp)) if tp else nd       # prec[-1] = tp / (tp + fp); the two bare classes: all fp / empty
            low, ignored = fp - dup, nd - tp - fp
            print("%-14s %4d dets %3d gt (npos %3d): tp %3d  dup fp %3d  low-IoU fp %3d  ignored %3d  ap %.6f"
                  % (cname, nd, len(objs), npos, tp, dup, low, ignored, ap))
            total += nd
            if cname in FULL:
                assert min(tp, dup, low, ignored) > 0, (cname, tp, dup, low, ignored)
                assert len(rec) == nd and rec[-1] == tp / float(npos)
            elif cname == NO_GT:
                assert nd > 0 and not objs and ap == 0.0 and np.isnan(rec).all() and len(rec) == nd
            else:
                assert nd == 0 and objs and ap == 0.0 and len(rec) == 0
        assert total >= 300, total
    np.savez_compressed(os.path.join(HERE, "scene_eval.npz"), **fx)
    print("wrote", os.path.join(HERE, "scene_eval.npz"), os.path.getsize(os.path.join(HERE, "scene_eval.npz")), "bytes")


if __name__ == "__main__":
    main()
