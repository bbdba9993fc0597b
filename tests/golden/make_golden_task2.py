#!/usr/bin/env python3
"""Generate tests/golden/task2_merge.npz by RUNNING THE REFERENCE's horizontal-box half of the tile merge here.

Only runs where /root/reference exists.  The reference's dafne/utils/ResultMerge_multi_process.py (py_cpu_nms,
mergesingle) and dafne/utils/dota_utils.py (dots4ToRec4) are imported from where they lie under the stand-ins of
make_golden_eval.py (polyiou, shapely, detectron2 -> stub modules; neither function here reaches them).

Stored: the inputs and, for each, what the reference returns --
  nms_in_<case> [M,5] f64, nms_keep_<case>_<10|30> (py_cpu_nms at 0.1 / 0.3)
  rec_in [N,8] f64, rec_out [N,4] (dots4ToRec4)
  task1_in_<class> (tile-level Task1 lines), task2_in_<class> (the same lines as Task2 text: dots4ToRec4 of the parsed
  floats written "%.2f"), task2_out_<class> (mergesingle(dst, py_cpu_nms, file) on that text).
numpy's default argsort is not stable (it reorders equal scores in arrays as short as 5), so every group the reference sorts
has pairwise distinct scores; the generator asserts it.  Equal scores are pinned against the stable numpy restatement
(tests/_task2_np.py) only.

Usage:  python tests/golden/make_golden_task2.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stubs, load_ref, rrects)

SIZES = (0, 1, 2, 63, 64, 65, 130, 1300)
THRESHOLDS = (0.1, 0.3)


def unique_scores(n, rng, lo=500, hi=9999):
    return rng.choice(np.arange(lo, hi), size=n, replace=False) / 10000.0


def boxes(n, rng, extent, lo=10.0, hi=120.0):
    c = rng.uniform(0, extent, (n, 2))
    wh = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    return np.round(np.concatenate([c - wh / 2, c + wh / 2], 1), 2)


def nms_cases(rng):
    cases = {}
    for n in SIZES:
        cases["n%d" % n] = boxes(n, rng, extent=40.0 * np.sqrt(max(n, 1)))
    # a dense cluster: long suppression chains (A removes B, so B must not remove C)
    c = boxes(300, rng, extent=90.0, lo=30.0, hi=70.0)
    chain = np.array([[10.0 * k, 500.0, 10.0 * k + 14.0, 520.0] for k in range(40)])     # neighbours overlap, second neighbours less
    cases["cluster"] = np.concatenate([c, chain])
    # boxes that touch within the +1: x1_j == x2_i (one shared pixel column), x1_j == x2_i + 1 (w = 0), one past it, half a pixel
    t = []
    for k, gap in enumerate((0.0, 1.0, 2.0, 0.5)):
        t.append([0.0, 40.0 * k, 2.0, 40.0 * k + 10.0])           # narrow: the shared pixel column decides at 0.1 (ovr 0.2)
        t.append([2.0 + gap, 40.0 * k, 4.0 + gap, 40.0 * k + 10.0])
    t.append([0.0, 200.0, 0.0, 200.0])          # a single pixel, twice: ovr 1
    t.append([0.0, 200.0, 0.0, 200.0])
    # one reversed box (x2 < x1 - 1: a negative "area") among boxes it overlaps
    t.append([100.0, 100.0, 140.0, 140.0])
    t.append([135.0, 105.0, 105.0, 135.0])
    t.append([110.0, 110.0, 150.0, 150.0])
    cases["touch"] = np.array(t)
    out = {}
    for name, b in cases.items():
        out[name] = np.concatenate([b, unique_scores(len(b), rng)[:, None]], 1) if len(b) else np.zeros((0, 5))
    return out


def synth_tiles(rng):
    """Two original images cut into 1024 tiles (stride 824) at rate 1 and 0.5; every object is reported by each tile it falls
    into, with sub-pixel jitter."""
    lines = {"plane": [], "small-vehicle": []}
    for img, size in (("P0001", 2000), ("P0706", 1024)):
        for cls, n in (("plane", 40), ("small-vehicle", 220)):
            objs = mg.rrects(n, rng, extent=float(size), lo=10.0 if cls != "plane" else 40.0,
                             hi=60.0 if cls == "small-vehicle" else 200.0).astype(np.float64)
            if cls == "small-vehicle":      # parking-lot cluster
                objs[: n // 2] = mg.rrects(n // 2, rng, extent=220.0, lo=10, hi=40).astype(np.float64) + 300.0
            for rate in (1.0, 0.5):
                scaled = size * rate
                starts = list(range(0, max(int(scaled) - 1024, 0) + 1, 824))
                if starts[-1] + 1024 < scaled:
                    starts.append(int(scaled) - 1024)
                for x in starts:
                    for y in starts:
                        t = objs * rate - np.array([x, y] * 4)
                        cx, cy = t[:, 0::2].mean(1), t[:, 1::2].mean(1)
                        inside = (cx > 0) & (cx < 1024) & (cy > 0) & (cy < 1024)
                        for k in np.nonzero(inside & (rng.uniform(size=n) < 0.8))[0]:
                            q = t[k] + rng.normal(0, 0.7, 8)
                            lines[cls].append(("%s__%s__%d___%d" % (img, "1" if rate == 1.0 else "0.5", x, y),
                                               " ".join("%.2f" % v for v in q)))
    for cls in lines:       # scores unique per FILE at the printed precision (see module docstring)
        sc = unique_scores(len(lines[cls]), rng)
        lines[cls] = ["%s %.4f %s" % (nm, s, q) for (nm, q), s in zip(lines[cls], sc)]
    return lines


def main():
    mg.install_stubs()
    mg._mod("polyiou", VectorDouble=list, iou_poly=None)
    mg._mod("shapely")
    mg._mod("shapely.geometry")
    du = mg.load_ref("dafne.utils.dota_utils")
    rm = mg.load_ref("dafne.utils.ResultMerge_multi_process")

    rng = np.random.default_rng(20261017)
    fx = {}
    for name, d in nms_cases(rng).items():
        assert np.unique(d[:, 4]).size == d.shape[0], name
        fx["nms_in_" + name] = d
        for th in THRESHOLDS:
            keep = np.array(rm.py_cpu_nms(d, th), dtype=np.int64)
            fx["nms_keep_%s_%d" % (name, round(th * 100))] = keep
            print("py_cpu_nms %-8s thr %.1f: %5d rows -> %5d kept" % (name, th, d.shape[0], keep.size))
    fx["nms_cases"] = np.array(sorted(k[len("nms_in_"):] for k in fx if k.startswith("nms_in_")))

    r8 = np.round(mg.rrects(200, rng, extent=3000.0).astype(np.float64), 2)
    r8[:20] = np.round(r8[:20])                      # equal coordinates among a box's corners
    fx["rec_in"] = r8
    fx["rec_out"] = np.array([du.dots4ToRec4([(p[0], p[1]), (p[2], p[3]), (p[4], p[5]), (p[6], p[7])]) for p in r8])

    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "Task2"), os.path.join(tmp, "Task2_merged")
        os.makedirs(src)
        os.makedirs(dst)
        for c, ls in synth_tiles(rng).items():
            t2 = []
            for line in ls:
                tok = line.split(" ")
                assert len(tok) == 10
                v = [float(x) for x in tok[2:]]
                rec = du.dots4ToRec4([(v[0], v[1]), (v[2], v[3]), (v[4], v[5]), (v[6], v[7])])
                t2.append(tok[0] + " " + tok[1] + " " + " ".join("%.2f" % x for x in rec))
            scores = [x.split(" ")[1] for x in t2]
            assert len(set(scores)) == len(scores), c
            with open(os.path.join(src, "Task2_%s.txt" % c), "w") as f:
                f.write("\n".join(t2) + "\n")
            rm.mergesingle(dst, rm.py_cpu_nms, os.path.join(src, "Task2_%s.txt" % c))
            with open(os.path.join(dst, "Task2_%s.txt" % c)) as f:
                merged = [x.rstrip("\n") for x in f.readlines()]
            fx["task1_in_" + c], fx["task2_in_" + c], fx["task2_out_" + c] = np.array(ls), np.array(t2), np.array(merged)
            print("mergebyrec %-14s %5d tile rows -> %5d merged rows" % (c, len(t2), len(merged)))
        fx["classes"] = np.array(sorted(k[len("task2_in_"):] for k in fx if k.startswith("task2_in_")))
    path = os.path.join(HERE, "task2_merge.npz")
    np.savez_compressed(path, **fx)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
