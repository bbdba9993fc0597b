"""GPU: whole-scene detections scored against scene labels on the device (dafne_amd/evaluation/scene_eval.py; the kernels
dafne_scene_match_hip / dafne_scene_mark_hip in csrc/poly_nms.hip).  Every comparison is exact.

  * both kernels against the numpy restatement (tests/_scene_eval_np.py, IoU from the CPU oracle) on random buckets: empty
    buckets, buckets of more than 64 and more than 4096 boxes, identical boxes (lowest index wins), hull-passing pairs with
    IoU 0, a pair with zero union, detections of scenes without labels of their class, N = 0 and G = 0;
  * score_scenes on tests/golden/scene_eval.npz equals the REFERENCE's rec / prec / ap;
  * against the file route on the same detections -- write_task1_merged + label files + imageset.txt + voc_eval per class /
    score_task1 -- with distinct scores as is, and with many equal scores with numpy.argsort in its kind="stable" form for the
    duration of the voc_eval calls: rec, prec, ap, the task1 dict and results.txt equal;
  * end to end for two configs (one through OneStageRCNNWithTTA.detect_scenes): labels made from the model's own detections,
    score_scenes equals score_task1 on the written files, 0 < map < 1;
  * per-detection tp / fp do not depend on the order of the scenes; two runs give the same bits;
  * tools/eval_net.py --scene-dir --scene-labels in a child process writes the same results.txt."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import oracle
import _scene_eval_np as ref
from conftest import rrects

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_SHAPES = [(700, 900), (1024, 1024), (1500, 1900)]
TTA_OPTS = ("TEST.AUG.MIN_SIZES", [600, 800], "TEST.AUG.MAX_SIZE", 1200, "TEST.AUG.HFLIP", True, "TEST.AUG.VFLIP", False)


def dev():
    return torch.device("cuda", 0)


def cfg_thr(thr):
    return types.SimpleNamespace(TEST=types.SimpleNamespace(IOU_TH=thr))


def to_device(results):
    return [{"corners": torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64)).to(dev()),
             "scores": torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)).to(dev()),
             "labels": torch.from_numpy(np.ascontiguousarray(l, dtype=np.int64)).to(dev())} for c, s, l in results]


def to_host(res):
    return [(r["corners"].cpu().numpy().astype(np.float64).reshape(-1, 8), r["scores"].cpu().numpy().astype(np.float64),
             r["labels"].cpu().numpy().astype(np.int64)) for r in res]


# ------------------------------------------------------------------------------------------------------------ the kernels
def run_match(dets, bucket, gt, offs):
    from dafne_amd import _lib
    L = _lib.load()
    n, g = dets.shape[0], gt.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(dets, dtype=np.float64)).to(dev())
    b = torch.from_numpy(np.ascontiguousarray(bucket, dtype=np.int32)).to(dev())
    t = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.float64)).to(dev())
    o = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.int32)).to(dev())
    ovmax = torch.full((n,), 7.0, dtype=torch.float64, device=dev())
    jmax = torch.full((n,), 7, dtype=torch.int32, device=dev())
    _lib.check(L.dafne_scene_match_hip(_lib.ptr(d), _lib.ptr(b), n, _lib.ptr(t), _lib.ptr(o), offs.shape[0] - 1, g, _lib.ptr(ovmax),
                                       _lib.ptr(jmax), _lib.current_stream()), "dafne_scene_match_hip")
    return ovmax.cpu().numpy(), jmax.cpu().numpy()


def run_mark(rank, ovmax, jmax, bucket, offs, difficult, thr):
    from dafne_amd import _lib
    L = _lib.load()
    n, g = rank.shape[0], difficult.shape[0]
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev())      # noqa: E731
    r, ov, jm, b, o, df = (up(rank, np.int32), up(ovmax, np.float64), up(jmax, np.int32), up(bucket, np.int32), up(offs, np.int32),
                           up(difficult, np.uint8))
    tp = torch.full((n,), 7, dtype=torch.uint8, device=dev())
    fp = torch.full((n,), 7, dtype=torch.uint8, device=dev())
    nbytes = L.dafne_scene_mark_workspace_bytes(g)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    _lib.check(L.dafne_scene_mark_hip(_lib.ptr(r), _lib.ptr(ov), _lib.ptr(jm), _lib.ptr(b), n, _lib.ptr(o), offs.shape[0] - 1,
                                      _lib.ptr(df), g, float(thr), _lib.ptr(tp), _lib.ptr(fp), _lib.ptr(ws), nbytes,
                                      _lib.current_stream()), "dafne_scene_mark_hip")
    return tp.cpu().numpy(), fp.cpu().numpy()


def square(x, y, s):
    return np.array([x, y, x + s, y, x + s, y + s, x, y + s], np.float64)


def kernel_case(rng):
    """-> dets [N,8], bucket [N], gt [G,8], offs [B+1], and the bucket index of every special case."""
    r64 = lambda n, ext, lo=10.0, hi=80.0: np.round(rrects(n, rng, extent=ext, lo=lo, hi=hi).astype(np.float64), 2)   # noqa: E731
    base = r64(10, 400.0)
    gts = [np.zeros((0, 8)),                                              # 0 empty
           r64(70, 300.0),                                                # 1 more than one ballot
           r64(4200, 7000.0),                                             # 2 more than 4096 boxes
           np.concatenate([base, base, base]),                            # 3 identical boxes: the lowest index wins
           np.zeros((0, 8)),                                              # 4 empty
           np.stack([square(21.0 * k, 0.0, 10.0) for k in range(12)]),    # 5 neighbours half a pixel from a detection's hull
           np.stack([square(5.0, 5.0, 0.0), square(50.0, 50.0, 8.0)]),    # 6 a point: zero union with the same point
           r64(65, 250.0),                                                # 7 one box past a ballot
           r64(64, 250.0)]                                                # 8 exactly one ballot
    dets, bucket = [], []
    for b, g in enumerate(gts):
        if b in (0, 4):
            d = r64(6, 300.0)
        elif b == 5:
            d = np.stack([square(21.0 * k + 10.5, 0.0, 10.0) for k in range(11)] + [square(0.0, 0.0, 10.0)])
        elif b == 6:
            d = np.stack([square(5.0, 5.0, 0.0), square(50.5, 50.0, 8.0)])
        else:
            k = min(len(g), 60)
            pick = rng.choice(len(g), k, replace=False)
            pick[0] = len(g) - 1                                          # an exact copy of the bucket's last box is among them
            d = np.concatenate([g[pick] + rng.normal(0, 1.5, (k, 8)), g[pick[:k // 3]] + rng.normal(0, 6.0, (k // 3, 8)),
                                g[pick[:k // 4]], r64(10, 300.0)])
        dets.append(np.round(d, 2))
        bucket += [b] * len(d)
    extra = r64(8, 300.0)                                                 # buckets that do not exist
    dets.append(extra)
    bucket += [-1] * 4 + [len(gts)] * 4
    dets, bucket = np.concatenate(dets), np.array(bucket, np.int32)
    perm = rng.permutation(len(bucket))                                   # detections are in no bucket order
    offs = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
    return dets[perm], bucket[perm], np.concatenate(gts), offs


def test_match_and_mark_kernels_equal_the_numpy_restatement():
    rng = np.random.default_rng(5)
    dets, bucket, gt, offs = kernel_case(rng)
    exp_ov, exp_j = ref.np_match(dets, bucket, gt, offs, oracle.iou_poly_pairs)
    ovmax, jmax = run_match(dets, bucket, gt, offs)
    assert ovmax.tobytes() == exp_ov.tobytes()
    assert np.array_equal(jmax, exp_j)
    # the cases are there
    none = (bucket == 0) | (bucket == 4) | (bucket < 0) | (bucket >= len(offs) - 1)
    assert np.isneginf(ovmax[none]).all() and (jmax[none] == -1).all()
    assert offs[3] - offs[2] > 4096 and (jmax[bucket == 2] == 4199).any() and (jmax[bucket == 1] == 69).any()
    assert (jmax[bucket == 7] == 64).any() and (jmax[bucket == 8] == 63).any()
    b3 = bucket == 3
    assert (ovmax[b3] > 0.999).any() and (jmax[b3][ovmax[b3] > 0.5] < 10).all()             # identical boxes: the first copy
    b5 = bucket == 5
    assert (ovmax[b5] == 0.0).any() and (jmax[b5][ovmax[b5] == 0.0] >= 0).all()              # hulls pass, polygons do not touch
    assert sorted(ovmax[bucket == 6].tolist())[-1] == 1.0                                    # (0 + 1) / (0 + 1)
    # marking
    n = len(bucket)
    rank = rng.permutation(n).astype(np.int32)
    difficult = rng.uniform(size=len(gt)) < 0.2
    for thr in (0.5, 0.0, 0.75):
        exp_tp, exp_fp = ref.np_mark(rank.astype(np.int64), ovmax, jmax, bucket, offs, difficult, thr)
        tp, fp = run_mark(rank, ovmax, jmax, bucket, offs, difficult, thr)
        assert np.array_equal(tp, exp_tp) and np.array_equal(fp, exp_fp), thr
        over = ovmax > thr
        assert tp.any() and (fp[over] == 1).any() and ((tp == 0) & (fp == 0)).any() and (fp[~over] == 1).all()
    # twice the same bits
    ov2, j2 = run_match(dets, bucket, gt, offs)
    assert ov2.tobytes() == ovmax.tobytes() and np.array_equal(j2, jmax)


def test_kernels_take_empty_inputs():
    rng = np.random.default_rng(6)
    dets = np.round(rrects(5, rng, extent=100.0).astype(np.float64), 2)
    bucket = np.array([0, 1, 2, 0, 1], np.int32)
    offs = np.zeros(4, np.int32)
    ovmax, jmax = run_match(dets, bucket, np.zeros((0, 8)), offs)                  # G = 0
    assert np.isneginf(ovmax).all() and (jmax == -1).all()
    tp, fp = run_mark(np.arange(5, dtype=np.int32), ovmax, jmax, bucket, offs, np.zeros(0, bool), 0.5)
    assert (tp == 0).all() and (fp == 1).all()
    ovmax, jmax = run_match(np.zeros((0, 8)), np.zeros(0, np.int32), dets, np.array([0, 5], np.int32))      # N = 0
    assert ovmax.shape == (0,) and jmax.shape == (0,)
    tp, fp = run_mark(np.zeros(0, np.int32), ovmax, jmax, np.zeros(0, np.int32), np.array([0, 5], np.int32), np.zeros(5, bool), 0.5)
    assert tp.shape == (0,) and fp.shape == (0,)


# ------------------------------------------------------------------------------------------------- fixture and file route
def test_score_scenes_equals_the_reference(golden, tmp_path):
    from dafne_amd.evaluation.scene_eval import load_scene_labels, score_scenes
    g = golden("scene_eval")
    names, classes, thr, results = ref.fixture_case(g, str(tmp_path / "labelTxt"))
    lab = load_scene_labels(str(tmp_path / "labelTxt"), names, classes)
    out = score_scenes(to_device(results), lab, classes, cfg_thr(thr), output_folder=str(tmp_path / "out"))
    total = 0.0
    for c in classes:
        assert ref.same(out["rec"][c], g["rec_" + c]), c
        assert ref.same(out["prec"][c], g["prec_" + c]), c
        assert out["task1"][c] == float(g["ap_" + c]), c
        total += float(g["ap_" + c])
    assert out["task1"]["map"] == total / len(classes)
    assert list(out["task1"]) == classes + ["map"]
    # the per-scene table adds up to the curves' ends
    ps = out["per_scene"]
    assert ps.shape == (len(names), len(classes), 3) and np.array_equal(ps[:, :, 2], lab["npos"])
    m = {k: v.cpu().numpy() for k, v in out["match"].items()}
    for k, c in enumerate(classes):
        sel = m["label"] == k
        assert ps[:, k, 0].sum() == m["tp"][sel].sum() and ps[:, k, 1].sum() == m["fp"][sel].sum()
        for s in range(len(names)):
            assert ps[s, k, 0] == m["tp"][sel & (m["scene"] == s)].sum()
    assert not os.path.exists(tmp_path / "out" / "scores_overlap.csv")


def file_route(results_host, names, classes, label_dir, out, thr, monkeypatch, stable):
    """write_task1_merged + imageset.txt + the project's voc_eval per class and score_task1 -> curves, task1 dict."""
    from dafne_amd.evaluation import voc_eval as ve
    from dafne_amd.evaluation.dota_evaluation import parse_gt
    from dafne_amd.evaluation.task1 import score_task1
    from dafne_amd.scene import write_task1_merged
    merged = os.path.join(out, "Task1_merged")
    write_task1_merged(to_device(results_host), names, classes, merged)
    with open(os.path.join(out, "imageset.txt"), "w") as f:
        f.write("\n".join(names))
    annopath = os.path.join(label_dir, "{:s}.txt")
    with monkeypatch.context() as mp:
        if stable:
            plain = np.argsort
            mp.setattr(np, "argsort", lambda a, *args, **kw: plain(a, kind="stable"))
        curves = {c: ve.voc_eval(os.path.join(merged, "Task1_{:s}.txt"), annopath, os.path.join(out, "imageset.txt"), c, ovthresh=thr,
                                 use_07_metric=True, parse_gt=parse_gt)[:3] for c in classes}
        res = {}
        task = score_task1(classes, merged, annopath, out, parse_gt, cfg_thr(thr), res)
    return curves, task


def assert_same_scores(out, curves, task, out_dir, file_dir):
    for c, (rec, prec, ap) in curves.items():
        assert ref.same(out["rec"][c], rec) and ref.same(out["prec"][c], prec) and out["task1"][c] == ap, c
    assert list(out["task1"].items()) == list(task.items())
    assert open(os.path.join(out_dir, "results.txt"), "rb").read() == open(os.path.join(file_dir, "results.txt"), "rb").read()


@pytest.mark.parametrize("tied", [False, True])
def test_score_scenes_equals_the_file_route(golden, tmp_path, monkeypatch, tied):
    from dafne_amd.evaluation.scene_eval import load_scene_labels, score_scenes
    names, classes, thr, results = ref.fixture_case(golden("scene_eval"), str(tmp_path / "labelTxt"))
    if tied:            # four-decimal scores from a short range, as merged files of dense scenes have
        rng = np.random.default_rng(9)
        results = [(c, rng.integers(500, 540, len(s)) / 10000.0, l) for c, s, l in results]
        allsc = np.concatenate([s for _, s, _ in results])
        assert np.unique(allsc).size * 10 < allsc.size
    lab = load_scene_labels(str(tmp_path / "labelTxt"), names, classes)
    os.makedirs(tmp_path / "files")
    curves, task = file_route(results, names, classes, str(tmp_path / "labelTxt"), str(tmp_path / "files"), thr, monkeypatch, tied)
    out = score_scenes(to_device(results), lab, classes, cfg_thr(thr), output_folder=str(tmp_path / "dev"))
    assert_same_scores(out, curves, task, str(tmp_path / "dev"), str(tmp_path / "files"))
    assert 0.0 < out["task1"]["map"] < 1.0


# ----------------------------------------------------------------------------------------------------------- end to end
def build(cfgname, seed, opts=(), bench_weights=False):
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    cfg = load_cfg(os.path.join(ROOT, "configs", cfgname), list(opts))
    m = build_model(cfg)
    if bench_weights:
        import bench
        m.load_state_dict(bench.seeded_state_dict(m, seed))
    else:
        from oracle import model as om
        m.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=seed))
    m.to(dev())
    m.invalidate()
    return cfg, m


def random_scene(rng, h, w):
    low = rng.uniform(0, 1, (max(h // 64, 2), max(w // 64, 2), 3)).astype(np.float32)
    t = torch.nn.functional.interpolate(torch.from_numpy(low).permute(2, 0, 1)[None], size=(h, w), mode="bilinear",
                                        align_corners=False)[0].permute(1, 2, 0).numpy()
    return np.clip(t * 220 + rng.uniform(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)


def classnames_of(cfg):
    from dafne_amd.evaluation import dota_evaluation as de
    return (list(de.CLASSNAMES_DOTA_1_0) + ["container-crane"])[:cfg.MODEL.DAFNE.NUM_CLASSES]


def labels_from_detections(res_host, names, classes, label_dir, rng):
    """labelTxt files made from the detections themselves: a jittered subset, some marked difficult, some written twice."""
    os.makedirs(label_dir, exist_ok=True)
    for name, (corners, _, labels) in zip(names, res_host):
        rows = ["imagesource:GoogleEarth", "gsd:0.146"]
        for i in np.nonzero(rng.uniform(size=len(labels)) < 0.5)[0]:
            q = corners[i] + rng.normal(0, 0.8, 8)
            line = " ".join("%.1f" % v for v in q) + " " + classes[int(labels[i])] + " %d" % int(rng.uniform() < 0.15)
            rows += [line] * (2 if rng.uniform() < 0.1 else 1)
        with open(os.path.join(label_dir, name + ".txt"), "w") as f:
            f.write("\n".join(rows) + "\n")


@pytest.mark.parametrize("cfgname,opts,tta", [("dota-1.0_r50.yaml", (), False), ("dota-1.0_r50.yaml", TTA_OPTS, True)])
def test_end_to_end_equals_score_task1(tmp_path, monkeypatch, cfgname, opts, tta):
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    cfg, m = build(cfgname, seed=31, opts=opts)
    if tta:
        from dafne_amd.modeling.tta import OneStageRCNNWithTTA
        runner = OneStageRCNNWithTTA(cfg, m)
    else:
        runner = m
    rng = np.random.default_rng(17)
    scenes = [torch.from_numpy(random_scene(rng, h, w)).to(dev()) for h, w in SCENE_SHAPES]
    names = ["P%04d" % (900 + i) for i in range(len(scenes))]
    classes = classnames_of(cfg)
    res = runner.detect_scenes(scenes)
    host = to_host(res)
    assert sum(len(h[1]) for h in host) > 0
    labels_from_detections(host, names, classes, str(tmp_path / "labelTxt"), rng)
    lab = load_scene_labels(str(tmp_path / "labelTxt"), names, classes)
    out = runner.score_scenes(res, lab, classes, output_folder=str(tmp_path / "dev"))
    os.makedirs(tmp_path / "files")
    curves, task = file_route(host, names, classes, str(tmp_path / "labelTxt"), str(tmp_path / "files"), cfg.TEST.IOU_TH, monkeypatch,
                              stable=True)
    assert_same_scores(out, curves, task, str(tmp_path / "dev"), str(tmp_path / "files"))
    print("end to end (%s): %d detections, %d boxes, map %.6f" % ("tta" if tta else "plain", sum(len(h[1]) for h in host),
                                                                   lab["boxes"].shape[0], out["task1"]["map"]))
    assert 0.0 < out["task1"]["map"] < 1.0


def test_flags_do_not_depend_on_the_scene_order(golden, tmp_path):
    from dafne_amd.evaluation.scene_eval import load_scene_labels, match_scenes
    names, classes, thr, results = ref.fixture_case(golden("scene_eval"), str(tmp_path))
    results = [(c, np.round(s, 2), l) for c, s, l in results]                   # equal scores inside and across the scenes
    C = len(classes)
    runs = []
    for order in ([0, 1, 2], [2, 0, 1], [0, 1, 2]):
        lab = load_scene_labels(str(tmp_path), [names[k] for k in order], classes)
        m = match_scenes(to_device([results[k] for k in order]), lab, C, thr)
        m = {k: v.cpu().numpy() for k, v in m.items()}
        per = {}
        for pos, k in enumerate(order):
            sel = m["scene"] == pos
            per[k] = (m["tp"][sel], m["fp"][sel], m["ovmax"][sel], m["jmax"][sel])
        runs.append((per, m))
    for k in range(3):
        for a, b, c in zip(runs[0][0][k], runs[1][0][k], runs[2][0][k]):
            assert a.tobytes() == c.tobytes()                                       # two runs: the same bits
            if a.dtype != np.uint8:
                assert a.tobytes() == b.tobytes()                                   # the match never depends on the order
    # tp / fp: a box is claimed among the detections of its own scene, whose relative order the stable sort keeps; ties
    # with other scenes' detections shift ranks between scenes, never inside one
    for k in range(3):
        assert np.array_equal(runs[0][0][k][0], runs[1][0][k][0]) and np.array_equal(runs[0][0][k][1], runs[1][0][k][1])
    for key in ("tp", "fp", "rank", "order"):
        assert np.array_equal(runs[0][1][key], runs[2][1][key])


def test_eval_net_scene_labels_writes_the_same_results(tmp_path):
    from PIL import Image
    from dafne_amd.data.loader import read_image
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    rng = np.random.default_rng(41)
    sd = tmp_path / "scenes"
    sd.mkdir()
    names = ["P0001", "P0002", "P0003"]
    for name, (h, w) in zip(names, SCENE_SHAPES):
        Image.fromarray(random_scene(rng, h, w)).save(sd / (name + ".png"))
    cfg, m = build("dota-1.0_r50.yaml", seed=0, bench_weights=True)
    classes = classnames_of(cfg)
    res = m.detect_scenes([torch.from_numpy(read_image(str(sd / (n + ".png")))).to(dev()) for n in names])
    labels_from_detections(to_host(res), names, classes, str(tmp_path / "labelTxt"), rng)
    lab = load_scene_labels(str(tmp_path / "labelTxt"), names, classes)
    exp = m.score_scenes(res, lab, classes, output_folder=str(tmp_path / "dev"))
    assert 0.0 < exp["task1"]["map"] < 1.0
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file",
                        os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), "--scene-dir", str(sd), "--task1-merged-dir", str(out),
                        "--scene-labels", str(tmp_path / "labelTxt")], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert open(out / "results.txt", "rb").read() == open(tmp_path / "dev" / "results.txt", "rb").read()
    assert os.path.isdir(out / "Task1_merged")
    assert ("%-18s: %2.4f" % ("map", exp["task1"]["map"])) in p.stdout, p.stdout[-2000:]
