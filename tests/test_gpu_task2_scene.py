"""GPU: DOTA Task2 through the whole-scene route (dafne_amd/scene.py, evaluation/scene_eval.py, tools/eval_net.py --task2).

  * acceptance: detect_scenes(tasks=("task1", "task2")) + write_task2_merged writes the same bytes as the file route -- numpy
    split, detect_packed on the tiles, write_task1_files, task1_to_task2, mergebyrec -- for DOTA 1.0 and DOTA 1.5 without
    container-crane (R50, scenes of 700 x 900 and 1848 x 1100: 1 + 4 tiles), and once through OneStageRCNNWithTTA.detect_scenes
    (one size, plain + hflip); the "task1" part and the Task1_merged/ bytes equal those of a call without "task2";
  * score_scenes(task="task2") equals the numpy restatement's rec / prec / ap on tests/golden/scene_eval.npz with both sides
    converted by dots4ToRec4 (this scoring has no counterpart in the reference tree: it restates the DOTA devkit's Task2
    evaluation, voc_eval stopped after its hull stage);
  * tools/eval_net.py --scene-dir --task2 --scene-labels in a child process writes Task2_merged/ and results_task2.txt and
    leaves results.txt and Task1_merged/ byte-equal to a run without --task2."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import _scene_eval_np as sev
import _task2_np as t2
import test_gpu_scene as plain_route
import test_gpu_scene_tta as tta_route

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_SHAPES = [(700, 900), (1848, 1100)]
TTA_OPTS = ("TEST.AUG.MIN_SIZES", [800], "TEST.AUG.MAX_SIZE", 1200, "TEST.AUG.HFLIP", True, "TEST.AUG.VFLIP", False)
DOTA15_R50 = ("MODEL.RESNETS.DEPTH", 50, "DATASETS.DOTA_REMOVE_CONTAINER_CRANE", True)


def dev():
    return torch.device("cuda", 0)


def same_result(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "origins":
            assert a[k] == b[k]
        else:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("cfgname,opts,tta", [("dota-1.0_r50.yaml", (), False), ("dota-1.5_r101.yaml", DOTA15_R50, False),
                                              ("dota-1.0_r50.yaml", TTA_OPTS, True)])
def test_task2_merged_equals_the_file_route(tmp_path, cfgname, opts, tta):
    from dafne_amd.evaluation.result_merge import mergebyrec, task1_to_task2
    from dafne_amd.scene import write_task1_merged, write_task2_merged
    cfg, m = plain_route.build(cfgname, seed=31, opts=opts)
    assert cfg.MODEL.RESNETS.DEPTH == 50
    rng = np.random.default_rng(17)
    scenes = [plain_route.random_scene(rng, h, w) for h, w in SCENE_SHAPES]
    names = ["P%04d" % (900 + i) for i in range(len(scenes))]
    classes = plain_route.classnames_of(cfg)
    dscenes = [torch.from_numpy(s).to(dev()) for s in scenes]
    if tta:
        from dafne_amd.modeling.tta import OneStageRCNNWithTTA
        runner = OneStageRCNNWithTTA(cfg, m)
        assert len(runner.tta_mapper.view_specs(1024, 1024, (1024, 1024))) == 2
    else:
        runner = m
    both = runner.detect_scenes(dscenes, tasks=("task1", "task2"))
    assert [len(r["origins"]) for r in both] == [1, 4]
    a = tmp_path / "a"
    write_task1_merged(both, names, classes, str(a / "Task1_merged"))
    write_task2_merged(both, names, classes, str(a / "Task2_merged"))
    # the file route: tiles -> Task1 files (the existing tests' route) -> Task2 text -> mergebyrec
    b = tmp_path / "b"
    route = tta_route if tta else plain_route
    merged1 = route.route_files(m, cfg, scenes, names, str(b))
    task1_to_task2(str(b / "Task1"), str(b / "Task2"))
    os.makedirs(b / "Task2_merged")
    mergebyrec(str(b / "Task2"), str(b / "Task2_merged"))
    n2 = plain_route.assert_same_dirs(str(a / "Task2_merged"), str(b / "Task2_merged"))
    assert n2 == sum(len(r["task2"]["scores"]) for r in both)
    n1 = plain_route.assert_same_dirs(str(a / "Task1_merged"), merged1)
    print("task2 acceptance (%s%s): %d tile rows -> %d oriented, %d horizontal" % (
        cfgname, ", tta" if tta else "", sum(len(open(b / "Task2" / f).readlines()) for f in os.listdir(b / "Task2")), n1, n2))
    # the default call: today's dicts, the same tensors
    only1 = runner.detect_scenes(dscenes)
    for r1, r12 in zip(only1, both):
        assert "task2" not in r1
        same_result(r1, {k: v for k, v in r12.items() if k != "task2"})
        tk = r12["task2"]
        assert sorted(tk) == ["boxes", "labels", "row", "scores", "tile"]
        assert tk["boxes"].dtype == torch.float64 and tuple(tk["boxes"].shape) == (len(tk["scores"]), 4)
        assert tk["scores"].dtype == torch.float64 and bool((tk["labels"][1:] >= tk["labels"][:-1]).all())
    if cfg.DATASETS.DOTA_REMOVE_CONTAINER_CRANE:
        assert all(not (r["task2"]["labels"] == 15).any() for r in both)
    # horizontal boxes of different objects overlap where the oriented ones do not: the two merges keep different sets
    assert n2 != n1 or any(not torch.equal(r["task2"]["row"], r["row"]) for r in both)


def cfg_thr(thr):
    return types.SimpleNamespace(TEST=types.SimpleNamespace(IOU_TH=thr))


def task2_results(results):
    """(corners, scores, labels) per scene -> detect_scenes-like dicts whose "task2" entry holds dots4ToRec4 of the corners."""
    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev())      # noqa: E731
    return [{"corners": up(c, np.float64), "scores": up(s, np.float64), "labels": up(l, np.int64),
             "task2": {"boxes": up(t2.rec4(c), np.float64), "scores": up(s, np.float64), "labels": up(l, np.int64)}}
            for c, s, l in results]


@pytest.mark.parametrize("tied", [False, True])
def test_score_scenes_task2_equals_the_restatement(golden, tmp_path, tied):
    from dafne_amd.evaluation.scene_eval import load_scene_labels, score_scenes
    names, classes, thr, results = sev.fixture_case(golden("scene_eval"), str(tmp_path / "labelTxt"))
    if tied:
        rng = np.random.default_rng(9)
        results = [(c, rng.integers(500, 540, len(s)) / 10000.0, l) for c, s, l in results]
    lab = load_scene_labels(str(tmp_path / "labelTxt"), names, classes)
    det, curves = t2.np_score_hbb([(t2.rec4(c), s, l) for c, s, l in results], lab, len(classes), thr)
    dres = task2_results(results)
    out = score_scenes(dres, lab, classes, cfg_thr(thr), output_folder=str(tmp_path / "out"), task="task2")
    assert "task1" not in out and list(out["task2"]) == classes + ["map"]
    total = 0.0
    for k, c in enumerate(classes):
        rec, prec, ap = curves[k]
        assert sev.same(out["rec"][c], rec) and sev.same(out["prec"][c], prec), c
        assert out["task2"][c] == ap, c
        total += ap
    assert out["task2"]["map"] == total / len(classes) and 0.0 < out["task2"]["map"] < 1.0
    mt = {k: v.cpu().numpy() for k, v in out["match"].items()}
    assert mt["ovmax"].tobytes() == det["ovmax"].tobytes() and np.array_equal(mt["jmax"], det["jmax"])
    assert np.array_equal(mt["tp"], det["tp"]) and np.array_equal(mt["fp"], det["fp"]) and np.array_equal(mt["rank"], det["rank"])
    assert sorted(os.listdir(tmp_path / "out")) == ["results_task2.txt"]                  # never results.txt
    want = "".join(f"{k: <18}: {v:2.4f}\n" for k, v in out["task2"].items())
    assert open(tmp_path / "out" / "results_task2.txt").read() == want
    # the oriented task on the same dicts is untouched by the "task2" entries, and is another score
    o1 = score_scenes(dres, lab, classes, cfg_thr(thr))
    o1b = score_scenes([{k: v for k, v in r.items() if k != "task2"} for r in dres], lab, classes, cfg_thr(thr))
    assert list(o1["task1"].items()) == list(o1b["task1"].items()) and o1["task1"]["map"] != out["task2"]["map"]


def test_eval_net_task2_writes_task2_files_and_leaves_task1_alone(tmp_path):
    from PIL import Image
    from dafne_amd.data.loader import read_image
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    from dafne_amd.scene import write_task2_merged
    rng = np.random.default_rng(41)
    sd = tmp_path / "scenes"
    sd.mkdir()
    names = ["P0001", "P0002"]
    for name, (h, w) in zip(names, SCENE_SHAPES):
        Image.fromarray(plain_route.random_scene(rng, h, w)).save(sd / (name + ".png"))
    cfg, m = plain_route.build("dota-1.0_r50.yaml", seed=0, bench_weights=True)
    classes = plain_route.classnames_of(cfg)
    res = m.detect_scenes([torch.from_numpy(read_image(str(sd / (n + ".png")))).to(dev()) for n in names], tasks=("task1", "task2"))
    host = [(r["corners"].cpu().numpy().reshape(-1, 8), r["scores"].cpu().numpy(), r["labels"].cpu().numpy()) for r in res]
    # labelTxt made from the detections themselves: a jittered subset, some marked difficult
    lab_dir = tmp_path / "labelTxt"
    lab_dir.mkdir()
    for name, (corners, _, labels) in zip(names, host):
        rows = ["imagesource:GoogleEarth", "gsd:0.146"]
        for i in np.nonzero(rng.uniform(size=len(labels)) < 0.5)[0]:
            rows.append(" ".join("%.1f" % v for v in corners[i] + rng.normal(0, 0.8, 8)) + " " + classes[int(labels[i])] +
                        " %d" % int(rng.uniform() < 0.15))
        (lab_dir / (name + ".txt")).write_text("\n".join(rows) + "\n")
    lab = load_scene_labels(str(lab_dir), names, classes)
    exp = m.score_scenes(res, lab, classes, output_folder=str(tmp_path / "dev"), task="task2")
    assert 0.0 < exp["task2"]["map"] < 1.0
    write_task2_merged(res, names, classes, str(tmp_path / "dev" / "Task2_merged"))
    base = [sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file", os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"),
            "--scene-dir", str(sd), "--scene-labels", str(lab_dir), "--zip"]
    outs = {}
    for tag, extra in (("with", ["--task2"]), ("without", [])):
        outs[tag] = tmp_path / tag
        p = subprocess.run(base + ["--task1-merged-dir", str(outs[tag])] + extra, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        if tag == "with":
            assert ("%-18s: %2.4f" % ("map", exp["task2"]["map"])) in p.stdout, p.stdout[-2000:]
    w, wo = outs["with"], outs["without"]
    plain_route.assert_same_dirs(str(w / "Task2_merged"), str(tmp_path / "dev" / "Task2_merged"))
    assert sorted(os.listdir(w / "Task2_merged")) == sorted("Task2_%s.txt" % c for c in classes)
    assert open(w / "results_task2.txt", "rb").read() == open(tmp_path / "dev" / "results_task2.txt", "rb").read()
    assert open(w / "results.txt", "rb").read() == open(wo / "results.txt", "rb").read()
    assert open(w / "results.txt", "rb").read() != open(w / "results_task2.txt", "rb").read()
    plain_route.assert_same_dirs(str(w / "Task1_merged"), str(wo / "Task1_merged"))
    assert not any("ask2" in f for f in os.listdir(wo))
    assert sorted(set(os.listdir(w)) - set(os.listdir(wo))) == ["Task2_merged", "results_task2.txt", "task2_merged.zip"]
    import zipfile
    with zipfile.ZipFile(w / "task2_merged.zip") as z:
        assert sorted(z.namelist()) == sorted(os.listdir(w / "Task2_merged"))
        for f in z.namelist():
            assert z.read(f) == open(w / "Task2_merged" / f, "rb").read()
