"""CPU: the host half of the scene scorer (dafne_amd/evaluation/scene_eval.py) and its definition.

  * load_scene_labels against parse_gt on label files written from tests/golden/scene_eval.npz (bucket order, difficult flags,
    npos, classes outside the list dropped), the missing-file error;
  * the definition -- voc_eval for fixed inputs, the greedy marking as a rank minimum per ground-truth box -- restated in plain
    numpy (tests/_scene_eval_np.py, IoU from the CPU oracle) equals the REFERENCE's rec / prec / ap stored in the fixture
    (made by tests/golden/make_golden_scene_eval.py from the reference's own voc_eval and parse_gt);
  * curves_from_flags (the host part of score_scenes) on that restatement's flags gives the same arrays;
  * tools/eval_net.py refuses --scene-labels without --scene-dir."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import _scene_eval_np as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_load_scene_labels_matches_parse_gt(golden, tmp_path):
    from dafne_amd.evaluation.dota_evaluation import parse_gt
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    names, classes, _, _ = ref.fixture_case(golden("scene_eval"), str(tmp_path))
    lab = load_scene_labels(str(tmp_path), names, classes)
    objs = [parse_gt(str(tmp_path / (n + ".txt"))) for n in names]
    assert any(o["name"] not in classes for o in objs[0]), "the fixture holds an object of a class outside the list"
    exp = ref.pack_labels(objs, classes)
    assert lab["boxes"].dtype == np.float64 and lab["offsets"].dtype == np.int32 and lab["difficult"].dtype == bool
    for k in ("boxes", "offsets", "difficult", "npos", "npos_class"):
        assert np.array_equal(lab[k], exp[k]), k
    S, C = len(names), len(classes)
    assert lab["offsets"].shape == (S * C + 1,) and lab["npos"].shape == (S, C)
    # bucket-major: bucket s * C + c holds the objects of class c of scene s in file order
    for s in range(S):
        for c, cname in enumerate(classes):
            a, b = lab["offsets"][s * C + c], lab["offsets"][s * C + c + 1]
            sel = [o for o in objs[s] if o["name"] == cname]
            assert np.array_equal(lab["boxes"][a:b], np.array([o["bbox"] for o in sel], np.float64).reshape(-1, 8))
            assert lab["difficult"][a:b].tolist() == [bool(o["difficult"]) for o in sel]
    assert lab["difficult"].any() and not lab["difficult"].all()
    # the order of the scenes is the caller's
    rev = load_scene_labels(str(tmp_path), names[::-1], classes)
    assert np.array_equal(rev["npos"], lab["npos"][::-1]) and rev["boxes"].shape == lab["boxes"].shape


def test_load_scene_labels_names_the_missing_file(golden, tmp_path):
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    names, classes, _, _ = ref.fixture_case(golden("scene_eval"), str(tmp_path))
    with pytest.raises(FileNotFoundError, match="P9999"):
        load_scene_labels(str(tmp_path), names + ["P9999"], classes)


def test_load_scene_labels_takes_another_parser(golden, tmp_path):
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    names, classes, _, _ = ref.fixture_case(golden("scene_eval"), str(tmp_path))
    seen = []

    def parser(path):
        seen.append(os.path.basename(path))
        return [{"name": classes[1], "difficult": 1, "bbox": [0.0, 0.0, 4.0, 0.0, 4.0, 4.0, 0.0, 4.0]}]
    lab = load_scene_labels(str(tmp_path), names, classes, parse_gt=parser)
    assert seen == [n + ".txt" for n in names]
    assert lab["boxes"].shape == (len(names), 8) and lab["difficult"].all() and lab["npos"].sum() == 0


def test_numpy_restatement_equals_the_reference(golden, tmp_path):
    from dafne_amd.evaluation.scene_eval import curves_from_flags, load_scene_labels
    g = golden("scene_eval")
    names, classes, thr, results = ref.fixture_case(g, str(tmp_path))
    assert len(names) >= 3 and sum(len(r[1]) for r in results) >= 300
    lab = load_scene_labels(str(tmp_path), names, classes)
    det, curves = ref.np_score(results, lab, len(classes), thr, oracle.iou_poly_pairs)
    kinds = set()
    for c, cname in enumerate(classes):
        rec, prec, ap = curves[c]
        assert ref.same(rec, g["rec_" + cname]), cname
        assert ref.same(prec, g["prec_" + cname]), cname
        assert ap == float(g["ap_" + cname]), cname
        sel = det["label"] == c
        order = np.nonzero(sel)[0][np.argsort(det["rank"][sel])]
        r2, p2, a2 = curves_from_flags(det["tp"][order], det["fp"][order], lab["npos_class"][c])
        assert ref.same(r2, g["rec_" + cname]) and ref.same(p2, g["prec_" + cname]) and a2 == float(g["ap_" + cname])
        if sel.any() and lab["npos_class"][c]:
            tp, fp, over = det["tp"][sel] == 1, det["fp"][sel] == 1, det["ovmax"][sel] > thr
            assert tp.any() and (fp & over).any() and (fp & ~over).any() and (~tp & ~fp).any(), cname      # all four outcomes
            kinds.add(cname)
        elif sel.any():
            assert np.isnan(g["rec_" + cname]).all() and float(g["ap_" + cname]) == 0.0            # no ground truth
        else:
            assert g["rec_" + cname].shape == (0,) and float(g["ap_" + cname]) == 0.0              # no detections
    assert len(kinds) >= 4
    # pairwise distinct scores per class: the reference's unstable sort has one answer
    sc = np.concatenate([r[1] for r in results])
    for c in range(len(classes)):
        assert np.unique(sc[det["label"] == c]).size == int((det["label"] == c).sum())


def test_hull_candidates_keep_the_plus_one_on_the_intersection():
    """Hulls one pixel apart pass voc_eval's test (+1 on the intersection's width) and fail the tile merge's strict test."""
    gt = np.array([[0.0, 0.0, 10.0, 0.0, 10.0, 10.0, 0.0, 10.0]])
    near = np.array([10.5, 0.0, 20.0, 0.0, 20.0, 10.0, 10.5, 10.0])
    far = np.array([11.5, 0.0, 20.0, 0.0, 20.0, 10.0, 11.5, 10.0])
    assert ref.hull_candidates(gt, near).tolist() == [0] and ref.hull_candidates(gt, far).tolist() == []
    from dafne_amd.evaluation.voc_eval import hull_candidates
    assert hull_candidates(gt, near).tolist() == [0] and hull_candidates(gt, far).tolist() == []


def test_eval_net_refuses_scene_labels_without_scene_dir(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file",
           os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), "--scene-labels", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode != 0
    assert "--scene-labels" in p.stderr and "--scene-dir" in p.stderr, p.stderr
