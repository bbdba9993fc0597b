"""CPU: the host restatement of the scene-label split (tests/_scene_labels_np.py) against the reference's own tile label
files (tests/golden/scene_labels.npz, made by tests/golden/make_golden_scene_labels.py), the training filter on hand-made rows,
and the ABI of the two new entry points."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _scene_labels_np as sl  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_labels.npz")


def golden_cases(tmp_path):
    """-> [(name, (h, w), patch, overlap, labels, {tile stem: text})] of the fixture."""
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    z = np.load(GOLDEN)
    classnames = [str(c) for c in z["classnames"]]
    out = []
    for i, name in enumerate(str(n) for n in z["names"]):
        h, w, patch, overlap = [int(v) for v in z["cases"][i]]
        with open(os.path.join(str(tmp_path), name + ".txt"), "w") as f:
            f.write(str(z["scene_%d" % i]))
        labels = load_scene_labels(str(tmp_path), [name], classnames)
        texts = {str(t): str(x) for t, x in zip(z["tiles_%d" % i], z["texts_%d" % i])}
        out.append((name, (h, w), patch, overlap, labels, texts))
    return out


def test_loader_carries_file_order(tmp_path):
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    with open(os.path.join(str(tmp_path), "S.txt"), "w") as f:
        f.write("gsd:1\n1 1 9 1 9 9 1 9 ship 0\n2 2 8 2 8 8 2 8 other 0\n3 3 7 3 7 7 3 7 plane 1\n4 4 6 4 6 6 4 6 ship 2\n")
    lab = load_scene_labels(str(tmp_path), ["S"], ["plane", "ship"])
    assert lab["boxes"][:, 0].tolist() == [3.0, 1.0, 4.0]                 # bucket-major, as before
    assert lab["file_index"].tolist() == [2, 0, 3] and lab["file_index"].dtype == np.int32
    assert lab["difficult_value"].tolist() == [1, 0, 2] and lab["difficult"].tolist() == [True, False, True]
    per_scene, cls = sl.scene_objects(lab)
    assert per_scene[0].tolist() == [1, 0, 2] and cls.tolist() == [0, 1, 1]


def test_restatement_reproduces_the_reference_tile_files(tmp_path):
    from dafne_amd.scene_labels import format_row
    seen = np.zeros(sl.N_CODES, dtype=np.int64)
    n_tiles = 0
    for name, size, patch, overlap, labels, texts in golden_cases(tmp_path):
        res = sl.split_labels(labels, [size], patch, overlap)
        mine = sl.tile_texts(res, [name], labels["classnames"])
        assert list(mine) == list(texts), "tile names or their order differ"
        for stem in texts:
            assert mine[stem] == texts[stem], (stem, mine[stem], texts[stem])
        seen += res["stats"][:sl.N_CODES]
        n_tiles += len(texts)
        assert res["stats"][7] == sum(len(t.splitlines()) for t in texts.values())
    assert n_tiles == 14
    assert all(seen[c] > 0 for c in (sl.NONE, sl.INSIDE, sl.CUT4, sl.CUT5, sl.DROP_LT4, sl.DROP_GT5)), seen
    assert sl.format_row([1, 2, 3, 4, 5, 6, 7, 128], "ship", 2) == format_row([1, 2, 3, 4, 5, 6, 7, 128], "ship", 2) \
        == "1.0 2.0 3.0 4.0 5.0 6.0 7.0 128.0 ship 2"


def test_training_filter_on_handmade_rows():
    sq = lambda s: [10, 10, 10 + s, 10, 10 + s, 10 + s, 10, 10 + s]       # noqa: E731
    assert sl.keep_row(sq(4), 0, 10, 2) and sl.keep_row(sq(4), 1, 10, 2)
    assert not sl.keep_row(sq(4), 2, 10, 2)                               # DOTA2COCO drops the split's difficult 2
    rect = [0, 0, 5, 0, 5, 2, 0, 2]                                       # area exactly 10 = MIN_AREA: dropped (<=)
    assert not sl.keep_row(rect, 0, 10, 2) and sl.keep_row(rect, 0, 9.5, 2)
    assert sl.keep_row([0, 0, 11, 0, 11, 1, 0, 1], 0, 10, 2)              # area 11
    thin = [0, 0, 30, 0, 30, 1, 0, 1]                                     # max side exactly MIN_SIDE = 30: kept (>=)
    assert sl.keep_row(thin, 0, 10, 30) and not sl.keep_row(thin, 0, 10, 31)
    assert not sl.keep_row([0, 0, 20, 0, 20, 0, 0, 20], 0, 10, 2)         # two equal corners (a triangle of area 200)
    assert sl.keep_row([10, 14, 14, 14, 14, 10, 10, 10], 0, 10, 2)        # the other orientation: |area|


def test_pair_rules_on_handmade_objects():
    rect = (0, 0, 127, 99)                                                # a 128-wide scene of height 100: right = w - 1
    on_edge = [0, 0, 127, 0, 127, 99, 0, 99]
    code, row, d = sl.split_pair(on_edge, 1, rect, 128)
    assert (code, row, d) == (sl.INSIDE, on_edge, 1)                      # on the closed rectangle: inside, no clamp
    bow = [10, 10, 50, 50, 50, 10, 10, 50]
    assert sl.split_pair(bow, 0, rect, 128)[0] == sl.NONCONVEX
    assert sl.split_pair([5, 5, 5, 5, 5, 5, 5, 5], 0, rect, 128)[0] == sl.NONE
    assert sl.split_pair([200, 10, 240, 10, 240, 30, 200, 30], 0, rect, 128)[0] == sl.NONE
    # a diamond whose right corner lies ON the right edge and whose bottom is cut: the corner comes out of two passes once
    code, row, d = sl.split_pair([107, 60, 117, 80, 127, 60, 117, 40], 0, (0, 0, 127, 70), 128)
    assert code == sl.CUT5 and d == 0
    # truncation on load: 10.9 -> 10
    code, row, d = sl.split_pair([10.9, 10.9, 50.9, 10.9, 50.9, 30.9, 10.9, 30.9], 0, rect, 128)
    assert (code, row) == (sl.INSIDE, [10, 10, 50, 10, 50, 30, 10, 30])
    # cut with less than the threshold left: difficult 2, clamped to [1, patch]
    code, row, d = sl.split_pair([-60, 10, 20, 10, 20, 30, -60, 30], 0, rect, 128)
    assert code == sl.CUT4 and d == 2 and min(row) == 1


def test_abi_version_and_symbols():
    from dafne_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.dafne_abi_version() >= 151
    for name in ("dafne_scene_split_labels_hip", "dafne_scene_pack_tile_gt_hip", "dafne_scene_pack_tile_gt_workspace_bytes"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.dafne_scene_pack_tile_gt_workspace_bytes(10) >= 10 * 9 * 4
    # the pair count is refused before anything is launched or dereferenced
    rc = L.dafne_scene_split_labels_hip(None, None, 1, None, 1, None, None, 1, 128, 0.7, 10.0, 2.0, None, 2 ** 31, None)
    assert rc != 0 and b"overflow" in L.dafne_last_error()
    # compiled inside decode.hip: no contraction, no SLP vectoriser
    assert {"-ffp-contract=off", "-fno-slp-vectorize"} <= set(build.PER_FILE["decode.hip"])
    assert '#include "scene_labels_kernels.h"' in open(os.path.join(build.CSRC, "decode.hip")).read()


def test_eval_net_val_loss_scene_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_net
    finally:
        sys.path.pop(0)
    base = ["--config-file", os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")]
    err = lambda *a: eval_net.scene_args_error(eval_net.parse_args(base + list(a)))      # noqa: E731
    assert err("--val-loss", "--image-dir", "i", "--label-dir", "l") is None             # the tile route is untouched
    assert err("--val-loss", "--scene-dir", "d", "--scene-labels", "l") is None
    assert err("--val-loss", "--scene-dir", "d", "--scene-labels", "l", "--tile-labels-dir", "o") is None
    assert "needs --scene-labels" in err("--val-loss", "--scene-dir", "d")
    assert "rate 1" in err("--val-loss", "--scene-dir", "d", "--scene-labels", "l", "--scene-tta")
    assert "rate 1" in err("--val-loss", "--scene-dir", "d", "--scene-labels", "l", "--scene-scales", "1,0.5")
    assert "--tile-labels-dir needs" in err("--scene-dir", "d", "--tile-labels-dir", "o")
    assert err("--scene-dir", "d", "--scene-labels", "l") is None                        # scoring stays as it was
    import inspect
    from dafne_amd.modeling.one_stage_detector import OneStageDetector
    p = inspect.signature(OneStageDetector.validation_losses_scenes).parameters
    assert [p[k].default for k in ("patch_size", "overlap", "batch", "layout_hwc", "filter_empty")] == [1024, 200, 8, None, True]


def test_clip_with_duplicate_vertices():
    """A corner on the cutting edge: the cut point and the corner are equal and are merged; last = first likewise."""
    pts = [(-10.0, 20.0), (0.0, 10.0), (30.0, 20.0), (0.0, 30.0)]
    raw = sl.clip_edge(pts, 0, 0.0)
    assert raw == [(0.0, 30.0), (0.0, 10.0), (0.0, 10.0), (30.0, 20.0), (0.0, 30.0)]
    assert sl.merge_equal(raw) == [(0.0, 30.0), (0.0, 10.0), (30.0, 20.0)]
    assert sl.split_pair([-10, 20, 0, 10, 30, 20, 0, 30], 0, (0, 0, 128, 128), 128)[0] == sl.DROP_LT4


def test_split_refuses_cpu_and_count_mismatch(tmp_path):
    from dafne_amd import _lib
    from dafne_amd.scene_labels import split_scene_labels
    labels = sl.labels_from_objects([[{"name": "ship", "difficult": 0, "bbox": [1, 1, 9, 1, 9, 9, 1, 9]}]], ["S"], ["ship"])
    with pytest.raises(ValueError):
        split_scene_labels(labels, [(100, 100), (50, 50)], device="cuda")
    with pytest.raises(_lib.DafneHipError):
        split_scene_labels(labels, [(100, 100)], device="cpu")
