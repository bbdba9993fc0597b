"""GPU: scene labels -> the ground truth of every tile on the device (dafne_amd/scene_labels.py; the kernels of
csrc/scene_labels_kernels.h behind dafne_scene_split_labels_hip / dafne_scene_pack_tile_gt_hip).  Every comparison is exact.

  * both entry points against the host restatement (tests/_scene_labels_np.py) on the golden scenes (all three in one call)
    and on three seeded random scenes: outcome codes, int32 rows, difficult, kept, both offset arrays, src, stats, and the
    fp32 packed arrays bitwise with ratio (1, 1) and (0.78125, 0.78125), sorted and unsorted;
  * write_tile_labels equals the reference's tile files (tests/golden/scene_labels.npz);
  * targeted: a bow-tie object, a scene without objects, a tile without rows, an object on the rectangle's edge, an object
    whose clip yields a duplicate vertex;
  * end to end (R50, seeded weights, one 400 x 330 scene, patch 256, overlap 64): validation_losses_scenes equals, bit for
    bit, the weighted mean of validation_losses over the same tiles cropped on the host with ground truth made by
    gt_instances_from_objects from the restatement's kept rows; filter_empty drops exactly the tiles without kept rows; a
    repeat is identical;
  * refusals: a CPU scene, a labels / scenes count mismatch, training mode."""
import os

import numpy as np
import pytest
import torch

import _scene_labels_np as sl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_labels.npz")
NAMES = ["plane", "ship", "harbor", "small-vehicle", "bridge"]


def dev():
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_against_restatement(gt, ref):
    """TileGroundTruth (device) == the restatement's dict, field for field."""
    rec = gt.records.cpu().numpy()
    assert rec.shape == (ref["codes"].shape[0], 12)
    assert np.array_equal(rec[:, 0], ref["codes"]), np.nonzero(rec[:, 0] != ref["codes"])[0][:8]
    assert np.array_equal(rec[:, 1:9], ref["rows"]), np.nonzero((rec[:, 1:9] != ref["rows"]).any(1))[0][:8]
    assert np.array_equal(rec[:, 9], ref["pair_difficult"]) and np.array_equal(rec[:, 10], ref["pair_kept"])
    assert not rec[:, 11].any()
    off, koff = gt.host_offsets()
    assert np.array_equal(off, ref["offsets"]) and np.array_equal(koff, ref["kept_offsets"])
    n, nk = int(off[-1]), int(koff[-1])
    assert np.array_equal(gt.corners[:n].cpu().numpy(), ref["corners"])
    assert np.array_equal(gt.classes[:n].cpu().numpy(), ref["classes"])
    assert np.array_equal(gt.difficult[:n].cpu().numpy(), ref["difficult"])
    assert np.array_equal(gt.src[:n].cpu().numpy(), ref["src"])
    assert np.array_equal(bits(gt.kept_corners[:nk].cpu().numpy()), bits(ref["kept_corners"]))
    assert np.array_equal(bits(gt.kept_hbox[:nk].cpu().numpy()), bits(ref["kept_hbox"]))
    assert np.array_equal(bits(gt.kept_area[:nk].cpu().numpy()), bits(ref["kept_area"]))
    assert np.array_equal(gt.kept_classes[:nk].cpu().numpy(), ref["kept_classes"])
    assert np.array_equal(gt.kept_src[:nk].cpu().numpy(), ref["kept_src"])
    assert np.array_equal(gt.stats.cpu().numpy().astype(np.int64), ref["stats"])
    assert np.array_equal(gt.origins, ref["origins"]) and np.array_equal(gt.tile_scene, ref["tile_scene"])


VARIANTS = [((1, 1), True), ((1, 1), False), ((0.78125, 0.78125), True), ((0.78125, 0.78125), False)]


def run_both(labels, sizes, patch, overlap, **kw):
    from dafne_amd.scene_labels import split_scene_labels
    out = None
    for ratio, sort in VARIANTS:
        gt = split_scene_labels(labels, sizes, patch, overlap, ratio=ratio, sort=sort, device=dev(), **kw)
        ref = sl.split_labels(labels, sizes, patch, overlap, ratio=ratio, sort=sort, **kw)
        check_against_restatement(gt, ref)
        out = out or (gt, ref)
    return out


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    z = np.load(GOLDEN)
    td = str(tmp_path_factory.mktemp("scene_labels"))
    names = [str(n) for n in z["names"]]
    for i, name in enumerate(names):
        with open(os.path.join(td, name + ".txt"), "w") as f:
            f.write(str(z["scene_%d" % i]))
    classnames = [str(c) for c in z["classnames"]]
    texts = {}
    for i in range(len(names)):
        texts.update({str(t): str(x) for t, x in zip(z["tiles_%d" % i], z["texts_%d" % i])})
    cases = [tuple(int(v) for v in c) for c in z["cases"]]
    assert len({c[2:] for c in cases}) == 1
    return {"labels": load_scene_labels(td, names, classnames), "names": names, "classnames": classnames, "texts": texts,
            "sizes": [c[:2] for c in cases], "patch": cases[0][2], "overlap": cases[0][3]}


def test_golden_scenes_against_restatement_and_reference_files(golden, tmp_path):
    from dafne_amd.scene_labels import write_tile_labels
    gt, ref = run_both(golden["labels"], golden["sizes"], golden["patch"], golden["overlap"])
    assert all(ref["stats"][c] > 0 for c in range(6)) and ref["stats"][8] > 0 and ref["stats"][8] < ref["stats"][7]
    paths = write_tile_labels(gt, golden["names"], golden["classnames"], str(tmp_path))
    assert [os.path.basename(p)[:-4] for p in paths] == list(golden["texts"])
    for p in paths:
        assert open(p).read() == golden["texts"][os.path.basename(p)[:-4]], p


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_random_scenes_against_restatement(seed):
    labels = sl.labels_from_objects([sl.random_objects(300, 260, 60, seed, NAMES)], ["R"], NAMES)
    _, ref = run_both(labels, [(300, 260)], 128, 32)
    assert ref["stats"][sl.INSIDE] > 0 and ref["stats"][sl.CUT4] > 0 and ref["stats"][sl.CUT5] > 0


def test_targeted_cases():
    o = lambda name, box, d=0: {"name": name, "difficult": d, "bbox": [float(v) for v in box]}      # noqa: E731
    scene0 = [o("ship", [10, 10, 50, 50, 50, 10, 10, 50]),                      # bow-tie
              o("plane", [0, 0, 128, 0, 128, 128, 0, 128], 1),                  # exactly the first tile's rectangle
              o("harbor", [-10, 20, 0, 10, 30, 20, 0, 30]),                     # cut at x = 0: duplicate vertices, a triangle is left
              o("ship", [107, 60, 117, 80, 127, 60, 117, 40]),
              o("bridge", [5, 5, 5, 5, 5, 5, 5, 5])]                            # no area
    labels = sl.labels_from_objects([scene0, [], [o("ship", [200, 200, 220, 200, 220, 215, 200, 215])]], ["A", "B", "C"], NAMES)
    sizes = [(300, 260), (150, 150), (300, 260)]
    gt, ref = run_both(labels, sizes, 128, 32)
    n0 = 9                                                                       # tiles of a 300 x 260 scene
    st = gt.stats_dict()
    assert st["nonconvex"] == n0 and ref["stats"][sl.NONCONVEX] == n0            # counted on every tile, no row anywhere
    rec = gt.records.cpu().numpy()
    assert gt.pair_offsets.tolist()[:n0 + 1] == [5 * t for t in range(n0 + 1)]
    assert gt.pair_offsets[n0 + 4] == gt.pair_offsets[n0]                        # scene B: 4 tiles, no pairs
    assert rec[1, 0] == sl.INSIDE and rec[1, 1:9].tolist() == [0, 0, 128, 0, 128, 128, 0, 128] and rec[1, 9] == 1
    assert rec[2, 0] == sl.DROP_LT4 and rec[4, 0] == sl.NONE
    off = gt.host_offsets()[0]
    assert (np.diff(off)[n0:n0 + 4] == 0).all()                                  # tiles without rows: scene B's ...
    assert (np.diff(off)[n0 + 4:] == 0).sum() >= 4                               # ... and most of scene C's
    assert np.diff(off)[n0 + 4:].sum() >= 1


def test_no_objects_at_all():
    from dafne_amd.scene_labels import split_scene_labels
    labels = sl.labels_from_objects([[]], ["E"], NAMES)
    gt = split_scene_labels(labels, [(100, 90)], 128, 32, device=dev())
    assert gt.host_offsets()[0].tolist() == [0, 0] and gt.host_offsets()[1].tolist() == [0, 0]
    assert gt.stats.cpu().tolist() == [0] * 9 and gt.records.shape[0] == 0
    assert len(gt.instances([0])[0]) == 0


# ------------------------------------------------------------------------------------------------ end to end
H, W, PATCH, OVERLAP = 400, 330, 256, 64


@pytest.fixture(scope="module")
def e2e():
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
    m = build_model(cfg)
    m.load_state_dict(om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=5))
    m.to(dev())
    m.invalidate()
    from dafne_amd.evaluation import dota_evaluation as de
    classnames = list(de.CLASSNAMES_DOTA_1_0)
    # every object in the upper band: the two lower tiles (up = 144) get no row at all
    objs = sl.random_objects(H, W, 25, 7, classnames[:6], side_a=(8, 40), side_b=(8, 20), box=(10, 20, W - 10, 100))
    labels = sl.labels_from_objects([objs], ["S"], classnames)
    scene = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    return {"model": m, "cfg": cfg, "labels": labels, "scene": scene, "classnames": classnames}


def reference_losses(e, tile_ids, batch):
    """validation_losses over host-cropped tiles with ground truth made on the host from the restatement's kept rows."""
    from dafne_amd.data.loader import _to_chw_resized, inference_resize_shape
    from dafne_amd.data.targets import gt_instances_from_objects
    m, cfg = e["model"], e["cfg"]
    nh, nw = inference_resize_shape(cfg, PATCH, PATCH)
    assert (nh, nw) != (PATCH, PATCH)
    ref = sl.split_labels(e["labels"], [(H, W)], PATCH, OVERLAP, min_area=cfg.INPUT.MIN_AREA, min_side=cfg.INPUT.MIN_SIDE)
    # (the restatement's kept rows at ratio 1, unsorted, are the integer tile rows)
    unsorted = sl.split_labels(e["labels"], [(H, W)], PATCH, OVERLAP, min_area=cfg.INPUT.MIN_AREA, min_side=cfg.INPUT.MIN_SIDE,
                               sort=False)["kept_corners"]
    img = e["scene"].numpy()
    inputs = []
    for t in tile_ids:
        left, up = [int(v) for v in ref["origins"][t]]
        tile = np.zeros((PATCH, PATCH, 3), np.uint8)
        crop = img[up:up + PATCH, left:left + PATCH]
        tile[:crop.shape[0], :crop.shape[1]] = crop
        a, b = int(ref["kept_offsets"][t]), int(ref["kept_offsets"][t + 1])
        rows = unsorted[a:b]
        objs = [{"name": e["classnames"][int(c)], "difficult": 0, "bbox": [float(v) for v in r]}
                for r, c in zip(rows, ref["kept_classes"][a:b])]
        inst = gt_instances_from_objects(objs, e["classnames"], (nh, nw), ratio=(nw / PATCH, nh / PATCH),
                                         sort=bool(cfg.MODEL.DAFNE.SORT_CORNERS_DATALOADER))
        x = _to_chw_resized(torch.from_numpy(tile).to(dev()), nh, nw)
        inputs.append({"image": x, "height": PATCH, "width": PATCH, "instances": inst})
    sums, keys = None, None
    for b0 in range(0, len(inputs), batch):
        part = inputs[b0:b0 + batch]
        vals = m.validation_losses(part)
        keys = sorted(vals)
        row = torch.stack([vals[k].double() for k in keys]) * len(part)
        sums = row if sums is None else sums + row
    return dict(zip(keys, (sums / len(inputs)).cpu().tolist())), ref


def test_validation_losses_scenes_filter_empty(e2e):
    m = e2e["model"]
    scene = e2e["scene"].to(dev())
    got = m.validation_losses_scenes([scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP, batch=3)
    kept = np.diff(sl.split_labels(e2e["labels"], [(H, W)], PATCH, OVERLAP, min_area=e2e["cfg"].INPUT.MIN_AREA,
                                   min_side=e2e["cfg"].INPUT.MIN_SIDE)["kept_offsets"])
    assert kept.shape[0] == 4 and (kept == 0).sum() == 2 and (kept > 0).sum() == 2, kept     # (the case is what it is meant to be)
    assert got["tile_ids"] == [t for t in range(4) if kept[t] > 0] and got["tiles"] == 2
    want, _ = reference_losses(e2e, got["tile_ids"], 3)
    print("scenes:", got, "tiles on the host:", want)
    assert sorted(k for k in got if k.startswith("loss/")) == ["loss/center", "loss/cls", "loss/corners", "loss/ctr", "loss/total"]
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    again = m.validation_losses_scenes([scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP, batch=3)
    assert again == got


def test_validation_losses_scenes_all_tiles(e2e):
    """filter_empty=False: the four tiles in batches of 3 and 1 (the weights of the mean matter)."""
    m = e2e["model"]
    scene = e2e["scene"].to(dev())
    got = m.validation_losses_scenes([scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP, batch=3, filter_empty=False)
    assert got["tiles"] == 4 and got["tile_ids"] == [0, 1, 2, 3]
    want, _ = reference_losses(e2e, [0, 1, 2, 3], 3)
    print("scenes:", got, "tiles on the host:", want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])


def test_refusals(e2e):
    from dafne_amd import _lib
    m = e2e["model"]
    scene = e2e["scene"].to(dev())
    with pytest.raises(_lib.DafneHipError):
        m.validation_losses_scenes([e2e["scene"]], e2e["labels"], patch_size=PATCH, overlap=OVERLAP)
    with pytest.raises(ValueError):
        m.validation_losses_scenes([scene, scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP)
    empty = sl.labels_from_objects([[]], ["S"], e2e["classnames"])
    with pytest.raises(ValueError):
        m.validation_losses_scenes([scene], empty, patch_size=PATCH, overlap=OVERLAP)
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m.validation_losses_scenes([scene], e2e["labels"], patch_size=PATCH, overlap=OVERLAP)
    finally:
        m.eval()
