"""GPU: whole-scene inference (dafne_amd/scene.py; the kernels dafne_scene_tiles_u8_hip in csrc/resize.hip and
dafne_scene_merge_rows_hip in csrc/poly_nms.hip).

  * the tile gather is bit-equal to a numpy crop + zero pad (HWC and CHW scenes, several scenes per launch);
  * dafne_scene_merge_rows_hip equals its numpy restatement bit for bit (rows, bucket counts, order, skip mask, score mode);
  * the acceptance test: detect_scenes + write_task1_merged writes the same Task1_merged/ bytes as the file workflow it
    replaces -- split in numpy, detect_packed on the tiles, write_task1_files with <scene>__1__<left>___<up> names,
    mergebypoly -- for DOTA 1.0, DOTA 1.5 without container-crane, and a test size other than the patch (resize branch);
  * determinism and independence of the scene order; tools/eval_net.py --scene-dir end to end."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dafne_amd.scene import split_origins

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_SHAPES = [(700, 900), (1024, 1024), (1848, 1100), (3000, 4000)]


def dev():
    return torch.device("cuda", 0)


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


def crop(img_hwc, left, up, patch):
    t = np.zeros((patch, patch, 3), np.uint8)
    c = img_hwc[up:up + patch, left:left + patch]
    t[:c.shape[0], :c.shape[1]] = c
    return t


def random_scene(rng, h, w):
    """Seeded content with structure (smooth blobs + noise), so that the random network fires on something."""
    low = rng.uniform(0, 1, (max(h // 64, 2), max(w // 64, 2), 3)).astype(np.float32)
    t = torch.nn.functional.interpolate(torch.from_numpy(low).permute(2, 0, 1)[None], size=(h, w), mode="bilinear",
                                        align_corners=False)[0].permute(1, 2, 0).numpy()
    return np.clip(t * 220 + rng.uniform(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- tile gather
def test_tile_gather_is_a_zero_padded_crop(golden):
    from dafne_amd.scene import gather_tiles
    g = golden("scene_split")
    rng = np.random.default_rng(11)
    by_patch = {}
    for i, (h, w, patch, overlap) in enumerate(g["cases"].tolist()):
        by_patch.setdefault(patch, []).append((h, w, overlap))
    for patch, cases in by_patch.items():
        scenes, dscenes, origins = [], [], []
        for k, (h, w, overlap) in enumerate(cases):
            img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            scenes.append(img)
            hwc = k % 2 == 0
            t = torch.from_numpy(img).to(dev())
            dscenes.append(t if hwc else t.permute(2, 0, 1).contiguous())
            origins.append(split_origins(h, w, patch, overlap))
        got = gather_tiles(dscenes, origins, patch).cpu().numpy()      # every scene of this patch size in one launch
        assert got.shape == (sum(len(o) for o in origins), patch, patch, 3)
        k = 0
        for img, org in zip(scenes, origins):
            for left, up in org:
                assert np.array_equal(got[k], crop(img, left, up, patch)), (patch, img.shape, left, up)
                k += 1
    # a tile at an odd offset of a narrow scene, CHW and HWC of the same pixels in one launch
    img = rng.integers(0, 256, (37, 45, 3), dtype=np.uint8)
    t = torch.from_numpy(img).to(dev())
    org = [(0, 0), (3, 5), (44, 36), (13, 1)]
    got = gather_tiles([t, t.permute(2, 0, 1).contiguous()], [org, org], 16).cpu().numpy()
    for k, (left, up) in enumerate(org + org):
        assert np.array_equal(got[k], crop(img, left, up, 16)), (k, left, up)


def test_tile_gather_rejects_bad_arguments():
    from dafne_amd import _lib
    from dafne_amd.scene import gather_tiles
    t = torch.zeros((100, 120, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(_lib.DafneHipError, match="origin"):
        gather_tiles([t], [[(120, 0)]], 64)
    with pytest.raises(_lib.DafneHipError, match="multiple"):
        gather_tiles([t], [[(0, 0)]], 60)


# ------------------------------------------------------------------------------------------------------------ merge rows
def quantise(v, scale):
    return np.rint(v.astype(np.float64) * scale) / scale


def merge_rows_numpy(rows, counts, info, n_scenes, n_classes, skip, score_mode):
    """The text route restated: per (scene, class) bucket, tile order then row order; "%.2f" / "%.4f" as rint(v * 10^k) /
    10^k, shifted by the tile origin as poly2origpoly does; score^2 / centerness in float32 for score mode 1."""
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
            d = np.empty(9)
            d[0:8:2] = (quantise(row[0:8:2], 100.0) + left) / 1.0
            d[1:8:2] = (quantise(row[1:8:2], 100.0) + up) / 1.0
            sc = np.float32(np.float32(row[8] * row[8]) / row[9]) if score_mode else row[8]
            d[8] = quantise(np.array([sc], np.float32), 10000.0)[0]
            buckets[s * n_classes + c].append(d)
            srcs[s * n_classes + c].append(t * k_cap + r)
    return buckets, srcs


@pytest.mark.parametrize("skip,score_mode", [(0, 0), ((1 << 2) | (1 << 5), 1)])
def test_merge_rows_equal_the_numpy_restatement(skip, score_mode):
    from dafne_amd.scene import merge_tile_rows
    rng = np.random.default_rng(5 + score_mode)
    T, k_cap, C, S = 16, 2000, 8, 4
    rows = np.zeros((T, k_cap, 18), np.float32)
    rows[:, :, 0:8] = rng.uniform(-50, 1100, (T, k_cap, 8))
    rows[:, ::7, 0:8] = (rng.integers(-400, 8800, (T, (k_cap + 6) // 7, 8)) * 2 + 1) / 8.0     # exact half-ties of "%.2f"
    rows[:, ::11, 0] = -0.001                                                                       # rounds to -0.00
    rows[:, :, 8] = rng.uniform(0.05, 1, (T, k_cap))
    rows[:, ::5, 8] = np.float32(0.03125)                                                           # a tie of "%.4f"
    rows[:, :, 9] = rng.uniform(0.05, 1, (T, k_cap))
    rows[:, :, 10] = rng.integers(0, C, (T, k_cap))
    rows[:12, :, 10] = np.where(rng.uniform(0, 1, (12, k_cap)) < 0.9, 3, rows[:12, :, 10])         # >= 20 000 rows in one bucket
    rows[:, :, 10] = np.where(rows[:, :, 10] == 6, 7, rows[:, :, 10])                                # class 6: an empty bucket
    counts = np.full(T, k_cap, np.int32)
    counts[12:] = [0, 17, 1999, 640]
    rows[13, 17:] = 7.0                                                                               # past the count: ignored
    # scenes 0 (tiles 0-11), 1 (12-13), 3 (14-15); scene 2 has no tile: all its buckets are empty
    info = np.array([(824 * (t % 4), 824 * (t // 4 % 3), 0) for t in range(12)] + [(0, 0, 1), (76, 824, 1), (5, 9, 3), (2976, 0, 3)],
                    np.int32)
    dets, bc, src, m_cap = merge_tile_rows(torch.from_numpy(rows).to(dev()), torch.from_numpy(counts).to(dev()), info, S, C,
                                           skip, score_mode)
    want, wsrc = merge_rows_numpy(rows, counts, info, S, C, skip, score_mode)
    bc = bc.cpu().numpy()
    dets, src = dets.cpu().numpy(), src.cpu().numpy()
    assert max(len(b) for b in want) >= 20000 and m_cap == max(len(b) for b in want)
    assert sum(len(b) == 0 for b in want) >= C + 1
    for b in range(S * C):
        assert bc[b] == len(want[b]), b
        if want[b]:
            assert np.array_equal(dets[b, :bc[b]].view(np.int64), np.array(want[b]).view(np.int64)), b
            assert np.array_equal(src[b, :bc[b]], np.array(wsrc[b])), b


# ----------------------------------------------------------------------------------------------------- acceptance: bytes
def classnames_of(cfg):
    from dafne_amd.evaluation import dota_evaluation as de
    names = list(de.CLASSNAMES_DOTA_1_0) + ["container-crane"]
    n = cfg.MODEL.DAFNE.NUM_CLASSES
    return names[:15] if (n == 16 and cfg.DATASETS.DOTA_REMOVE_CONTAINER_CRANE) else names[:n]


def route_scene(m, cfg, scenes_bgr, names, dst, batch=8):
    from dafne_amd.scene import write_task1_merged
    res = m.detect_scenes([torch.from_numpy(s).to(dev()) for s in scenes_bgr], batch=batch)
    write_task1_merged(res, names, classnames_of(cfg), dst)
    return res


def route_files(m, cfg, scenes_bgr, names, out, batch=5):
    """The reference's workflow: split_dota tiles, the detector on the tiles, _generate_task_1_files, mergebypoly."""
    from dafne_amd.data.loader import _to_chw_resized, inference_resize_shape
    from dafne_amd.evaluation.result_merge import mergebypoly
    from dafne_amd.evaluation.task1 import write_task1_files
    from dafne_amd.postprocess import rows_to_instances
    tiles, fnames = [], []
    for name, img in zip(names, scenes_bgr):
        for left, up in split_origins(img.shape[0], img.shape[1], 1024, 200):
            tiles.append(crop(img, left, up, 1024))
            fnames.append("%s__1__%d___%d.png" % (name, left, up))
    nh, nw = inference_resize_shape(cfg, 1024, 1024)
    preds = []
    for b0 in range(0, len(tiles), batch):
        x = torch.from_numpy(np.stack(tiles[b0:b0 + batch])).to(dev())
        n = x.shape[0]
        if (nh, nw) != (1024, 1024):
            x = torch.stack([_to_chw_resized(x[i], nh, nw) for i in range(n)])
            rows, counts = m.detect_packed(x, out_hw=[(1024, 1024)] * n)
        else:
            rows, counts = m.detect_packed(x, layout_hwc=True)
        torch.cuda.synchronize()
        for inst, fn in zip(rows_to_instances(rows, counts, [(1024, 1024)] * n), fnames[b0:b0 + n]):
            inst = inst.to(torch.device("cpu"))
            preds.append({"file_name": fn, "height": 1024, "width": 1024, "corners": inst.pred_corners, "labels": inst.pred_classes,
                          "scores": inst.scores, "centerness": inst.centerness})
    t1 = os.path.join(out, "Task1")
    merged = os.path.join(out, "Task1_merged")
    os.makedirs(t1)
    os.makedirs(merged)
    skip = (15,) if bool(cfg.DATASETS.DOTA_REMOVE_CONTAINER_CRANE) else ()
    write_task1_files(preds, out, t1, classnames_of(cfg), cfg, require_square=True, skip_labels=skip)
    mergebypoly(t1, merged)
    return merged


def assert_same_dirs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    _, mismatch, errors = filecmp.cmpfiles(a, b, fa, shallow=False)
    assert not mismatch and not errors, mismatch
    lines = sum(len(open(os.path.join(a, f)).readlines()) for f in fa)
    assert lines > 0, "no detections at all: the comparison would show nothing"
    return lines


@pytest.mark.parametrize("cfgname,opts", [("dota-1.0_r50.yaml", ()),
                                          ("dota-1.5_r101.yaml", ("DATASETS.DOTA_REMOVE_CONTAINER_CRANE", True)),
                                          ("dota-1.0_r50.yaml", ("INPUT.MIN_SIZE_TEST", 800, "INPUT.MAX_SIZE_TEST", 800))])
def test_detect_scenes_writes_the_file_workflows_task1_merged(tmp_path, cfgname, opts):
    cfg, m = build(cfgname, seed=31, opts=opts)
    rng = np.random.default_rng(17)
    scenes = [random_scene(rng, h, w) for h, w in SCENE_SHAPES]
    names = ["P%04d" % (900 + i) for i in range(len(scenes))]
    a = str(tmp_path / "a" / "Task1_merged")
    res = route_scene(m, cfg, scenes, names, a)
    b = route_files(m, cfg, scenes, names, str(tmp_path / "b"))
    n = assert_same_dirs(a, b)
    assert n == sum(len(r["scores"]) for r in res)
    if cfg.DATASETS.DOTA_REMOVE_CONTAINER_CRANE:
        assert all(not (r["labels"] == 15).any() for r in res)


def test_detect_scenes_is_deterministic_and_independent_of_the_scene_order():
    cfg, m = build("dota-1.0_r50.yaml", seed=37)
    rng = np.random.default_rng(23)
    scenes = [torch.from_numpy(random_scene(rng, h, w)).to(dev()) for h, w in SCENE_SHAPES]
    scenes[1] = scenes[1].permute(2, 0, 1).contiguous()           # a CHW scene among HWC ones
    r1 = m.detect_scenes(scenes)
    r2 = m.detect_scenes(scenes, batch=3)
    rev = m.detect_scenes(scenes[::-1])

    def keys(res):
        out, base = [], 0
        for r in res:                    # a detection's tile as its origin in its own scene: call-order independent
            org = np.array(r["origins"]).reshape(-1, 2)
            out.append((r["corners"].cpu().numpy(), r["scores"].cpu().numpy(), r["labels"].cpu().numpy(), r["row"].cpu().numpy(),
                        org[r["tile"].cpu().numpy() - base]))
            base += len(r["origins"])
        return out
    k1, k2, kr = keys(r1), keys(r2), keys(rev)[::-1]
    assert sum(len(r["scores"]) for r in r1) > 0
    for x, y, z, r in zip(k1, k2, kr, r1):
        for u, v, w in zip(x, y, z):
            assert np.array_equal(u, v) and np.array_equal(u, w)
        assert r["corners"].dtype == torch.float64 and r["scores"].dtype == torch.float64


def test_eval_net_scene_dir_writes_the_same_files(tmp_path):
    from PIL import Image
    from dafne_amd.data.loader import read_image
    rng = np.random.default_rng(41)
    sd = tmp_path / "scenes"
    sd.mkdir()
    names = ["P0001", "P0002", "P0003"]
    for name, (h, w) in zip(names, SCENE_SHAPES[:3]):
        Image.fromarray(random_scene(rng, h, w)).save(sd / (name + ".png"))
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file",
                        os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), "--scene-dir", str(sd), "--task1-merged-dir", str(out),
                        "--zip"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    cfg, m = build("dota-1.0_r50.yaml", seed=0, bench_weights=True)
    scenes = [read_image(str(sd / (n + ".png"))) for n in names]
    a = str(tmp_path / "a")
    route_scene(m, cfg, scenes, names, a)
    assert_same_dirs(a, str(out / "Task1_merged"))
    assert open(out / "imageset.txt").read().split("\n") == names
    import zipfile
    with zipfile.ZipFile(out / "task1_merged.zip") as z:
        assert sorted(z.namelist()) == sorted(os.listdir(a))
        for f in z.namelist():
            assert z.read(f) == open(os.path.join(a, f), "rb").read()
