"""GPU: multi-scale whole-scene inference (dafne_amd/scene.py: gather_scaled_tiles, merge_tile_rows(tile_scales=), detect_scenes(
scales=); the kernels dafne_scene_scaled_tiles_u8_hip in csrc/resize.hip and dafne_scene_merge_rows_scaled_hip in csrc/poly_nms.hip).

  * the tiles of a resampled scene are bit-equal to crop_zero_pad(PIL.Image.resize(scene)) -- Pillow itself and its numpy
    restatement (tests/_resample_np.py, pinned to Pillow on the CPU), bilinear and bicubic, HWC and CHW, many scenes and scales
    (far more than 8 axes) per launch, content that clips at 0 / 255 in both passes; then one 700 x 900 scene at patch 1024;
  * the routes that share taps_for (dafne_resize_bilinear_u8_hip, scene_views) still give Pillow's bytes;
  * the scaled merge rows equal a numpy restatement bit for bit (both row widths), and the unscaled entries when no scale is given;
  * acceptance: detect_scenes(scales=...) + write_task1_merged / write_task2_merged write the bytes of the file route -- Pillow
    resize per scale, numpy split, detect_packed, write_task1_files with <scene>__<scale>__<left>___<up> names, mergebypoly /
    task1_to_task2 + mergebyrec -- with kept rows from every scale;
  * scales=(1,) is the call without scales; scene TTA refuses scales; tools/eval_net.py --scene-scales end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import _resample_np as rs
import test_gpu_scene as plain_route
from dafne_amd.scene import scaled_size, split_origins

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 45), (61, 83), (97, 131), (5, 300), (33, 70), (300, 7)]
SCALES = [0.3, 0.5, 0.75, 1.25, 1.5, 2.0]
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
ACCEPT_SHAPES = [(700, 900), (1848, 1100)]


def dev():
    return torch.device("cuda", 0)


# ----------------------------------------------------------------------------------------------------- the tiles' pixels
@pytest.fixture(scope="module")
def small_scenes():
    """The small scenes and, per (scene, scale, filter), Pillow's resize of the whole scene (computed once, left unchanged)."""
    imgs = [rs.overshoot_image(h, w, seed=h) for h, w in SHAPES]
    want = {}
    for k, img in enumerate(imgs):
        for s in SCALES:
            nh, nw = scaled_size(img.shape[0], img.shape[1], s)
            for f in PIL_FILTER:
                want[k, s, f] = np.asarray(Image.fromarray(img).resize((nw, nh), PIL_FILTER[f]))
                assert want[k, s, f].shape == (nh, nw, 3)
    return imgs, want


@pytest.mark.parametrize("patch", [16, 64])
@pytest.mark.parametrize("resample", ["bilinear", "bicubic"])
def test_scaled_tiles_equal_pillow(small_scenes, resample, patch):
    from dafne_amd.scene import gather_scaled_tiles
    imgs, want = small_scenes
    hwc = [torch.from_numpy(i).to(dev()) for i in imgs]
    chw = [t.permute(2, 0, 1).contiguous() for t in hwc]
    scenes, scales, origins, keys = [], [], [], []
    for k, img in enumerate(imgs):
        for s in SCALES:
            nh, nw = scaled_size(img.shape[0], img.shape[1], s)
            org = split_origins(nh, nw, patch, patch // 4)
            for t in (hwc[k], chw[k]):                     # HWC and CHW of the same pixels in one launch
                scenes.append(t)
                scales.append(s)
                origins.append(org)
                keys.append((k, s))
    got = gather_scaled_tiles(scenes, scales, origins, patch, resample).cpu().numpy()     # 72 (scene, scale) pairs: 144 axes
    assert got.shape == (sum(len(o) for o in origins), patch, patch, 3)
    zeros = full = padded = small = 0
    o = 0
    for (k, s), org in zip(keys, origins):
        ref = want[k, s, resample]
        small += ref.shape[0] < patch and ref.shape[1] < patch
        for left, up in org:
            exp = rs.crop_zero_pad(ref, left, up, patch)
            assert np.array_equal(got[o], exp), (SHAPES[k], s, left, up, resample, patch)
            padded += 2 * min(ref.shape[0] - up, patch) * min(ref.shape[1] - left, patch) < patch * patch      # mostly padding
            o += 1
        zeros += int((ref == 0).sum())
        full += int((ref == 255).sum())
    assert padded > 0 and small > 0
    if resample == "bicubic":
        assert zeros > 0 and full > 0                      # the overshoot clipped at both ends
    # the expectation itself: the numpy restatement of the resampler gives Pillow's bytes (one scene, every scale)
    for s in SCALES:
        nh, nw = scaled_size(*SHAPES[1], s)
        assert np.array_equal(rs.resize(imgs[1], nh, nw, resample), want[1, s, resample]), s


def test_scaled_tiles_of_a_realistic_scene():
    from dafne_amd.scene import gather_scaled_tiles
    img = rs.overshoot_image(700, 900, seed=1)
    t = torch.from_numpy(img).to(dev())
    for resample in ("bicubic", "bilinear"):
        origins = [split_origins(*scaled_size(700, 900, s), 1024, 200) for s in (0.5, 1.5)]
        assert [len(o) for o in origins] == [1, 4]
        got = gather_scaled_tiles([t, t.permute(2, 0, 1).contiguous()], [0.5, 1.5], origins, 1024, resample).cpu().numpy()
        o = 0
        for s, org in zip((0.5, 1.5), origins):
            nh, nw = scaled_size(700, 900, s)
            ref = np.asarray(Image.fromarray(img).resize((nw, nh), PIL_FILTER[resample]))
            for left, up in org:
                assert np.array_equal(got[o], rs.crop_zero_pad(ref, left, up, 1024)), (resample, s, left, up)
                o += 1


def test_scaled_tiles_reject_bad_arguments():
    from dafne_amd import _lib
    from dafne_amd.scene import gather_scaled_tiles
    t = torch.zeros((100, 120, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(_lib.DafneHipError, match="origin"):
        gather_scaled_tiles([t], [0.5], [[(60, 0)]], 64)
    with pytest.raises(_lib.DafneHipError, match="multiple"):
        gather_scaled_tiles([t], [0.5], [[(0, 0)]], 62)
    with pytest.raises(_lib.DafneHipError, match="downscale"):
        gather_scaled_tiles([t], [0.05], [[(0, 0)]], 64)
    with pytest.raises(ValueError, match="resample"):
        gather_scaled_tiles([t], [0.5], [[(0, 0)]], 64, resample="lanczos")


def test_bilinear_routes_still_equal_pillow():
    """dafne_resize_bilinear_u8_hip and dafne_scene_views_u8_hip share taps_for with the new kernel: their bytes are Pillow's."""
    from dafne_amd.data.loader import _to_chw_resized
    from dafne_amd.scene import scene_views
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (333, 517, 3), dtype=np.uint8)
    t = torch.from_numpy(img).to(dev())
    for nh, nw in ((200, 301), (500, 640)):
        want = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
        assert np.array_equal(_to_chw_resized(t, nh, nw).permute(1, 2, 0).cpu().numpy(), want), (nh, nw)
        got = scene_views([(t, True, 0, 0, 333, 517, 0, 0)], nh, nw)[0].permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(got, want), (nh, nw)
    got = scene_views([(t, True, 100, 50, 256, 256, 1, 0)], 180, 180)[0].permute(1, 2, 0).cpu().numpy()
    want = np.asarray(Image.fromarray(plain_route.crop(img, 100, 50, 256)).resize((180, 180), Image.BILINEAR))[:, ::-1]
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ merge rows
def quantise(v, scale):
    return np.rint(v.astype(np.float64) * scale) / scale


def merge_rows_scaled_numpy(rows, counts, info, tile_scale, n_scenes, n_classes, skip, score_mode, hbb):
    """test_gpu_scene.merge_rows_numpy with poly2origpoly's division by the tile's rate: (q + left | up) / scale in float64;
    hbb: dots4ToRec4 of those values (min / max after the division)."""
    k_cap = rows.shape[1]
    buckets = [[] for _ in range(n_scenes * n_classes)]
    srcs = [[] for _ in range(n_scenes * n_classes)]
    for t in range(rows.shape[0]):
        left, up, s = (int(v) for v in info[t])
        rate = float(tile_scale[t])
        for r in range(min(int(counts[t]), k_cap)):
            row = rows[t, r]
            c = int(row[10])
            if (skip >> c) & 1:
                continue
            d = np.empty(9)
            d[0:8:2] = (quantise(row[0:8:2], 100.0) + left) / rate
            d[1:8:2] = (quantise(row[1:8:2], 100.0) + up) / rate
            sc = np.float32(np.float32(row[8] * row[8]) / row[9]) if score_mode else row[8]
            d[8] = quantise(np.array([sc], np.float32), 10000.0)[0]
            if hbb:
                d = np.array([d[0:8:2].min(), d[1:8:2].min(), d[0:8:2].max(), d[1:8:2].max(), d[8]])
            buckets[s * n_classes + c].append(d)
            srcs[s * n_classes + c].append(t * k_cap + r)
    return buckets, srcs


def merge_case():
    rng = np.random.default_rng(77)
    T, k_cap, C, S = 8, 300, 6, 2
    rows = np.zeros((T, k_cap, 18), np.float32)
    rows[:, :, 0:8] = rng.uniform(-50, 1100, (T, k_cap, 8))
    rows[:, ::7, 0:8] = (rng.integers(-400, 8800, (T, (k_cap + 6) // 7, 8)) * 2 + 1) / 8.0     # exact half-ties of "%.2f"
    rows[:, ::11, 0] = -0.001                                                                       # rounds to -0.00
    rows[:, :, 8] = rng.uniform(0.05, 1, (T, k_cap))
    rows[:, ::5, 8] = np.float32(0.03125)                                                           # a tie of "%.4f"
    rows[:, :, 9] = rng.uniform(0.05, 1, (T, k_cap))
    rows[:, :, 10] = rng.integers(0, C, (T, k_cap))
    counts = np.array([300, 300, 0, 17, 299, 300, 64, 300], np.int32)
    rows[3, 17:] = 7.0                                                                               # past the count: ignored
    # scene 0: tiles 0-5 with all four scales mixed; scene 1: tiles 6-7
    info = np.array([(0, 0, 0), (824, 0, 0), (0, 824, 0), (0, 0, 0), (626, 1748, 0), (76, 0, 0), (0, 0, 1), (326, 26, 1)], np.int32)
    scale = np.array([1.0, 0.5, 1.5, 0.3, 1.5, 0.5, 0.3, 1.0])
    return rows, counts, info, scale, S, C


@pytest.mark.parametrize("hbb", [False, True])
@pytest.mark.parametrize("skip,score_mode", [(0, 0), (1 << 2, 1)])
def test_scaled_merge_rows_equal_the_numpy_restatement(skip, score_mode, hbb):
    from dafne_amd.scene import merge_tile_rows
    rows, counts, info, scale, S, C = merge_case()
    drows, dcounts = torch.from_numpy(rows).to(dev()), torch.from_numpy(counts).to(dev())
    dets, bc, src, m_cap = merge_tile_rows(drows, dcounts, info, S, C, skip, score_mode, hbb=hbb, tile_scales=scale)
    want, wsrc = merge_rows_scaled_numpy(rows, counts, info, scale, S, C, skip, score_mode, hbb)
    bc, dets, src = bc.cpu().numpy(), dets.cpu().numpy(), src.cpu().numpy()
    assert dets.shape[2] == (5 if hbb else 9) and m_cap == max(len(b) for b in want)
    if skip:
        assert all(len(want[s * C + 2]) == 0 for s in range(S))
    for b in range(S * C):
        assert bc[b] == len(want[b]), b
        if want[b]:
            assert np.array_equal(dets[b, :bc[b]].view(np.int64), np.array(want[b]).view(np.int64)), b
            assert np.array_equal(src[b, :bc[b]], np.array(wsrc[b])), b
    # the division changes the rows: the comparison above is not one of unscaled values
    valid = torch.arange(m_cap, device=dev())[None, :] < torch.from_numpy(bc).to(dev())[:, None]
    scaled = torch.from_numpy(dets).to(dev()).view(torch.int64)[valid]
    plain = merge_tile_rows(drows, dcounts, info, S, C, skip, score_mode, hbb=hbb)
    assert plain[3] == m_cap and not torch.equal(plain[0].view(torch.int64)[valid], scaled)
    # scales of 1.0 = no scales = the unscaled entry, bit for bit (x / 1.0 is x)
    ones = merge_tile_rows(drows, dcounts, info, S, C, skip, score_mode, hbb=hbb, tile_scales=np.ones(len(counts)))
    assert torch.equal(plain[0].view(torch.int64)[valid], ones[0].view(torch.int64)[valid])
    assert torch.equal(plain[1], ones[1]) and torch.equal(plain[2][valid], ones[2][valid])


def test_scaled_merge_entry_with_null_scales_is_the_unscaled_entry():
    from dafne_amd import _lib
    from dafne_amd.scene import merge_tile_rows
    rows, counts, info, _, S, C = merge_case()
    L = _lib.load()
    drows, dcounts = torch.from_numpy(rows).to(dev()), torch.from_numpy(counts).to(dev())
    want, wbc, wsrc, m_cap = merge_tile_rows(drows, dcounts, info, S, C)
    dinfo = torch.from_numpy(info).to(dev())
    T, k_cap = rows.shape[:2]
    nbytes = L.dafne_scene_merge_workspace_bytes(T, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    dets = torch.empty((S * C, m_cap, 9), dtype=torch.float64, device=dev())
    src = torch.empty((S * C, m_cap), dtype=torch.int32, device=dev())
    bc = torch.empty(S * C, dtype=torch.int32, device=dev())
    _lib.check(L.dafne_scene_merge_rows_scaled_hip(_lib.ptr(drows), _lib.ptr(dcounts), T, k_cap, _lib.ptr(dinfo), None, S, C, 0, 0,
                                                   m_cap, _lib.ptr(dets), _lib.ptr(bc), _lib.ptr(src), _lib.ptr(ws), nbytes,
                                                   _lib.current_stream()), "dafne_scene_merge_rows_scaled_hip")
    assert torch.equal(bc, wbc)
    valid = torch.arange(m_cap, device=dev())[None, :] < bc[:, None]
    assert torch.equal(dets.view(torch.int64)[valid], want.view(torch.int64)[valid]) and torch.equal(src[valid], wsrc[valid])
    with pytest.raises(ValueError, match="tile_scales"):
        merge_tile_rows(drows, dcounts, info, S, C, tile_scales=[1.0, 0.5])
    with pytest.raises(ValueError, match="tile_scales"):
        merge_tile_rows(drows, dcounts, info, S, C, tile_scales=[1.0] * 7 + [0.0])


# ----------------------------------------------------------------------------------------------------- acceptance: bytes
def route_files_scaled(m, cfg, scenes_bgr, names, out, scales, resample, batch=5):
    """The reference's workflow at several rates with Pillow as the resize: per scene and scale the resized scene, its split
    tiles named <scene>__<scale>__<left>___<up>, the detector on the tiles, _generate_task_1_files; the caller merges."""
    from dafne_amd.evaluation.task1 import write_task1_files
    from dafne_amd.postprocess import rows_to_instances
    tiles, fnames = [], []
    for name, img in zip(names, scenes_bgr):
        for s in scales:
            nh, nw = scaled_size(img.shape[0], img.shape[1], s)
            ref = img if s == 1 else np.asarray(Image.fromarray(img).resize((nw, nh), PIL_FILTER[resample]))
            for left, up in split_origins(nh, nw, 1024, 200):
                tiles.append(plain_route.crop(ref, left, up, 1024))
                fnames.append("%s__%s__%d___%d.png" % (name, str(s), left, up))
    preds = []
    for b0 in range(0, len(tiles), batch):
        x = torch.from_numpy(np.stack(tiles[b0:b0 + batch])).to(dev())
        n = x.shape[0]
        rows, counts = m.detect_packed(x, layout_hwc=True)
        torch.cuda.synchronize()
        for inst, fn in zip(rows_to_instances(rows, counts, [(1024, 1024)] * n), fnames[b0:b0 + n]):
            inst = inst.to(torch.device("cpu"))
            preds.append({"file_name": fn, "height": 1024, "width": 1024, "corners": inst.pred_corners, "labels": inst.pred_classes,
                          "scores": inst.scores, "centerness": inst.centerness})
    t1 = os.path.join(out, "Task1")
    os.makedirs(t1)
    write_task1_files(preds, out, t1, plain_route.classnames_of(cfg), cfg, require_square=True)
    return t1, fnames


def kept_per_scale(res):
    """{scale: kept rows from tiles of that scale} over all scenes ("tile" indexes the call's tiles, scene after scene)."""
    scales = [s for r in res for s in r["tile_scales"]]
    out = {}
    for r in res:
        for t in r["tile"].cpu().tolist():
            out[scales[t]] = out.get(scales[t], 0) + 1
    return out


@pytest.fixture(scope="module")
def r50():
    cfg, m = plain_route.build("dota-1.0_r50.yaml", seed=31)
    rng = np.random.default_rng(17)
    scenes = [plain_route.random_scene(rng, h, w) for h, w in ACCEPT_SHAPES]
    return cfg, m, scenes, ["P%04d" % (900 + i) for i in range(len(scenes))]


@pytest.mark.parametrize("scales,resample,task2", [((1, 0.5), "bicubic", True), ((1.5,), "bicubic", False), ((0.5, 1), "bilinear", False)])
def test_detect_scenes_scales_write_the_file_routes_bytes(tmp_path, r50, scales, resample, task2):
    from dafne_amd.evaluation.result_merge import mergebypoly, mergebyrec, task1_to_task2
    from dafne_amd.scene import write_task1_merged, write_task2_merged
    cfg, m, scenes, names = r50
    classes = plain_route.classnames_of(cfg)
    tasks = ("task1", "task2") if task2 else ("task1",)
    res = m.detect_scenes([torch.from_numpy(s).to(dev()) for s in scenes], scales=scales, resample=resample, tasks=tasks)
    a, b = tmp_path / "a", tmp_path / "b"
    write_task1_merged(res, names, classes, str(a / "Task1_merged"))
    t1, fnames = route_files_scaled(m, cfg, scenes, names, str(b), scales, resample)
    os.makedirs(b / "Task1_merged")
    mergebypoly(t1, str(b / "Task1_merged"))
    n1 = plain_route.assert_same_dirs(str(a / "Task1_merged"), str(b / "Task1_merged"))
    assert n1 == sum(len(r["scores"]) for r in res) > 0
    # the tiles and their order: scene, then scale in the given order, then split order
    text = {float(s): str(s) for s in scales}
    got_names = ["%s__%s__%d___%d.png" % (n, text[s], left, up)
                 for n, r in zip(names, res) for (left, up), s in zip(r["origins"], r["tile_scales"])]
    assert got_names == fnames
    kept = kept_per_scale(res)
    print("scales %r %s: %d tiles, kept rows per scale %r" % (scales, resample, len(fnames), kept))
    assert sorted(kept) == sorted(float(s) for s in scales) and min(kept.values()) > 0, kept
    if task2:
        write_task2_merged(res, names, classes, str(a / "Task2_merged"))
        task1_to_task2(t1, str(b / "Task2"))
        os.makedirs(b / "Task2_merged")
        mergebyrec(str(b / "Task2"), str(b / "Task2_merged"))
        n2 = plain_route.assert_same_dirs(str(a / "Task2_merged"), str(b / "Task2_merged"))
        assert n2 == sum(len(r["task2"]["scores"]) for r in res) > 0


def test_scales_of_one_is_the_call_without_scales(r50):
    cfg, m, scenes, names = r50
    d = [torch.from_numpy(s).to(dev()) for s in scenes]
    base = m.detect_scenes(d)
    one = m.detect_scenes(d, scales=(1,), resample="bilinear")
    assert len(base) == len(one) == 2 and sum(len(r["scores"]) for r in base) > 0
    for x, y in zip(base, one):
        assert sorted(x) == sorted(y) and "tile_scales" not in y
        for k in x:
            if k == "origins":
                assert x[k] == y[k]
            else:
                assert x[k].dtype == y[k].dtype and torch.equal(x[k], y[k]), k


def test_scene_tta_refuses_scales(r50):
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA
    cfg, m, scenes, _ = r50
    tta = OneStageRCNNWithTTA(cfg, m)
    with pytest.raises(NotImplementedError, match="scales"):
        tta.detect_scenes([torch.from_numpy(scenes[0]).to(dev())], scales=(1, 0.5))


def test_eval_net_scene_scales_end_to_end(tmp_path):
    from dafne_amd.data.loader import read_image
    from dafne_amd.scene import write_task1_merged
    rng = np.random.default_rng(41)
    sd = tmp_path / "scenes"
    sd.mkdir()
    names = ["P0001", "P0002"]
    for name, (h, w) in zip(names, ((700, 900), (1100, 1300))):
        Image.fromarray(plain_route.random_scene(rng, h, w)).save(sd / (name + ".png"))
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file",
                        os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), "--scene-dir", str(sd), "--task1-merged-dir", str(out),
                        "--scene-scales", "1,0.5"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "scene P0001 (700x900, 2 tiles: 1 at 1, 1 at 0.5)" in p.stdout, p.stdout[-2000:]
    assert "scene P0002 (1100x1300, 5 tiles: 4 at 1, 1 at 0.5)" in p.stdout, p.stdout[-2000:]
    cfg, m = plain_route.build("dota-1.0_r50.yaml", seed=0, bench_weights=True)
    res = m.detect_scenes([torch.from_numpy(read_image(str(sd / (n + ".png")))).to(dev()) for n in names], scales=(1, 0.5))
    write_task1_merged(res, names, plain_route.classnames_of(cfg), str(tmp_path / "a"))
    plain_route.assert_same_dirs(str(tmp_path / "a"), str(out / "Task1_merged"))
