"""GPU: scene-level TTA (dafne_amd/scene.py: scene_views, tta_candidates, tta_tile_rows, detect_scenes_tta; the kernels
dafne_scene_views_u8_hip in csrc/resize.hip and dafne_tta_candidates_hip in csrc/decode.hip).

  * the views kernel equals gather_tiles + resize_u8 bit for bit (the DOTA sizes, an identity size, every flip, edge tiles
    of scenes smaller than the patch, HWC and CHW scenes in one launch, a pre-resized source, a non-square output), and a
    few views equal Pillow's BILINEAR resize of the padded crop;
  * the candidates kernel equals _invert_and_concat_fast (corners bit for bit, order, counts) and reports overflow;
  * every tile's merged rows equal OneStageRCNNWithTTA(images_per_group=1) on that tile;
  * the acceptance test: OneStageRCNNWithTTA.detect_scenes + write_task1_merged writes the same Task1_merged/ bytes as the
    TTA file workflow (numpy split, OneStageRCNNWithTTA per tile, write_task1_files, mergebypoly);
  * batch and scene-order invariance; tools/eval_net.py --scene-dir --scene-tta end to end."""
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
SCENE_SHAPES = [(700, 900), (1024, 1024), (1500, 1900)]
RELEASED_AUG = ("TEST.AUG.MIN_SIZES", [450, 500, 600, 700, 800, 900, 1000, 1100, 1200], "TEST.AUG.MAX_SIZE", 1200,
                "TEST.AUG.HFLIP", True, "TEST.AUG.VFLIP", True)
PRE_RESIZE = ("INPUT.MIN_SIZE_TEST", 800, "INPUT.MAX_SIZE_TEST", 800, "TEST.AUG.MIN_SIZES", [600, 800, 1100],
              "TEST.AUG.MAX_SIZE", 1200, "TEST.AUG.HFLIP", True, "TEST.AUG.VFLIP", False)


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
    low = rng.uniform(0, 1, (max(h // 64, 2), max(w // 64, 2), 3)).astype(np.float32)
    t = torch.nn.functional.interpolate(torch.from_numpy(low).permute(2, 0, 1)[None], size=(h, w), mode="bilinear",
                                        align_corners=False)[0].permute(1, 2, 0).numpy()
    return np.clip(t * 220 + rng.uniform(0, 30, (h, w, 3)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- views kernel
FLIPS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def test_views_equal_gather_tiles_and_resize_u8():
    from dafne_amd.data.loader import _to_chw_resized
    from dafne_amd.modeling.tta import resize_u8
    from dafne_amd.scene import gather_tiles, scene_views
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((700, 900), (1300, 1100), (600, 500))]
    d = [torch.from_numpy(imgs[0]).to(dev()), torch.from_numpy(imgs[1]).to(dev()).permute(2, 0, 1).contiguous(),
         torch.from_numpy(imgs[2]).to(dev())]
    hwc = [True, False, True]
    origins = [split_origins(i.shape[0], i.shape[1], 1024, 200) for i in imgs]
    tiles = gather_tiles(d, origins, 1024)                                  # [T, 1024, 1024, 3]
    srcs = [(d[s], hwc[s], left, up, 1024, 1024) for s in range(3) for left, up in origins[s]]
    assert len(srcs) == tiles.shape[0] >= 4
    chw = [tiles[t].permute(2, 0, 1).contiguous() for t in range(len(srcs))]
    for size in (450, 500, 600, 700, 800, 900, 1000, 1024, 1100, 1200):
        views = [src + f for src in srcs for f in FLIPS]                   # HWC and CHW scenes in one launch
        out = scene_views(views, size, size)
        k = 0
        for t in range(len(srcs)):
            for hf, vf in FLIPS:
                want = resize_u8(chw[t], size, size, bool(hf), bool(vf))
                assert torch.equal(out[k], want), (size, t, hf, vf)
                k += 1
    # a pre-resized tile (the test loader's resize to MIN_SIZE_TEST), the window = the whole image; a non-square output
    pre = _to_chw_resized(tiles[1], 800, 800)
    for oh, ow in ((450, 450), (800, 800), (1100, 1100), (600, 900)):
        out = scene_views([(pre, False, 0, 0, 800, 800) + f for f in FLIPS], oh, ow)
        for k, (hf, vf) in enumerate(FLIPS):
            assert torch.equal(out[k], resize_u8(pre, oh, ow, bool(hf), bool(vf))), (oh, ow, hf, vf)
    out = scene_views([(d[2], True, 0, 0, 1024, 1024, 1, 0)], 700, 1000)   # non-square, edge of a scene smaller than the patch
    assert torch.equal(out[0], resize_u8(chw[len(srcs) - 1], 700, 1000, True, False))


def test_views_equal_pillow():
    from PIL import Image
    from dafne_amd.scene import scene_views
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (900, 1200, 3), dtype=np.uint8)
    t = torch.from_numpy(img).to(dev())
    for left, up, size, hf, vf in ((176, 0, 450, 0, 0), (0, 0, 1100, 1, 0), (176, 0, 800, 0, 1), (500, 300, 1200, 1, 1)):
        got = scene_views([(t, True, left, up, 1024, 1024, hf, vf)], size, size)[0].permute(1, 2, 0).cpu().numpy()
        want = np.asarray(Image.fromarray(crop(img, left, up, 1024)).resize((size, size), Image.BILINEAR))
        if hf:
            want = want[:, ::-1]
        if vf:
            want = want[::-1]
        assert np.array_equal(got, want), (left, up, size, hf, vf)


def test_views_reject_bad_arguments():
    from dafne_amd import _lib
    from dafne_amd.scene import scene_views
    t = torch.zeros((100, 120, 3), dtype=torch.uint8, device=dev())
    with pytest.raises(_lib.DafneHipError, match="window"):
        scene_views([(t, True, -1, 0, 64, 64, 0, 0)], 32, 32)
    with pytest.raises(_lib.DafneHipError, match="window"):
        scene_views([(t, True, 0, 0, 0, 64, 0, 0)], 32, 32)
    with pytest.raises(_lib.DafneHipError, match="downscale"):
        scene_views([(t, True, 0, 0, 100, 120, 0, 0)], 1, 1)
    with pytest.raises(_lib.DafneHipError, match="window widths"):
        scene_views([(t, True, 0, 0, 64, 20 + k, 0, 0) for k in range(9)], 32, 32)


# ------------------------------------------------------------------------------------------------------- candidates kernel
def test_candidates_equal_invert_and_concat_fast():
    from dafne_amd import _lib
    from dafne_amd.config import load_cfg
    from dafne_amd.modeling.tta import DotaDatasetMapperTTA, OneStageRCNNWithTTA
    from dafne_amd.postprocess import rows_to_instances
    from dafne_amd.scene import tta_candidates, tta_view_table
    rng = np.random.default_rng(9)
    k_cap, T = 600, 3
    for opts in (RELEASED_AUG, PRE_RESIZE):
        cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), list(opts))
        mapper = DotaDatasetMapperTTA(cfg)
        lh = int(cfg.INPUT.MIN_SIZE_TEST)
        specs = mapper.view_specs(lh, lh, (1024, 1024))
        table = tta_view_table(mapper, lh, lh, (1024, 1024))
        V = len(table)
        rows = np.zeros((T * V, k_cap, 18), np.float32)
        rows[..., 0:8] = rng.uniform(-20, 1250, (T * V, k_cap, 8))
        rows[..., 8:10] = rng.uniform(0, 1, (T * V, k_cap, 2))
        rows[..., 10] = rng.integers(0, 15, (T * V, k_cap))
        rows[..., 11] = rng.integers(0, 5, (T * V, k_cap))
        rows[..., 16:18] = rng.uniform(0, 1024, (T * V, k_cap, 2))
        counts = rng.integers(0, k_cap + 1, T * V).astype(np.int32)
        counts[0], counts[1], counts[V + 2] = 0, k_cap, 0
        counts[2 * V:] = [k_cap if v % 2 else 0 for v in range(V)]
        drows = torch.from_numpy(rows).to(dev())
        dcnt = torch.from_numpy(counts).to(dev())
        views = [(drows[t * V + v], dcnt[t * V + v:t * V + v + 1], t, v, table[v]) for t in range(T) for v in range(V)]
        cand, ovf = tta_candidates(views[::-1], T, k_cap)                   # the kernel orders by (image, slot)
        assert cand.m_cap == V * k_cap and not ovf.any()
        for t in range(T):
            outs = [{"instances": r} for r in rows_to_instances(drows[t * V:(t + 1) * V], dcnt[t * V:(t + 1) * V],
                                                                 [(1024, 1024)] * V)]
            want = OneStageRCNNWithTTA._invert_and_concat_fast(outs, [s[2] for s in specs])
            n = int(cand.counts[t])
            assert n == len(want) == int(counts[t * V:(t + 1) * V].sum())
            assert torch.equal(cand.corners[t, :n].view(torch.int32), want.pred_corners.view(torch.int32)), t
            assert torch.equal(cand.scores[t, :n], want.scores) and torch.equal(cand.ctr[t, :n], want.centerness)
            assert torch.equal(cand.classes[t, :n].to(torch.int64), want.pred_classes)
            c = want.pred_corners
            assert torch.equal(cand.hbox[t, :n, 0], c[:, 0::2].min(1).values)
            assert torch.equal(cand.hbox[t, :n, 3], c[:, 1::2].max(1).values)
        # a count above k_cap: reported, not silently truncated
        dcnt[V + 3] = k_cap + 1
        _, ovf = tta_candidates(views, T, k_cap)
        assert ovf.cpu().tolist() == [0, 1, 0]
    with pytest.raises(_lib.DafneHipError, match="65536"):
        tta_candidates(views[:2], 1, k_cap, m_cap=65537)
    with pytest.raises(_lib.DafneHipError, match="twice"):
        tta_candidates([views[0], views[0]], 1, k_cap)
    with pytest.raises(_lib.DafneHipError, match="exceed m_cap"):
        tta_candidates(views[:3], 1, k_cap, m_cap=2 * k_cap)


# ------------------------------------------------------------------------------------------------------------------ per tile
def tile_inputs(cfg, scenes_bgr):
    """The test loader's inputs of the split tiles: CHW uint8 on the device, resized to MIN_SIZE_TEST when that differs."""
    from dafne_amd.data.loader import _to_chw_resized, inference_resize_shape
    nh, nw = inference_resize_shape(cfg, 1024, 1024)
    out, fnames = [], []
    for name, img in scenes_bgr:
        for left, up in split_origins(img.shape[0], img.shape[1], 1024, 200):
            t = torch.from_numpy(crop(img, left, up, 1024)).to(dev())
            x = _to_chw_resized(t, nh, nw) if (nh, nw) != (1024, 1024) else t.permute(2, 0, 1).contiguous()
            out.append({"image": x, "height": 1024, "width": 1024})
            fnames.append("%s__1__%d___%d.png" % (name, left, up))
    return out, fnames


@pytest.mark.parametrize("opts", [RELEASED_AUG, PRE_RESIZE])
def test_tile_rows_equal_per_image_tta(opts):
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA
    from dafne_amd.scene import tta_tile_rows
    cfg, m = build("dota-1.0_r50.yaml", seed=31, opts=opts)
    rng = np.random.default_rng(13)
    scenes = [random_scene(rng, h, w) for h, w in ((700, 900), (1500, 1900))]
    tta = OneStageRCNNWithTTA(cfg, m)
    rows, counts, overflow, info, _ = tta_tile_rows(tta, [torch.from_numpy(s).to(dev()) for s in scenes], batch=3)
    torch.cuda.synchronize()
    assert int(overflow.item()) == 0
    inputs, _ = tile_inputs(cfg, [("s%d" % i, s) for i, s in enumerate(scenes)])
    assert len(inputs) == rows.shape[0] == len(info) == 7
    ref = OneStageRCNNWithTTA(cfg, m, images_per_group=1)
    total = 0
    for t, x in enumerate(inputs):
        want = ref([x])[0]["instances"]
        n = int(counts[t])
        assert n == len(want), t
        r = rows[t, :n]
        assert torch.equal(r[:, 0:8].contiguous().view(torch.int32), want.pred_corners.view(torch.int32)), t
        assert torch.equal(r[:, 8], want.scores) and torch.equal(r[:, 9], want.centerness), t
        assert torch.equal(r[:, 10].to(torch.int64), want.pred_classes), t
        total += n
    assert total > 0


# ------------------------------------------------------------------------------------------------------- acceptance: bytes
def classnames_of(cfg):
    from dafne_amd.evaluation import dota_evaluation as de
    names = list(de.CLASSNAMES_DOTA_1_0) + ["container-crane"]
    n = cfg.MODEL.DAFNE.NUM_CLASSES
    return names[:15] if (n == 16 and cfg.DATASETS.DOTA_REMOVE_CONTAINER_CRANE) else names[:n]


def route_scene(m, cfg, scenes_bgr, names, dst, batch=8):
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA
    from dafne_amd.scene import write_task1_merged
    res = OneStageRCNNWithTTA(cfg, m).detect_scenes([torch.from_numpy(s).to(dev()) for s in scenes_bgr], batch=batch)
    write_task1_merged(res, names, classnames_of(cfg), dst)
    return res


def route_files(m, cfg, scenes_bgr, names, out):
    """The released TTA workflow: split_dota tiles, do_test_with_TTA (OneStageRCNNWithTTA called on one tile at a time),
    _generate_task_1_files, mergebypoly."""
    from dafne_amd.evaluation.result_merge import mergebypoly
    from dafne_amd.evaluation.task1 import write_task1_files
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA
    tta = OneStageRCNNWithTTA(cfg, m, images_per_group=1)
    inputs, fnames = tile_inputs(cfg, list(zip(names, scenes_bgr)))
    preds = []
    for x, fn in zip(inputs, fnames):
        for o in tta([x]):
            inst = o["instances"].to(torch.device("cpu"))
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


@pytest.mark.parametrize("cfgname,opts", [("dota-1.0_r50.yaml", RELEASED_AUG),
                                          ("dota-1.5_r101.yaml", ("DATASETS.DOTA_REMOVE_CONTAINER_CRANE", True)),
                                          ("dota-1.0_r50.yaml", PRE_RESIZE)])
def test_scene_tta_writes_the_file_workflows_task1_merged(tmp_path, cfgname, opts):
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


def test_scene_tta_is_independent_of_batch_and_scene_order():
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA
    cfg, m = build("dota-1.0_r50.yaml", seed=37, opts=RELEASED_AUG)
    rng = np.random.default_rng(23)
    scenes = [torch.from_numpy(random_scene(rng, h, w)).to(dev()) for h, w in SCENE_SHAPES]
    scenes[1] = scenes[1].permute(2, 0, 1).contiguous()           # a CHW scene among HWC ones
    tta = OneStageRCNNWithTTA(cfg, m)
    r1 = tta.detect_scenes(scenes)
    r2 = tta.detect_scenes(scenes, batch=3)
    rev = tta.detect_scenes(scenes[::-1])

    def keys(res):
        out, base = [], 0
        for r in res:
            org = np.array(r["origins"]).reshape(-1, 2)
            out.append((r["corners"].cpu().numpy(), r["scores"].cpu().numpy(), r["labels"].cpu().numpy(), r["row"].cpu().numpy(),
                        org[r["tile"].cpu().numpy() - base]))
            base += len(r["origins"])
        return out
    k1, k2, kr = keys(r1), keys(r2), keys(rev)[::-1]
    assert sum(len(r["scores"]) for r in r1) > 0
    for x, y, z in zip(k1, k2, kr):
        for u, v, w in zip(x, y, z):
            assert np.array_equal(u, v) and np.array_equal(u, w)


def test_eval_net_scene_tta_writes_the_same_files(tmp_path):
    from PIL import Image
    from dafne_amd.data.loader import read_image
    rng = np.random.default_rng(41)
    sd = tmp_path / "scenes"
    sd.mkdir()
    names = ["P0001", "P0002"]
    for name, (h, w) in zip(names, SCENE_SHAPES[:2]):
        Image.fromarray(random_scene(rng, h, w)).save(sd / (name + ".png"))
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file",
                        os.path.join(ROOT, "configs", "dota-1.0_r101.yaml"), "--scene-dir", str(sd), "--scene-tta",
                        "--task1-merged-dir", str(out), "--zip"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    cfg, m = build("dota-1.0_r101.yaml", seed=0, bench_weights=True)
    scenes = [read_image(str(sd / (n + ".png"))) for n in names]
    a = str(tmp_path / "a")
    route_scene(m, cfg, scenes, names, a)
    assert_same_dirs(a, str(out / "Task1_merged"))
    import zipfile
    with zipfile.ZipFile(out / "task1_merged.zip") as z:
        assert sorted(z.namelist()) == sorted(os.listdir(a))
        for f in z.namelist():
            assert z.read(f) == open(os.path.join(a, f), "rb").read()
