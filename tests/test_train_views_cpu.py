"""CPU: the definition of the training views (tests/_train_views_np.py) against np.rot90 and PIL, the
random parameters of data.train_views.TrainAugmentation, and the ABI of the new entry points."""
import copy
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _train_views_np as tv  # noqa: E402

ORIENTATIONS = list(itertools.product((0, 1), (0, 1), (0, 1, 2, 3)))


def image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("hw", [(5, 8), (6, 6), (7, 4), (1, 1), (1, 6)])
def test_rot_forms_agree_with_rot90(hw):
    """A marked pixel's centre maps to the marked pixel's centre, for every orientation, odd and even sizes."""
    h, w = hw
    for (hf, vf, rot) in ORIENTATIONS:
        for (py, px) in {(0, 0), (h - 1, w - 1), (h // 2, w // 3), (h - 1, 0)}:
            img = np.zeros((h, w, 3), np.uint8)
            img[py, px] = 255
            out = tv.view_pixels(img, 0, 0, h, w, hf, vf, h, w, rot)
            assert out.shape[:2] == tv.out_hw(h, w, rot)
            ys, xs = np.nonzero(out[:, :, 0])
            assert ys.shape[0] == 1
            centre = np.array([[px + 0.5, py + 0.5] * 4], dtype=np.float32)
            x, y = tv.view_coords(centre, h, w, hf, vf, h, w, rot)
            assert (x[0, 0], y[0, 0]) == (xs[0] + 0.5, ys[0] + 0.5), (hf, vf, rot, py, px)


def test_pixels_are_rot90_of_flipped_resize():
    img = image(9, 13, 0)
    for (hf, vf, rot) in ORIENTATIONS:
        w = img[:, ::-1] if hf else img
        w = w[::-1] if vf else w
        assert np.array_equal(tv.view_pixels(img, 0, 0, 9, 13, hf, vf, 9, 13, rot), np.rot90(w, rot))


def test_inverse_view_restores_pixels_and_integer_coordinates():
    img = image(11, 14, 1)
    pts = np.array([[0, 0, 14, 0, 14, 11, 0, 11], [3, 2, 9, 4, 8, 10, 1, 7]], dtype=np.float32)
    for (hf, vf, rot) in ORIENTATIONS:
        out = tv.view_pixels(img, 0, 0, 11, 14, hf, vf, 11, 14, rot)
        oh, ow = out.shape[:2]
        ihf, ivf, irot = tv.inverse_view(hf, vf, rot)
        back = tv.view_pixels(out, 0, 0, oh, ow, ihf, ivf, oh, ow, irot)
        assert np.array_equal(back, img), (hf, vf, rot)
        x, y = tv.view_coords(pts, 11, 14, hf, vf, 11, 14, rot)
        q = np.stack((x, y), 2).reshape(-1, 8).astype(np.float32)
        bx, by = tv.view_coords(q, oh, ow, ihf, ivf, oh, ow, irot)
        assert np.array_equal(np.stack((bx, by), 2).reshape(-1, 8), pts.astype(np.float64)), (hf, vf, rot)


@pytest.mark.parametrize("case", [((37, 53), (4, 6, 30, 40), (35, 51)), ((37, 53), (20, 30, 30, 40), (60, 90)),
                                  ((40, 64), (0, 0, 40, 64), (19, 23)), ((40, 64), (3, 5, 31, 53), (31, 53))])
def test_pixel_route_equals_pil_on_flipped_crops(case):
    from PIL import Image
    (h, w), (left, up, wh, ww), (nh, nw) = case
    img = image(h, w, 2)
    for (hf, vf, rot) in ORIENTATIONS:
        crop = np.zeros((wh, ww, 3), np.uint8)
        part = img[up:up + wh, left:left + ww]
        crop[:part.shape[0], :part.shape[1]] = part
        crop = crop[:, ::-1] if hf else crop
        crop = crop[::-1] if vf else crop
        want = np.asarray(Image.fromarray(np.ascontiguousarray(crop)).resize((nw, nh), Image.BILINEAR))
        assert np.array_equal(tv.view_pixels(img, left, up, wh, ww, hf, vf, nh, nw, rot), np.rot90(want, rot)), (hf, vf, rot)


def test_gt_filter_sort_area_and_order():
    rect = [10, 20, 30, 20, 30, 28, 10, 28]                    # axis-aligned: ties in sort_quadrilateral's argmin
    zero_w = [5, 5, 5, 9, 5, 12, 5, 7]
    zero_h = [5, 5, 9, 5, 12, 5, 7, 5]
    quad = [12.5, 3.25, 40, 9, 33, 30.5, 8, 21]
    corners = np.array([rect, zero_w, quad, zero_h, rect], dtype=np.float32)
    classes = np.array([3, 1, 4, 1, 5], dtype=np.int32)
    for (hf, vf, rot) in ORIENTATIONS:
        for (nh, nw) in ((48, 64), (36, 80), (31, 45)):
            g = tv.view_gt(corners, classes, 48, 64, hf, vf, nh, nw, rot, sort=True)
            assert g["src"].tolist() == [0, 2, 4] and g["classes"].tolist() == [3, 4, 5]
            assert g["corners"].dtype == np.float32 and g["hbox"].dtype == np.float32 and g["area"].dtype == np.float32
            assert np.array_equal(g["corners"][0], g["corners"][2])
            sx, sy = nw / 64.0, nh / 48.0
            assert abs(float(g["area"][0]) - 20 * 8 * sx * sy) < 1e-3 * 160 * sx * sy
            # sorted: the first corner has the minimal x; the corner set is the transformed set
            assert (g["corners"][:, 0] == g["corners"][:, 0::2].min(1)).all()
            u = tv.view_gt(corners, classes, 48, 64, hf, vf, nh, nw, rot, sort=False)
            assert np.array_equal(np.sort(u["corners"].reshape(-1, 4, 2), axis=1), np.sort(g["corners"].reshape(-1, 4, 2), axis=1))
            assert np.array_equal(u["hbox"], g["hbox"]) and np.array_equal(u["area"], g["area"])
    e = tv.view_gt(np.zeros((0, 8), np.float32), np.zeros(0, np.int32), 48, 64, 1, 0, 48, 64, 1)
    assert e["corners"].shape == (0, 8) and e["src"].shape == (0,)


def test_batch_gt_offsets():
    rs = np.random.RandomState(5)
    counts = [0, 3, 70, 0]
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    corners = rs.uniform(0, 60, size=(off[-1], 8)).astype(np.float32)
    corners[5] = [1, 1, 1, 4, 1, 6, 1, 2]
    views = [(48, 64, 0, 0, 48, 64, 0), (48, 64, 1, 0, 30, 40, 1), (48, 64, 0, 1, 96, 128, 3), (48, 64, 1, 1, 48, 64, 2)]
    out = tv.batch_gt(views, corners, np.arange(off[-1]), off)
    assert out["offsets"].tolist() == [0, 0, 3, 72, 72] and out["src"].tolist() == [i for i in range(73) if i != 5]


# ------------------------------------------------------------------------------------------------ TrainAugmentation
def cfg_with(**kw):
    from dafne_amd.config import get_cfg
    cfg = copy.deepcopy(get_cfg())
    for k, v in kw.items():
        cfg.INPUT[k] = v
    return cfg


def test_sampler_draw_order_and_reproducibility():
    from dafne_amd.data.train_views import TrainAugmentation, ViewParams
    from dafne_amd.data.loader import shortest_edge_size
    sizes = [450, 500, 600, 700, 800, 900, 1000, 1100, 1200]
    cfg = cfg_with(MIN_SIZE_TRAIN=sizes, MAX_SIZE_TRAIN=1200, MIN_SIZE_TRAIN_SAMPLING="choice")
    aug = TrainAugmentation(cfg)
    wins = [(1024, 1024), (600, 1000), (1000, 400)] * 6
    got = aug.sample(wins, np.random.default_rng(11))
    rng = np.random.default_rng(11)                        # the documented order: hflip, vflip, size, angle
    for (h, w), p in zip(wins, got):
        hf, vf = int(rng.random() < 0.5), int(rng.random() < 0.5)
        s = sizes[int(rng.integers(len(sizes)))]
        rot = [0, 1, 2, 3][int(rng.integers(4))]
        assert p == ViewParams(hf, vf, *shortest_edge_size(h, w, s, 1200), rot)
        assert max(p.new_h, p.new_w) <= 1200                                       # MAX_SIZE_TRAIN is applied
    assert got == aug.sample(wins, np.random.default_rng(11))
    assert got != aug.sample(wins, np.random.default_rng(12))
    assert any(max(p.new_h, p.new_w) == 1200 and min(p.new_h, p.new_w) < 1000 for p in got)     # ... and it bit on a long image
    assert {p.rot for p in got} == {0, 1, 2, 3} and {p.hflip for p in got} == {0, 1} and {p.vflip for p in got} == {0, 1}


def test_sampler_range_both_and_no_angles():
    from dafne_amd.data.train_views import TrainAugmentation
    aug = TrainAugmentation(cfg_with(MIN_SIZE_TRAIN=[300, 310], MAX_SIZE_TRAIN=2000, MIN_SIZE_TRAIN_SAMPLING="range", ROTATION_AUG_ANGLES=[]))
    got = aug.sample([(500, 500)] * 200, np.random.default_rng(0))
    assert {p.new_h for p in got} == set(range(300, 311)) and all(p.rot == 0 and p.new_h == p.new_w for p in got)
    both = TrainAugmentation(cfg_with(RESIZE_TYPE="both", RESIZE_HEIGHT_TRAIN=320, RESIZE_WIDTH_TRAIN=480, ROTATION_AUG_ANGLES=[90.0, 270.0]))
    got = both.sample([(500, 700), (64, 64)], np.random.default_rng(0))
    assert all((p.new_h, p.new_w) == (320, 480) and p.rot in (1, 3) and p.out_hw() == (480, 320) for p in got)
    neg = TrainAugmentation(cfg_with(ROTATION_AUG_ANGLES=[-90.0, 360.0]))
    assert neg.rots == [3, 0]


def test_sampler_refusals():
    from dafne_amd.data.train_views import TrainAugmentation
    with pytest.raises(NotImplementedError):
        TrainAugmentation(cfg_with(ROTATION_AUG_ANGLES=[0.0, 45.0]))
    with pytest.raises(NotImplementedError):
        TrainAugmentation(cfg_with(ROTATION_AUG_SAMPLE_STYLE="range", ROTATION_AUG_ANGLES=[0.0, 90.0]))
    with pytest.raises(NotImplementedError):
        TrainAugmentation(cfg_with(USE_COLOR_AUGMENTATIONS=True))
    with pytest.raises(RuntimeError):
        TrainAugmentation(cfg_with(RESIZE_TYPE="longest"))
    with pytest.raises(ValueError):
        TrainAugmentation(cfg_with(MIN_SIZE_TRAIN=[300, 400, 500], MIN_SIZE_TRAIN_SAMPLING="range"))


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_version_symbols_and_refusals_without_a_device():
    from dafne_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.dafne_abi_version() >= 153
    for name in ("dafne_train_views_u8_hip", "dafne_train_views_workspace_bytes", "dafne_train_gt_hip", "dafne_train_gt_workspace_bytes"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert ctypes.sizeof(_lib.TrainView) == 56
    v = (_lib.TrainView * 1)()
    a = v[0]
    a.d_src, a.h, a.w, a.layout_hwc, a.left, a.up, a.win_h, a.win_w, a.new_h, a.new_w, a.rot = 4096, 10, 10, 1, 0, 0, 10, 10, 10, 10, 0
    assert L.dafne_train_views_workspace_bytes(v, 1) > 0
    assert L.dafne_train_views_workspace_bytes(None, 1) == 0 and L.dafne_train_views_workspace_bytes(v, 0) == 0
    a.rot = 4
    assert L.dafne_train_views_workspace_bytes(v, 1) == 0
    a.rot, a.new_h = 1, 0
    assert L.dafne_train_views_workspace_bytes(v, 1) == 0
    assert L.dafne_train_gt_workspace_bytes(0, 5) == 0 and L.dafne_train_gt_workspace_bytes(2, -1) == 0
    assert L.dafne_train_gt_workspace_bytes(2, 100) >= 100 * 14 * 4
    # refused on the host, before anything is launched or dereferenced (the pointers are never read)
    a.new_h = 10
    fake = ctypes.c_void_p(4096)
    rc = L.dafne_train_views_u8_hip(v, 1, 16, 18, fake, fake, fake, 1 << 20, None)
    assert rc != 0 and b"multiple of 4" in L.dafne_last_error()
    rc = L.dafne_train_views_u8_hip(v, 1, 16, 16, ctypes.c_void_p(4098), fake, fake, 1 << 20, None)
    assert rc != 0 and b"aligned" in L.dafne_last_error()
    rc = L.dafne_train_views_u8_hip(v, 1, 8, 16, fake, fake, fake, 1 << 20, None)
    assert rc != 0 and b"does not fit" in L.dafne_last_error()
    a.win_h, a.h, a.new_h, a.rot = 400, 400, 10, 0
    rc = L.dafne_train_views_u8_hip(v, 1, 16, 16, fake, fake, fake, 1 << 20, None)
    assert rc != 0 and b"downscale" in L.dafne_last_error()
    # compiled inside the two existing matrix-free units: no contraction, no SLP vectoriser
    for unit in ("decode.hip", "resize.hip"):
        assert {"-ffp-contract=off", "-fno-slp-vectorize"} <= set(build.PER_FILE[unit])
    assert '#include "train_views_kernels.h"' in open(os.path.join(build.CSRC, "decode.hip")).read()


def test_eval_net_train_aug_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_net
    finally:
        sys.path.pop(0)
    base = ["--config-file", os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")]
    err = lambda *a: eval_net.scene_args_error(eval_net.parse_args(base + list(a)))      # noqa: E731
    scene = ("--val-loss", "--scene-dir", "d", "--scene-labels", "l")
    assert err(*scene) is None and err(*scene, "--train-aug", "--seed", "3") is None
    assert err(*scene, "--train-aug", "--steps", "5") is None
    assert "--train-aug needs" in err("--train-aug")
    assert "--train-aug needs" in err("--val-loss", "--image-dir", "i", "--label-dir", "l", "--train-aug")
    assert "--steps needs" in err(*scene, "--steps", "5")


# ------------------------------------------------------------------------------------------------ the reference's mapper
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_views.npz")


def golden_cases():
    """-> [(name, (win_h, win_w, hflip, vflip, new_h, new_w, rot), sort, corners_in, {corners, hbox, area, src})]: what the
    reference's DAFNeDatasetMapper made of build_train_loader's augmentation list (tests/golden/make_golden_train_views.py)."""
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(str(n) for n in z["names"]):
        p = [int(v) for v in z["case_%d_params" % i]]
        want = {k: z["case_%d_%s" % (i, k)] for k in ("corners", "hbox", "area", "src")}
        out.append((name, tuple(p[:7]), bool(p[7]), z["case_%d_corners_in" % i], want))
    return out


def test_restatement_equals_the_reference_mapper():
    cases = golden_cases()
    names = {c[0] for c in cases}
    assert names >= {"o%d%d%d" % (a, b, r) for a in (0, 1) for b in (0, 1) for r in range(4)} | {"up", "down", "nondyadic", "empty", "unsorted"}
    dropped = 0
    for name, p, sort, corners, want in cases:
        got = tv.view_gt(corners, np.arange(corners.shape[0]), *p, sort=sort)
        assert np.array_equal(got["src"], want["src"]), name                      # kept rows and their order
        for k in ("corners", "hbox", "area"):
            assert got[k].dtype == np.float32 and want[k].dtype == np.float32
            assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (name, k)
        dropped += corners.shape[0] - want["src"].shape[0]
    assert dropped >= 2 * 16                                                       # the zero-width and zero-height boxes
