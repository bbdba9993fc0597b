"""CPU: multi-scale whole-scene inference's host half (dafne_amd/scene.py: scaled_size, scale_plan, the scales= arguments).

  * scaled_size rounds half to even and never gives a size of 0;
  * tests/_resample_np.py -- the expectation of the GPU tests of dafne_scene_scaled_tiles_u8_hip -- equals PIL.Image.resize bit
    for bit, both filters, on the GPU tests' shapes and scales (so a wrong expectation cannot hide a wrong kernel);
  * the tile order of scales=(1, 0.5): scene-major, then scale, then split order;
  * the refused arguments of detect_scenes / detect_scenes_tta / tools/eval_net.py that need no GPU;
  * the new entries in the header, the ctypes table and the library; split_origins(rate != 1) still refuses."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import _resample_np as rs
from test_abi import _header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 45), (61, 83), (97, 131), (5, 300), (33, 70), (300, 7)]
SCALES = [0.3, 0.5, 0.75, 1.25, 1.5, 2.0]
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def test_scaled_size_rounds_half_to_even():
    from dafne_amd.scene import scaled_size
    assert scaled_size(5, 7, 0.5) == (2, 4)            # 2.5 -> 2, 3.5 -> 4
    assert scaled_size(1, 3, 0.5) == (1, 2)            # 0.5 -> 0 -> at least 1; 1.5 -> 2
    assert scaled_size(9, 11, 0.5) == (4, 6)           # 4.5 -> 4, 5.5 -> 6
    assert scaled_size(3, 1, 1.5) == (4, 2)            # 4.5 -> 4, 1.5 -> 2
    assert scaled_size(1, 1, 0.01) == (1, 1) and scaled_size(2, 300, 0.2) == (1, 60)
    assert scaled_size(700, 900, 1) == (700, 900) and scaled_size(4000, 3999, 1.0) == (4000, 3999)
    assert scaled_size(700, 900, 0.5) == (350, 450) and scaled_size(37, 45, 0.3) == (11, 14)     # 11.1, 13.5 -> 14
    assert all(isinstance(v, int) for v in scaled_size(37, 45, 0.3))


@pytest.mark.parametrize("resample", ["bilinear", "bicubic"])
def test_numpy_resampler_equals_pillow(resample):
    from dafne_amd.scene import scaled_size
    clipped = [0, 0]
    for h, w in SHAPES:
        img = rs.overshoot_image(h, w, seed=h)
        for s in SCALES:
            nh, nw = scaled_size(h, w, s)
            want = np.asarray(Image.fromarray(img).resize((nw, nh), PIL_FILTER[resample]))
            got = rs.resize(img, nh, nw, resample)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (h, w, s)
            clipped[0] += int((want == 0).sum())
            clipped[1] += int((want == 255).sum())
    assert min(clipped) > 0
    # the realistic size of the GPU test, and a downscale with many taps
    img = rs.overshoot_image(700, 900, seed=1)
    for nh, nw in ((350, 450), (1050, 1350), (70, 64)):
        assert np.array_equal(rs.resize(img, nh, nw, resample), np.asarray(Image.fromarray(img).resize((nw, nh), PIL_FILTER[resample])))


def test_bicubic_overshoot_clips_in_the_horizontal_pass():
    """The uint8 intermediate is clipped after the horizontal pass: an unclipped intermediate gives other bytes."""
    img = rs.overshoot_image(33, 70, seed=3)
    k = rs.coeffs(70, 105, "bicubic")
    acc = np.stack([(1 << 21) + (img[:, x0:x0 + len(c)].astype(np.int64) * c[None, :, None]).sum(1) for x0, c in k], 1) >> 22
    assert (acc < 0).any() and (acc > 255).any()
    assert any((c < 0).any() for _, c in k)


def test_crop_zero_pad():
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3) + 1
    t = rs.crop_zero_pad(img, 4, 2, 8)
    assert t.shape == (8, 8, 3) and np.array_equal(t[:3, :3], img[2:, 4:]) and not t[3:].any() and not t[:, 3:].any()


def test_tile_order_is_scene_then_scale_then_split():
    from dafne_amd.scene import scale_plan, scaled_size, split_origins
    sizes = [(1848, 1100), (3000, 4000)]
    plan = scale_plan(sizes, (1.0, 0.5), 1024, 200)
    assert len(plan) == 2
    for (h, w), per in zip(sizes, plan):
        assert [s for s, _, _ in per] == [1.0, 0.5]
        assert per[0][1] == (h, w) and per[0][2] == split_origins(h, w, 1024, 200)
        assert per[1][1] == scaled_size(h, w, 0.5) and per[1][2] == split_origins(*scaled_size(h, w, 0.5), 1024, 200)
    assert [len(o) for _, _, o in plan[0]] == [4, 1] and [len(o) for _, _, o in plan[1]] == [20, 6]      # 924 x 550: one tile; 1500 x 2000: 3 x 2
    # the given order is kept: 0.5 before 1
    rev = scale_plan(sizes[:1], (0.5, 1.0), 1024, 200)[0]
    assert [s for s, _, _ in rev] == [0.5, 1.0] and rev[0][2] == plan[0][1][2]


def test_split_rate_other_than_one_is_still_refused():
    from dafne_amd.scene import split_origins
    with pytest.raises(NotImplementedError, match="INTER_CUBIC"):
        split_origins(2000, 2000, rate=0.5)


@pytest.mark.parametrize("scales", [(), (1, 1), (1, 0.5, 0.5), (float("nan"),), (1, float("inf")), (0,), (-0.5,), (4.5,)])
def test_detect_scenes_refuses_bad_scales(scales):
    from dafne_amd import scene
    with pytest.raises(ValueError, match="scale"):
        scene.detect_scenes(None, [], scales=scales)
    with pytest.raises(ValueError, match="scale"):
        scene.detect_scenes_tta(None, [], scales=scales)


def test_detect_scenes_argument_refusals():
    from dafne_amd import scene
    with pytest.raises(ValueError, match="resample"):
        scene.detect_scenes(None, [], scales=(1, 0.5), resample="lanczos")
    with pytest.raises(ValueError, match="resample"):
        scene.detect_scenes(None, [], resample="nearest")
    assert scene.detect_scenes(None, [], scales=(1, 0.5)) == [] and scene.detect_scenes(None, [], scales=(4,), resample="bilinear") == []
    assert scene.detect_scenes(None, [], scales=[1]) == []
    with pytest.raises(NotImplementedError, match="scales"):
        scene.detect_scenes_tta(None, [], scales=(1, 0.5))
    with pytest.raises(NotImplementedError, match="scales"):
        scene.detect_scenes_tta(None, [], scales=(0.5,))
    assert scene.detect_scenes_tta(None, [], scales=(1,)) == []


def test_wrappers_pass_scales_through():
    import inspect
    from dafne_amd.modeling.one_stage_detector import OneStageDetector
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA
    p = inspect.signature(OneStageDetector.detect_scenes).parameters
    assert p["scales"].default == (1,) and p["resample"].default == "bicubic"
    assert inspect.signature(OneStageRCNNWithTTA.detect_scenes).parameters["scales"].default == (1,)


def test_eval_net_scene_scales_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import eval_net
    finally:
        sys.path.pop(0)
    base = ["--config-file", os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")]
    err = lambda *a: eval_net.scene_args_error(eval_net.parse_args(base + list(a)))      # noqa: E731
    assert eval_net.parse_args(base).scene_scales == "1" and eval_net.parse_args(base).scene_resample == "bicubic"
    assert eval_net.parse_scene_scales("1,0.5") == (1.0, 0.5) and eval_net.parse_scene_scales(" 1.5 ") == (1.5,)
    assert "need --scene-dir" in err("--scene-scales", "1,0.5")
    assert "need --scene-dir" in err("--scene-resample", "bilinear")
    assert err("--scene-scales", "1") is None
    assert err("--scene-dir", "x", "--scene-scales", "1,0.5") is None
    assert err("--scene-dir", "x", "--scene-scales", "1,0.5", "--scene-resample", "bilinear", "--task2") is None
    assert "--scene-tta does not support --scene-scales" in err("--scene-dir", "x", "--scene-scales", "1,0.5", "--scene-tta")
    assert err("--scene-dir", "x", "--scene-scales", "1", "--scene-tta") is None
    for bad in ("1,,0.5", "half", ""):
        assert "comma-separated" in err("--scene-dir", "x", "--scene-scales", bad)
    with pytest.raises(SystemExit, match="need --scene-dir"):
        eval_net.main(base + ["--scene-scales", "1,0.5"])
    with pytest.raises(SystemExit):
        eval_net.parse_args(base + ["--scene-resample", "lanczos"])


NEW_ENTRIES = {
    "dafne_scene_scaled_tiles_workspace_bytes": ["ptr", "int"],
    "dafne_scene_scaled_tiles_u8_hip": ["ptr", "int", "int", "ptr", "ptr", "size", "ptr"],
    "dafne_scene_merge_rows_scaled_hip": ["ptr", "ptr", "int", "int", "ptr", "ptr", "int", "int", "struct", "int", "int", "ptr", "ptr",
                                          "ptr", "ptr", "size", "ptr"],
    "dafne_scene_merge_hbb_rows_scaled_hip": ["ptr", "ptr", "int", "int", "ptr", "ptr", "int", "int", "struct", "int", "int", "ptr",
                                              "ptr", "ptr", "ptr", "size", "ptr"],
}


def test_header_exports_and_ctypes_agree_on_the_new_entries():
    from dafne_amd import _lib, build
    protos = _header_prototypes()
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    by_kind = {"ptr": "ptr", "int": ctypes.c_int, "size": ctypes.c_size_t, "struct": ctypes.c_uint64}
    for name, kinds in NEW_ENTRIES.items():
        assert protos.get(name) == kinds, (name, protos.get(name))
        assert name in exported, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(kinds), name
        for a, k in zip(args, kinds):
            if k == "ptr":
                assert a is ctypes.c_void_p or issubclass(a, ctypes._Pointer), (name, a)
            else:
                assert a is by_kind[k], (name, a)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
    L = _lib.load()
    assert L.dafne_abi_version() >= 148
    # the descriptor: the header's field order and size
    assert [f for f, _ in _lib.ScaledTile._fields_] == ["d_scene", "h", "w", "layout_hwc", "new_h", "new_w", "left", "up", "filter"]
    assert ctypes.sizeof(_lib.ScaledTile) == 40
    text = open(os.path.join(ROOT, "include", "dafne_amd.h")).read()
    assert "int32_t new_h, new_w;" in text and "DAFNE_FILTER_BICUBIC 1" in text
    assert (_lib.FILTER_BILINEAR, _lib.FILTER_BICUBIC) == (0, 1)


def test_scaled_tiles_descriptors_are_checked_on_the_host():
    """The host-side checks need no GPU: the workspace size of invalid descriptors is 0, and the entry refuses them before any
    device call."""
    from dafne_amd import _lib
    L = _lib.load()

    def tile(**kw):
        a = (_lib.ScaledTile * 1)()
        d = dict(d_scene=4096, h=100, w=120, layout_hwc=1, new_h=50, new_w=60, left=0, up=0, filter=1)
        d.update(kw)
        for k, v in d.items():
            setattr(a[0], k, v)
        return a
    assert L.dafne_scene_scaled_tiles_workspace_bytes(tile(), 1) > 0
    assert L.dafne_scene_scaled_tiles_workspace_bytes(tile(), 0) == 0
    fake = ctypes.c_void_p(4096)
    for kw in (dict(left=60), dict(up=50), dict(left=-1), dict(new_h=0), dict(w=0), dict(filter=2), dict(layout_hwc=2),
               dict(d_scene=None)):
        assert L.dafne_scene_scaled_tiles_workspace_bytes(tile(**kw), 1) == 0, kw
        assert L.dafne_scene_scaled_tiles_u8_hip(tile(**kw), 1, 64, fake, fake, 1 << 30, None) != 0, kw
    # patch: a positive multiple of 4
    assert L.dafne_scene_scaled_tiles_u8_hip(tile(), 1, 0, fake, fake, 1 << 30, None) != 0
    assert L.dafne_scene_scaled_tiles_u8_hip(tile(), 1, 62, fake, fake, 1 << 30, None) != 0
    assert b"multiple" in L.dafne_last_error()
    # the tap limit: bicubic above 15x, bilinear above 31x
    assert L.dafne_scene_scaled_tiles_u8_hip(tile(h=1600, w=1600, new_h=100, new_w=100), 1, 64, fake, fake, 1 << 30, None) != 0
    assert b"downscale" in L.dafne_last_error()
    assert L.dafne_scene_scaled_tiles_u8_hip(tile(h=3300, w=3300, new_h=100, new_w=100, filter=0), 1, 64, fake, fake, 1 << 30, None) != 0
    assert b"downscale" in L.dafne_last_error()
    # too small a workspace is refused before the copy
    assert L.dafne_scene_scaled_tiles_u8_hip(tile(), 1, 64, fake, fake, 16, None) != 0
    assert b"workspace" in L.dafne_last_error()
