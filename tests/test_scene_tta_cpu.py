"""CPU: scene-level TTA's host half -- the refused eval_net options, and the per-view table of dafne_amd.scene.tta_view_table
(view order, resize targets, flips, float32 inverse ratios) against DotaDatasetMapperTTA.view_specs and against the corners
OneStageRCNNWithTTA._invert_and_concat_fast computes from the same transforms."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELEASED_AUG = ("TEST.AUG.MIN_SIZES", [450, 500, 600, 700, 800, 900, 1000, 1100, 1200], "TEST.AUG.MAX_SIZE", 1200,
                "TEST.AUG.HFLIP", True, "TEST.AUG.VFLIP", True)


def _eval_net(args):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file",
           os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_scene_tta_needs_scene_dir():
    p = _eval_net(["--scene-tta"])
    assert p.returncode != 0
    assert "--scene-tta" in p.stderr and "--scene-dir" in p.stderr, p.stderr


def test_scene_tta_refuses_several_gpus(tmp_path):
    p = _eval_net(["--scene-dir", str(tmp_path), "--scene-tta", "--num-gpus", "2"])
    assert p.returncode != 0
    assert "--scene-dir" in p.stderr and "one GPU" in p.stderr, p.stderr


def test_scene_dir_with_tta_points_to_scene_tta(tmp_path):
    p = _eval_net(["--scene-dir", str(tmp_path), "--tta"])
    assert p.returncode != 0
    assert "--scene-dir" in p.stderr and "--tta" in p.stderr and "--scene-tta" in p.stderr, p.stderr


def _mapper(cfgname, opts):
    from dafne_amd.config import load_cfg
    from dafne_amd.data.loader import inference_resize_shape
    from dafne_amd.modeling.tta import DotaDatasetMapperTTA
    cfg = load_cfg(os.path.join(ROOT, "configs", cfgname), list(opts))
    return DotaDatasetMapperTTA(cfg), inference_resize_shape(cfg, 1024, 1024)


@pytest.mark.parametrize("cfgname,opts", [("dota-1.0_r101.yaml", ()),
                                          ("dota-1.0_r50.yaml", RELEASED_AUG + ("INPUT.MIN_SIZE_TEST", 800, "INPUT.MAX_SIZE_TEST", 800)),
                                          ("dota-1.0_r50.yaml", ("TEST.AUG.MIN_SIZES", [600, 800, 1100], "TEST.AUG.MAX_SIZE", 1200,
                                                                 "TEST.AUG.HFLIP", True, "TEST.AUG.VFLIP", False,
                                                                 "INPUT.MIN_SIZE_TEST", 800, "INPUT.MAX_SIZE_TEST", 800))])
def test_view_table_matches_view_specs_and_the_inverse_transforms(cfgname, opts):
    from dafne_amd.modeling.tta import HFlipT, OneStageRCNNWithTTA, VFlipT
    from dafne_amd.scene import tta_view_table
    from dafne_amd.structures import Instances
    mapper, (nh, nw) = _mapper(cfgname, opts)
    specs = mapper.view_specs(nh, nw, (1024, 1024))
    table = tta_view_table(mapper, nh, nw, (1024, 1024))
    assert len(table) == len(specs) == len(mapper.min_sizes) * (1 + int(mapper.hflip) + int(mapper.vflip))
    for row, (sh, sw, tfl) in zip(table, specs):
        assert row[:2] == (sh, sw)
        last = tfl.tfms[-1]
        assert row[2] == isinstance(last, HFlipT) and row[3] == isinstance(last, VFlipT)
        assert row[4] == (sw if row[2] else 0) and row[5] == (sh if row[3] else 0)
        assert all(isinstance(v, np.float32) for v in row[4:])
        assert row[8] == np.float32(1024 / nw) and row[9] == np.float32(1024 / nh)
        assert row[6] == np.float32(nw / sw) and row[7] == np.float32(nh / sh)
    # the corners the table maps to are the ones _invert_and_concat_fast computes, bit for bit (its table is built from the
    # same transforms; here on the CPU)
    rng = np.random.default_rng(7)
    outputs, want = [], []
    for row in table:
        n = int(rng.integers(0, 40))
        c = rng.uniform(-30, 1300, (n, 8)).astype(np.float32)
        inst = Instances((1024, 1024))
        inst.pred_corners = torch.from_numpy(c)
        inst.scores = torch.from_numpy(rng.uniform(0, 1, n).astype(np.float32))
        inst.centerness = torch.from_numpy(rng.uniform(0, 1, n).astype(np.float32))
        inst.pred_classes = torch.from_numpy(rng.integers(0, 15, n))
        outputs.append({"instances": inst})
        x, y = c[:, 0::2], c[:, 1::2]
        x = np.where(row[2], row[4] - x, x).astype(np.float32)
        y = np.where(row[3], row[5] - y, y).astype(np.float32)
        x = (x * row[6]).astype(np.float32) * row[8]
        y = (y * row[7]).astype(np.float32) * row[9]
        want.append(np.stack([x, y], axis=2).reshape(-1, 8).astype(np.float32))
    got = OneStageRCNNWithTTA._invert_and_concat_fast(outputs, [s[2] for s in specs])
    assert got is not None
    w = np.concatenate(want)
    assert w.shape[0] > 100
    assert np.array_equal(got.pred_corners.numpy().view(np.int32), w.view(np.int32))


def test_view_table_refuses_rotation():
    from dafne_amd.config import load_cfg
    from dafne_amd.modeling.tta import DotaDatasetMapperTTA
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r101.yaml"), ["TEST.AUG.ROTATION_ANGLES", [90.0]])
    with pytest.raises(NotImplementedError):
        DotaDatasetMapperTTA(cfg)
