"""CPU: whole-scene inference's host half -- the split grid against the reference's own SplitSingle (tests/golden/
scene_split.npz, make_golden_scene.py), the "%.2f" / "%.4f" round trip restated as rint(v * 10^k) / 10^k (what
dafne_scene_merge_rows_hip computes) against Python's formatting, and the refused options."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dafne_amd.scene import split_origins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_origins_equal_the_reference_split(golden):
    g = golden("scene_split")
    cases = g["cases"]
    assert len(cases) >= 15
    for i, (h, w, patch, overlap) in enumerate(cases.tolist()):
        want = [tuple(v) for v in g["origins_%d" % i].tolist()]
        assert split_origins(h, w, patch, overlap) == want, (h, w, patch, overlap)


def test_split_origins_cover_the_scene():
    for h, w in ((700, 900), (1848, 1100), (3000, 4000), (1, 5000), (4000, 4000)):
        org = split_origins(h, w)
        cov = np.zeros((h, w), bool)
        for left, up in org:
            assert 0 <= left < w and 0 <= up < h
            cov[up:up + 1024, left:left + 1024] = True
        assert cov.all() and len(set(org)) == len(org)
    assert len(split_origins(4000, 4000)) == 25


def test_split_rate_other_than_one_is_refused():
    with pytest.raises(NotImplementedError, match="INTER_CUBIC"):
        split_origins(2000, 2000, rate=0.5)


def quantise(v, scale):
    """The device rule: rint(double(v) * scale) / scale (the product of a float32 and 10^2 / 10^4 is exact in float64)."""
    return np.rint(v.astype(np.float64) * scale) / scale


def _values(rng, n, lim):
    v = rng.uniform(-lim, lim, n).astype(np.float32)
    ties = np.array([0.125, 0.375, 0.625, 12.345, -12.345, 0.005, -0.005, 0.015, 2.5, 0.03125, -0.03125, 0.00005, 0.00015,
                     -0.004, -0.0049, -0.00004, 1e-9, -1e-9, 0.0, -0.0, 2e4, -2e4, 19999.995, -19999.995, 1023.995, 0.99995],
                    dtype=np.float32)
    # exact half-ties in float32: k / 200 and k / 20000 that are representable (k odd, denominator a power of two)
    k = rng.integers(-4000, 4000, n // 20)
    half2 = ((2 * k + 1) / 8.0).astype(np.float32)            # x.125 / x.375 / ...: ties at the third decimal
    half4 = ((2 * k + 1) / 32.0 / 16.0).astype(np.float32)     # ties at the fifth decimal
    small = rng.uniform(-0.01, 0.01, n // 20).astype(np.float32)   # many round to -0.00
    v[:len(ties)] = ties
    v[len(ties):len(ties) + len(half2)] = half2
    o = len(ties) + len(half2)
    v[o:o + len(half4)] = half4
    o += len(half4)
    v[o:o + len(small)] = small
    return v


def test_quantisation_rule_equals_python_formatting():
    rng = np.random.default_rng(2026)
    n = 1000000
    coords = _values(rng, n, 2e4)
    got = quantise(coords, 100.0)
    want = np.array([float("%.2f" % x) for x in coords.tolist()])
    assert np.array_equal(got.view(np.int64), want.view(np.int64))          # bit for bit, signed zeros included
    assert np.any(np.signbit(got) & (got == 0))
    scores = np.abs(_values(rng, n, 1.0))
    scores[:4] = np.float32([0.03125, 0.00005, 0.99995, 0.15625])
    got = quantise(scores, 10000.0)
    want = np.array([float("%.4f" % x) for x in scores.tolist()])
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    # shifted into the scene as poly2origpoly does: float(q + left) / 1.0
    left = rng.integers(0, 4000, 1000)
    q = quantise(coords[:1000], 100.0)
    assert np.array_equal(((q + left) / 1.0).view(np.int64),
                          np.array([float(a + int(b)) / float("1") for a, b in zip(q.tolist(), left.tolist())]).view(np.int64))


def test_task1_score_transform_is_float32():
    """score^2 / centerness in float32 (evaluation.task1.task1_scores), as the device computes it without contraction."""
    from types import SimpleNamespace
    from dafne_amd.evaluation.task1 import task1_scores
    rng = np.random.default_rng(3)
    s = rng.uniform(0.05, 1, 10000).astype(np.float32)
    c = rng.uniform(0.05, 1, 10000).astype(np.float32)
    cfg = SimpleNamespace(MODEL=SimpleNamespace(DAFNE=SimpleNamespace(CENTERNESS="oriented", CENTERNESS_USE_IN_SCORE=False)))
    want = task1_scores(s, c, cfg)
    got = np.array([np.float32(np.float32(a * a) / b) for a, b in zip(s, c)], dtype=np.float32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("extra,msg", [(["--num-gpus", "2"], "one GPU"), (["--tta"], "--tta")])
def test_eval_net_scene_dir_refuses_multi_gpu_and_tta(tmp_path, extra, msg):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval_net.py"), "--config-file", os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"),
           "--scene-dir", str(tmp_path)] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode != 0
    assert "--scene-dir" in p.stderr and msg in p.stderr, p.stderr
