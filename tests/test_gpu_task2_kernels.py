"""GPU: the three DOTA Task2 kernels of csrc/poly_nms.hip against the reference's results (tests/golden/task2_merge.npz) and the
numpy restatement (tests/_task2_np.py).  Every comparison is exact.

  * dafne_hbb_nms_f64_batched_hip: keep lists equal py_cpu_nms' on buckets of 0, 1, 2, 63, 64, 65, 130 and 1300 rows, a dense
    cluster with suppression chains, boxes that touch within the +1 and a reversed box, at 0.1 and 0.3 -- all buckets in one
    launch with m_cap above every count, and each alone with m_cap = its count; equal 4-decimal scores and a NaN overlap
    against the restatement; two runs bit-equal;
  * dafne_scene_merge_hbb_rows_hip equals the restatement bit for bit (skip mask, score mode 1, the counts-only call), and
    its buckets are the Task1 merge's;
  * dafne_scene_match_hbb_hip equals the restatement bit for bit on buckets of 0, 1, 65 and 500 boxes."""
import numpy as np
import pytest
import torch

import _task2_np as t2

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def up(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev())


# ----------------------------------------------------------------------------------------------------------------- NMS
def run_hbb_nms(arrays, thresh, m_cap, with_counts=True):
    """One launch over all arrays (rows past a bucket's count hold a box that would suppress everything)."""
    from dafne_amd import _lib
    L = _lib.load()
    n = len(arrays)
    host = np.zeros((n, m_cap, 5), np.float64)
    host[:, :, :] = [-1e6, -1e6, 1e6, 1e6, 2.0]
    counts = np.array([len(a) for a in arrays], np.int32)
    for k, a in enumerate(arrays):
        host[k, :len(a)] = a
    d, c = up(host, np.float64), up(counts, np.int32)
    keep = torch.full((n, m_cap), -7, dtype=torch.int64, device=dev())
    nk = torch.full((n,), -7, dtype=torch.int32, device=dev())
    nbytes = L.dafne_hbb_nms_f64_workspace_bytes(n, m_cap)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev())          # the library zeroes what it needs zeroed
    _lib.check(L.dafne_hbb_nms_f64_batched_hip(_lib.ptr(d), _lib.ptr(c) if with_counts else None, n, m_cap, float(thresh),
                                               _lib.ptr(keep), _lib.ptr(nk), _lib.ptr(ws), nbytes, _lib.current_stream()),
               "dafne_hbb_nms_f64_batched_hip")
    kh, nh = keep.cpu().numpy(), nk.cpu().numpy()
    return [kh[k, :nh[k]].tolist() for k in range(n)], kh, nh


@pytest.mark.parametrize("thresh", [0.1, 0.3])
def test_hbb_nms_equals_the_reference(golden, thresh):
    from dafne_amd.evaluation.result_merge import py_cpu_nms
    g = golden("task2_merge")
    cases = [str(c) for c in g["nms_cases"]]
    arrays = [g["nms_in_" + c] for c in cases]
    want = [g["nms_keep_%s_%d" % (c, round(thresh * 100))].tolist() for c in cases]
    assert sorted(len(a) for a in arrays)[:7] == [0, 1, 2, 13, 63, 64, 65] and max(len(a) for a in arrays) == 1300
    got, kh, nh = run_hbb_nms(arrays, thresh, m_cap=1307)                  # unequal counts, m_cap above every one
    for c, a, w, k in zip(cases, arrays, want, got):
        assert k == w, c
        assert k == t2.np_hbb_nms(a, thresh), c
    again, kh2, nh2 = run_hbb_nms(arrays, thresh, m_cap=1307)
    assert np.array_equal(nh, nh2) and all(a == b for a, b in zip(got, again))          # two runs: the same lists
    for c, a, w in zip(cases, arrays, want):                               # alone, m_cap = the count (no padding rows at all)
        assert py_cpu_nms(a, thresh) == w, c
    # d_counts NULL: every bucket holds m_cap rows
    a130 = g["nms_in_n130"]
    got, _, _ = run_hbb_nms([a130, a130[::-1].copy()], thresh, m_cap=130, with_counts=False)
    w130 = g["nms_keep_n130_%d" % round(thresh * 100)].tolist()
    assert got[0] == w130 and got[1] == [129 - i for i in w130]


def test_hbb_nms_equal_scores_and_nan_overlap_equal_the_restatement():
    rng = np.random.default_rng(3)
    arrays = []
    for n, ext, levels in ((200, 300.0, 40), (1300, 900.0, 40), (65, 120.0, 8)):
        c = rng.uniform(0, ext, (n, 2))
        wh = np.exp(rng.uniform(np.log(8.0), np.log(90.0), (n, 2)))
        sc = rng.integers(500, 500 + levels, n) / 10000.0               # four-decimal scores: every value is shared by many rows
        arrays.append(np.concatenate([np.round(np.concatenate([c - wh / 2, c + wh / 2], 1), 2), sc[:, None]], 1))
        assert np.unique(sc).size * 4 < n                               # levels * 4 < n: at least 4 rows per score on average
    arrays.append(np.array([[5.0, 5.0, 25.0, 25.0, 0.3]] * 7))          # identical rows: the last one stays
    # area_i + area_j - inter == 0 with inter == 0: ovr is 0 / 0, and a NaN suppresses
    arrays.append(np.array([[0.0, 0.0, 30.0, 30.0, 0.9], [1032.0, 0.0, 1000.0, 30.0, 0.8], [2000.0, 0.0, 2030.0, 30.0, 0.7]]))
    got, _, _ = run_hbb_nms(arrays, 0.1, m_cap=1300)
    for k, a in enumerate(arrays):
        assert got[k] == t2.np_hbb_nms(a, 0.1), k
    assert got[3] == [6] and got[4] == [0, 2]


# ---------------------------------------------------------------------------------------------------------- merge rows
@pytest.mark.parametrize("skip,score_mode", [(0, 0), ((1 << 2) | (1 << 5), 1)])
def test_merge_hbb_rows_equal_the_numpy_restatement(skip, score_mode):
    from dafne_amd import _lib
    from dafne_amd.scene import merge_tile_rows
    rng = np.random.default_rng(5 + score_mode)
    T, k_cap, C, S = 7, 300, 8, 4
    rows = np.zeros((T, k_cap, 18), np.float32)
    rows[:, :, 0:8] = rng.uniform(-50, 1100, (T, k_cap, 8))
    rows[:, ::7, 0:8] = (rng.integers(-400, 8800, (T, (k_cap + 6) // 7, 8)) * 2 + 1) / 8.0     # exact half-ties of "%.2f"
    rows[:, ::11, 0] = -0.001                                                                       # rounds to -0.00
    rows[:, ::13, 2] = rows[:, ::13, 0]                                                             # two corners share the minimum
    rows[:, :, 8] = rng.uniform(0.05, 1, (T, k_cap))
    rows[:, ::5, 8] = np.float32(0.03125)                                                           # a tie of "%.4f"
    rows[:, :, 9] = rng.uniform(0.05, 1, (T, k_cap))
    rows[:, :, 10] = rng.integers(0, C, (T, k_cap))
    rows[:, :, 10] = np.where(rows[:, :, 10] == 6, 7, rows[:, :, 10])                                # class 6: an empty bucket
    counts = np.array([k_cap, k_cap, k_cap, 0, 17, 299, 64], np.int32)
    rows[4, 17:] = 7.0                                                                                # past the count: ignored
    # scenes 0 (tiles 0-2), 1 (3-4), 3 (5-6); scene 2 has no tile: all its buckets are empty
    info = np.array([(0, 0, 0), (824, 0, 0), (824, 76, 0), (0, 0, 1), (76, 824, 1), (5, 9, 3), (2976, 0, 3)], np.int32)
    drows, dcounts = up(rows, np.float32), up(counts, np.int32)
    dets, bc, src, m_cap = merge_tile_rows(drows, dcounts, info, S, C, skip, score_mode, hbb=True)
    want, wsrc = t2.merge_hbb_rows_numpy(rows, counts, info, S, C, skip, score_mode)
    assert tuple(dets.shape) == (S * C, m_cap, 5) and m_cap == max(len(b) for b in want) > 64
    assert sum(len(b) == 0 for b in want) >= C + 1
    bch, dh, sh = bc.cpu().numpy(), dets.cpu().numpy(), src.cpu().numpy()
    for b in range(S * C):
        assert bch[b] == len(want[b]), b
        if want[b]:
            assert np.array_equal(dh[b, :bch[b]].view(np.int64), np.array(want[b]).view(np.int64)), b
            assert np.array_equal(sh[b, :bch[b]], np.array(wsrc[b])), b
    # the same buckets as the Task1 merge: counts, back-index, scores; the box is the hull of the Task1 row
    d9, bc9, src9, m9 = merge_tile_rows(drows, dcounts, info, S, C, skip, score_mode)
    assert m9 == m_cap and torch.equal(bc9, bc)
    valid = (torch.arange(m_cap, device=dev())[None, :] < bc[:, None]).cpu().numpy()
    d9 = d9.cpu().numpy()
    assert np.array_equal(src9.cpu().numpy()[valid], sh[valid]) and np.array_equal(d9[valid][:, 8], dh[valid][:, 4])
    assert np.array_equal(t2.rec4(d9[valid][:, :8]), dh[valid][:, :4])
    # the counts-only call (m_cap = 0, no output rows)
    L = _lib.load()
    nbytes = L.dafne_scene_merge_workspace_bytes(T, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    only = torch.full((S * C,), -7, dtype=torch.int32, device=dev())
    _lib.check(L.dafne_scene_merge_hbb_rows_hip(_lib.ptr(drows), _lib.ptr(dcounts), T, k_cap, _lib.ptr(up(info, np.int32)), S, C,
                                                int(skip), int(score_mode), 0, None, _lib.ptr(only), None, _lib.ptr(ws), nbytes,
                                                _lib.current_stream()), "dafne_scene_merge_hbb_rows_hip")
    assert torch.equal(only, bc)
    # a smaller m_cap truncates every bucket and writes nothing past it
    small = torch.full((S * C, 10, 5), -7.0, dtype=torch.float64, device=dev())
    ssrc = torch.full((S * C, 10), -7, dtype=torch.int32, device=dev())
    _lib.check(L.dafne_scene_merge_hbb_rows_hip(_lib.ptr(drows), _lib.ptr(dcounts), T, k_cap, _lib.ptr(up(info, np.int32)), S, C,
                                                int(skip), int(score_mode), 10, _lib.ptr(small), _lib.ptr(only), _lib.ptr(ssrc),
                                                _lib.ptr(ws), nbytes, _lib.current_stream()), "dafne_scene_merge_hbb_rows_hip")
    small = small.cpu().numpy()
    for b in range(S * C):
        k = min(10, len(want[b]))
        assert np.array_equal(small[b, :k], dh[b, :k]) and (small[b, k:] == -7.0).all(), b


# --------------------------------------------------------------------------------------------------------------- match
def run_match_hbb(dets, bucket, gt, offs):
    from dafne_amd import _lib
    L = _lib.load()
    n, g = dets.shape[0], gt.shape[0]
    d, b, t, o = up(dets, np.float64), up(bucket, np.int32), up(gt, np.float64), up(offs, np.int32)
    ovmax = torch.full((n,), 7.0, dtype=torch.float64, device=dev())
    jmax = torch.full((n,), 7, dtype=torch.int32, device=dev())
    _lib.check(L.dafne_scene_match_hbb_hip(_lib.ptr(d), _lib.ptr(b), n, _lib.ptr(t), _lib.ptr(o), offs.shape[0] - 1, g,
                                           _lib.ptr(ovmax), _lib.ptr(jmax), _lib.current_stream()), "dafne_scene_match_hbb_hip")
    return ovmax.cpu().numpy(), jmax.cpu().numpy()


def rects(n, rng, ext, lo=8.0, hi=90.0):
    c = rng.uniform(0, ext, (n, 2))
    wh = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))
    return np.round(np.concatenate([c - wh / 2, c + wh / 2], 1), 2)


def test_match_hbb_equals_the_numpy_restatement():
    rng = np.random.default_rng(5)
    base = rects(10, rng, 300.0)
    gts = [np.zeros((0, 4)),                                   # 0 empty
           rects(1, rng, 100.0),                               # 1 one box
           rects(65, rng, 300.0),                              # 2 one box past a wave
           rects(500, rng, 900.0),                             # 3 several strides
           np.concatenate([base, base, base]),                 # 4 identical boxes: the lowest index wins
           np.zeros((0, 4))]                                   # 5 empty
    dets, bucket = [], []
    for b, g in enumerate(gts):
        if len(g) == 0:
            d = rects(5, rng, 300.0)
        else:
            k = min(len(g), 40)
            pick = rng.choice(len(g), k, replace=False)
            pick[0] = len(g) - 1                               # an exact copy of the bucket's last box is among them
            d = np.concatenate([g[pick] + np.round(rng.normal(0, 1.5, (k, 4)), 2), g[pick[:max(k // 4, 1)]], rects(6, rng, 300.0),
                                np.array([[5000.0, 5000.0, 5040.0, 5030.0]])])      # disjoint from every box: ovmax 0, jmax 0
        dets.append(d)
        bucket += [b] * len(d)
    dets.append(rects(8, rng, 300.0))                          # buckets that do not exist
    bucket += [-1] * 4 + [len(gts)] * 4
    dets, bucket = np.concatenate(dets), np.array(bucket, np.int32)
    perm = rng.permutation(len(bucket))
    dets, bucket = dets[perm], bucket[perm]
    gt = np.concatenate(gts)
    offs = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
    exp_ov, exp_j = t2.np_match_hbb(dets, bucket, gt, offs)
    ovmax, jmax = run_match_hbb(dets, bucket, gt, offs)
    assert ovmax.tobytes() == exp_ov.tobytes()
    assert np.array_equal(jmax, exp_j)
    # the cases are there
    none = (bucket == 0) | (bucket == 5) | (bucket < 0) | (bucket >= len(gts))
    assert np.isneginf(ovmax[none]).all() and (jmax[none] == -1).all()
    far = dets[:, 0] == 5000.0
    assert far.sum() == 4 and (ovmax[far] == 0.0).all() and (jmax[far] == 0).all()
    assert (jmax[bucket == 2] == 64).any() and (jmax[bucket == 3] == 499).any() and (ovmax[bucket == 1] == 1.0).any()
    b4 = bucket == 4
    assert (ovmax[b4] == 1.0).any() and (jmax[b4][ovmax[b4] > 0.5] < 10).all()
    ov2, j2 = run_match_hbb(dets, bucket, gt, offs)
    assert ov2.tobytes() == ovmax.tobytes() and np.array_equal(j2, jmax)
    # G = 0 and N = 0
    ov, j = run_match_hbb(dets[:5], np.array([0, 1, 2, 0, 1], np.int32), np.zeros((0, 4)), np.zeros(4, np.int32))
    assert np.isneginf(ov).all() and (j == -1).all()
    ov, j = run_match_hbb(np.zeros((0, 4)), np.zeros(0, np.int32), gt, offs)
    assert ov.shape == (0,) and j.shape == (0,)
