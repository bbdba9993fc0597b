"""tests/_decode_cases.py does what it claims (no device): on the oracle alone, every case keeps its distinct scores far enough apart
for an exact comparison, reaches the regime its `why` names, and decodes to exactly representable coordinates.  Plus the refusals of
dafne_decode_workspace_bytes."""
import ctypes

import numpy as np
import pytest

import _decode_cases as D

F32 = np.float32
# distinct scores at least this far apart (relative): about 30 times below the 2.9e-4 the [-8, 8] grid gives, about 40 times above
# a few-ulp difference between the device's expf and numpy's exp
MIN_GAP = 1e-5


def _pair_code(case, im, l):
    """[HW,C] code of the unordered (class logit, centerness logit) pair behind each score (the product commutes)."""
    a = D.arrays(case)[l]
    lg = a["lg"][im].reshape(-1, case.C).astype(np.int64) + 100
    if case.flags & D.NO_CTRNESS:
        return lg
    ct = np.broadcast_to(a["ct"][im].reshape(-1, 1).astype(np.int64) + 100, lg.shape)
    return np.minimum(lg, ct) * 1000 + np.maximum(lg, ct)


@pytest.mark.parametrize("name", D.NAMES)
def test_case_reaches_its_regime(name):
    case = D.CASES[name]
    src = D.CASES[case.same_as or name]
    assert (case.levels, case.C, case.topk, case.thresh, case.twc, case.sortc, case.flags) == \
        (src.levels, src.C, src.topk, src.thresh, src.twc, src.sortc, src.flags)
    assert case.N <= 3 and 1 <= case.topk <= D.K_MAX_TOPK and 1 <= len(case.levels) <= D.K_MAX_LEVELS and case.why
    claims, ref, thr = src.claims, D.reference(case), F32(case.thresh)
    zero_quads = zero_tails = 0
    for im in range(case.N):
        per, tot = ref[im]
        assert tot["scores"].shape[0] == sum(p["scores"].shape[0] for p in per)
        for l, (h, w, s, scale) in enumerate(case.levels):
            a = D.arrays(case)[l]
            for k, v in a.items():      # the grid: integers in [-8, 8]; 30 only where a case saturates on purpose
                assert v is None or (np.all(v == np.rint(v)) and np.all((np.abs(v) <= 8) | ((v == 30) & (k in ("lg", "ct"))))), k
            tv, sc = D.thresholded_and_score(case, im, l)
            cand = tv > thr
            n = int(cand.sum())
            # nothing within rounding distance of the threshold but the values that equal it
            near = np.abs(tv.astype(np.float64) - float(thr)) <= MIN_GAP * abs(float(thr))
            assert np.all(tv[near] == thr)
            # distinct scores lie apart, and each belongs to one input pair (equal inputs <=> equal scores)
            if n:
                u = np.unique(sc[cand])
                assert u[0] > 0
                if u.size > 1:
                    assert (np.diff(u.astype(np.float64)) / u[:-1]).min() >= MIN_GAP, (im, l)
                code = _pair_code(case, im, l)[cand]
                both = np.unique(np.stack((sc[cand].view(np.int32).astype(np.int64), code), 1), axis=0)
                assert both.shape[0] == u.size == np.unique(code).size, (im, l)
            got = per[l]
            assert got["scores"].shape[0] == min(n, case.topk)
            flat = D.flat_index(case, l, got)
            assert np.all(np.diff(flat) > 0) and np.array_equal(got["scores"], sc.reshape(-1)[flat])
            rel = claims.get("count", {}).get((im, l))
            if rel is not None:
                assert {">": n > case.topk, "<": 0 < n < case.topk, "==": n == case.topk, "+1": n == case.topk + 1,
                        "0": n == 0}[rel], (im, l, rel, n)
            if (im, l) in claims.get("cut_tie", ()):
                assert n > case.topk
                cut = got["scores"].min()
                taken, held = int((got["scores"] == cut).sum()), int((sc[cand] == cut).sum())
                assert 1 <= taken < held, (im, l, taken, held)
            if (im, l) in claims.get("lowest", ()):
                assert np.array_equal(flat, np.arange(case.topk))
            if (im, l) in claims.get("at_thresh", ()):
                at = np.nonzero((tv == thr).reshape(-1))[0]
                assert at.size > 0 and not np.isin(at, flat).any()
            for (i2, l2, f) in claims.get("taken", ()):
                if (i2, l2) == (im, l):
                    assert f in flat
            # every decoded coordinate is an integer or a half-integer below 2^24: the fp32 decode is exact
            for k in ("pred_corners", "pred_boxes", "locations"):
                v = got[k].astype(np.float64)
                assert np.all(2 * v == np.rint(2 * v)) and np.all(np.abs(v) < 2 ** 24), k
            if case.sortc:
                zero_quads += int(np.all(got["pred_corners"] == 0, axis=1).sum())
                zero_tails += int(np.all(got["pred_corners"][:, 2:] == 0, axis=1).sum())
    if claims.get("zero_quad"):
        assert zero_quads > 0 and zero_tails > zero_quads, (zero_quads, zero_tails)


def _counts(case, im):
    return [int((D.thresholded_and_score(case, im, l)[0] > F32(case.thresh)).sum()) for l in range(len(case.levels))]


def test_shapes_against_the_kernel_constants():
    n_elem = {name: [h * w * c.C for h, w, _, _ in c.levels] for name, c in D.CASES.items()}
    for name in ("cut-ragged-twc", "cut-ragged-notwc", "fused9"):
        assert all(n > D.K_CHUNK and n % D.K_CHUNK for n in n_elem[name][:2]) and n_elem[name][2] <= D.K_BINS
        assert D.CASES[name].topk & (D.CASES[name].topk - 1)                 # no power of two: kp has padding entries
    assert n_elem["chunk-exact"] == [D.K_CHUNK] and n_elem["all-tied-4096"] == [D.K_CHUNK]
    assert n_elem["chunk-plus-one"] == [D.K_CHUNK + 1] and D.CASES["chunk-plus-one"].C == 1
    assert max(n_elem["one-index-step"]) == D.K_BINS                         # 11 index bits: one radix step
    assert n_elem["all-tied"][0] > 1 << 11                                   # more than 11 index bits: two steps
    assert D.CASES["topk-one"].topk == 1 and D.CASES["topk-max"].topk == D.K_MAX_TOPK
    assert len(D.CASES["eight-levels"].levels) == D.K_MAX_LEVELS
    assert D.CASES["one-class"].C == 1 and D.CASES["chunk-exact"].C == 16
    assert D.CASES["thresh-zero-twc"].thresh == 0.0 and D.CASES["thresh-negative-twc"].thresh < 0 and D.CASES["thresh-zero-twc"].twc
    for name in ("exactly-topk", "topk-plus-one"):                           # the placed elements reach every chunk
        case = D.CASES[name]
        for im in range(case.N):
            tv, _ = D.thresholded_and_score(case, im, 0)
            chunks = np.unique(np.nonzero((tv > F32(case.thresh)).reshape(-1))[0] // D.K_CHUNK)
            assert chunks.size == (n_elem[name][0] + D.K_CHUNK - 1) // D.K_CHUNK > 1
    case = D.CASES["saturated"]
    for im, more in ((0, True), (1, False)):
        _, sc = D.thresholded_and_score(case, im, 0)
        assert sc.max() == 1.0 and (int((sc == 1.0).sum()) > case.topk) == more
        assert np.all(D.reference(case)[im][0][0]["scores"][: 5] <= 1.0)
    assert D.reference(case)[0][1]["scores"].min() == 1.0                     # image 0: the whole selection is saturated
    case = D.CASES["empty-level-first"]
    assert _counts(case, 1) == [0, 0, 0] and D.reference(case)[1][1]["scores"].shape[0] == 0
    assert _counts(case, 0)[0] == 0 and D.reference(case)[0][1]["fpn_levels"][0] == 1
    assert {c.layout for c in D.CASES.values()} == {"packed", "fused9"}
    assert D.CASES["fused9-no-center"].flags == D.NO_CENTER and D.arrays(D.CASES["fused9-no-center"])[0]["ce"] is None


def test_decode_refuses_what_it_cannot_do():
    """dafne_decode_workspace_bytes returns 0 and dafne_last_error names the reason."""
    from dafne_amd import _lib
    L = _lib.load()

    def ask(n_levels=2, C=15, topk=100, m_cap=None, flags=0, H=5, n_images=2):
        prm = _lib.DecodeParams(n_images, n_levels, C, topk, 0.05, 1, 1, n_levels * topk if m_cap is None else m_cap, flags)
        descs = (_lib.LevelDesc * max(n_levels, 1))()
        for i in range(len(descs)):
            descs[i] = _lib.LevelDesc(None, None, None, None, C, 8, 2, 1, H, 7, 8, 1.0)
        return L.dafne_decode_workspace_bytes(ctypes.byref(prm), descs)

    assert ask() > 0 and ask(topk=D.K_MAX_TOPK) > 0 and ask(n_levels=D.K_MAX_LEVELS) > 0 and ask(topk=1, n_levels=1, C=1) > 0
    assert ask(flags=_lib.DECODE_NO_CENTER | _lib.DECODE_NO_CTRNESS) > 0
    assert (_lib.DECODE_NO_CENTER, _lib.DECODE_NO_CTRNESS) == (D.NO_CENTER, D.NO_CTRNESS)
    for kw, msg in ((dict(topk=0), b"pre_nms_topk 0"), (dict(topk=D.K_MAX_TOPK + 1), b"pre_nms_topk 4097"),
                    (dict(n_levels=0), b"n_levels 0"), (dict(n_levels=D.K_MAX_LEVELS + 1), b"n_levels 9"),
                    (dict(C=0), b"bad sizes"), (dict(m_cap=199), b"m_cap too small"), (dict(flags=4), b"unknown flags 0x4"),
                    (dict(H=0), b"level 0 size")):
        assert ask(**kw) == 0, kw
        assert msg in L.dafne_last_error(), (kw, L.dafne_last_error())
