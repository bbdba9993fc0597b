"""GPU: decode / top-k / gather / corner sort of dafne_amd/csrc/decode.hip at their edges, exact against the numpy oracle.

test_decode_case_equals_oracle runs the case table of tests/_decode_cases.py (quantised inputs: the selection is fully determined
and the box decode exact, so there is no "a few candidates may differ" clause), test_gather_compaction drives gather_kernel
directly over several passes of its 1024-row loop with rows that Boxes.nonempty drops, test_sort_quadrilateral_small_grid walks
every collinear / coincident / min-x-tie arrangement of a 3 x 3 grid."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _decode_cases as D
from oracle import postprocess as opp

pytestmark = pytest.mark.gpu
F32 = np.float32
FLOAT_FIELDS = ("corners", "scores", "ctr", "locs", "hbox")
INT_FIELDS = ("classes", "levels", "counts")


def dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.array(a)).to(dev())      # a copy: the cases' arrays are read-only


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def device_levels(case):
    """The case's arrays on the device in its layout.  fused9 is what modeling/dafne/dafne.py head_levels hands over: delta and
    centerness in one [N,H,W,9] buffer, centerness as a flat view from offset 8; the logits carry padding channels of +30."""
    from dafne_amd import postprocess as pp
    lv = []
    for a, (h, w, s, scale) in zip(D.arrays(case), case.levels):
        ce = None if a["ce"] is None else _t(a["ce"])
        if case.layout == "packed":
            lv.append(pp.LevelInput(_t(a["lg"]), _t(a["dl"]), ce, None if a["ct"] is None else _t(a["ct"]), s, scale))
        else:
            lg = np.full((case.N, h, w, D.LOGITS_PAD), 30, F32)
            lg[..., :case.C] = a["lg"]
            dc = _t(np.concatenate((a["dl"], a["ct"]), -1))
            assert dc.shape[-1] == 9
            lv.append(pp.LevelInput(_t(lg), dc, ce, dc.view(-1)[8:], s, scale, delta_ps=9, center_ps=2, ctrness_ps=9,
                                    logits_ps=D.LOGITS_PAD))
    return lv


def _prefill(cand):
    for k in FLOAT_FIELDS:
        getattr(cand, k).fill_(float("nan"))
    for k in INT_FIELDS:
        getattr(cand, k).fill_(-1)


def _snapshot(cand):
    torch.cuda.synchronize()
    snap = {k: getattr(cand, k).cpu().numpy() for k in FLOAT_FIELDS + INT_FIELDS}
    return snap, {k: (_bits(v) if k in FLOAT_FIELDS else v) for k, v in snap.items()}


def _decode_into(case, lv, cand, ws):
    """dafne_decode_levels_hip into the given outputs and workspace."""
    from dafne_amd import _lib
    L = _lib.load()
    prm = _lib.DecodeParams(case.N, len(lv), case.C, case.topk, float(case.thresh), int(case.twc), int(case.sortc), cand.m_cap,
                            case.flags)
    descs = (_lib.LevelDesc * len(lv))()
    for i, v in enumerate(lv):
        descs[i] = _lib.LevelDesc(v.logits.data_ptr(), v.delta.data_ptr(), _lib.ptr(v.center), _lib.ptr(v.ctrness), v.logits_ps,
                                  v.delta_ps, v.center_ps, v.ctrness_ps, v.H, v.W, v.stride, v.scale)
    nbytes = L.dafne_decode_workspace_bytes(ctypes.byref(prm), descs)
    assert nbytes > 0, L.dafne_last_error()
    if ws is None:
        # what an earlier call may have left behind: every 64-bit word a plausible list entry (score 0.5, element 0) and a
        # nonzero count, so a read of workspace that this call did not write shows as a wrong row
        assert nbytes % 8 == 0
        ws = torch.full((nbytes // 8,), 0x3F00000000000000, dtype=torch.int64, device=dev()).view(torch.uint8)
    assert ws.numel() == nbytes
    _lib.check(L.dafne_decode_levels_hip(
        ctypes.byref(prm), descs, _lib.ptr(cand.corners), _lib.ptr(cand.scores), _lib.ptr(cand.ctr), _lib.ptr(cand.classes),
        _lib.ptr(cand.locs), _lib.ptr(cand.levels), _lib.ptr(cand.hbox), _lib.ptr(cand.counts), _lib.ptr(ws), nbytes,
        _lib.current_stream()), "dafne_decode_levels_hip")
    return ws


@pytest.mark.parametrize("name", D.NAMES)
def test_decode_case_equals_oracle(name):
    """Counts, (level, location, class) keys in order, corners / hbox / locations bit for bit, scores and centerness within 1e-6,
    equal inputs -> equal score bits, rows past the count untouched; the same bits from a second and third call into one
    workspace."""
    from dafne_amd import postprocess as pp
    case = D.CASES[name]
    ref, lv = D.reference(case), device_levels(case)
    cand = pp.Candidates(case.N, len(lv) * case.topk, dev())
    _prefill(cand)
    out = pp.decode_levels(lv, num_classes=case.C, pre_nms_thresh=case.thresh, pre_nms_topk=case.topk, thresh_with_ctr=case.twc,
                           sort_corners=case.sortc, out=cand)
    assert out is cand and pp.decode_flags(lv) == case.flags
    got, got_bits = _snapshot(cand)
    ws = None
    for _ in range(2):          # again, twice into one workspace (filled with junk before its first use) and the same outputs
        ws = _decode_into(case, lv, cand, ws)
        again = _snapshot(cand)[1]
        for k in got_bits:
            assert np.array_equal(again[k], got_bits[k]), k

    worst, codes, score_bits = 0.0, [], []
    for im in range(case.N):
        per, exp = ref[im]
        n = int(got["counts"][im])
        assert n == exp["scores"].shape[0], (im, n, exp["scores"].shape[0])
        assert np.array_equal(got["levels"][im, :n], exp["fpn_levels"]), im
        assert np.array_equal(_bits(got["locs"][im, :n]), _bits(exp["locations"])), im
        assert np.array_equal(got["classes"][im, :n], exp["pred_classes"]), im
        assert np.array_equal(_bits(got["corners"][im, :n]), _bits(exp["pred_corners"])), im
        assert np.array_equal(_bits(got["hbox"][im, :n]), _bits(exp["pred_boxes"])), im
        if n:
            worst = max(worst, float(np.abs(got["scores"][im, :n] - exp["scores"]).max()))
            assert np.abs(got["scores"][im, :n] - exp["scores"]).max() < 1e-6
            assert np.abs(got["ctr"][im, :n] - exp["centerness"]).max() < 1e-6
        for k in FLOAT_FIELDS:  # rows at and past the count keep the pre-fill
            assert np.all(np.isnan(got[k][im, n:])), (im, k)
        assert np.all(got["classes"][im, n:] == -1) and np.all(got["levels"][im, n:] == -1)
        for l, p in enumerate(per):
            a = D.arrays(case)[l]
            flat = D.flat_index(case, l, p)
            code = a["lg"][im].reshape(-1)[flat].astype(np.int64) * 1000
            if a["ct"] is not None:
                code = code + a["ct"][im].reshape(-1)[flat // case.C].astype(np.int64)
            codes.append(code)
        score_bits.append(got_bits["scores"][im, :n].astype(np.int64))
    codes, score_bits = np.concatenate(codes), np.concatenate(score_bits)
    if codes.size:              # equal inputs -> the same score bits, wherever they sit
        assert np.unique(np.stack((codes, score_bits), 1), axis=0).shape[0] == np.unique(codes).size
    print("decode case %s: largest |score - oracle| = %.3g" % (name, worst))


# --------------------------------------------------------------------------------------------------------------------- gather
GN, GM, GUARD = 3, 3000, 8
G_SIZES = np.array([(128, 192, 256, 384, 128, 190),      # net_h, net_w, out_h, out_w, orig_h, orig_w: scale exactly 2
                    (64, 64, 64, 64, 64, 64),
                    (120, 180, 300, 200, 121, 177)], F32)  # ratios that round


def _gather_inputs():
    """Rows in keep order ("positions") with planned empty boxes, scattered to their source rows through a permutation.
    Of every six 64-row waves of a pass one drops everything, two keep everything, one alternates, two drop a random third."""
    rng = np.random.default_rng(31)
    pos, keep = [], np.empty((GN, GM), np.int64)
    for im in range(GN):
        net_h, net_w = float(G_SIZES[im, 0]), float(G_SIZES[im, 1])
        r = np.arange(GM)
        wave = (r // 64) % 6
        empty = (wave == 0) | ((wave == 3) & (r % 2 == 1)) | ((wave >= 4) & (rng.random(GM) < 1 / 3))
        x1 = rng.uniform(-10, net_w - 20, GM)                                    # kept rows: clipped on either side, never empty
        y1 = rng.uniform(-10, net_h - 20, GM)
        hb = np.stack((x1, y1, x1 + rng.uniform(10.5, 60, GM), y1 + rng.uniform(10.5, 60, GM)), 1)
        kind = r % 5
        u = rng.uniform(0, 20, GM)
        for k, (a, b) in enumerate(((-50 - u, -5 - u),                          # wholly left of the image
                                    (net_w * 1.2 + u, net_w * 1.2 + u + 10),    # wholly beyond out_w
                                    (-30 - u, np.zeros(GM)),                    # zero width after the clip
                                    (np.full(GM, net_w), np.full(GM, net_w)))):  # x1 = x2 = out_w after the scale
            m = empty & (kind == k)
            hb[m, 0], hb[m, 2] = a[m], b[m]
        m = empty & (kind == 4)                                                  # wholly above the image
        hb[m, 1], hb[m, 3] = (-40 - u)[m], (-1 - u)[m]
        pos.append(dict(pred_boxes=hb.astype(F32), pred_corners=rng.uniform(-50, 400, (GM, 8)).astype(F32),
                        scores=rng.uniform(0.05, 1, GM).astype(F32), centerness=rng.uniform(0, 1, GM).astype(F32),
                        pred_classes=rng.integers(0, 15, GM), locations=rng.uniform(0, 400, (GM, 2)).astype(F32),
                        fpn_levels=rng.integers(0, 5, GM), planned_empty=empty))
        keep[im] = rng.permutation(GM)
    return pos, keep


def _rows(det):
    return np.concatenate((det["pred_corners"], det["scores"][:, None], det["centerness"][:, None],
                           det["pred_classes"][:, None].astype(F32), det["fpn_levels"][:, None].astype(F32), det["pred_boxes"],
                           det["locations"]), 1).astype(F32)


def _gather_expected(pos, num_keep, mode):
    out = []
    for im in range(GN):
        det = opp.index(pos[im], np.arange(min(max(int(num_keep[im]), 0), GM)))
        if mode:
            sz = [int(v) for v in G_SIZES[im]]
            n_planned = int((~det["planned_empty"]).sum())
            det = opp.detector_postprocess(det, (sz[0], sz[1]), (sz[2], sz[3]), (sz[4], sz[5]) if mode == 2 else (sz[2], sz[3]))
            assert det["scores"].shape[0] == n_planned and not det["planned_empty"].any()     # the plan of _gather_inputs holds
        out.append(_rows(det))
    return out


def test_gather_compaction():
    """gather_kernel alone: several passes of the 1024-row loop (3, 0 and 2, the last one partial), ordered compaction across the 16
    waves of a pass and across passes, rows dropped by Boxes.nonempty, do_postprocess 2 / 1 / 0, k_cap below the survivors,
    num_keep above m_cap and negative.  Each output field is one fp32 multiply or min / max on the oracle's operands: bit for bit."""
    from dafne_amd import _lib
    from dafne_amd import postprocess as pp
    L = _lib.load()
    pos, keep = _gather_inputs()
    cand = pp.Candidates(GN, GM, dev())
    for field, key in (("corners", "pred_corners"), ("scores", "scores"), ("ctr", "centerness"), ("classes", "pred_classes"),
                       ("locs", "locations"), ("levels", "fpn_levels"), ("hbox", "pred_boxes")):
        src = np.empty((GN,) + pos[0][key].shape, pos[0][key].dtype)
        for im in range(GN):
            src[im, keep[im]] = pos[im][key]
        getattr(cand, field).copy_(torch.from_numpy(src).to(getattr(cand, field).dtype))
    keep_d, sizes_d = _t(keep), _t(G_SIZES)

    def run(mode, k_cap, num_keep):
        buf = torch.full(((GN * k_cap + 2 * GUARD) * _lib.DET_ROW,), float("nan"), dtype=torch.float32, device=dev())
        cnt = torch.full((GN,), -7, dtype=torch.int32, device=dev())
        nk = torch.tensor(num_keep, dtype=torch.int32, device=dev())
        _lib.check(L.dafne_gather_detections_hip(
            _lib.ptr(cand.corners), _lib.ptr(cand.scores), _lib.ptr(cand.ctr), _lib.ptr(cand.classes), _lib.ptr(cand.locs),
            _lib.ptr(cand.levels), _lib.ptr(cand.hbox), _lib.ptr(keep_d), _lib.ptr(nk), _lib.ptr(sizes_d) if mode else None, mode,
            GN, GM, k_cap, ctypes.c_void_p(buf.data_ptr() + GUARD * _lib.DET_ROW * 4), _lib.ptr(cnt), _lib.current_stream()),
            "dafne_gather_detections_hip")
        torch.cuda.synchronize()
        rows = buf.cpu().numpy().reshape(-1, _lib.DET_ROW)
        assert np.all(np.isnan(rows[:GUARD])) and np.all(np.isnan(rows[-GUARD:])), "guard rows written"
        return rows[GUARD:-GUARD].reshape(GN, k_cap, _lib.DET_ROW), cnt.cpu().numpy()

    def check(mode, k_cap, num_keep):
        exp = _gather_expected(pos, num_keep, mode)
        rows, cnt = run(mode, k_cap, num_keep)
        for im in range(GN):
            k = exp[im].shape[0]
            assert int(cnt[im]) == k, (mode, k_cap, im, int(cnt[im]), k)       # all survivors, also past k_cap
            w = min(k, k_cap)
            for name, sl in (("corners", slice(0, 8)), ("score, centerness, class, level", slice(8, 12)), ("hbox", slice(12, 16)),
                             ("locations", slice(16, 18))):
                assert np.array_equal(_bits(rows[im, :w, sl]), _bits(exp[im][:w, sl])), (mode, k_cap, im, name)
            assert np.all(np.isnan(rows[im, w:])), (mode, k_cap, im)
        return exp

    num_keep = (2500, 0, 1030)
    exp = check(2, GM, num_keep)
    dropped = [1 - exp[im].shape[0] / num_keep[im] for im in (0, 2)]
    assert all(0.25 < d < 0.45 for d in dropped), dropped                     # about a third of the rows are empty boxes
    check(1, GM, num_keep)
    assert [e.shape[0] for e in check(0, GM, num_keep)] == list(num_keep)     # nothing is dropped without the post-process
    assert min(exp[0].shape[0], exp[2].shape[0]) > 600                        # k_cap below the survivors of both images
    for mode in (2, 1, 0):
        check(mode, 600, num_keep)
    check(2, GM, (GM + 500, -5, GM))                                          # clamped to m_cap; negative: count 0


# ---------------------------------------------------------------------------------------------------------------- corner sort
def test_sort_quadrilateral_small_grid():
    """Every quad with coordinates in {0, 1, 2} (all collinear, coincident and min-x-tie arrangements, where the reference leaves
    zeros) and 4096 random fp32 quads, bit for bit."""
    from dafne_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(32)
    grid = np.array(list(itertools.product((0, 1, 2), repeat=8)), F32)
    rand = (rng.normal(0, 1, (4096, 8)) * np.exp(rng.uniform(-3, 6, (4096, 1)))).astype(F32)
    quads = np.concatenate((grid, rand))
    exp = opp.sort_quadrilateral(quads)
    assert grid.shape[0] == 3 ** 8 and int(np.all(exp[:, 2:] == 0, axis=1).sum()) > 1000     # the degenerate branch is there
    n = quads.shape[0]
    src = _t(quads)
    out = torch.full((n + 1, 8), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(L.dafne_sort_quadrilateral_hip(_lib.ptr(src), _lib.ptr(out), n, _lib.current_stream()),
               "dafne_sort_quadrilateral_hip")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[n]))
    bad = np.nonzero(np.any(_bits(got[:n]) != _bits(exp), axis=1))[0]
    assert bad.size == 0, (bad[:5], quads[bad[:1]], got[bad[:1]], exp[bad[:1]])
