"""GPU parity: decode / top-k / corner sort / fused predict_proposals through the
C-ABI vs fixtures produced by the reference's own dafne_outputs.py (bit-exact
keys and order; coordinates and scores within 1e-3 as BASELINE.json states --
observed differences are ~1e-7 from expf/sigmoid rounding)."""
import numpy as np
import pytest
import torch

from oracle import postprocess as opp

pytestmark = pytest.mark.gpu
VARIANTS = ["d10", "d15", "hrsc", "ucas", "d10_topk", "d15_topk"]
NO_STRIDE_NORM = ["d10_nsn", "d15_nsn"]       # ENABLE_FPN_STRIDE_NORM false (make_golden_stride_norm.py)
TOL = 1e-3


def dev():
    return torch.device("cuda", 0)


def _cfg(C, topk, post, twc, sortc, thr, nms_thr):
    from dafne_amd.config import get_cfg
    cfg = get_cfg()
    d = cfg.MODEL.DAFNE
    d.NUM_CLASSES, d.PRE_NMS_TOPK_TEST, d.POST_NMS_TOPK_TEST = C, topk, post
    d.THRESH_WITH_CTR, d.SORT_CORNERS, d.INFERENCE_TH_TEST, d.NMS_TH = bool(twc), bool(sortc), thr, nms_thr
    return cfg


def _key(levels, locs, classes):
    return levels.astype(np.int64) * (1 << 40) + locs[:, 1].astype(np.int64) * (1 << 24) \
        + locs[:, 0].astype(np.int64) * 64 + classes.astype(np.int64)


def test_sort_quadrilateral_golden(golden):
    from dafne_amd.utils.sort_corners import sort_quadrilateral
    g = golden("sort_corners")
    out = sort_quadrilateral(torch.from_numpy(g["boxes"]).to(dev())).cpu().numpy()
    assert np.array_equal(out, g["sorted"])


@pytest.mark.parametrize("name", VARIANTS + NO_STRIDE_NORM)
def test_predict_proposals_golden(golden, name):
    from dafne_amd.modeling.dafne.dafne_outputs import DAFNeOutputs
    nsn = name in NO_STRIDE_NORM
    g = golden("predict_no_stride_norm" if nsn else "predict_proposals")
    C, topk, post, twc, sortc = [int(v) for v in g[name + "_cfg"]]
    thr, nms_thr = [float(v) for v in g[name + "_thr"]]
    cfg = _cfg(C, topk, post, twc, sortc, thr, nms_thr)
    cfg.MODEL.DAFNE.ENABLE_FPN_STRIDE_NORM = not nsn
    outs = DAFNeOutputs(cfg)
    logits = [torch.from_numpy(g["%s_logits%d" % (name, l)]).to(dev()) for l in range(5)]
    regs = [torch.from_numpy(g["%s_reg%d" % (name, l)]).to(dev()) for l in range(5)]
    ctrs = [torch.from_numpy(g["%s_ctr%d" % (name, l)]).to(dev()) for l in range(5)]
    res = outs.predict_proposals(logits, regs, ctrs, None, [(256, 256)] * 2, [])
    for im in range(2):
        ref = {k: g["%s_im%d_%s" % (name, im, k)] for k in
               ("pred_boxes", "pred_corners", "scores", "centerness", "pred_classes", "locations", "fpn_levels")}
        r = res[im]
        assert len(r) == len(ref["scores"])
        got_key = _key(r.fpn_levels.cpu().numpy(), r.locations.cpu().numpy(), r.pred_classes.cpu().numpy())
        assert np.array_equal(got_key, _key(ref["fpn_levels"], ref["locations"], ref["pred_classes"]))
        assert r.pred_classes.dtype == torch.int64
        assert np.allclose(r.scores.cpu().numpy(), ref["scores"], atol=TOL)
        assert np.abs(r.scores.cpu().numpy() - ref["scores"]).max() < 1e-6
        assert np.allclose(r.pred_corners.cpu().numpy(), ref["pred_corners"], atol=TOL)
        assert np.allclose(r.pred_boxes.tensor.cpu().numpy(), ref["pred_boxes"], atol=TOL)
        assert np.allclose(r.centerness.cpu().numpy(), ref["centerness"], atol=1e-6)


def test_decode_candidates_vs_oracle_all_levels():
    """Candidate sets before NMS (incl. the top-k cut and tie handling) vs the numpy oracle."""
    from dafne_amd import postprocess as pp
    rng = np.random.default_rng(21)
    N, C = 3, 15
    sizes = [(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)]
    strides = [8, 16, 32, 64, 128]
    for twc, sortc, topk in ((True, True, 300), (False, False, 300), (True, False, 4096)):
        lv, raw = [], []
        for (h, w), s in zip(sizes, strides):
            lg = rng.normal(-2.0, 2.0, (N, h, w, C)).astype(np.float32)
            lg[0, : h // 2] = np.round(lg[0, : h // 2])        # many exactly equal scores
            dl = rng.normal(0, 1.0, (N, h, w, 8)).astype(np.float32)
            ce = rng.normal(0, 1.0, (N, h, w, 2)).astype(np.float32)
            ct = rng.normal(0, 2.0, (N, h, w, 1)).astype(np.float32)
            ct[0] = np.round(ct[0])
            scale = float(rng.uniform(0.8, 1.2))
            raw.append((lg, dl, ce, ct, scale))
            lv.append(pp.LevelInput(*(torch.from_numpy(a).to(dev()) for a in (lg, dl, ce, ct)), s, scale))
        cand = pp.decode_levels(lv, num_classes=C, pre_nms_thresh=0.05, pre_nms_topk=topk,
                                thresh_with_ctr=twc, sort_corners=sortc)
        torch.cuda.synchronize()
        for im in range(N):
            per = []
            for l, ((lg, dl, ce, ct, scale), s) in enumerate(zip(raw, strides)):
                reg = ((np.tile(ce[im], (1, 1, 4)) + dl[im]).astype(np.float32) * np.float32(scale)).astype(np.float32)
                per.append(opp.decode_level(np.transpose(lg[im], (2, 0, 1)), np.transpose(reg, (2, 0, 1)),
                                            np.transpose(ct[im], (2, 0, 1)), s, thresh=0.05, topk=topk,
                                            thresh_with_ctr=twc, sort_corners=sortc, level=l))
            exp = opp.cat(per)
            n = int(cand.counts[im])
            assert n == exp["scores"].shape[0]
            gk = _key(cand.levels[im, :n].cpu().numpy(), cand.locs[im, :n].cpu().numpy(), cand.classes[im, :n].cpu().numpy())
            ek = _key(exp["fpn_levels"], exp["locations"], exp["pred_classes"])
            gs, es = cand.scores[im, :n].cpu().numpy(), exp["scores"]
            gi, ei = np.arange(n), np.arange(n)
            if not np.array_equal(gk, ek):
                # expf vs numpy exp may move a score by an ulp across a level's cut: the symmetric difference must be a handful
                # of entries whose scores sit at the cut value of their level (a level that was cut reports topk rows)
                diff = np.setxor1d(gk, ek)
                assert len(diff) <= 4, len(diff)
                for k_ in diff:
                    lvl = int(k_ >> 40)
                    of_level = es[exp["fpn_levels"] == lvl]
                    assert of_level.shape[0] == topk, (lvl, of_level.shape[0])
                    cut = float(of_level.min())
                    sc = gs[gk == k_] if k_ in gk else es[ek == k_]
                    assert abs(float(sc[0]) - cut) <= 2e-7 * max(cut, 1e-30) + 1e-12, (int(k_), float(sc[0]), cut)
                _, gi, ei = np.intersect1d(gk, ek, assume_unique=True, return_indices=True)    # the keys both sides share
                assert gi.size >= n - 4 and np.all(np.diff(gi) > 0) and np.all(np.diff(ei) > 0)   # ... in the same order
            assert np.abs(gs[gi] - es[ei]).max() < 1e-6
            assert np.abs(cand.corners[im, :n].cpu().numpy()[gi] - exp["pred_corners"][ei]).max() < TOL
            assert np.abs(cand.hbox[im, :n].cpu().numpy()[gi] - exp["pred_boxes"][ei]).max() < TOL


def test_topk_ranks_below_threshold_scores_without_ctr_threshold():
    """THRESH_WITH_CTR false (hrsc / dota-1.5 / ucas configs): the candidate test is cls > thresh but the ranked score
    is sqrt(cls * ctr), which may lie far below the threshold (dafne_outputs.py:812-829).  With more candidates than
    PRE_NMS_TOPK and the k-th best score BELOW the threshold the cut must still be taken by score (then lowest flat
    index among equal scores), exactly as the oracle's topk."""
    from dafne_amd import postprocess as pp
    rng = np.random.default_rng(77)
    N, C, topk = 2, 3, 200
    sizes = [(24, 32), (12, 16)]
    strides = [8, 16]
    lv, raw = [], []
    for (h, w), s in zip(sizes, strides):
        lg = rng.normal(1.0, 1.0, (N, h, w, C)).astype(np.float32)          # cls > 0.05 almost everywhere
        dl = rng.normal(0, 1.0, (N, h, w, 8)).astype(np.float32)
        ce = rng.normal(0, 1.0, (N, h, w, 2)).astype(np.float32)
        ct = rng.normal(-9.0, 1.5, (N, h, w, 1)).astype(np.float32)         # ctr ~ 1e-4: scores ~ 1e-2 < thresh
        ct[0, : h // 2] = np.round(ct[0, : h // 2])                         # ties below the threshold too
        lg[0, : h // 2] = np.round(lg[0, : h // 2])
        raw.append((lg, dl, ce, ct))
        lv.append(pp.LevelInput(*(torch.from_numpy(a).to(dev()) for a in (lg, dl, ce, ct)), s, 1.0))
    cand = pp.decode_levels(lv, num_classes=C, pre_nms_thresh=0.05, pre_nms_topk=topk, thresh_with_ctr=False,
                            sort_corners=False)
    torch.cuda.synchronize()
    for im in range(N):
        per = []
        for l, ((lg, dl, ce, ct), s) in enumerate(zip(raw, strides)):
            reg = (np.tile(ce[im], (1, 1, 4)) + dl[im]).astype(np.float32)
            per.append(opp.decode_level(np.transpose(lg[im], (2, 0, 1)), np.transpose(reg, (2, 0, 1)),
                                        np.transpose(ct[im], (2, 0, 1)), s, thresh=0.05, topk=topk,
                                        thresh_with_ctr=False, sort_corners=False, level=l))
            assert per[-1]["scores"].shape[0] == topk and np.sort(per[-1]["scores"])[0] < 0.05   # the regime under test
        exp = opp.cat(per)
        n = int(cand.counts[im])
        assert n == exp["scores"].shape[0]
        gk = _key(cand.levels[im, :n].cpu().numpy(), cand.locs[im, :n].cpu().numpy(), cand.classes[im, :n].cpu().numpy())
        ek = _key(exp["fpn_levels"], exp["locations"], exp["pred_classes"])
        gs, es = cand.scores[im, :n].cpu().numpy(), exp["scores"]
        if not np.array_equal(gk, ek):
            # expf vs numpy exp may move a score by an ulp across the cut: the symmetric difference must be a handful of
            # entries whose scores sit at the cut value
            diff = np.setxor1d(gk, ek)
            assert len(diff) <= 4, len(diff)
            cut = np.sort(es)[0]
            for k_ in diff:
                sc = gs[gk == k_] if k_ in gk else es[ek == k_]
                assert abs(float(sc[0]) - cut) <= 2e-7 * max(cut, 1e-30) + 1e-12
            continue
        assert np.abs(gs - es).max() < 1e-6


def test_gather_postprocess_vs_oracle():
    from dafne_amd import postprocess as pp
    rng = np.random.default_rng(22)
    N, C = 2, 4
    lv, strides = [], [8, 16]
    raw = []
    for (h, w), s in zip([(16, 24), (8, 12)], strides):
        arrs = [rng.normal(-1.0, 2.0, (N, h, w, C)), rng.normal(0, 3.0, (N, h, w, 8)),
                rng.normal(0, 3.0, (N, h, w, 2)), rng.normal(0, 2.0, (N, h, w, 1))]
        arrs = [a.astype(np.float32) for a in arrs]
        raw.append(arrs)
        lv.append(pp.LevelInput(*(torch.from_numpy(a).to(dev()) for a in arrs), s, 1.0))
    cand = pp.decode_levels(lv, num_classes=C, pre_nms_thresh=0.05, pre_nms_topk=500, thresh_with_ctr=False,
                            sort_corners=True)
    keep, nk = pp.select(cand, 0.1, 100)
    sizes = [(128, 192, 300, 200, 128, 190), (120, 180, 120, 180, 120, 180)]
    rows, cnt = pp.gather(cand, keep, nk, sizes=sizes)
    torch.cuda.synchronize()
    for im in range(N):
        per = []
        for l, (arrs, s) in enumerate(zip(raw, strides)):
            lg, dl, ce, ct = [a[im] for a in arrs]
            reg = (np.tile(ce, (1, 1, 4)) + dl).astype(np.float32)
            per.append(opp.decode_level(np.transpose(lg, (2, 0, 1)), np.transpose(reg, (2, 0, 1)),
                                        np.transpose(ct, (2, 0, 1)), s, thresh=0.05, topk=500,
                                        thresh_with_ctr=False, sort_corners=True, level=l))
        det = opp.select_over_all_levels(opp.cat(per), 0.1, 100, fast=True)
        sz = sizes[im]
        exp = opp.detector_postprocess(det, (sz[0], sz[1]), (sz[2], sz[3]), (sz[4], sz[5]))
        n = int(cnt[im])
        r = rows[im, :n].cpu().numpy()
        assert n == exp["scores"].shape[0]
        assert np.array_equal(r[:, 10].astype(np.int64), exp["pred_classes"])
        assert np.abs(r[:, 0:8] - exp["pred_corners"]).max() < TOL
        assert np.abs(r[:, 12:16] - exp["pred_boxes"]).max() < TOL
        assert np.abs(r[:, 16:18] - exp["locations"]).max() < TOL
        assert np.abs(r[:, 8] - exp["scores"]).max() < 1e-6
