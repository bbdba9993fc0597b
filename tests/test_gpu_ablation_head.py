"""GPU: the paper's ablation heads (CORNER_PREDICTION direct / offset / iterative, CENTERNESS none) on the engine.

  * head forward vs the reference's own DAFNeHead (tests/golden/head_ablation.npz): relative L2 < 2.5e-2 per tensor, the bound
    of tests/test_gpu_model.py; centerness of a CENTERNESS none head is exactly 1
  * dafne_corner_chain_hip vs torch.nn.functional.conv2d on the concatenated chain, fp32 on the CPU (a few ulps apart)
  * decode with CENTERNESS none vs the reference's predict_proposals (tests/golden/predict_ctr_none.npz), and the
    DAFNE_DECODE_* flag checks
  * OneStageDetector end to end, serial == sub-batch rows, batch composition and TTA, for direct / none and iterative / plain
"""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as om
from oracle import postprocess as opp
from oracle.model import fill_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_MODES = {      # fixture name -> (CORNER_PREDICTION, CENTERNESS); NUM_CLASSES is in the fixture
    "direct_none": ("direct", "none"),
    "offset_oriented": ("offset", "oriented"),
    "iterative_plain": ("iterative", "plain"),
    "c2c_none": ("center-to-corner", "none"),
    "iterative_none_c2": ("iterative", "none"),
}


def dev():
    return torch.device("cuda", 0)


def rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def cfg_for(strategy, centerness, cfgname="dota-1.0_r50.yaml", num_classes=None):
    from dafne_amd.config import load_cfg
    opts = ["MODEL.DAFNE.CORNER_PREDICTION", strategy, "MODEL.DAFNE.CENTERNESS", centerness]
    if num_classes is not None:
        opts += ["MODEL.DAFNE.NUM_CLASSES", str(num_classes)]
    return load_cfg(os.path.join(ROOT, "configs", cfgname), opts)


@pytest.mark.parametrize("name", sorted(HEAD_MODES))
def test_head_forward_vs_reference(golden, name):
    from dafne_amd.modeling.dafne.dafne import DAFNeHead
    g = golden("head_ablation")
    strategy, centerness = HEAD_MODES[name]
    cfg = cfg_for(strategy, centerness, num_classes=int(g[name + "_cfg"][0]))
    head = DAFNeHead(cfg, [types.SimpleNamespace(channels=256)] * 5)
    fill_params(head, seed=7)
    if strategy == "offset":
        with torch.no_grad():
            head.base_corners.copy_(torch.from_numpy(g[name + "_base_corners"]).view(1, 8, 1, 1))
    head.to(dev())
    head.invalidate()
    feats = [torch.from_numpy(g["feat%d" % l]).to(dev()) for l in range(5)]
    logits, regs, centers, _, ctrs, _, _ = head(None, feats)
    torch.cuda.synchronize()
    assert len(centers) == (5 if strategy == "center-to-corner" else 0)
    for l in range(5):
        assert rel(logits[l].cpu(), torch.from_numpy(g["%s_logits%d" % (name, l)])) < 2.5e-2, ("logits", l)
        assert rel(regs[l].cpu(), torch.from_numpy(g["%s_reg%d" % (name, l)])) < 2.5e-2, ("reg", l)
        if centers:
            assert rel(centers[l].cpu(), torch.from_numpy(g["%s_center%d" % (name, l)])) < 2.5e-2, ("center", l)
        if centerness == "none":
            assert tuple(ctrs[l].shape) == g["%s_ctr%d" % (name, l)].shape and bool((ctrs[l] == 1).all())
        else:
            assert rel(ctrs[l].cpu(), torch.from_numpy(g["%s_ctr%d" % (name, l)])) < 2.5e-2, ("ctr", l)


def _chain_ref(t, w1, w2, w3):
    """fp32 CPU chain on [N,H,W,>=8] T: the reference's c{k}_pred minus its tower part (dafne.py:381-387)."""
    tc = t.permute(0, 3, 1, 2)
    cs = [tc[:, 0:2]]
    for k, w in ((1, w1), (2, w2), (3, w3)):
        cs.append(tc[:, 2 * k:2 * k + 2] + F.conv2d(torch.cat(cs, 1), w, padding=1))
    return torch.cat(cs, 1).permute(0, 2, 3, 1)


@pytest.mark.parametrize("n,sizes,t_ps", [
    (1, [(1, 1)], 9),
    (2, [(2, 2), (1, 1)], 8),
    (3, [(5, 7), (3, 1), (1, 4)], 9),
    (2, [(37, 45), (16, 16), (17, 33), (9, 9), (2, 3)], 9),      # > 2 tiles each way: tile edges and halos crossed
    (1, [(64, 80), (32, 40), (16, 20), (8, 10), (4, 5)], 8),
])
def test_corner_chain_vs_conv2d(n, sizes, t_ps):
    from dafne_amd import _lib
    L = _lib.load()
    g = torch.Generator().manual_seed(11)
    ws = [torch.randn(2, 2 * k, 3, 3, generator=g) * 0.3 for k in (1, 2, 3)]
    wflat = torch.cat([w.reshape(-1) for w in ws]).to(dev())
    ts = [torch.randn(n, h, w, t_ps, generator=g) for h, w in sizes]
    td = [t.to(dev()) for t in ts]
    outs = [torch.full((n, h, w, 8), float("nan"), device=dev()) for h, w in sizes]
    segs = (_lib.ChainSeg * len(sizes))()
    for k, (t, o, (h, w)) in enumerate(zip(td, outs, sizes)):
        segs[k] = _lib.ChainSeg(t.data_ptr(), o.data_ptr(), h, w)
    _lib.check(L.dafne_corner_chain_hip(segs, len(sizes), n, t_ps, _lib.ptr(wflat), _lib.current_stream()),
               "dafne_corner_chain_hip")
    torch.cuda.synchronize()
    for t, tdv, o in zip(ts, td, outs):
        assert torch.equal(tdv.cpu(), t)                    # out of place: T untouched
        ref = _chain_ref(t, *ws)
        got = o.cpu()
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got[..., 0:2], t[..., 0:2])
        for k in range(1, 4):
            r, q = ref[..., 2 * k:2 * k + 2], got[..., 2 * k:2 * k + 2]
            assert rel(q, r) < 1e-5, (k, rel(q, r))
            assert float((q - r).abs().max()) <= 1e-5 * (1.0 + float(r.abs().max())), k


def test_corner_chain_rejects_aliasing_and_bad_args():
    from dafne_amd import _lib
    L = _lib.load()
    t = torch.zeros(1, 4, 4, 9, device=dev())
    w = torch.zeros(216, device=dev())
    segs = (_lib.ChainSeg * 1)()
    segs[0] = _lib.ChainSeg(t.data_ptr(), t.data_ptr(), 4, 4)
    assert L.dafne_corner_chain_hip(segs, 1, 1, 9, _lib.ptr(w), _lib.current_stream()) != 0
    o = torch.zeros(1, 4, 4, 8, device=dev())
    segs[0] = _lib.ChainSeg(t.data_ptr(), o.data_ptr(), 4, 4)
    assert L.dafne_corner_chain_hip(segs, 1, 1, 7, _lib.ptr(w), _lib.current_stream()) != 0
    assert L.dafne_corner_chain_hip(segs, 1, 1, 9, None, _lib.current_stream()) != 0


def _outputs_for(g, name):
    """The engine's DAFNeOutputs configured like the fixture's reference config, CENTERNESS none."""
    from dafne_amd.modeling.dafne.dafne_outputs import DAFNeOutputs
    C, topk, post, twc, sortc = (int(v) for v in g[name + "_cfg"])
    thr, nms = (float(v) for v in g[name + "_thr"])
    cfg = cfg_for("direct", "none", num_classes=C)
    d = cfg.MODEL.DAFNE
    d.PRE_NMS_TOPK_TEST, d.POST_NMS_TOPK_TEST, d.THRESH_WITH_CTR, d.SORT_CORNERS = topk, post, bool(twc), bool(sortc)
    d.INFERENCE_TH_TEST, d.NMS_TH = thr, nms
    return DAFNeOutputs(cfg)


@pytest.mark.parametrize("name", ["d10_none", "d15_none"])
def test_decode_ctr_none_vs_reference(golden, name):
    """predict_proposals with CENTERNESS none (THRESH_WITH_CTR true for d10, false for d15): score = sigmoid(cls), no
    square root, centerness 1.  Keys (level, location, class) bit-exact, scores within 1e-6, corners within 1e-3."""
    g = golden("predict_ctr_none")
    outs = _outputs_for(g, name)
    assert bool(g[name + "_cfg"][3]) == (name == "d10_none")
    logits = [torch.from_numpy(g["%s_logits%d" % (name, l)]).to(dev()) for l in range(5)]
    regs = [torch.from_numpy(g["%s_reg%d" % (name, l)]).to(dev()) for l in range(5)]
    ctrs = [torch.ones(x.shape[0], 1, x.shape[2], x.shape[3], device=dev()) for x in logits]
    res = outs.predict_proposals(logits, regs, ctrs, None, [(256, 256)] * 2)
    for i, inst in enumerate(res):
        e = {k: g["%s_im%d_%s" % (name, i, k)] for k in ("pred_corners", "scores", "centerness", "pred_classes",
                                                          "locations", "fpn_levels")}
        assert len(inst) == e["scores"].shape[0] > 0

        def keys(lv, loc, cl):
            return lv.astype(np.int64) * (1 << 40) + loc[:, 1].astype(np.int64) * (1 << 24) + loc[:, 0].astype(np.int64) * 64 + cl

        gk = keys(inst.fpn_levels.cpu().numpy(), inst.locations.cpu().numpy(), inst.pred_classes.cpu().numpy())
        ek = keys(e["fpn_levels"], e["locations"], e["pred_classes"])
        assert np.array_equal(np.sort(gk), np.sort(ek))
        go, eo = np.argsort(gk), np.argsort(ek)
        assert np.abs(inst.scores.cpu().numpy()[go] - e["scores"][eo]).max() < 1e-6
        assert np.abs(inst.pred_corners.cpu().numpy()[go] - e["pred_corners"][eo]).max() < 1e-3
        assert bool((inst.centerness == 1).all()) and np.all(e["centerness"] == 1)


def test_decode_flags_are_checked():
    from dafne_amd import _lib
    from dafne_amd import postprocess as pp
    n, h, w, C = 1, 4, 4, 3
    lg = torch.zeros(n, h, w, C, device=dev())
    dl = torch.zeros(n, h, w, 8, device=dev())
    ce = torch.zeros(n, h, w, 2, device=dev())
    ct = torch.zeros(n, h, w, 1, device=dev())
    kw = dict(num_classes=C, pre_nms_thresh=0.05, pre_nms_topk=16, thresh_with_ctr=False, sort_corners=True)

    def run(center, ctr, flags=None):
        return pp.decode_levels([pp.LevelInput(lg, dl, center, ctr, 8, 1.0)], flags=flags, **kw)

    run(ce, ct, flags=0)
    run(None, None)                                   # flags from the inputs: NO_CENTER | NO_CTRNESS
    with pytest.raises(_lib.DafneHipError):
        run(ce, ct, flags=4)                          # unknown bit
    with pytest.raises(_lib.DafneHipError):
        run(None, ct, flags=0)                        # NULL center without DAFNE_DECODE_NO_CENTER
    with pytest.raises(_lib.DafneHipError):
        run(ce, None, flags=_lib.DECODE_NO_CENTER)    # NULL ctrness without DAFNE_DECODE_NO_CTRNESS
    cand = run(None, None)
    torch.cuda.synchronize()
    k = int(cand.counts[0])
    assert k == min(16, h * w * C)                    # sigmoid(0) = 0.5 > 0.05 everywhere: no sqrt, no centerness
    assert bool((cand.scores[0, :k] == 0.5).all()) and bool((cand.ctr[0, :k] == 1).all())


def _decode_level_none(logits, reg, stride, *, thresh, topk, sort_corners, level):
    """dafne_outputs.py:792-905 for CENTERNESS none (oracle.postprocess.decode_level without the centerness factor)."""
    C, H, W = logits.shape
    loc = opp.compute_locations(H, W, stride)
    rcf = np.transpose((reg.astype(np.float32) * np.float32(stride)).astype(np.float32), (1, 2, 0)).reshape(-1, 8)
    cls = opp.sigmoid32(np.transpose(logits, (1, 2, 0)).reshape(-1, C))
    li, ci = np.nonzero(cls > np.float32(thresh))
    sc = cls[li, ci]
    if li.shape[0] > topk:
        order = np.lexsort((li.astype(np.int64) * C + ci, -sc.astype(np.float64)))
        sel = np.sort(order[:topk])
        li, ci, sc = li[sel], ci[sel], sc[sel]
    poly = np.empty((li.shape[0], 8), np.float32)
    for j in range(8):
        poly[:, j] = (loc[li, j % 2] + rcf[li, j]).astype(np.float32)
    if sort_corners:
        poly = opp.sort_quadrilateral(poly)
    hb = (np.stack((poly[:, 0::2].min(1), poly[:, 1::2].min(1), poly[:, 0::2].max(1), poly[:, 1::2].max(1)), axis=1)
          if poly.shape[0] else np.zeros((0, 4), np.float32))
    return {"pred_boxes": hb.astype(np.float32), "pred_corners": poly, "scores": sc.astype(np.float32),
            "centerness": np.ones(li.shape[0], np.float32), "pred_classes": ci.astype(np.int64),
            "locations": loc[li].astype(np.float32), "fpn_levels": np.full(li.shape[0], level, np.int64)}


_MODELS = {}


def ablation_model(strategy, centerness, seed=5):
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.registry import build_model
    key = (strategy, centerness, seed)
    if key not in _MODELS:
        cfg = cfg_for(strategy, centerness)
        m = build_model(cfg)
        # the trunk of oracle.model.make_params, the head's parameters by name (the released head's keys do not all exist)
        fill_params(m.proposal_generator.dafne_head, seed=seed)
        sd = m.state_dict()
        sd.update({k: v for k, v in om.make_params(cfg.MODEL.RESNETS.DEPTH, cfg.MODEL.DAFNE.NUM_CLASSES, seed=seed).items()
                   if k.startswith("backbone.")})
        m.load_state_dict(sd)
        m.to(dev())
        m.invalidate()
        _MODELS[key] = (cfg, m)
    return _MODELS[key]


@pytest.mark.parametrize("strategy,centerness", [("direct", "none"), ("iterative", "plain")])
def test_end_to_end_detections_vs_oracle_postprocess(strategy, centerness):
    """OneStageDetector.forward vs: the engine's head outputs -> numpy decode -> the oracle's NMS / cap /
    detector_postprocess; the same keys and bounds as tests/test_gpu_model.py's end-to-end test."""
    cfg, m = ablation_model(strategy, centerness)
    d = cfg.MODEL.DAFNE
    g = torch.Generator().manual_seed(1)
    ims = [torch.randint(0, 256, (3, 160, 192), generator=g, dtype=torch.uint8),
           torch.randint(0, 256, (3, 128, 150), generator=g, dtype=torch.uint8)]
    inputs = [{"image": ims[0], "height": 320, "width": 384}, {"image": ims[1], "height": 128, "width": 150}]
    out = m(inputs)
    torch.cuda.synchronize()
    hp = m._last_head
    assert hp.center is None and (hp.corners is not None) == (strategy == "iterative")
    for i, o in enumerate(out):
        inst = o["instances"]
        per = []
        for l, s in enumerate(d.FPN_STRIDES):
            lg = np.transpose(hp.logits[l][i].cpu().numpy(), (2, 0, 1))
            dc = hp.delta_ctr[l][i].cpu().numpy()
            src = hp.corners[l][i].cpu().numpy() if hp.corners is not None else dc[..., :8]
            reg = np.transpose((src * np.float32(hp.scales[l])).astype(np.float32), (2, 0, 1))
            if centerness == "none":
                per.append(_decode_level_none(lg, reg, s, thresh=d.INFERENCE_TH_TEST, topk=d.PRE_NMS_TOPK_TEST,
                                              sort_corners=d.SORT_CORNERS, level=l))
            else:
                per.append(opp.decode_level(lg, reg, np.transpose(dc[..., 8:9], (2, 0, 1)), s, thresh=d.INFERENCE_TH_TEST,
                                            topk=d.PRE_NMS_TOPK_TEST, thresh_with_ctr=d.THRESH_WITH_CTR,
                                            sort_corners=d.SORT_CORNERS, level=l))
        det = opp.select_over_all_levels(opp.cat(per), d.NMS_TH, d.POST_NMS_TOPK_TEST, fast=True)
        hw = tuple(ims[i].shape[1:])
        exp = opp.detector_postprocess(det, hw, (inputs[i]["height"], inputs[i]["width"]), hw)
        assert len(inst) == exp["scores"].shape[0] and len(inst) > 0
        gs = inst.scores.cpu().numpy()
        assert np.all(np.diff(gs) <= 0)
        if centerness == "none":
            lmax = max(float(hp.logits[l][i].max()) for l in range(5))
            assert gs.max() <= 1.0 / (1.0 + np.exp(-lmax)) + 1e-6          # no square root applied
            assert bool((inst.centerness == 1).all())
        sx, sy = inputs[i]["width"] / hw[1], inputs[i]["height"] / hw[0]

        def keys(levels_, locs_, classes_):
            x = np.rint(locs_[:, 0] / sx).astype(np.int64)
            y = np.rint(locs_[:, 1] / sy).astype(np.int64)
            return levels_.astype(np.int64) * (1 << 40) + y * (1 << 24) + x * 64 + classes_.astype(np.int64)
        gk = keys(inst.fpn_levels.cpu().numpy(), inst.locations.cpu().numpy(), inst.pred_classes.cpu().numpy())
        ek = keys(exp["fpn_levels"], exp["locations"], exp["pred_classes"])
        assert len(np.unique(gk)) == len(gk)
        assert np.array_equal(np.sort(gk), np.sort(ek)), "different detection sets"
        go, eo = np.argsort(gk), np.argsort(ek)
        assert np.abs(gs[go] - exp["scores"][eo]).max() < 1e-6
        assert np.abs(inst.pred_corners.cpu().numpy()[go] - exp["pred_corners"][eo]).max() < 1e-3
        assert np.abs(inst.pred_boxes.tensor.cpu().numpy()[go] - exp["pred_boxes"][eo]).max() < 1e-3


@pytest.mark.parametrize("strategy,centerness", [("direct", "none"), ("iterative", "plain")])
def test_serial_pipelined_and_batch_composition_agree(strategy, centerness):
    """The project's determinism guarantees for an ablation head: the serial plan and the sub-batch-stream layout give
    the same rows bit for bit, and an image gets the same detections alone, in a batch, run to run."""
    cfg, m = ablation_model(strategy, centerness)
    g = torch.Generator().manual_seed(2)
    img = torch.randint(0, 256, (3, 3, 128, 128), generator=g, dtype=torch.uint8).to(dev())
    r0, c0 = m.detect_packed(img)
    torch.cuda.synchronize()
    r1, c1 = m.detect_packed(img, pipelined=True, splits=2)
    torch.cuda.synchronize()
    r2, c2 = m.detect_packed(img, pipelined=True, splits=3)
    torch.cuda.synchronize()
    assert torch.equal(c0, c1) and torch.equal(c0, c2) and int(c0.min()) > 0
    for i in range(3):
        k = int(c0[i])
        assert torch.equal(r0[i, :k], r1[i, :k]) and torch.equal(r0[i, :k], r2[i, :k])
    inputs = [{"image": im.cpu(), "height": 128, "width": 128} for im in img]
    a = m(inputs)
    b = m(inputs)
    single = [m([inp])[0] for inp in inputs]
    for x, y, z in zip(a, b, single):
        assert len(x["instances"]) > 0
        assert torch.equal(x["instances"].pred_corners, y["instances"].pred_corners)
        assert torch.equal(x["instances"].scores, y["instances"].scores)
        assert torch.equal(x["instances"].pred_corners, z["instances"].pred_corners)
        assert torch.equal(x["instances"].scores, z["instances"].scores)


def test_tta_packed_chunks_equal_the_reference_style_loop():
    """TEST.AUG with a direct / none head: the packed TTA path returns the detections of the per-view loop
    (tta.py:170-179)."""
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA
    cfg, m = ablation_model("direct", "none")
    cfg.TEST.AUG.MIN_SIZES = [96, 128]
    cfg.TEST.AUG.MAX_SIZE = 192
    tta = OneStageRCNNWithTTA(cfg, m)
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (3, 128, 160), generator=g, dtype=torch.uint8).to(dev())
    aug, _ = tta._get_augmented_inputs({"image": img, "height": 128, "width": 160})
    a = tta._batch_inference(aug)
    b = tta._batch_inference_packed(aug)
    assert len(a) == len(b) == len(aug) > 0
    for x, y in zip(a, b):
        ix, iy = x["instances"], y["instances"]
        assert len(ix) == len(iy) and ix.image_size == iy.image_size
        assert torch.equal(ix.pred_corners, iy.pred_corners) and torch.equal(ix.scores, iy.scores)
        assert torch.equal(ix.pred_classes, iy.pred_classes)
    merged = tta([{"image": img, "height": 128, "width": 160}])
    assert len(merged[0]["instances"]) > 0
