"""Fixtures of the paper's ablation heads from the reference's own dafne.py / dafne_outputs.py (CORNER_PREDICTION direct,
offset, iterative and center-to-corner crossed with CENTERNESS oriented / plain / none), under the stubs of make_golden.py.

head_ablation.npz     DAFNeHead forward per mode on one set of small NCHW features (N = 2, levels 12x16 .. 1x1), weights
                      from oracle.model.fill_params(head, seed=7) except base_corners, which keeps the reference's constant
                      (stored as <mode>_base_corners); plus each mode's state-dict names and shapes (<mode>_keys,
                      <mode>_shapes, padded with -1).  Weights are NOT stored: the tests regenerate them by name.
predict_ctr_none.npz  DAFNeOutputs.predict_proposals with CENTERNESS none on direct-style regressions (no center), with
                      THRESH_WITH_CTR true and false; the layout of make_golden.gen_predict.

    python tests/golden/make_golden_ablation.py        (build container only: imports the reference under stubs)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

# name -> (reference config dump, CORNER_PREDICTION, CENTERNESS)
HEAD_MODES = {
    "direct_none": ("dota-1.0_r101_ms.yaml", "direct", "none"),
    "offset_oriented": ("dota-1.0_r101_ms.yaml", "offset", "oriented"),
    "iterative_plain": ("dota-1.0_r101_ms.yaml", "iterative", "plain"),
    "c2c_none": ("dota-1.0_r101_ms.yaml", "center-to-corner", "none"),
    "iterative_none_c2": ("ucas_aod_r101_ms.yaml", "iterative", "none"),
}
LEVEL_SIZES = ((12, 16), (6, 8), (3, 4), (2, 2), (1, 1))


def gen_head(out, dafne_mod):
    from oracle.model import fill_params
    SS = sys.modules["detectron2.layers"].ShapeSpec
    rng = np.random.default_rng(506)
    feats = [torch.from_numpy(rng.normal(0, 1, (2, 256, h, w)).astype(np.float32)) for h, w in LEVEL_SIZES]
    res = {"feat%d" % l: feats[l].numpy() for l in range(5)}
    for name, (cfgfile, strategy, ctr_mode) in HEAD_MODES.items():
        cfg = mg.load_cfg(cfgfile, CORNER_PREDICTION=strategy, CENTERNESS=ctr_mode)
        head = dafne_mod.DAFNeHead(cfg, [SS(channels=256)] * 5)
        head.eval()
        fill_params(head, seed=7)
        if strategy == "offset":          # a constant of the reference (dafne.py:231-235), not a learned value
            with torch.no_grad():
                head.base_corners.copy_(torch.tensor([-2.0, 2.0, 2.0, 2.0, 2.0, -2.0, -2.0, -2.0]).view(1, 8, 1, 1))
            res[name + "_base_corners"] = head.base_corners.detach().numpy().reshape(8)
        sd = head.state_dict()
        res[name + "_keys"] = np.array(list(sd.keys()))
        shapes = np.full((len(sd), 4), -1, np.int64)
        for i, v in enumerate(sd.values()):
            shapes[i, :v.dim()] = v.shape
        res[name + "_shapes"] = shapes
        res[name + "_cfg"] = np.array([cfg.MODEL.DAFNE.NUM_CLASSES], np.int64)
        with torch.no_grad():
            logits, reg, center, _, ctr, _, _ = head(None, feats, None, False)
        assert (len(center) == 5) == (strategy == "center-to-corner")
        for l in range(5):
            res["%s_logits%d" % (name, l)] = logits[l].numpy()
            res["%s_reg%d" % (name, l)] = reg[l].numpy()
            res["%s_ctr%d" % (name, l)] = ctr[l].numpy()
            if center:
                res["%s_center%d" % (name, l)] = center[l].numpy()
        print("head", name, "keys", len(sd), "params", sum(p.numel() for p in head.parameters()))
    np.savez_compressed(out, **res)


def gen_predict(out, outputs_mod, dafne_mod):
    rng = np.random.default_rng(407)
    strides = [8, 16, 32, 64, 128]
    sizes = [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2)]
    res = {}
    for name, cfgfile, over in [("d10_none", "dota-1.0_r101_ms.yaml", {"CENTERNESS": "none", "CORNER_PREDICTION": "direct"}),
                                ("d15_none", "dota-1.5_r101_ms.yaml", {"CENTERNESS": "none", "CORNER_PREDICTION": "direct"})]:
        cfg = mg.load_cfg(cfgfile, **over)
        C = cfg.MODEL.DAFNE.NUM_CLASSES
        outs = outputs_mod.DAFNeOutputs(cfg)
        outs.eval()
        N = 2
        logits, regs, ctrs, locs = [], [], [], []
        for (h, w), s in zip(sizes, strides):
            logits.append(torch.from_numpy(rng.normal(-3.0, 2.0, (N, C, h, w)).astype(np.float32)))
            regs.append(torch.from_numpy(rng.normal(0, 1.5, (N, 8, h, w)).astype(np.float32)))
            ctrs.append(torch.ones(N, 1, h, w))            # what the head returns without centerness (dafne.py:474-480)
            locs.append(dafne_mod.compute_locations(h, w, s, "cpu"))
        with torch.no_grad():
            boxlists = outs.predict_proposals(logits, regs, ctrs, locs, [(256, 256)] * N, [])
        res[name + "_cfg"] = np.array([C, cfg.MODEL.DAFNE.PRE_NMS_TOPK_TEST, cfg.MODEL.DAFNE.POST_NMS_TOPK_TEST,
                                       int(cfg.MODEL.DAFNE.THRESH_WITH_CTR), int(cfg.MODEL.DAFNE.SORT_CORNERS)], np.int64)
        res[name + "_thr"] = np.array([cfg.MODEL.DAFNE.INFERENCE_TH_TEST, cfg.MODEL.DAFNE.NMS_TH])
        for l in range(5):
            res["%s_logits%d" % (name, l)] = logits[l].numpy()
            res["%s_reg%d" % (name, l)] = regs[l].numpy()
        for i, bl in enumerate(boxlists):
            f = bl.get_fields()
            res["%s_im%d_pred_boxes" % (name, i)] = f["pred_boxes"].tensor.numpy()
            for k in ("pred_corners", "scores", "centerness", "pred_classes", "locations", "fpn_levels"):
                res["%s_im%d_%s" % (name, i, k)] = f[k].numpy()
            print("predict", name, "twc", int(cfg.MODEL.DAFNE.THRESH_WITH_CTR), "im", i, "dets", len(bl))
    np.savez_compressed(out, **res)


def main():
    assert os.path.isdir(mg.REF), "reference tree not present: fixtures can only be made in the build container"
    mg.install_stubs()
    mg.load_ref("dafne.utils.sort_corners")
    mg.load_ref("dafne.layers.deform_conv")
    mg.load_ref("dafne.modeling.losses.utils")
    mg.load_ref("dafne.modeling.losses.smooth_l1")
    mg.load_ref("dafne.modeling.nms.nms")
    outputs_mod = mg.load_ref("dafne.modeling.dafne.dafne_outputs")
    dafne_mod = mg.load_ref("dafne.modeling.dafne.dafne")
    gen_head(os.path.join(HERE, "head_ablation.npz"), dafne_mod)
    gen_predict(os.path.join(HERE, "predict_ctr_none.npz"), outputs_mod, dafne_mod)


if __name__ == "__main__":
    main()
