"""dafne_targets.npz: the reference's own DAFNeOutputs._get_ground_truth and .losses on the CPU, under the stand-ins
make_golden.py uses for the packages the build container lacks.  fvcore's two functions are written out here from their
formulas:

    sigmoid focal loss   p = sigmoid(x), ce = BCEWithLogits(x, t), p_t = p t + (1 - p)(1 - t),
                         loss = ce (1 - p_t)^gamma (alpha t + (1 - alpha)(1 - t))
    smooth L1            n = |x - y|;  n for beta < 1e-5, else 0.5 n^2 / beta below beta and n - 0.5 beta above

Inputs are regenerated from seeds (tests/_targets_np.py: case_a, case_b_predictions, handmade_targets), so only the
reference's results are stored.

The assignment is defined in correctly rounded fp32 operations, and the fixture must not depend on the CPU it was made on.
torch.sqrt on the CPU goes to MKL's vector library, whose result depends on the instruction set MKL dispatches to: on its
AVX512 path sqrt(388.43658447265625f) comes out as 19.70879364013672, one ulp below the correctly rounded 19.70879554748535
(the exact root is 19.7087945971...); its AVX2 path rounds correctly.  The maker therefore pins MKL to AVX2 before torch is
loaded and then CHECKS the premise instead of trusting it: fp32 sqrt and division of 2^22 values each (and of that one) must
equal the fp64 result rounded once to fp32 -- which is the correctly rounded fp32 result, 53 >= 2 * 24 + 2 bits -- or the maker
stops.

    python tests/golden/make_golden_targets.py        (build container only: imports /root/reference under stubs)
"""
import os
import sys

os.environ.setdefault("MKL_ENABLE_INSTRUCTIONS", "AVX2")       # before torch loads MKL: see the module docstring

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import _targets_np as tn  # noqa: E402


def sigmoid_focal_loss(inputs, targets, alpha=-1, gamma=2, reduction="none"):
    p = torch.sigmoid(inputs)
    ce = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def smooth_l1_loss(input, target, beta, reduction="none"):
    if beta < 1e-5:
        loss = torch.abs(input - target)
    else:
        n = torch.abs(input - target)
        loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def ref_instances(gt, hw):
    return mg.Instances(hw, gt_boxes=mg.Boxes(torch.from_numpy(gt["hbox"].copy())), gt_corners=torch.from_numpy(gt["corners"].copy()),
                        gt_corners_area=torch.from_numpy(gt["area"].copy()), gt_classes=torch.from_numpy(gt["cls"].copy()))


REF_KEYS = {"center_sample_only": "CENTER_SAMPLE_ONLY", "in_box_check": "ENABLE_IN_BOX_CHECK", "stride_norm": "ENABLE_FPN_STRIDE_NORM"}


def nchw(flat, n, shapes):
    return [torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))) for a in tn.split_levels(flat, n, shapes)]


def check_correctly_rounded():
    """torch's fp32 sqrt and division on this CPU, in this process, against fp64-then-round (= correctly rounded)."""
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.rand(1 << 22, generator=g) * 1000.0, torch.tensor([388.43658447265625])])
    y = torch.rand(x.shape[0], generator=g) * 30.0 + 1e-3
    bad_sqrt = int((torch.sqrt(x) != torch.sqrt(x.double()).float()).sum())
    bad_div = int(((x / y) != (x.double() / y.double()).float()).sum())
    assert bad_sqrt == 0 and bad_div == 0, (
        "torch's CPU fp32 sqrt / division is not correctly rounded here (%d / %d of %d values differ from fp64-then-round): "
        "the fixture would record this machine's library, not the arithmetic the assignment is defined in.  "
        "MKL_ENABLE_INSTRUCTIONS=%s" % (bad_sqrt, bad_div, x.shape[0], os.environ.get("MKL_ENABLE_INSTRUCTIONS")))


def main():
    assert os.path.isdir(mg.REF), "reference tree not present: fixtures can only be made in the build container"
    check_correctly_rounded()
    mg.install_stubs()
    sys.modules["fvcore.nn"].sigmoid_focal_loss_jit = sigmoid_focal_loss
    sys.modules["fvcore.nn"].smooth_l1_loss = smooth_l1_loss
    mg.load_ref("dafne.utils.sort_corners")
    mg.load_ref("dafne.layers.deform_conv")
    mg.load_ref("dafne.modeling.losses.utils")
    mg.load_ref("dafne.modeling.losses.smooth_l1")
    mg.load_ref("dafne.modeling.nms.nms")
    outputs_mod = mg.load_ref("dafne.modeling.dafne.dafne_outputs")
    dafne_mod = mg.load_ref("dafne.modeling.dafne.dafne")
    res = {}

    # ---- case A: assignment
    gts, shapes = tn.case_a()
    locs = [dafne_mod.compute_locations(h, w, s, "cpu") for (h, w), s in zip(shapes, tn.STRIDES)]
    targets = {}
    for name, over in tn.ASSIGN_CONFIGS.items():
        cfg = mg.load_cfg("dota-1.0_r101_ms.yaml", **{REF_KEYS[k]: v for k, v in over.items()})
        outs = outputs_mod.DAFNeOutputs(cfg)
        with torch.no_grad():
            tt = outs._get_ground_truth(locs, [ref_instances(g, tn.CASE_A_HW) for g in gts])
        cat = lambda k: torch.cat([x.reshape(len(x), -1) for x in tt[k]], 0).numpy()  # noqa: E731
        t = dict(labels=cat("labels")[:, 0], target_inds=cat("target_inds")[:, 0], corners=cat("reg_targets_corners"),
                 ltrb=cat("reg_targets_ltrb"), abcd=cat("reg_targets_abcd"))
        targets[name] = t
        res["a_%s_labels" % name] = t["labels"].astype(np.int16)
        res["a_%s_target_inds" % name] = t["target_inds"].astype(np.int16)
        for k in ("corners", "ltrb", "abcd"):
            res["a_%s_%s" % (name, k)] = t[k].astype(np.float32)
        if name == "released":
            st = {}
            mine = tn.assign(gts, shapes, tn.assign_config(name), stats=st)
            assert np.array_equal(mine["labels"], t["labels"]), "the restatement the statistics come from disagrees"
            print("case A:", st)
            assert sum(1 for v in st["pos_per_level"] if v > 0) >= 4, st
            assert st["multi"] >= 20 and st["ties"] >= 1 and st["near_eps"] >= 1, st
            res["a_stats"] = np.array(st["pos_per_level"] + [st["multi"], st["ties"], st["near_eps"]], np.int64)
            P = t["labels"].shape[0]
            # the reference's own centerness targets (fp32 pow) at the positives, both modes
            pos = t["labels"] != 15
            res["a_ctr_oriented"] = outputs_mod.compute_ctrness_targets(torch.from_numpy(t["abcd"][pos]), 3).numpy()
            res["a_ctr_plain"] = outputs_mod.compute_ctrness_targets(torch.from_numpy(t["ltrb"][pos]), 3).numpy()
        print("case A", name, "positives", int((t["labels"] != 15).sum()))

    # ---- case B: losses
    def run_losses(tg, preds, Lc, n, shp, gt_list=None):
        cfg = mg.load_cfg("dota-1.0_r101_ms.yaml", CORNER_PREDICTION="center-to-corner" if Lc["has_center_reg"] else "direct",
                          CENTERNESS=Lc["ctr_mode"], ENABLE_LOSS_MODULATION=Lc["modulation"], ENABLE_LOSS_LOG=Lc["logspace"],
                          LOSS_SMOOTH_L1_BETA=Lc["beta"])
        outs = outputs_mod.DAFNeOutputs(cfg)
        logits, corners, center, ctr = preds
        with torch.no_grad():
            if gt_list is not None:
                lc = [dafne_mod.compute_locations(h, w, s, "cpu") for (h, w), s in zip(shp, tn.STRIDES)]
                extras, ls = outs.losses(nchw(logits, n, shp), nchw(corners, n, shp), nchw(center, n, shp), [],
                                         nchw(ctr[:, None], n, shp), lc, [ref_instances(g, tn.CASE_A_HW) for g in gt_list], top_feats=[])
            else:
                inst = mg.Instances((0, 0), labels=torch.from_numpy(tg["labels"]), reg_targets_corners=torch.from_numpy(tg["corners"]),
                                    reg_targets_ltrb=torch.from_numpy(tg["ltrb"]), reg_targets_abcd=torch.from_numpy(tg["abcd"]),
                                    logits_pred=torch.from_numpy(logits), corners_reg_pred=torch.from_numpy(corners),
                                    center_reg_pred=torch.from_numpy(center), ctrness_pred=torch.from_numpy(ctr))
                extras, ls = outs.dafne_losses(inst)
        row = [float(ls["loss/cls"]), float(ls["loss/corners"]), float(ls.get("loss/center", 0.0)), float(ls.get("loss/ctr", 0.0)),
               float(len(extras["instances"])), float(extras["loss_denorm"])]
        return np.array(row, np.float64)

    tg = targets["released"]
    preds = tn.case_b_predictions(tg, seed=21)
    for name, Lc in tn.loss_configs():
        res["b_" + name] = run_losses(tg, preds, Lc, 3, shapes, gt_list=gts)
    print("case B released:", res["b_c2c_oriented_m1_l1_b1"])
    empty = [tn.gt_of(np.zeros((0, 8), np.float32), np.zeros(0, np.int64))] * 3
    tg0 = tn.assign(empty, shapes, tn.assign_config("released"))
    res["b_nopos"] = run_losses(tg0, tn.case_b_predictions(tg0, seed=22), tn.LOSS_RELEASED, 3, shapes, gt_list=empty)
    assert res["b_nopos"][4] == 0
    for kind in ("zero_ctr", "nan_ctr"):
        th = tn.handmade_targets(kind)
        for mode in ("oriented", "plain"):
            res["b_%s_%s" % (kind, mode)] = run_losses(th, tn.case_b_predictions(th, seed=23), dict(tn.LOSS_RELEASED, ctr_mode=mode), 1,
                                                       [(8, 8)])
            print("case B", kind, mode, res["b_%s_%s" % (kind, mode)])
    out = os.path.join(HERE, "dafne_targets.npz")
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 1000000


if __name__ == "__main__":
    main()
