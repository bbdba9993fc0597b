"""dafne_targets_grad.npz: the gradients the reference's own autograd gives for DAFNeOutputs.dafne_losses on the CPU -- the
reference's code under make_golden_targets.py's stand-ins, its inputs made leaves that require grad,
sum(losses.values()).backward() -- once in fp32 (the reference as it runs) and once with every input .double().  The fp64
gradients are stored, and per tensor the largest |fp32 - fp64| seen: the reference's own rounding error, which is the unit the
CPU test's bound is expressed in.

Inputs are regenerated from seeds (tests/_targets_grad_np.py, tests/_targets_np.py), so only the reference's results are stored:
  small case     2 images of 128 x 160, all 48 tn.loss_configs(): regression / centerness gradients at the positives, the
                 logits gradient once per distinct normalised lambda_cls
  handmade case  one positive of each kind of gn.HANDMADE_KINDS, under gn.handmade_configs() (beta = 0.5)
  centerness     tn.handmade_targets("zero_ctr" / "nan_ctr"), oriented and plain
  no positives   a batch whose every label is background

    python tests/golden/make_golden_targets_grad.py        (build container only: imports the reference under stubs)
"""
import os
import sys

import make_golden_targets as mgt       # sets MKL_ENABLE_INSTRUCTIONS before torch loads: see its docstring

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
mg, tn = mgt.mg, mgt.tn
import _targets_grad_np as gn  # noqa: E402

TENSORS = ("logits", "corners", "center", "ctr")


def main():
    assert os.path.isdir(mg.REF), "reference tree not present: fixtures can only be made in the build container"
    mgt.check_correctly_rounded()
    mg.install_stubs()
    sys.modules["fvcore.nn"].sigmoid_focal_loss_jit = mgt.sigmoid_focal_loss
    sys.modules["fvcore.nn"].smooth_l1_loss = mgt.smooth_l1_loss
    for m in ("dafne.utils.sort_corners", "dafne.layers.deform_conv", "dafne.modeling.losses.utils", "dafne.modeling.losses.smooth_l1",
              "dafne.modeling.nms.nms"):
        mg.load_ref(m)
    outputs_mod = mg.load_ref("dafne.modeling.dafne.dafne_outputs")

    def ref_grads(tg, preds, Lc, dtype):
        cfg = mg.load_cfg("dota-1.0_r101_ms.yaml", CORNER_PREDICTION="center-to-corner" if Lc["has_center_reg"] else "direct",
                          CENTERNESS=Lc["ctr_mode"], ENABLE_LOSS_MODULATION=Lc["modulation"], ENABLE_LOSS_LOG=Lc["logspace"],
                          LOSS_SMOOTH_L1_BETA=Lc["beta"], SORT_CORNERS=Lc["sort_corners"])
        outs = outputs_mod.DAFNeOutputs(cfg)
        assert outs.focal_loss_alpha == Lc["alpha"] and outs.focal_loss_gamma == Lc["gamma"]
        lam = tn.normalized_lambdas(Lc)
        assert abs(outs.lambda_cls - lam["cls"]) < 1e-15 and abs(outs.lambda_corners - lam["corners"]) < 1e-15
        leaves = [torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True) for a in preds]
        tgt = lambda k: torch.from_numpy(tg[k]).to(dtype)  # noqa: E731
        inst = mg.Instances((0, 0), labels=torch.from_numpy(tg["labels"]), reg_targets_corners=tgt("corners"),
                            reg_targets_ltrb=tgt("ltrb"), reg_targets_abcd=tgt("abcd"), logits_pred=leaves[0],
                            corners_reg_pred=leaves[1], center_reg_pred=leaves[2], ctrness_pred=leaves[3])
        _, ls = outs.dafne_losses(inst)
        sum(ls.values()).backward()
        out = {}
        for name, leaf in zip(TENSORS, leaves):
            used = name in ("logits", "corners") or (name == "center" and Lc["has_center_reg"]) or (name == "ctr" and Lc["ctr_mode"] != "none")
            if used:
                assert leaf.grad is not None, name
                out[name] = leaf.grad.numpy().astype(np.float64)
            else:
                assert leaf.grad is None or not leaf.grad.any(), name
        return out

    def both(tg, preds, Lc, tag):
        """fp64 gradients and, per tensor, max |fp32 - fp64| (nan for a tensor the configuration lacks)."""
        g32, g64 = ref_grads(tg, preds, Lc, torch.float32), ref_grads(tg, preds, Lc, torch.float64)
        md = np.full(4, np.nan)
        for i, k in enumerate(TENSORS):
            if k in g64:
                assert np.isfinite(g64[k]).all() and np.isfinite(g32[k]).all(), (tag, k)
                md[i] = np.abs(g32[k] - g64[k]).max()
                top = np.abs(g64[k]).max()
                assert md[i] <= 1e-4 * top, (tag, k, md[i], top)
                assert np.array_equal(g32[k] == 0, g64[k] == 0), (tag, k, "the two precisions disagree about which elements are zero")
        return g64, md

    res = {}
    stats = dict(shifts=np.zeros(3, np.int64), quadratic=0, linear=0, dead_slots=0)

    def note(tg, preds, Lc):
        info = {}
        gn.grads(preds[0], preds[1], preds[2], preds[3], tg, Lc, info=info)
        if info:
            if Lc["modulation"]:
                stats["shifts"] += info["shifts"]
            stats["quadratic"] += info["quadratic"]
            stats["linear"] += info["linear"]
            if Lc["sort_corners"]:
                stats["dead_slots"] += info["dead_slots"]

    # ---- small seeded case, all 48 configurations
    _, shapes, tg, preds = gn.small_grad_case()
    pos = np.nonzero(tg["labels"] != 15)[0]
    print("small case: positions", tg["labels"].shape[0], "positives", len(pos))
    assert len(pos) >= 30
    res["s_pos"] = pos.astype(np.int32)
    logit_keys = []
    for name, Lc in tn.loss_configs():
        g64, md = both(tg, preds, Lc, name)
        note(tg, preds, Lc)
        key = gn.lam_cls_key(Lc)
        if key not in logit_keys:
            logit_keys.append(key)
            res["s_logits_%d" % logit_keys.index(key)] = g64["logits"]
        else:
            assert np.array_equal(res["s_logits_%d" % logit_keys.index(key)], g64["logits"]), name
        for k in TENSORS[1:]:
            if k in g64:
                rest = np.ones(g64[k].shape[0], bool)
                rest[pos] = False
                assert not g64[k][rest].any(), (name, k, "a gradient at a non-positive")
                res["s_%s_%s" % (name, k)] = g64[k][pos]
        res["s_%s_maxdiff" % name] = md
    res["s_logit_keys"] = np.array(logit_keys)

    # ---- handmade positives
    th, hp, where = gn.handmade_grad_case()
    for name, Lc in gn.handmade_configs():
        g64, md = both(th, hp, Lc, name)
        note(th, hp, Lc)
        for k in TENSORS:
            res["h_%s_%s" % (name, k)] = g64[k]
        res["h_%s_maxdiff" % name] = md
        if Lc["sort_corners"]:
            gc = g64["corners"].reshape(-1, 4, 2)
            assert gc[where["collinear"], 0].all() and not gc[where["collinear"], 1:].any(), "collinear: only the leftmost corner"
            assert not gc[where["all_equal"], 1:].any(), "all equal: only the first corner is copied"
        assert not g64["corners"][where["n_zero"]].any() and not g64["center"][where["n_zero"]].any(), "n = 0: sign(0) = 0"

    # ---- centerness targets of 0 and NaN
    for kind in ("zero_ctr", "nan_ctr"):
        tz = tn.handmade_targets(kind)
        pz = tn.case_b_predictions(tz, seed=23)
        for mode in ("oriented", "plain"):
            g64, md = both(tz, pz, dict(tn.LOSS_RELEASED, ctr_mode=mode), (kind, mode))
            for k in TENSORS:
                res["z_%s_%s_%s" % (kind, mode, k)] = g64[k]
            res["z_%s_%s_maxdiff" % (kind, mode)] = md

    # ---- a batch without positives
    t0 = dict(th, labels=np.full(64, 15, np.int64))
    g64, md = both(t0, hp, tn.LOSS_RELEASED, "nopos")
    for k in TENSORS[1:]:
        assert not g64[k].any(), k
    for k in TENSORS:
        res["n_%s" % k] = g64[k]
    res["n_maxdiff"] = md

    print("branches:", stats)
    assert (stats["shifts"] > 0).all(), "a shift of the modulated loss never wins"
    assert stats["quadratic"] > 0 and stats["linear"] > 0, "a smooth-L1 branch never occurs"
    assert stats["dead_slots"] > 0, "no sorted slot is a constant zero"
    res["stats"] = np.array(list(stats["shifts"]) + [stats["quadratic"], stats["linear"], stats["dead_slots"]], np.int64)
    out = os.path.join(HERE, "dafne_targets_grad.npz")
    np.savez_compressed(out, **res)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 1000000


if __name__ == "__main__":
    main()
