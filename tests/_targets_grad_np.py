"""numpy restatement of the gradient of the four loss terms with respect to the head outputs (what
dafne_losses_backward_hip computes), built on the pieces of tests/_targets_np.py, plus the inputs the gradient fixture's maker
and the tests share.

The definition is the derivative of tn.losses() with the conventions of the reference's autograd: the centerness target is a
constant, the modulated minimum sends its gradient to the first of equal shifts, sort_quadrilateral sends none to the output
slots it leaves at zero, sign(0) = 0 and the smooth L1 is linear from |x - y| == beta on.  fp64 from the fp32 inputs.
"""
import numpy as np

import _targets_np as tn
from dafne_amd.data.targets import _cross

f32 = np.float32


def sort_with_sources(boxes):
    """dafne_amd.data.targets.sort_quadrilateral_np's selection made visible: -> (sorted [n, 8] fp32, src [n, 4] int: the input
    corner each output corner was copied from, -1 where the reference leaves its zeros)."""
    b = np.ascontiguousarray(boxes, dtype=f32).reshape(-1, 8)
    n = b.shape[0]
    S = b.reshape(n, 4, 2)
    ar = np.arange(n)
    k1 = np.argmin(S[:, :, 0], axis=1)
    p1 = S[ar, k1]
    keep = np.ones((n, 4), bool)
    keep[ar, k1] = False
    R = S[keep].reshape(n, 3, 2)
    RS = np.tile(np.arange(4), (n, 1))[keep].reshape(n, 3)
    p3, A, B = np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.zeros((n, 2), f32)
    s3, sa, sb = np.full(n, -1), np.full(n, -1), np.full(n, -1)
    done = np.zeros(n, bool)
    for i in range(3):
        i2, i3 = (1 if i == 0 else 0), (1 if i == 2 else 2)
        d = R[:, i] - p1
        with np.errstate(all="ignore"):
            cond = ((_cross(d, R[:, i2] - p1) * _cross(d, R[:, i3] - p1)) < 0) & ~done
        p3[cond], A[cond], B[cond] = R[cond, i], R[cond, i2], R[cond, i3]
        s3[cond], sa[cond], sb[cond] = RS[cond, i], RS[cond, i2], RS[cond, i3]
        done |= cond
    e = p3 - p1
    with np.errstate(all="ignore"):
        swap = ~(_cross(e, A - p1) > 0) & (_cross(e, B - p1) > 0)
    p2 = np.where(swap[:, None], B, A)
    p4 = np.where(swap[:, None], A, B)
    src = np.stack((k1, np.where(swap, sb, sa), s3, np.where(swap, sa, sb)), axis=1)
    return np.stack((p1, p2, p3, p4), axis=1).reshape(n, 8), src


def _sl1_grad(d, beta, logspace):
    """d/dd of tn._sl1(|d|)."""
    n = np.abs(d)
    if beta < 1e-5:
        v, dv = n, np.ones_like(n)
    else:
        v = np.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)
        dv = np.where(n < beta, n / beta, 1.0)
    if logspace:
        dv = dv / (1.0 + v)
    return np.sign(d) * dv


SHIFTS = (0, 2, 6)      # component k of the target meets sorted slot (k + shift) & 7: no shift, [1,2,3,0], [3,0,1,2]


def grads(logits, corners_pred, center_pred, ctr_pred, tg, Lc, upstream=(1.0, 1.0, 1.0, 1.0), info=None):
    """fp64 gradients of upstream . (cls, corners, center, ctr) of tn.losses().  -> dict logits [P, C], corners [P, 8],
    center [P, 2] or None, ctr [P] or None (zeros at non-positives).  info: a dict that receives the branch statistics the
    fixture's maker asserts (shift counts, smooth-L1 branches, dead sort slots)."""
    C = Lc["num_classes"]
    lam = tn.normalized_lambdas(Lc)
    labels = tg["labels"]
    P = labels.shape[0]
    pos = np.nonzero(labels != C)[0]
    num_pos = len(pos)
    num_pos_avg = max(float(num_pos), 1.0)
    up = [float(u) for u in upstream]
    x = logits.astype(np.float64)
    t = np.zeros_like(x)
    t[pos, labels[pos]] = 1.0
    gamma, alpha = Lc["gamma"], Lc["alpha"]
    with np.errstate(all="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        pt = p * t + (1.0 - p) * (1.0 - t)
        om = 1.0 - pt
        g = np.power(om, gamma) * (p - t)
        if gamma != 0:
            g = g - gamma * np.power(om, gamma - 1.0) * tn._bce(x, t) * ((2.0 * t - 1.0) * p * (1.0 - p))
        if alpha >= 0:
            g = (alpha * t + (1.0 - alpha) * (1.0 - t)) * g
        out = {"logits": g / num_pos_avg * (lam["cls"] * up[0])}
    has_center, has_ctr = Lc["has_center_reg"], Lc["ctr_mode"] != "none"
    out["corners"] = np.zeros((P, 8))
    out["center"] = np.zeros((P, 2)) if has_center else None
    out["ctr"] = np.zeros(P) if has_ctr else None
    if not num_pos:
        return out
    if Lc["ctr_mode"] == "plain":
        cw = tn.ctrness_targets(tg["ltrb"][pos], Lc["ctr_alpha"])
    elif Lc["ctr_mode"] == "oriented":
        cw = tn.ctrness_targets(tg["abcd"][pos], Lc["ctr_alpha"])
    else:
        cw = np.ones(num_pos, np.float64)
    csum = cw.sum()
    denorm = max(csum, 1e-6)
    w = (cw if csum > 0 else np.ones(num_pos)) / denorm
    beta, ls = Lc["beta"], Lc["logspace"]
    q = corners_pred[pos].astype(f32)
    src = np.tile(np.arange(4), (num_pos, 1))
    if Lc["sort_corners"]:
        q, src = sort_with_sources(q)
    q = q.astype(np.float64)
    tc = tg["corners"][pos].astype(np.float64)
    ar = np.arange(num_pos)
    sh = np.zeros(num_pos, np.int64)
    with np.errstate(all="ignore"):
        if Lc["modulation"]:
            ks = np.arange(8)
            l = [tn._sl1(np.abs(q[:, (ks + s) & 7] - tc), beta, ls).sum(1) for s in SHIFTS]
            best = l[0].copy()
            for j in (1, 2):
                take = l[j] < best
                best[take] = l[j][take]
                sh[take] = j
        off = np.array(SHIFTS)[sh]
        slot = (np.arange(8)[None, :] + off[:, None]) & 7            # [n, 8]: the sorted slot component k meets
        d = q[ar[:, None], slot] - tc
        gk = _sl1_grad(d, beta, ls) * (w * (lam["corners"] * up[1]))[:, None]
        gs = np.zeros((num_pos, 8))
        gs[ar[:, None], slot] = gk
        gq = np.zeros((num_pos, 8))
        for j in range(4):
            ok = src[:, j] >= 0
            for c in range(2):
                gq[ar[ok], 2 * src[ok, j] + c] = gs[ok, 2 * j + c]
        out["corners"][pos] = gq
        if info is not None:
            info["shifts"] = np.bincount(sh, minlength=3)
            nn = np.abs(d)
            info["quadratic"] = int((nn < beta).sum()) if beta >= 1e-5 else 0
            info["linear"] = int((nn >= beta).sum()) if beta >= 1e-5 else int(nn.size)
            info["dead_slots"] = int((src < 0).sum())
        if has_center:
            tcen = tc.reshape(-1, 4, 2).sum(1) / 4.0
            dc = center_pred[pos].astype(np.float64) - tcen
            out["center"][pos] = _sl1_grad(dc, beta, ls) * (w * (lam["center"] * up[2]))[:, None]
        if has_ctr:
            xc = ctr_pred[pos].astype(np.float64)
            out["ctr"][pos] = (1.0 / (1.0 + np.exp(-xc)) - cw) / num_pos_avg * (lam["ctr"] * up[3])
    return out


# --------------------------------------------------------------------------------------------- the fixture's inputs
SMALL_HW = (128, 160)
SMALL_SEED = 31


def small_grad_case():
    """2 images of 128 x 160 with 9 and 4 boxes -> (gts, shapes, targets, predictions).  The predictions are
    tn.case_b_predictions': targets plus noise in a rolled corner order, so every shift and both smooth-L1 branches occur."""
    rng = np.random.default_rng(SMALL_SEED)
    h, w = SMALL_HW
    gts = [tn.gt_of(tn.random_quads(9, rng, h, w, lo=12.0, hi=100.0), rng.integers(0, 15, 9)),
           tn.gt_of(tn.random_quads(4, rng, h, w, lo=30.0, hi=150.0), rng.integers(0, 15, 4))]
    shapes = tn.level_shapes(h, w)
    tg = tn.assign(gts, shapes, tn.assign_config("released"))
    return gts, shapes, tg, tn.case_b_predictions(tg, seed=SMALL_SEED + 1)


HANDMADE_KINDS = ("all_equal", "collinear", "three_collinear", "xmin_tie", "n_zero", "n_beta")


def handmade_grad_case(num_classes=15):
    """One image, 8 x 8 positions, one positive of each kind of HANDMADE_KINDS at positions 5, 12, 19, 26, 33, 40 -> (targets,
    predictions, {kind: position}).  Meant for handmade_configs()' beta = 0.5, which fp32 and fp64 both hold exactly: "n_beta"
    has components with |x - y| == 0.5 exactly, below it, above it and 0."""
    rng = np.random.default_rng(91)
    P = 64
    where = {k: 5 + 7 * i for i, k in enumerate(HANDMADE_KINDS)}
    labels = np.full(P, num_classes, np.int64)
    for i, k in enumerate(HANDMADE_KINDS):
        labels[where[k]] = (3 * i + 1) % num_classes
    tg = dict(labels=labels, target_inds=np.zeros(P, np.int64), corners=rng.normal(0, 3.0, (P, 8)).astype(f32),
              ltrb=rng.uniform(0.5, 6.0, (P, 4)).astype(f32), abcd=rng.uniform(0.5, 6.0, (P, 4)).astype(f32))
    logits, corners, center, ctr = tn.case_b_predictions(tg, seed=92, num_classes=num_classes)
    corners[where["all_equal"]] = np.tile(np.array([1.5, -0.75], f32), 4)
    corners[where["collinear"]] = np.array([0, 0, 1, 1, 2, 2, 3, 3], f32)
    corners[where["three_collinear"]] = np.array([0, 0, 1, 1, 2, 2, 1, 5], f32)
    corners[where["xmin_tie"]] = np.array([1, 4, 1, 0, 5, 0.5, 4, 5], f32)
    # a prediction equal to its target: a sorted quadrilateral whose sort is the identity, so every component has n = 0
    sq = np.array([0, 1, 1, 4, 4, 2, 2, 0], f32)
    assert np.array_equal(sort_with_sources(sq[None])[1][0], np.arange(4)), "n_zero: pick a quadrilateral the sort leaves alone"
    tg["corners"][where["n_zero"]] = sq
    corners[where["n_zero"]] = sq
    center[where["n_zero"]] = sq.reshape(4, 2).astype(np.float64).sum(0) / 4.0
    # n == beta exactly for beta = 0.5: target components at multiples of 1/4, the prediction 0.5 away (sort = identity)
    sb = np.array([0, 1, 1, 4, 4, 2, 2, 0], f32)
    tg["corners"][where["n_beta"]] = sb
    corners[where["n_beta"]] = sb + np.array([0.5, -0.5, 0.5, 0.25, 0.0, 0.5, -0.5, 1.0], f32)
    assert np.array_equal(sort_with_sources(corners[where["n_beta"]][None])[1][0], np.arange(4))
    center[where["n_beta"]] = (sb.reshape(4, 2).astype(np.float64).sum(0) / 4.0 + np.array([0.5, -0.5])).astype(f32)
    return tg, (logits, corners, center, ctr), where


HANDMADE_BETA = 0.5      # exact in fp32 and fp64: "n == beta" is a statement about the inputs, not about a rounding


def handmade_configs():
    """The handmade cases' configurations: released but beta 0.5, with and without the sort / the modulation / log space."""
    out = []
    for sort in (True, False):
        for mod in (True, False):
            for ls in (True, False):
                out.append(("s%d_m%d_l%d" % (sort, mod, ls), dict(tn.LOSS_RELEASED, beta=HANDMADE_BETA, sort_corners=sort, modulation=mod,
                                                                  logspace=ls)))
    return out


def lam_cls_key(Lc):
    """The logits gradient depends on the configuration only through lambda_cls: one stored tensor per distinct value."""
    return "%.17g" % tn.normalized_lambdas(Lc)["cls"]
