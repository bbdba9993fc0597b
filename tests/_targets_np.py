"""numpy restatement of the reference's target assignment and losses (dafne/modeling/dafne/dafne_outputs.py:44-731,
dafne/modeling/losses/smooth_l1.py), and the seeded inputs the fixture maker and the tests share.

Assignment: fp32, dense [K, G] per image, every operation in the reference's order (numpy rounds each fp32 operation once and
fuses nothing), so integers and floats are meant to equal torch's on the CPU bit for bit.
Losses: fp64 from the fp32 inputs -- the engine's definition; the reference's fp32 value is one rounding of the same formulas.
Output order everywhere: level first, then image, then location.
"""
import numpy as np

from dafne_amd.data.targets import polygon_area, sort_quadrilateral_np

f32 = np.float32
INF = f32(100000000)
STRIDES = (8, 16, 32, 64, 128)
SOI = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 100000000))

RELEASED = dict(num_classes=15, strides=STRIDES, soi=SOI, center_sample=True, center_sample_only=False, combine=True,
                radius=2.0, in_box_check=True, size_filter=True, stride_norm=True)
ASSIGN_CONFIGS = {
    "released": {},
    "cs_only": {"center_sample_only": True},
    "no_box_check": {"in_box_check": False},
    "no_stride_norm": {"stride_norm": False},
}


def assign_config(name, **over):
    d = dict(RELEASED)
    d.update(ASSIGN_CONFIGS.get(name, {}))
    d.update(over)
    return d


def level_shapes(h, w, strides=STRIDES):
    return [((h + s - 1) // s, (w + s - 1) // s) for s in strides]


def compute_locations(shapes, strides=STRIDES):
    """dafne.py:37-44 per level -> (xs, ys, level) over all locations of one image, fp32."""
    xs, ys, lv = [], [], []
    for l, ((h, w), s) in enumerate(zip(shapes, strides)):
        sx = np.arange(0, w * s, s, dtype=f32) + f32(s // 2)
        sy = np.arange(0, h * s, s, dtype=f32) + f32(s // 2)
        yy, xx = np.meshgrid(sy, sx, indexing="ij")
        xs.append(xx.reshape(-1))
        ys.append(yy.reshape(-1))
        lv.append(np.full(h * w, l, np.int64))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(lv)


def _tri(ax, ay, bx, by, x, y):
    x0, x1, y0, y1 = ax - x, ay - y, bx - x, by - y
    return f32(0.5) * np.abs(x0 * y1 - x1 * y0)


def assign_image(xs, ys, lv, gt, T, stats=None):
    """compute_targets_for_locations for one image.  gt: dict corners [G,8], hbox [G,4], area [G] (fp32), cls [G]."""
    K = xs.shape[0]
    G = gt["cls"].shape[0]
    C = T["num_classes"]
    if G == 0:
        return (np.full(K, C, np.int64), np.full(K, -1, np.int64), np.zeros((K, 8), f32), np.zeros((K, 4), f32),
                np.zeros((K, 4), f32))
    c, b, area = gt["corners"].astype(f32), gt["hbox"].astype(f32), gt["area"].astype(f32)
    X, Y = xs[:, None], ys[:, None]
    with np.errstate(all="ignore"):
        ltrb = np.stack([X - b[None, :, 0], Y - b[None, :, 1], b[None, :, 2] - X, b[None, :, 3] - Y], axis=2)
        abcd = []
        for e in range(4):
            n = (e + 1) % 4
            x1, y1, x2, y2 = c[None, :, 2 * e], c[None, :, 2 * e + 1], c[None, :, 2 * n], c[None, :, 2 * n + 1]
            dy, dx = y2 - y1, x2 - x1
            nom = np.abs(((dy * X - dx * Y) + x2 * y1) - y2 * x1)
            abcd.append(nom / np.sqrt(dy * dy + dx * dx))
        abcd = np.stack(abcd, axis=2)
        cor = np.stack([c[None, :, q] - (X if q % 2 == 0 else Y) for q in range(8)], axis=2)
        if T["center_sample"]:
            cx = (b[:, 0] + b[:, 2]) * f32(0.5)
            cy = (b[:, 1] + b[:, 3]) * f32(0.5)
            if cx[0] == 0:                       # get_sample_region's early return
                in_cs = np.zeros((K, G), bool)
            else:
                rad = np.array([f32(s * T["radius"]) for s in T["strides"]], f32)[lv][:, None]
                xmin, ymin, xmax, ymax = cx[None] - rad, cy[None] - rad, cx[None] + rad, cy[None] + rad
                q0 = np.where(xmin > b[None, :, 0], xmin, b[None, :, 0])
                q1 = np.where(ymin > b[None, :, 1], ymin, b[None, :, 1])
                q2 = np.where(xmax > b[None, :, 2], b[None, :, 2], xmax)
                q3 = np.where(ymax > b[None, :, 3], b[None, :, 3], ymax)
                in_cs = np.stack([X - q0, Y - q1, q2 - X, q3 - Y], -1).min(-1) > 0
        else:
            in_cs = ltrb.min(axis=2) > 0
        s = ((_tri(c[None, :, 0], c[None, :, 1], c[None, :, 2], c[None, :, 3], X, Y)
              + _tri(c[None, :, 2], c[None, :, 3], c[None, :, 4], c[None, :, 5], X, Y))
             + _tri(c[None, :, 4], c[None, :, 5], c[None, :, 6], c[None, :, 7], X, Y)) \
            + _tri(c[None, :, 6], c[None, :, 7], c[None, :, 0], c[None, :, 1], X, Y)
        thr = area[None] + f32(1e-3)
        in_q = ~(s > thr)
        if T["center_sample_only"]:
            in_box = in_cs
        else:
            in_box = (in_cs & in_q) if T["combine"] else in_q
        mx = ltrb.max(axis=2)
        soi = np.array(T["soi"], f32)[lv]
        cared = (mx >= soi[:, [0]]) & (mx <= soi[:, [1]])
        a = np.repeat(area[None], K, axis=0)
        if T["in_box_check"]:
            a[~in_box] = INF
        if T["size_filter"]:
            a[~cared] = INF
    idx = np.argmin(a, axis=1)                   # the first index among equal minima
    amin = a[np.arange(K), idx]
    labels = gt["cls"].astype(np.int64)[idx]
    labels[amin == INF] = C
    if stats is not None:
        pos = amin != INF
        stats["multi"] = stats.get("multi", 0) + int(((a != INF).sum(1) >= 2).sum())
        stats["ties"] = stats.get("ties", 0) + int((pos & ((a == amin[:, None]).sum(1) >= 2)).sum())
        stats["near_eps"] = stats.get("near_eps", 0) + int((np.abs(s.astype(np.float64) - thr.astype(np.float64)) < 1e-2).any(1).sum())
        for l in range(len(T["strides"])):
            stats.setdefault("pos_per_level", [0] * len(T["strides"]))[l] += int((pos & (lv == l)).sum())
    ar = np.arange(K)
    return labels, idx.astype(np.int64), cor[ar, idx], ltrb[ar, idx], abcd[ar, idx]


def assign(gts, shapes, T, stats=None):
    """-> dict labels [P], target_inds [P], corners [P,8], ltrb [P,4], abcd [P,4], level first."""
    xs, ys, lv = compute_locations(shapes, T["strides"])
    per = []
    off = 0
    for gt in gts:
        lab, ind, tc, tl, ta = assign_image(xs, ys, lv, gt, T, stats)
        G = gt["cls"].shape[0]
        if G:
            ind = ind + off
            off += G
        if T["stride_norm"]:
            sd = np.array(T["strides"], f32)[lv][:, None]
            tc, tl, ta = tc / sd, tl / sd, ta / sd
        per.append((lab, ind, tc, tl, ta))
    out = []
    for f in range(5):
        out.append(np.concatenate([np.concatenate([p[f][lv == l] for p in per]) for l in range(len(shapes))]))
    return dict(labels=out[0], target_inds=out[1], corners=out[2].astype(f32), ltrb=out[3].astype(f32), abcd=out[4].astype(f32))


# ------------------------------------------------------------------------------------------------------- losses
LOSS_RELEASED = dict(num_classes=15, alpha=0.25, gamma=2.0, beta=1.0 / 9.0, logspace=True, modulation=True, ctr_mode="oriented",
                     ctr_alpha=3.0, sort_corners=True, has_center_reg=True, lambdas=dict(cls=10.0, corners=1.0, center=1.0, ctr=1.0),
                     lambda_norm=True)


def normalized_lambdas(Lc):
    lam = dict(Lc["lambdas"])
    if Lc.get("lambda_norm", True):
        s = lam["cls"] + lam["corners"]
        if Lc["ctr_mode"] != "none":
            s += lam["ctr"]
        if Lc["has_center_reg"]:
            s += lam["center"]
        lam = {k: v / s for k, v in lam.items()}
    return lam


def ctrness_targets(reg, alpha):
    """The engine's centerness target: the reference's fp32 ratio, raised to float32(1 / alpha) in fp64 (NaN -> 0)."""
    reg = reg.astype(f32)
    with np.errstate(all="ignore"):
        lr_min, lr_max = np.minimum(reg[:, 0], reg[:, 2]), np.maximum(reg[:, 0], reg[:, 2])
        tb_min, tb_max = np.minimum(reg[:, 1], reg[:, 3]), np.maximum(reg[:, 1], reg[:, 3])
        r = (lr_min / lr_max) * (tb_min / tb_max)
        c = np.power(r.astype(np.float64), np.float64(f32(1.0 / alpha)))
    c[np.isnan(c)] = 0.0
    return c


def _bce(x, t):
    return (np.maximum(x, 0.0) - x * t) + np.log1p(np.exp(-np.abs(x)))


def _sl1(n, beta, logspace):
    v = n if beta < 1e-5 else np.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta)
    return np.log1p(v) if logspace else v


def losses(logits, corners_pred, center_pred, ctr_pred, tg, Lc):
    """fp64 loss values.  logits [P,C], corners_pred [P,8] (the finished regression, unsorted), center_pred [P,2] or None,
    ctr_pred [P] or None: fp32; tg: assign()'s dict.  -> dict cls, corners, center, ctr, num_pos, loss_denorm, ctr_targets."""
    C = Lc["num_classes"]
    lam = normalized_lambdas(Lc)
    labels = tg["labels"]
    pos = np.nonzero(labels != C)[0]
    num_pos = len(pos)
    num_pos_avg = max(float(num_pos), 1.0)
    x = logits.astype(np.float64)
    t = np.zeros_like(x)
    t[pos, labels[pos]] = 1.0
    with np.errstate(all="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        ce = _bce(x, t)
        pt = p * t + (1.0 - p) * (1.0 - t)
        v = ce * np.power(1.0 - pt, Lc["gamma"])
        if Lc["alpha"] >= 0:
            v = (Lc["alpha"] * t + (1.0 - Lc["alpha"]) * (1.0 - t)) * v
    out = {"cls": v.sum() / num_pos_avg * lam["cls"], "num_pos": float(num_pos)}
    if Lc["ctr_mode"] == "plain":
        cw = ctrness_targets(tg["ltrb"][pos], Lc["ctr_alpha"])
    elif Lc["ctr_mode"] == "oriented":
        cw = ctrness_targets(tg["abcd"][pos], Lc["ctr_alpha"])
    else:
        cw = np.ones(num_pos, np.float64)
    out["ctr_targets"] = cw
    csum = cw.sum() if num_pos else 0.0
    denorm = max(csum, 1e-6)
    out["loss_denorm"] = denorm
    out["corners"] = out["center"] = out["ctr"] = 0.0
    if num_pos:
        q = corners_pred[pos].astype(f32)
        if Lc["sort_corners"]:
            q = sort_quadrilateral_np(q)
        q = q.astype(np.float64)
        tc = tg["corners"][pos].astype(np.float64)
        beta, ls = Lc["beta"], Lc["logspace"]
        l0 = _sl1(np.abs(q - tc), beta, ls).sum(1)
        if Lc["modulation"]:
            q4 = q.reshape(-1, 4, 2)
            l1 = _sl1(np.abs(q4[:, [1, 2, 3, 0]].reshape(-1, 8) - tc), beta, ls).sum(1)
            l2 = _sl1(np.abs(q4[:, [3, 0, 1, 2]].reshape(-1, 8) - tc), beta, ls).sum(1)
            l0 = np.minimum(np.minimum(l0, l1), l2)
        w = cw if csum > 0 else 1.0
        out["corners"] = (l0 * w).sum() / denorm * lam["corners"]
        if Lc["has_center_reg"]:
            tcen = tc.reshape(-1, 4, 2).sum(1) / 4.0
            le = _sl1(np.abs(center_pred[pos].astype(np.float64) - tcen), beta, ls).sum(1)
            out["center"] = (le * w).sum() / denorm * lam["center"]
        if Lc["ctr_mode"] != "none":
            out["ctr"] = _bce(ctr_pred[pos].astype(np.float64), cw).sum() / num_pos_avg * lam["ctr"]
    return out


# --------------------------------------------------------------------------------------------- seeded inputs
def random_quads(n, rng, h, w, lo=10.0, hi=120.0):
    c = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1)
    long_side = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    bw, bh = long_side, long_side / rng.uniform(1, 4, n)
    a = rng.uniform(0, np.pi, n)
    ca, sa = np.cos(a), np.sin(a)
    ux = np.stack([bw / 2 * ca - bh / 2 * sa, -bw / 2 * ca - bh / 2 * sa, -bw / 2 * ca + bh / 2 * sa, bw / 2 * ca + bh / 2 * sa], 1)
    uy = np.stack([bw / 2 * sa + bh / 2 * ca, -bw / 2 * sa + bh / 2 * ca, -bw / 2 * sa - bh / 2 * ca, bw / 2 * sa - bh / 2 * ca], 1)
    p = np.empty((n, 8))
    p[:, 0::2] = c[:, :1] + ux
    p[:, 1::2] = c[:, 1:] + uy
    return (p + rng.normal(0, 0.5, p.shape)).astype(f32)


def gt_of(corners, classes):
    """The four arrays compute_targets_for_locations reads, from raw corners: sorted corners, hull, shoelace area, class."""
    c = sort_quadrilateral_np(np.asarray(corners, f32).reshape(-1, 8))
    if c.shape[0]:
        hbox = np.stack((c[:, 0::2].min(1), c[:, 1::2].min(1), c[:, 0::2].max(1), c[:, 1::2].max(1)), 1).astype(f32)
    else:
        hbox = np.zeros((0, 4), f32)
    return dict(corners=c, hbox=hbox, area=polygon_area(c), cls=np.asarray(classes, np.int64).reshape(-1))


CASE_A_HW = (256, 320)
CASE_A_SEED = 11


def case_a(seed=CASE_A_SEED):
    """3 images of 256 x 320 with 70, 0 and 5 boxes: an exact duplicate (an area tie), an axis-aligned box whose edges pass
    through locations (the in-quad epsilon), one box larger than 256 px and one smaller than 8 px."""
    rng = np.random.default_rng(seed)
    h, w = CASE_A_HW
    q0 = random_quads(70, rng, h, w)
    q0[3] = [12, 20, 60, 20, 60, 52, 12, 52]          # edges through the stride-8 locations x = 12, y = 20, 52
    q0[7] = q0[3]                                     # the tie
    q0[11] = [-20, -30, 300, -10, 310, 250, -10, 240]  # > 256 px
    q0[12] = [100, 100, 105, 101, 104, 106, 99, 105]   # < 8 px
    q0[13] = [130, 40, 250, 40, 250, 200, 130, 200]    # a 120 x 160 box: levels 2 and 3 care
    q2 = random_quads(5, rng, h, w, lo=40.0, hi=200.0)
    q2[0] = [-40, -40, 330, -40, 330, 280, -40, 280]   # covers the image: the upper levels
    cl0, cl2 = rng.integers(0, 15, 70), rng.integers(0, 15, 5)
    return [gt_of(q0, cl0), gt_of(np.zeros((0, 8), f32), np.zeros(0, np.int64)), gt_of(q2, cl2)], level_shapes(h, w)


def small_case(seed):
    """The seeded small cases of the kernel test: 2 images, 64 x 96 .. 256 x 320, G from {0, 1, 63, 64, 65, 130}."""
    rng = np.random.default_rng(1000 + seed)
    h = int(rng.choice([64, 96, 128, 200, 256]))
    w = int(rng.choice([96, 128, 160, 250, 320]))
    Gs = [(0, 1, 63, 64, 65, 130)[(seed + k) % 6] for k in range(2)]
    gts = []
    for G in Gs:
        q = random_quads(G, rng, h, w, lo=6.0, hi=300.0)
        if G >= 2 and seed % 2:
            q[G - 1] = q[0]
        if G >= 1 and seed % 3 == 0:
            q[0] = np.round(q[0] / 8) * 8 + 4
        gts.append(gt_of(q, rng.integers(0, 15, G)))
    T = assign_config("released", center_sample=bool(seed % 5 != 4), center_sample_only=bool(seed % 7 == 3),
                      combine=bool(seed % 4 != 2), radius=(2.0, 1.5, 1.0)[seed % 3], in_box_check=bool(seed % 6 != 5),
                      size_filter=bool(seed % 8 != 7), stride_norm=bool(seed % 2 == 0))
    return gts, level_shapes(h, w), T


def case_b_predictions(tg, seed, num_classes=15):
    """Head outputs from a seed, flat in the targets' order: logits [P,C], corners [P,8], center [P,2], ctr [P], fp32.  The
    regressions are the targets plus noise so that every branch of the smooth L1 is taken."""
    rng = np.random.default_rng(seed)
    P = tg["labels"].shape[0]
    logits = rng.normal(-3.0, 2.0, (P, num_classes)).astype(f32)
    noise = rng.normal(0, 1.0, (P, 8)) * rng.choice([0.01, 0.1, 1.0, 4.0], (P, 1))
    corners = (tg["corners"].astype(np.float64) + noise).astype(f32)
    roll = rng.integers(0, 4, P)                       # some predictions arrive in a shifted corner order
    corners = np.stack([np.roll(corners[i].reshape(4, 2), roll[i], axis=0).reshape(8) for i in range(P)]).astype(f32)
    center = (tg["corners"].astype(np.float64).reshape(P, 4, 2).mean(1) + rng.normal(0, 0.5, (P, 2))).astype(f32)
    ctr = rng.normal(0, 2.0, P).astype(f32)
    return logits, corners, center, ctr


def loss_configs():
    """Case B's configurations: {center-to-corner, direct} x centerness x modulation x logspace, at beta 1/9 and 0."""
    out = []
    for c2c in (True, False):
        for mode in ("oriented", "plain", "none"):
            for mod in (True, False):
                for ls in (True, False):
                    for beta in (1.0 / 9.0, 0.0):
                        name = "%s_%s_m%d_l%d_b%d" % ("c2c" if c2c else "direct", mode, mod, ls, int(beta > 0))
                        d = dict(LOSS_RELEASED, has_center_reg=c2c, ctr_mode=mode, modulation=mod, logspace=ls, beta=beta)
                        out.append((name, d))
    return out


def handmade_targets(kind, num_classes=15):
    """64 positions, 6 positives.  kind "zero_ctr": every positive sits on an edge (centerness target 0: the weights are
    ignored and loss_denorm is 1e-6); "nan_ctr": one positive has a 0 / 0 ratio (NaN -> 0) among ordinary ones."""
    rng = np.random.default_rng(77)
    P = 64
    labels = np.full(P, num_classes, np.int64)
    pos = np.array([3, 10, 11, 30, 47, 63])
    labels[pos] = rng.integers(0, num_classes, len(pos))
    abcd = rng.uniform(0.5, 6.0, (P, 4)).astype(f32)
    ltrb = rng.uniform(0.5, 6.0, (P, 4)).astype(f32)
    if kind == "zero_ctr":
        abcd[pos, 0] = 0.0
        ltrb[pos, 1] = 0.0
    else:
        abcd[pos[2]] = [0.0, 1.0, 0.0, 2.0]
        ltrb[pos[2]] = [1.0, 0.0, 2.0, 0.0]
    return dict(labels=labels, target_inds=np.zeros(P, np.int64), corners=rng.normal(0, 3.0, (P, 8)).astype(f32), ltrb=ltrb,
                abcd=abcd)


def split_levels(flat, n_images, shapes):
    """[P, ch] in level-first order -> per-level NHWC arrays [N, H, W, ch]."""
    out, off = [], 0
    for h, w in shapes:
        n = n_images * h * w
        out.append(flat[off:off + n].reshape(n_images, h, w, -1))
        off += n
    return out
