"""Times of the target-assignment and loss kernels at the workload's shape (batch 8, 1024 x 1024, about 100 boxes per image),
next to a plain torch-on-GPU transcription of the reference's dense formulation (a dozen [K, G] tensors per image, fp32
losses): profiles/NOTES_targets.md.

    python scripts/targets_bench.py [--batch 8] [--size 1024] [--boxes 100] [--iters 200] [--out FILE]
    python scripts/targets_bench.py --backward [--iters 50] [--out FILE]

Device events around `iters` back-to-back calls after a warm-up; the two assignments are compared (labels and indices equal)
at the timed size before anything is timed.

--backward: forward + backward of the losses.  The device path (dafne_losses_hip + dafne_losses_backward_hip on NHWC levels and
assigned targets) against torch autograd on dense_losses, on the same device inputs with the same targets; the two alternate
within one call, five times after a warm-up of each, at the workload's shape and at batch 2 x 512 x 512; medians with min - max.
Also timed, for information: DAFNeOutputs.losses() on NCHW leaves + .backward(), which adds the assignment and the layout copies.

    python scripts/targets_bench.py --tail [--iters 50] [--out FILE]

--tail: dafne_pred_dgrad_gn_hip (the data gradient of a prediction convolution through the last GroupNorm of its tower) for the
three prediction layers (Cout 15, 9, 2) at the workload's pyramid, against torch autograd on the dense formulation on the same
device (group_norm -> relu -> conv2d in fp32 NCHW: forward + backward, and the forward alone so that the backward's share can
be read off) and against the bytes of the kernel's two-pass scheme (2176 per pixel): profiles/NOTES_head_tail.md.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dafne_amd import postprocess as pp  # noqa: E402
from dafne_amd.config import get_cfg  # noqa: E402
from dafne_amd.data.targets import make_gt_instances  # noqa: E402
from dafne_amd.modeling.dafne.dafne_outputs import DAFNeOutputs  # noqa: E402

STRIDES = (8, 16, 32, 64, 128)
INF = 100000000.0


def random_boxes(n, rng, size):
    c = rng.uniform(0, size, (n, 2))
    long_side = np.exp(rng.uniform(np.log(12.0), np.log(400.0), n))
    w, h = long_side, long_side / rng.uniform(1, 5, n)
    a = rng.uniform(0, np.pi, n)
    ca, sa = np.cos(a), np.sin(a)
    ux = np.stack([w / 2 * ca - h / 2 * sa, -w / 2 * ca - h / 2 * sa, -w / 2 * ca + h / 2 * sa, w / 2 * ca + h / 2 * sa], 1)
    uy = np.stack([w / 2 * sa + h / 2 * ca, -w / 2 * sa + h / 2 * ca, -w / 2 * sa - h / 2 * ca, w / 2 * sa - h / 2 * ca], 1)
    p = np.empty((n, 8))
    p[:, 0::2], p[:, 1::2] = c[:, :1] + ux, c[:, 1:] + uy
    return p.astype(np.float32)


# ---- the dense formulation in plain torch (what the reference's compute_targets_for_locations / dafne_losses do, op by op)
def dense_assign(outs, xs, ys, lv, gts):
    K = xs.shape[0]
    X, Y = xs[:, None], ys[:, None]
    rad = torch.tensor([s * outs.radius for s in outs.strides], device=xs.device)[lv][:, None]
    soi = torch.tensor(outs.sizes_of_interest, dtype=torch.float32, device=xs.device)[lv]
    res, off = [], 0
    for g in gts:
        c, b, area, cls = g
        G = cls.shape[0]
        ltrb = torch.stack([X - b[None, :, 0], Y - b[None, :, 1], b[None, :, 2] - X, b[None, :, 3] - Y], 2)
        abcd = []
        for e in range(4):
            n = (e + 1) % 4
            x1, y1, x2, y2 = c[None, :, 2 * e], c[None, :, 2 * e + 1], c[None, :, 2 * n], c[None, :, 2 * n + 1]
            abcd.append(torch.abs((y2 - y1) * X - (x2 - x1) * Y + x2 * y1 - y2 * x1) / torch.sqrt((y2 - y1) ** 2 + (x2 - x1) ** 2))
        abcd = torch.stack(abcd, 2)
        cor = torch.stack([c[None, :, q] - (X if q % 2 == 0 else Y) for q in range(8)], 2)
        cx, cy = (b[:, 0] + b[:, 2]) * 0.5, (b[:, 1] + b[:, 3]) * 0.5
        q0 = torch.maximum(cx[None] - rad, b[None, :, 0])
        q1 = torch.maximum(cy[None] - rad, b[None, :, 1])
        q2 = torch.minimum(cx[None] + rad, b[None, :, 2])
        q3 = torch.minimum(cy[None] + rad, b[None, :, 3])
        in_cs = torch.stack([X - q0, Y - q1, q2 - X, q3 - Y], -1).min(-1)[0] > 0

        def tri(i, j):
            ax, ay, bx, by = c[None, :, 2 * i] - X, c[None, :, 2 * i + 1] - Y, c[None, :, 2 * j] - X, c[None, :, 2 * j + 1] - Y
            return 0.5 * torch.abs(ax * by - ay * bx)
        in_q = ~((tri(0, 1) + tri(1, 2) + tri(2, 3) + tri(3, 0)) > (area[None] + 1e-3))
        mx = ltrb.max(2)[0]
        cared = (mx >= soi[:, [0]]) & (mx <= soi[:, [1]])
        a = area[None].repeat(K, 1)
        a[~(in_cs & in_q)] = INF
        a[~cared] = INF
        amin, idx = a.min(1)
        ar = torch.arange(K, device=xs.device)
        lab = cls[idx].clone()
        lab[amin == INF] = outs.num_classes
        sd = torch.tensor(outs.strides, dtype=torch.float32, device=xs.device)[lv][:, None]
        res.append((lab, idx + off, cor[ar, idx] / sd, ltrb[ar, idx] / sd, abcd[ar, idx] / sd))
        off += G
    return res


def level_first(per, lv, n_levels):
    return [torch.cat([torch.cat([p[f][lv == l] for p in per]) for l in range(n_levels)]) for f in range(5)]


def sort_quadrilateral_torch(b):
    """sort_quadrilateral in differentiable torch ops (gathers and selects), for the autograd baseline of --backward: the same
    selection as dafne_amd.data.targets.sort_quadrilateral_np, zeros where no candidate has l * r < 0."""
    n = b.shape[0]
    S = b.view(n, 4, 2)
    ar = torch.arange(n, device=b.device)
    k1 = S[:, :, 0].argmin(1)
    p1 = S[ar, k1]
    j = torch.arange(3, device=b.device)[None]
    R = S[ar[:, None], j + (j >= k1[:, None])]
    d = R - p1[:, None]
    cross = lambda u, v: u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]  # noqa: E731
    c = torch.stack([cross(d[:, 0], d[:, 1]) * cross(d[:, 0], d[:, 2]), cross(d[:, 1], d[:, 0]) * cross(d[:, 1], d[:, 2]),
                     cross(d[:, 2], d[:, 0]) * cross(d[:, 2], d[:, 1])], 1) < 0
    found = c.any(1)[:, None]
    i = c.int().argmax(1)
    i2 = torch.tensor([1, 0, 0], device=b.device)[i]
    i3 = torch.tensor([2, 2, 1], device=b.device)[i]
    zero = torch.zeros_like(p1)
    p3, A, B = torch.where(found, R[ar, i], zero), torch.where(found, R[ar, i2], zero), torch.where(found, R[ar, i3], zero)
    e = p3 - p1
    swap = (~(cross(e, A - p1) > 0) & (cross(e, B - p1) > 0))[:, None]
    return torch.stack((p1, torch.where(swap, B, A), p3, torch.where(swap, A, B)), 1).view(n, 8)


def dense_losses(outs, logits, corners, center, ctr, tg, sort=pp.sort_quadrilateral):
    lab, _, tc, _, ta = tg
    C = outs.num_classes
    pos = torch.nonzero(lab != C).squeeze(1)
    num_pos = max(pos.numel(), 1.0)
    t = torch.zeros_like(logits)
    t[pos, lab[pos]] = 1
    p = torch.sigmoid(logits)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(logits, t, reduction="none")
    pt = p * t + (1 - p) * (1 - t)
    a = outs.focal_loss_alpha
    cls = ((a * t + (1 - a) * (1 - t)) * ce * (1 - pt) ** outs.focal_loss_gamma).sum() / num_pos
    r = ta[pos]
    lr, tb = r[:, [0, 2]], r[:, [1, 3]]
    cw = ((lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0])) ** (1 / outs.centerness_alpha)
    cw[torch.isnan(cw)] = 0
    denorm = max(float(cw.sum()), 1e-6)          # the reference's .item()
    beta = outs.loss_beta

    def sl1(x, y):
        n = torch.abs(x - y)
        return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).log1p()
    q = sort(corners[pos])
    q4 = q.view(-1, 4, 2)
    l0 = sl1(q, tc[pos]).sum(1)
    l1 = sl1(q4[:, [1, 2, 3, 0]].reshape(-1, 8), tc[pos]).sum(1)
    l2 = sl1(q4[:, [3, 0, 1, 2]].reshape(-1, 8), tc[pos]).sum(1)
    cor = (torch.stack((l0, l1, l2), -1).min(-1)[0] * cw).sum() / denorm
    cen = (sl1(center[pos], tc[pos].view(-1, 4, 2).mean(1)) * cw[:, None]).sum() / denorm
    cl = torch.nn.functional.binary_cross_entropy_with_logits(ctr[pos], cw, reduction="sum") / num_pos
    return torch.stack([cls * outs.lambda_cls, cor * outs.lambda_corners, cen * outs.lambda_center, cl * outs.lambda_ctr])


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # microseconds per call


def setup(outs, n, size, boxes, dev, seed=0):
    """Boxes on the device, NHWC head outputs, level shapes."""
    rng = np.random.default_rng(seed)
    C = outs.num_classes
    shapes = [((size + s - 1) // s, (size + s - 1) // s) for s in STRIDES]
    insts = [make_gt_instances(random_boxes(boxes, rng, size), rng.integers(0, C, boxes), (size, size)) for _ in range(n)]
    for g in insts:                                   # the boxes live on the device, as a training loop would hold them
        g.gt_corners, g.gt_corners_area, g.gt_classes = g.gt_corners.to(dev), g.gt_corners_area.to(dev), g.gt_classes.to(dev)
        g.gt_boxes.tensor = g.gt_boxes.tensor.to(dev)
    levels = []
    gen = torch.Generator(device=dev).manual_seed(seed)
    for (h, w), s in zip(shapes, STRIDES):
        rnd = lambda ch, m, sd: torch.randn(n, h, w, ch, device=dev, generator=gen) * sd + m  # noqa: E731
        levels.append(pp.LevelInput(rnd(C, -3.0, 2.0), rnd(8, 0.0, 1.5), rnd(2, 0.0, 0.5), rnd(1, 0.0, 2.0), s, 1.0))
    return shapes, insts, levels


def backward_bench(outs, n, size, boxes, iters, dev):
    from dafne_amd.modeling.dafne import loss_function as lf
    C = outs.num_classes
    shapes, insts, levels = setup(outs, n, size, boxes, dev)
    tg = outs.assign_targets(shapes, insts, dev)
    # dense_losses reads the targets the kernel assigned: the same labels, corner and abcd targets for both paths
    dense_tg = (tg.labels.long(), None, tg.corners, None, tg.abcd)
    flat = lambda k, ch: torch.cat([getattr(l, k).reshape(-1, ch) for l in levels])  # noqa: E731
    leaves = [flat("logits", C), flat("delta", 8), flat("center", 2), flat("ctrness", 1)[:, 0].contiguous()]
    leaves = [t.clone().requires_grad_(True) for t in leaves]
    up = torch.ones(4, dtype=torch.float64, device=dev)

    def device_path():
        call = {}
        outs.dafne_losses_packed(levels, tg, cooked=True, _call=call)
        grads = [(torch.empty_like(lv.logits), torch.empty_like(lv.delta), torch.empty_like(lv.center), torch.empty_like(lv.ctrness))
                 for lv in levels]
        lf._backward_call(call, levels, tg, up, grads)
        return grads

    def dense_path():
        for t in leaves:
            t.grad = None
        dense_losses(outs, leaves[0], leaves[1], leaves[2], leaves[3], dense_tg, sort=sort_quadrilateral_torch).sum().backward()

    nchw = [[getattr(lv, k).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for lv in levels]
            for k in ("logits", "delta", "center", "ctrness")]

    def module_path():
        for ts in nchw:
            for t in ts:
                t.grad = None
        _, ls = outs.losses(nchw[0], nchw[1], nchw[2], None, nchw[3], None, insts)
        sum(ls.values()).backward()

    # the two gradients agree (fp64 kernel against fp32 autograd: a loose comparison, the tests hold the tight one)
    g = device_path()
    dense_path()
    torch.cuda.synchronize()
    gl = torch.cat([x[0].reshape(-1, C) for x in g])
    gc = torch.cat([x[1].reshape(-1, 8) for x in g])
    agree = {"logits_max_abs_diff": float((gl - leaves[0].grad).abs().max()), "logits_max_abs": float(gl.abs().max()),
             "corners_max_abs_diff": float((gc - leaves[1].grad).abs().max()), "corners_max_abs": float(gc.abs().max())}
    t_dev, t_dense = [], []
    for _ in range(5):
        t_dev.append(timed(device_path, iters, warmup=5))
        t_dense.append(timed(dense_path, max(5, iters // 4), warmup=3))
    t_mod = timed(module_path, iters, warmup=5)
    stat = lambda v: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))}  # noqa: E731
    return {"batch": n, "size": size, "boxes_per_image": boxes, "positions": int(tg.P), "agreement": agree,
            "device_fwd_bwd": stat(t_dev), "dense_torch_fwd_bwd": stat(t_dense), "losses_module_fwd_bwd_us": t_mod, "iters": iters}


def tail_bench(n, size, iters, dev):
    import ctypes
    import types
    from dafne_amd import _lib, engine
    from dafne_amd.modeling.dafne.tail_backward import pred_dgrad_gn
    C = 256
    shapes = [((size + s - 1) // s, (size + s - 1) // s) for s in STRIDES]
    pixels = n * sum(h * w for h, w in shapes)
    gen = torch.Generator(device=dev).manual_seed(0)
    raws, stats = [], []
    for h, w in shapes:
        x = (torch.randn(n, h, w, C, device=dev, generator=gen) + 0.3).to(torch.bfloat16)
        m = torch.zeros(n, h + 2, w + 2, C, dtype=torch.bfloat16, device=dev)
        m[:, 1:-1, 1:-1] = x
        raws.append(m)
        xg = x.float().reshape(n, h * w, C // 8, 8)
        stats.append(torch.stack((xg.mean((1, 3)), 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + 1e-5)), -1))
    stats = torch.stack(stats).contiguous()                     # [levels, n, 32, 2]
    gamma = torch.rand(C, device=dev, generator=gen) + 0.5
    beta = torch.randn(C, device=dev, generator=gen) * 0.3
    res = {"batch": n, "size": size, "pixels": pixels, "bytes_per_pixel": 2176, "iters": iters, "layers": {}}
    for name, cout in (("cls_logits", 15), ("corners_ctrness", 9), ("center_pred", 2)):
        W = (torch.randn(cout, C, 3, 3, generator=torch.Generator().manual_seed(cout)) * 0.05).to(torch.bfloat16).float()
        wp = engine.pack_conv(W, None, dev)[0]
        prm = _lib.ConvParams(n, len(raws), C, cout, 3, 3, 1, 1, 8 | 32, None, None, None, stats.data_ptr(), gamma.data_ptr(),
                              beta.data_ptr(), None, None, 0.0)
        segs = (_lib.ConvSeg * len(raws))()
        for i, (m, (h, w)) in enumerate(zip(raws, shapes)):
            segs[i] = _lib.ConvSeg(m.data_ptr(), None, None, h, w, h, w)
        call = types.SimpleNamespace(prm=prm, segs=segs)
        gs = [torch.randn(n, h, w, cout, device=dev, generator=gen) * 1e-3 for h, w in shapes]
        # the dense formulation: fp32 NCHW leaves, the parameters shared by the levels
        xs = [m[:, 1:-1, 1:-1].float().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for m in raws]
        gn = [g.permute(0, 3, 1, 2).contiguous() for g in gs]
        ga, be, Wd = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True), W.to(dev)

        def dense_forward():
            return [torch.nn.functional.conv2d(torch.relu(torch.nn.functional.group_norm(x, 32, ga, be, 1e-5)), Wd, padding=1) for x in xs]

        def dense_path():
            for t in xs + [ga, be]:
                t.grad = None
            torch.autograd.backward(dense_forward(), gn)

        def dense_forward_only():
            with torch.no_grad():
                dense_forward()
        gx, dgamma, dbeta, _ = pred_dgrad_gn(call, wp, gs)
        dense_path()
        torch.cuda.synchronize()
        agree = {"gx_max_abs_diff": max(float((a - x.grad.permute(0, 2, 3, 1)).abs().max()) for a, x in zip(gx, xs)),
                 "gx_max_abs": max(float(a.abs().max()) for a in gx),
                 "dgamma_max_abs_diff": float((dgamma - ga.grad).abs().max()), "dgamma_max_abs": float(dgamma.abs().max()),
                 "dbeta_max_abs_diff": float((dbeta - be.grad).abs().max()), "dbeta_max_abs": float(dbeta.abs().max())}
        t_dev, t_dense, t_fwd = [], [], []
        for _ in range(5):
            t_dev.append(timed(lambda: pred_dgrad_gn(call, wp, gs), iters, warmup=5))
            t_dense.append(timed(dense_path, max(5, iters // 4), warmup=3))
            t_fwd.append(timed(dense_forward_only, max(5, iters // 4), warmup=3))
        stat = lambda v: {"median_us": float(np.median(v)), "min_us": float(min(v)), "max_us": float(max(v))}  # noqa: E731
        d = stat(t_dev)
        res["layers"][name] = {"cout": cout, "agreement_fp32_autograd": agree, "device": d, "dense_torch_fwd_bwd": stat(t_dense),
                               "dense_torch_fwd": stat(t_fwd), "scheme_gbytes_per_s": pixels * 2176 / d["median_us"] / 1e3}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--backward", action="store_true", help="forward + backward of the losses against torch autograd")
    ap.add_argument("--tail", action="store_true", help="the head-tail data gradient against torch autograd and its byte count")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("targets_bench.py needs an MI355X: a time from a CPU says nothing")
    dev = torch.device("cuda", 0)
    if args.tail:
        line = json.dumps({"tail": tail_bench(args.batch, args.size, args.iters, dev)})
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    cfg = get_cfg()
    outs = DAFNeOutputs(cfg)
    if args.backward:
        res = {"backward": [backward_bench(outs, args.batch, args.size, args.boxes, args.iters, dev),
                            backward_bench(outs, 2, 512, args.boxes, args.iters, dev)]}
        line = json.dumps(res)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    n, C = args.batch, outs.num_classes
    shapes, insts, levels = setup(outs, n, args.size, args.boxes, dev)
    tg = outs.assign_targets(shapes, insts, dev)
    # the dense formulation on the same inputs
    from dafne_amd.modeling.dafne.dafne import compute_locations
    locs = [compute_locations(h, w, s, dev) for (h, w), s in zip(shapes, STRIDES)]
    xs, ys = torch.cat([l[:, 0] for l in locs]), torch.cat([l[:, 1] for l in locs])
    lv = torch.cat([torch.full((l.shape[0],), i, device=dev) for i, l in enumerate(locs)])
    gts = [(g.gt_corners, g.gt_boxes.tensor, g.gt_corners_area, g.gt_classes) for g in insts]
    dense = level_first(dense_assign(outs, xs, ys, lv, gts), lv, len(shapes))
    torch.cuda.synchronize()
    same_labels = bool(torch.equal(dense[0].to(torch.int32), tg.labels))
    same_inds = bool(torch.equal(dense[1].to(torch.int32), tg.target_inds))
    flat = lambda k, ch: torch.cat([getattr(l, k).reshape(-1, ch) for l in levels])  # noqa: E731
    logits, corners, center, ctr = flat("logits", C), flat("delta", 8), flat("center", 2), flat("ctrness", 1)[:, 0]
    extras, _ = outs.dafne_losses_packed(levels, tg, cooked=True)
    ref = dense_losses(outs, logits, corners, center, ctr, dense)
    torch.cuda.synchronize()
    k64 = extras["values_f64"][:4].cpu().numpy()
    res = {
        "shape": {"batch": n, "size": args.size, "boxes_per_image": args.boxes, "locations_per_image": int(xs.shape[0]),
                  "positives": float(extras["values_f64"][4])},
        "labels_equal": same_labels, "target_inds_equal": same_inds,
        "loss_kernel_fp64": k64.tolist(), "loss_dense_fp32": ref.cpu().tolist(),
        "assign_call_us": timed(lambda: outs.assign_targets(shapes, insts, dev), args.iters),
        "loss_call_us": timed(lambda: outs.dafne_losses_packed(levels, tg, cooked=True), args.iters),
        "assign_dense_torch_us": timed(lambda: dense_assign(outs, xs, ys, lv, gts), max(5, args.iters // 20), warmup=3),
        "loss_dense_torch_us": timed(lambda: dense_losses(outs, logits, corners, center, ctr, dense), max(5, args.iters // 4), warmup=3),
        "iters": args.iters,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
