"""Times the training views (dafne_amd/data/train_views.py) on the MI355X.

    python scripts/train_views_bench.py [--iters 30] [--rounds 5] [--seed 0]

Pixels: 8 views of 1024 x 1024 windows of a 4000 x 4000 scene with the sizes and angles of the reference's
configs/pre-trained/dota-1.0_r101_ms.yaml (INPUT.MIN_SIZE_TRAIN 450 .. 1200, MAX_SIZE_TRAIN 1200, quarter turns), drawn from --seed.
  one launch     augment_views: dafne_train_views_u8_hip into a preallocated slab
  composed       what the code before this kernel offers: dafne_scene_views_u8_hip per distinct size (flips in its store), then
                 torch.rot90(...).contiguous() per view and a copy into a zeroed slab
Ground truth: 8 x 100 objects -- dafne_train_gt_hip against the host route (numpy transform, make_gt_instances, upload).
Each figure is the median over --rounds alternations of the two routes (min - max in brackets); a round is --iters calls between
two device events after a warm-up of every shape.  The two pixel routes are compared byte for byte before anything is timed.
One JSON line.  No GPU: it fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MS_SIZES = [450, 500, 600, 700, 800, 900, 1000, 1100, 1200]        # dota-1.0_r101_ms.yaml INPUT.MIN_SIZE_TRAIN
MS_MAX = 1200


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def host_timed(fn, iters):
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def summary(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_views_bench.py needs an MI355X")
    from dafne_amd.config import get_cfg
    from dafne_amd.data.targets import make_gt_instances
    from dafne_amd.data.train_views import TrainAugmentation, augment_views, train_gt
    from dafne_amd.scene import scene_views
    dev = torch.device("cuda", 0)
    cfg = get_cfg()
    cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING = list(MS_SIZES), MS_MAX, "choice"
    cfg.INPUT.ROTATION_AUG_ANGLES = [0.0, 90.0, 180.0, 270.0]
    aug = TrainAugmentation(cfg)
    rng = np.random.default_rng(args.seed)
    n, patch = 8, 1024
    scene = torch.randint(0, 256, (4000, 4000, 3), generator=torch.Generator().manual_seed(args.seed), dtype=torch.uint8).to(dev)
    origins = [(824 * (k % 4), 824 * (k // 4)) for k in range(n)]
    windows = [(l, u, patch, patch) for l, u in origins]
    params = aug.sample([(patch, patch)] * n, rng)
    cap = (max(p.out_hw()[0] for p in params) + 31) // 32 * 32, (max(p.out_hw()[1] for p in params) + 31) // 32 * 32
    slab = torch.empty((n, 3) + cap, dtype=torch.uint8, device=dev)

    def one_launch():
        return augment_views([(scene, True)] * n, windows, params, cap_hw=cap, out=slab)

    groups = {}
    for k, p in enumerate(params):
        groups.setdefault((p.new_h, p.new_w), []).append(k)
    slab2 = torch.empty_like(slab)

    def composed():
        slab2.zero_()
        for (nh, nw), ks in groups.items():
            x = scene_views([(scene, True) + windows[k] + (params[k].hflip, params[k].vflip) for k in ks], nh, nw)
            for i, k in enumerate(ks):
                y = torch.rot90(x[i], params[k].rot, dims=(1, 2)).contiguous()
                slab2[k, :, :y.shape[1], :y.shape[2]] = y
        return slab2

    one_launch()
    composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(slab, slab2))          # (flip before / after the resize: equal bytes in every trial so far)

    # ground truth: 8 x 100 objects
    rs = np.random.RandomState(args.seed)
    per = 100
    c = rs.uniform(60, patch - 60, size=(n * per, 1, 2))
    th = rs.uniform(0, np.pi, size=(n * per, 1))
    a, b = rs.uniform(8, 50, size=(n * per, 1)), rs.uniform(4, 25, size=(n * per, 1))
    u = np.stack([np.cos(th), np.sin(th)], 2) * a[:, :, None]
    w = np.stack([-np.sin(th), np.cos(th)], 2) * b[:, :, None]
    corners = np.concatenate([c - u - w, c + u - w, c + u + w, c - u + w], 1).reshape(n * per, 8).astype(np.float32)
    classes = rs.randint(0, 15, size=n * per).astype(np.int32)
    off = (np.arange(n + 1) * per).astype(np.int32)
    d_corners, d_classes, d_off = (torch.from_numpy(x).to(dev) for x in (corners, classes, off))

    def gt_device():
        return train_gt(windows, params, d_corners, d_classes, d_off, sort=True, device=dev)

    def gt_host():
        out = []
        for v, p in enumerate(params):
            q = corners[v * per:(v + 1) * per].astype(np.float64).reshape(-1, 4, 2)
            x, y = q[:, :, 0], q[:, :, 1]
            x = patch - x if p.hflip else x
            y = patch - y if p.vflip else y
            x, y = x * (p.new_w / patch), y * (p.new_h / patch)
            if p.rot == 1:
                x, y = y, p.new_w - x
            elif p.rot == 2:
                x, y = p.new_w - x, p.new_h - y
            elif p.rot == 3:
                x, y = p.new_h - y, x
            inst = make_gt_instances(np.stack((x, y), 2).reshape(-1, 8), classes[v * per:(v + 1) * per], p.out_hw(), sort=True)
            out.append((inst.gt_corners.to(dev), inst.gt_boxes.tensor.to(dev), inst.gt_corners_area.to(dev), inst.gt_classes.to(dev)))
        return out

    gt_device()
    gt_host()
    torch.cuda.synchronize()
    t = {"one_launch": [], "composed": [], "gt_device": [], "gt_host": []}
    for _ in range(args.rounds):
        t["one_launch"].append(timed(one_launch, args.iters))
        t["composed"].append(timed(composed, args.iters))
        t["gt_device"].append(host_timed(gt_device, args.iters))
        t["gt_host"].append(host_timed(gt_host, args.iters))
    out = {"views": n, "window": patch, "scene": 4000, "seed": args.seed, "iters": args.iters, "rounds": args.rounds,
           "params": [p.astuple() for p in params], "slab": list(cap), "routes_equal_bytes": same,
           "pixels": {k: summary(t[k]) for k in ("one_launch", "composed")},
           "gt_800_objects": {k: summary(t[k]) for k in ("gt_device", "gt_host")}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
