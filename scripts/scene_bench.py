"""Whole-scene inference against tile inference alone, in one process: detect_scenes on --scenes seeded 4000 x 4000 scenes (25
tiles each at 1024 / 200) against detect_packed on the same tiles in batches of --batch (the pipelined step detect_scenes
uses), same R101 DOTA 1.0 model, same warm-up.  Alternates the two --rounds times and prints one JSON line: median tiles/s of
each, their ratio, and the device time of the tile gather launch and of the merge (merge rows + NMS + kept-row gather, host
reads included).

    python scripts/scene_bench.py --scenes 16 --batch 8 --rounds 5 --warmup 2

--tta: scene-level TTA (the config's TEST.AUG views on every tile) -- OneStageRCNNWithTTA.detect_scenes against the route it
replaces on the same tiles: gather_tiles, OneStageRCNNWithTTA over the tiles (default images_per_group), the merged rows,
merge_scenes.  Alternates the two --rounds times (median tiles/s of each, their ratio), and times on the device one batch's
view launches against the gather_tiles + per-view resize_u8 calls they replace.  --out writes the JSON line to a file too.

    python scripts/scene_bench.py --tta --scenes 4 --batch 8 --rounds 5 --warmup 1 --out profiles/scene_tta_bench.json

--score: scoring merged scene detections against scene labels, no detector involved -- synthetic merged results and labelTxt
files of val-like size (--score-scenes scenes of 1000 .. 5000 px, 16 classes, about --score-dets detections and --score-gt
ground-truth boxes, 70 % of both in two dense classes, scene sizes skewed) timed both ways on the same inputs: the file route
(scene.write_task1_merged + evaluation.task1.score_task1) and evaluation.scene_eval (load_scene_labels + score_scenes),
alternating after one untimed warm-up of each, every timing ending in a device synchronise; five repeats of score_scenes,
five of the file route or three if one of them takes more than a minute.  Prints median / min / max of both, whether the two
dicts are equal (as run, and with voc_eval's argsort made stable: the synthetic scores tie), and the time detect_scenes needs for scenes of these sizes (their tile count from split_origins over the
tiles/s recorded in profiles/scene_bench.json).

    python scripts/scene_bench.py --score --out profiles/scene_score_bench.json

--scales 1,0.5: multi-scale whole-scene inference.  (a) the pixels: gather_scaled_tiles(resample="bilinear") on every scene at
0.5 and at 1.5 (one launch) against the two-step device route it replaces for that filter -- dafne_resize_bilinear_u8_hip of
each whole scene, then gather_tiles on the resized scenes --, alternating --rounds times, device time by events: median, min
and max of both (bicubic has no two-step route on the device; its launch is timed alone).  (b) detect_scenes(scales=...)
against detect_packed alone on the same tiles, as in the default mode.

    python scripts/scene_bench.py --scales 1,0.5 --scenes 16 --batch 8 --rounds 5 --warmup 2 --out profiles/scene_scales_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="dota-1.0_r101.yaml")
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tta", action="store_true", help="scene-level TTA against the per-tile TTA route")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    ap.add_argument("--views-per-call", type=int, default=0, help="--tta: views per detector call (0: the library's default)")
    ap.add_argument("--scales", default="", help="multi-scale: comma-separated scales of detect_scenes, e.g. 1,0.5")
    ap.add_argument("--score", action="store_true", help="score_scenes against write_task1_merged + score_task1 on synthetic results")
    ap.add_argument("--score-scenes", type=int, default=400)
    ap.add_argument("--score-dets", type=int, default=200000)
    ap.add_argument("--score-gt", type=int, default=50000)
    args = ap.parse_args()
    if args.score:
        return bench_score(args)
    import torch
    import bench
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd import scene as sc
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model

    dev = torch.device("cuda", 0)
    cfg = load_cfg(os.path.join(ROOT, "configs", args.config))
    m = build_model(cfg)
    m.load_state_dict(bench.seeded_state_dict(m, 0))
    m.to(dev)
    m.invalidate()
    g = torch.Generator().manual_seed(1)
    scenes = []
    for _ in range(args.scenes):
        low = torch.rand(1, 3, args.size // 32, args.size // 32, generator=g)
        img = torch.nn.functional.interpolate(low, size=(args.size, args.size), mode="bilinear", align_corners=False)[0]
        img = (img * 220 + torch.rand(3, args.size, args.size, generator=g) * 12).clamp_(0, 255).to(torch.uint8)
        scenes.append(img.permute(1, 2, 0).contiguous().to(dev))
    origins = [sc.split_origins(args.size, args.size) for _ in scenes]
    info = [(l, u, s) for s, org in enumerate(origins) for l, u in org]
    tiles = sc.gather_tiles(scenes, origins, 1024)
    T = tiles.shape[0]
    splits = max(1, int(cfg.ENGINE.PIPELINE_SPLITS))
    if args.tta:
        return bench_tta(args, cfg, m, scenes, origins, info, tiles)
    if args.scales:
        del tiles
        return bench_scales(args, cfg, m, scenes)

    def tiles_only():
        parts = [m.detect_packed(tiles[b:b + args.batch], layout_hwc=True, pipelined=True, splits=splits)
                 for b in range(0, T, args.batch)]
        torch.cuda.current_stream().wait_stream(m.side_stream)
        torch.cuda.synchronize()
        return parts

    def scene_path():
        r = m.detect_scenes(scenes, batch=args.batch)
        torch.cuda.synchronize()
        return r

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        return time.perf_counter() - t0, out

    for _ in range(args.warmup):
        tiles_only()
        scene_path()
    t_tiles, t_scene = [], []
    for _ in range(args.rounds):
        t_tiles.append(timed(tiles_only)[0])
        dt, res = timed(scene_path)
        t_scene.append(dt)
    # the two new stages on their own: the gather launch (events) and the merge on the tile rows of one tile-only pass
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    gather_ms = []
    for _ in range(5):
        ev[0].record()
        sc.gather_tiles(scenes, origins, 1024)
        ev[1].record()
        torch.cuda.synchronize()
        gather_ms.append(ev[0].elapsed_time(ev[1]))
    parts = tiles_only()
    rows = torch.cat([r for r, _ in parts])
    counts = torch.cat([c for _, c in parts])
    C = int(cfg.MODEL.DAFNE.NUM_CLASSES)
    merge_ms = []
    for _ in range(5):
        dt, _ = timed(lambda: sc.merge_scenes(rows, counts, info, len(scenes), C, sc.skip_mask(cfg), sc.task1_score_mode(cfg)))
        merge_ms.append(dt * 1e3)
    dets, bc, _, m_cap = sc.merge_tile_rows(rows, counts, info, len(scenes), C, sc.skip_mask(cfg), sc.task1_score_mode(cfg))
    rate_tiles = T / statistics.median(t_tiles)
    rate_scene = T / statistics.median(t_scene)
    print(json.dumps({
        "config": args.config, "scenes": args.scenes, "size": args.size, "tiles": int(T), "batch": args.batch, "rounds": args.rounds,
        "tiles_per_s_detect_packed": round(rate_tiles, 1), "tiles_per_s_detect_scenes": round(rate_scene, 1),
        "ratio": round(rate_scene / rate_tiles, 4),
        "gather_ms_median": round(statistics.median(gather_ms), 3), "merge_ms_median": round(statistics.median(merge_ms), 3),
        "tile_rows": int(counts.sum()), "buckets": int(bc.numel()), "m_cap": int(m_cap),
        "merged_detections": int(sum(len(r["scores"]) for r in res)),
        "s_tiles": [round(v, 4) for v in t_tiles], "s_scene": [round(v, 4) for v in t_scene]}))


def bench_scales(args, cfg, m, scenes):
    import torch
    from dafne_amd import scene as sc
    from dafne_amd.data.loader import _to_chw_resized
    scales = tuple(float(v) for v in args.scales.split(","))
    splits = max(1, int(cfg.ENGINE.PIPELINE_SPLITS))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def device_ms(f):
        torch.cuda.synchronize()
        ev[0].record()
        out = f()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), out

    # (a) the pixels of the scaled splits at 0.5 and 1.5, every scene: the fused launch against resize + gather
    pix_scales = (0.5, 1.5)
    pairs = [(img, s) for img in scenes for s in pix_scales]
    sizes = [sc.scaled_size(args.size, args.size, s) for _, s in pairs]
    porg = [sc.split_origins(nh, nw) for nh, nw in sizes]

    def fused(resample):
        return sc.gather_scaled_tiles([p[0] for p in pairs], [p[1] for p in pairs], porg, 1024, resample)

    def two_step():
        resized = [_to_chw_resized(img, nh, nw) for (img, _), (nh, nw) in zip(pairs, sizes)]
        return sc.gather_tiles(resized, porg, 1024, layout_hwc=False)

    same = bool(torch.equal(fused("bilinear"), two_step()))
    ms_fused, ms_two, ms_cubic = [], [], []
    for _ in range(args.rounds):
        ms_fused.append(device_ms(lambda: fused("bilinear"))[0])
        ms_two.append(device_ms(two_step)[0])
        ms_cubic.append(device_ms(lambda: fused("bicubic"))[0])
    torch.cuda.empty_cache()

    # (b) detect_scenes(scales=...) against detect_packed alone on the same tiles
    plan = sc.scale_plan([(args.size, args.size)] * len(scenes), scales)
    parts = []
    for img, per in zip(scenes, plan):
        for s, _, org in per:
            parts.append(sc.gather_tiles([img], [org], 1024) if s == 1.0 else sc.gather_scaled_tiles([img], [s], [org], 1024))
    tiles = torch.cat(parts)
    del parts
    T = int(tiles.shape[0])

    def tiles_only():
        out = [m.detect_packed(tiles[b:b + args.batch], layout_hwc=True, pipelined=True, splits=splits) for b in range(0, T, args.batch)]
        torch.cuda.current_stream().wait_stream(m.side_stream)
        torch.cuda.synchronize()
        return out

    def scene_path():
        r = m.detect_scenes(scenes, batch=args.batch, scales=scales)
        torch.cuda.synchronize()
        return r

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        return time.perf_counter() - t0, out

    for _ in range(args.warmup):
        tiles_only()
        scene_path()
    t_tiles, t_scene = [], []
    for _ in range(args.rounds):
        t_tiles.append(timed(tiles_only)[0])
        dt, res = timed(scene_path)
        t_scene.append(dt)
    stat = lambda v: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}      # noqa: E731
    rate_tiles, rate_scene = T / statistics.median(t_tiles), T / statistics.median(t_scene)
    line = json.dumps({
        "mode": "scales", "config": args.config, "scenes": args.scenes, "size": args.size, "scales": list(scales), "batch": args.batch,
        "rounds": args.rounds, "pixel_scales": list(pix_scales), "pixel_tiles": int(sum(len(o) for o in porg)),
        "fused_bilinear_ms": stat(ms_fused), "resize_then_gather_bilinear_ms": stat(ms_two), "fused_bicubic_ms": stat(ms_cubic),
        "fused_over_two_step": round(statistics.median(ms_fused) / statistics.median(ms_two), 3), "fused_equals_two_step": same,
        "tiles": T, "tiles_per_s_detect_packed": round(rate_tiles, 1), "tiles_per_s_detect_scenes": round(rate_scene, 1),
        "ratio": round(rate_scene / rate_tiles, 4), "merged_detections": int(sum(len(r["scores"]) for r in res)),
        "kept_per_scale": {str(s): int(sum(sum(1 for t in r["tile"].cpu().tolist() if ts[t] == s) for r in res))
                           for ts in [[x for r in res for x in r["tile_scales"]]] for s in scales},
        "ms_fused": [round(v, 3) for v in ms_fused], "ms_two_step": [round(v, 3) for v in ms_two],
        "s_tiles": [round(v, 4) for v in t_tiles], "s_scene": [round(v, 4) for v in t_scene]})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def bench_tta(args, cfg, m, scenes, origins, info, tiles):
    import torch
    from dafne_amd import scene as sc
    from dafne_amd.evaluation.driver import instances_to_rows
    from dafne_amd.modeling.tta import OneStageRCNNWithTTA, resize_u8
    tta = OneStageRCNNWithTTA(cfg, m)
    if args.views_per_call:
        sc._TTA_VIEWS_PER_CALL = args.views_per_call
    T = int(tiles.shape[0])
    C = int(cfg.MODEL.DAFNE.NUM_CLASSES)
    k_cap = m.proposal_generator.dafne_outputs.packed_k_cap()

    def tile_route():                        # today's route: the tiles, per-tile TTA, merged rows, the tile merge
        t = sc.gather_tiles(scenes, origins, 1024)
        outs = tta([{"image": t[i].permute(2, 0, 1), "height": 1024, "width": 1024} for i in range(T)])
        rows, counts = instances_to_rows([o["instances"] for o in outs], k_cap)
        r = sc.merge_scenes(rows, counts, info, len(scenes), C, sc.skip_mask(cfg), sc.task1_score_mode(cfg))
        torch.cuda.synchronize()
        return r

    def scene_route():
        r = tta.detect_scenes(scenes, batch=args.batch)
        torch.cuda.synchronize()
        return r

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        return time.perf_counter() - t0, out

    for _ in range(args.warmup):
        tile_route()
        scene_route()
    t_tile, t_scene = [], []
    for _ in range(args.rounds):
        t_tile.append(timed(tile_route)[0])
        dt, res = timed(scene_route)
        t_scene.append(dt)
    # one batch's pixels: the view launches (one per TTA size) against gather_tiles + one resize_u8 per view
    table = sc.tta_view_table(tta.tta_mapper, 1024, 1024, (1024, 1024))
    b = min(args.batch, T)
    srcs = [(scenes[s], True, left, up, 1024, 1024) for left, up, s in info[:b]]
    runs = sorted(set((t[0], t[1]) for t in table))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    views_ms, resize_ms = [], []
    for _ in range(5):
        ev[0].record()
        for vh, vw in runs:
            sc.scene_views([s + (t[2], t[3]) for s in srcs for t in table if t[:2] == (vh, vw)], vh, vw)
        ev[1].record()
        torch.cuda.synchronize()
        views_ms.append(ev[0].elapsed_time(ev[1]))
        org = [[] for _ in scenes]
        for left, up, s in info[:b]:
            org[s].append((left, up))
        ev[0].record()
        tl = sc.gather_tiles(scenes, org, 1024)
        for i in range(b):
            x = tl[i].permute(2, 0, 1).contiguous()
            for t in table:
                resize_u8(x, t[0], t[1], t[2], t[3])
        ev[1].record()
        torch.cuda.synchronize()
        resize_ms.append(ev[0].elapsed_time(ev[1]))
    rate_tile = T / statistics.median(t_tile)
    rate_scene = T / statistics.median(t_scene)
    line = json.dumps({
        "mode": "tta", "config": args.config, "views_per_call": sc._TTA_VIEWS_PER_CALL, "scenes": args.scenes, "size": args.size, "tiles": T, "views_per_tile": len(table),
        "batch": args.batch, "rounds": args.rounds,
        "tiles_per_s_tile_route": round(rate_tile, 2), "tiles_per_s_detect_scenes_tta": round(rate_scene, 2),
        "ratio": round(rate_scene / rate_tile, 4),
        "batch_views_ms_median": round(statistics.median(views_ms), 3),
        "batch_gather_resize_ms_median": round(statistics.median(resize_ms), 3),
        "merged_detections": int(sum(len(r["scores"]) for r in res)),
        "s_tile_route": [round(v, 4) for v in t_tile], "s_scene": [round(v, 4) for v in t_scene]})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _boxes(rng, n, size, lo, hi):
    """n rotated rectangles inside a size x size scene, [n,8] float64."""
    import numpy as np
    c = rng.uniform(0, size, (n, 2))
    w = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    h = w / rng.uniform(1, 4, n)
    a = rng.uniform(0, np.pi, n)
    ca, sa = np.cos(a), np.sin(a)
    ux = np.stack([w / 2 * ca - h / 2 * sa, -w / 2 * ca - h / 2 * sa, -w / 2 * ca + h / 2 * sa, w / 2 * ca + h / 2 * sa], 1)
    uy = np.stack([w / 2 * sa + h / 2 * ca, -w / 2 * sa + h / 2 * ca, -w / 2 * sa - h / 2 * ca, w / 2 * sa - h / 2 * ca], 1)
    p = np.empty((n, 8))
    p[:, 0::2] = c[:, :1] + ux
    p[:, 1::2] = c[:, 1:] + uy
    return p


def synthetic_val(args, label_dir):
    """Seeded merged results + labelTxt files of val-like size.  -> scene names, class names, scene sizes, per-scene host
    results (corners two decimals, scores four decimals: many equal scores, as real merged files have)."""
    import numpy as np
    from dafne_amd.evaluation import dota_evaluation as de
    rng = np.random.default_rng(7)
    classes = list(de.CLASSNAMES_DOTA_1_0) + ["container-crane"]
    S, C = args.score_scenes, len(classes)
    sizes = rng.choice([1000, 2000, 3000, 4000, 5000], S, p=[0.15, 0.2, 0.25, 0.3, 0.1])
    share = np.full(C, 0.3 / (C - 2))
    share[[4, 5]] = 0.35                                          # small-vehicle, large-vehicle
    weight = rng.lognormal(0.0, 1.2, (S, C)) * share[None, :] * (sizes[:, None] / 4000.0) ** 2     # a few scenes hold most boxes
    n_gt = rng.poisson(weight / weight.sum() * args.score_gt)
    n_fp = rng.poisson(weight / weight.sum() * (args.score_dets - 1.15 * args.score_gt))
    names, results = [], []
    os.makedirs(label_dir, exist_ok=True)
    for s in range(S):
        name = "P%04d" % s
        names.append(name)
        rows = ["imagesource:GoogleEarth", "gsd:0.146"]
        corners, labels = [], []
        for c in range(C):
            lo, hi = (10.0, 40.0) if c in (4, 5) else (20.0, 150.0)
            g = np.round(_boxes(rng, int(n_gt[s, c]), float(sizes[s]), lo, hi), 1)
            diff = rng.uniform(size=len(g)) < 0.1
            rows += [" ".join("%.1f" % v for v in q) + " %s %d" % (classes[c], d) for q, d in zip(g, diff)]
            first = g[rng.uniform(size=len(g)) < 0.85]
            second = g[rng.uniform(size=len(g)) < 0.3]
            d = np.concatenate([first + rng.normal(0, 1.0, first.shape), second + rng.normal(0, 2.0, second.shape),
                                _boxes(rng, int(n_fp[s, c]), float(sizes[s]), lo, hi)])
            corners.append(np.round(d, 2))
            labels.append(np.full(len(d), c, np.int64))
        with open(os.path.join(label_dir, name + ".txt"), "w") as f:
            f.write("\n".join(rows) + "\n")
        corners, labels = np.concatenate(corners), np.concatenate(labels)
        results.append((corners, np.round(rng.uniform(0.05, 1.0, len(labels)), 4), labels))
    return names, classes, sizes, results


def bench_score(args):
    import tempfile
    import types
    import numpy as np
    import torch
    from dafne_amd import scene as sc
    from dafne_amd.evaluation import dota_evaluation as de
    from dafne_amd.evaluation.scene_eval import load_scene_labels, score_scenes
    from dafne_amd.evaluation.task1 import score_task1
    dev = torch.device("cuda", 0)
    cfg = types.SimpleNamespace(TEST=types.SimpleNamespace(IOU_TH=0.5))
    with tempfile.TemporaryDirectory() as tmp:
        label_dir = os.path.join(tmp, "labelTxt")
        names, classes, sizes, host = synthetic_val(args, label_dir)
        res = [{"corners": torch.from_numpy(c).to(dev), "scores": torch.from_numpy(s).to(dev), "labels": torch.from_numpy(l).to(dev)}
               for c, s, l in host]
        n_det = sum(len(l) for _, _, l in host)
        out = os.path.join(tmp, "files")
        os.makedirs(out)
        with open(os.path.join(out, "imageset.txt"), "w") as f:
            f.write("\n".join(names))
        last = {}

        def file_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            merged = os.path.join(out, "Task1_merged")
            sc.write_task1_merged(res, names, classes, merged)
            last["file"] = score_task1(classes, merged, os.path.join(label_dir, "{:s}.txt"), out, de.parse_gt, cfg, {})
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def device_route():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lab = load_scene_labels(label_dir, names, classes)
            t1 = time.perf_counter()
            last["dev"] = score_scenes(res, lab, classes, cfg, output_folder=os.path.join(tmp, "dev"))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            last["labels_s"], last["gt"] = t1 - t0, int(lab["boxes"].shape[0])
            return t2 - t0

        w_file, w_dev = file_route(), device_route()              # untimed warm-up of each
        print("warm-up: file route %.2f s, score_scenes %.3f s" % (w_file, w_dev), flush=True)
        n_file = 3 if w_file > 60.0 else 5
        t_file, t_dev, t_lab = [], [], []
        for r in range(5):
            if r < n_file:
                t_file.append(file_route())
                if t_file[-1] > 60.0:
                    n_file = 3
            t_dev.append(device_route())
            t_lab.append(last["labels_s"])
            print("repeat %d: file route %s s, score_scenes %.3f s" % (r, ("%.2f" % t_file[-1]) if r < len(t_file) else "-", t_dev[-1]),
                  flush=True)
        # equal scores: numpy's unstable argsort may order them differently from the stable order score_scenes defines, so the
        # two dicts are compared once more (untimed) with voc_eval's argsort in its kind="stable" form
        same = list(last["file"].items()) == list(last["dev"]["task1"].items())
        plain = np.argsort
        np.argsort = lambda a, *x, **k: plain(a, kind="stable")
        try:
            stable = score_task1(classes, os.path.join(out, "Task1_merged"), os.path.join(label_dir, "{:s}.txt"), out, de.parse_gt, cfg, {})
        finally:
            np.argsort = plain
        same_stable = list(stable.items()) == list(last["dev"]["task1"].items())
        tiles = int(sum(len(sc.split_origins(int(v), int(v))) for v in sizes))
        with open(os.path.join(ROOT, "profiles", "scene_bench.json")) as f:
            rate = float(json.loads(f.read())["tiles_per_s_detect_scenes"])
        line = json.dumps({
            "scenes": len(names), "classes": len(classes), "detections": n_det, "gt_boxes": last["gt"], "tiles": tiles,
            "file_route_s": {"median": round(statistics.median(t_file), 3), "min": round(min(t_file), 3), "max": round(max(t_file), 3)},
            "score_scenes_s": {"median": round(statistics.median(t_dev), 4), "min": round(min(t_dev), 4), "max": round(max(t_dev), 4)},
            "of_which_load_scene_labels_s_median": round(statistics.median(t_lab), 4),
            "ratio_of_medians": round(statistics.median(t_file) / statistics.median(t_dev), 1),
            "detect_scenes_s_for_these_tiles": round(tiles / rate, 2), "tiles_per_s_detect_scenes_recorded": rate,
            "slowest_score_scenes_faster_than_fastest_file_route": bool(max(t_dev) < min(t_file)),
            "score_scenes_median_below_detect_scenes": bool(statistics.median(t_dev) < tiles / rate),
            "task1_dicts_equal": bool(same), "task1_dicts_equal_with_stable_argsort": bool(same_stable), "map_file_route": last["file"]["map"], "map_score_scenes": last["dev"]["task1"]["map"],
            "s_file_route": [round(v, 3) for v in t_file], "s_score_scenes": [round(v, 4) for v in t_dev]})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
