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
    args = ap.parse_args()
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


if __name__ == "__main__":
    main()
