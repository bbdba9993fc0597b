"""Released head vs the ablation (direct, CENTERNESS none) head through OneStageDetector.detect_packed, in one process,
alternating: same trunk weights, same batch, the pipelined step of bench.py (sub-batches on --splits streams, post-process
enqueued behind each step).  Prints one JSON line with the median img/s of each head over --rounds alternations.

    python scripts/head_ab.py --depth 101 --batch 8 --size 1024 --steps 10 --rounds 6
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=101, choices=[50, 101])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--splits", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="timed steps per model per round")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    models = {}
    sd0 = None
    for name, opts in (("released", []), ("direct_none", ["MODEL.DAFNE.CORNER_PREDICTION", "direct",
                                                          "MODEL.DAFNE.CENTERNESS", "none"])):
        cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r%d.yaml" % args.depth), opts)
        m = build_model(cfg)
        if sd0 is None:
            sd0 = om.make_params(args.depth, cfg.MODEL.DAFNE.NUM_CLASSES, seed=0)
        sd = m.state_dict()
        sd.update({k: v for k, v in sd0.items() if k in sd})       # the direct head's parameters are a subset
        m.load_state_dict(sd)
        m.to(dev)
        m.invalidate()
        models[name] = m
    g = torch.Generator().manual_seed(0)
    batch = torch.randint(0, 256, (args.batch, 3, args.size, args.size), generator=g, dtype=torch.uint8).to(dev)

    def run(m, k):
        for _ in range(k):
            m.detect_packed(batch, pipelined=True, splits=args.splits)
        torch.cuda.synchronize()

    for m in models.values():
        run(m, args.warmup)
    rates = {k: [] for k in models}
    for _ in range(args.rounds):
        for name, m in models.items():
            t0 = time.perf_counter()
            run(m, args.steps)
            rates[name].append(args.batch * args.steps / (time.perf_counter() - t0))
    res = {k: float(np.median(v)) for k, v in rates.items()}
    print(json.dumps({"metric": "img/s median over rounds", "depth": args.depth, "batch": args.batch, "size": args.size,
                      "splits": args.splits, "steps": args.steps, "rounds": args.rounds, **res,
                      "direct_over_released": res["direct_none"] / res["released"],
                      "per_round": {k: [round(x, 1) for x in v] for k, v in rates.items()}}))


if __name__ == "__main__":
    main()
