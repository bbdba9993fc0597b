"""The device SGD step (dafne_sgd_step_hip, dafne_amd/solver.py DeviceSGD; DESIGN row F14) on R50, batch 8, 1024^2:

  kernel  the one launch over tower_parameters() of the released head (8 x 589 824 tower weights + ~60 k more), device events,
          median of --rounds after warm-up, against its byte floor: per tower-weight element p, g, buf read, p, buf written, g
          zeroed and two bf16 forms written = 28 B, at the 6.3 TB/s the microarchitecture guide gives as achievable;
  step    the fine-tune step as profiles/NOTES_pred_backward.md measured it -- host wall, device idle at both ends, median of
          three -- for the parent's route (torch.optim.SGD + invalidate()), the device route (DeviceSGD.step()) and
          backward_towers alone, alternating in one process.

One JSON line.    python scripts/solver_bench.py [--rounds 9] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 8
ACHIEVABLE_TBPS = 6.3


def model_and_inputs(d, seed):
    import bench
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.data.targets import make_gt_instances
    from dafne_amd.registry import build_model
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
    model = build_model(cfg)
    model.load_state_dict(bench.seeded_state_dict(model, seed))
    model.to(d)
    model.invalidate()
    rng = np.random.default_rng(0)
    gi = torch.Generator().manual_seed(0)
    inputs = []
    for _ in range(N):
        c = rng.uniform(100, 900, (12, 2))
        wh = rng.uniform(20, 120, (12, 2))
        q = np.stack([c[:, 0] - wh[:, 0], c[:, 1] - wh[:, 1], c[:, 0] + wh[:, 0], c[:, 1] - wh[:, 1], c[:, 0] + wh[:, 0],
                      c[:, 1] + wh[:, 1], c[:, 0] - wh[:, 0], c[:, 1] + wh[:, 1]], 1).astype(np.float32)
        inputs.append({"image": torch.randint(0, 256, (3, 1024, 1024), generator=gi, dtype=torch.uint8).to(d), "height": 1024,
                       "width": 1024, "instances": make_gt_instances(q, rng.integers(0, 15, 12), (1024, 1024))})
    return model, inputs


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from dafne_amd import _lib
    from dafne_amd.solver import DeviceSGD
    d = torch.device("cuda", 0)
    out = {"batch": N, "rounds": args.rounds}
    with torch.cuda.device(d):
        model, inputs = model_and_inputs(d, 0)
        params = model.tower_parameters()
        model.backward_towers(inputs)                      # the plans, and with them every fragment-major form, exist
        model.zero_grad(set_to_none=True)
        opt = DeviceSGD(model, params, lr=0.0, momentum=0.9, weight_decay=1e-4)       # lr 0: the weights stay what they are
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
        us = []
        for _ in range(max(5, args.rounds)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tb = opt._table
            _lib.check(_lib.load().dafne_sgd_step_hip(tb["desc"], len(params), _lib.ptr(tb["dev"]), tb["bytes"], 0.0, 0.9, 0, 1,
                                                      _lib.current_stream()), "dafne_sgd_step_hip")
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        P = model._packed
        nbytes = 0
        for p, (kind, key, _, _) in zip(params, opt.places):
            forms = 1 + sum(1 for f in ("frag", "frag16", "wr") if key is not None and key + "." + f in P) if kind == "conv" else 0
            nbytes += p.numel() * (24 + 2 * forms + (4 if kind in ("bias", "gn", "scale") else 0))
        floor_us = nbytes / (ACHIEVABLE_TBPS * 1e6)
        out.update({"tensors": len(params), "elements": sum(p.numel() for p in params), "kernel_MB": round(nbytes / 1e6, 1),
                    "kernel_us": round(statistics.median(us), 1), "kernel_min_us": round(min(us), 1),
                    "floor_us_at_6.3TBps": round(floor_us, 1), "kernel_over_floor": round(statistics.median(us) / floor_us, 2)})
        if not args.no_step:
            model.zero_grad(set_to_none=True)
            del opt
            # two models with the same weights, one per route, alternating; lr 0 keeps the loss surface where it is
            host_model, _ = model_and_inputs(d, 0)
            host_opt = torch.optim.SGD(host_model.tower_parameters(), lr=0.0, momentum=0.9, weight_decay=1e-4)
            dev_opt = DeviceSGD(model, params, lr=0.0, momentum=0.9, weight_decay=1e-4)

            def parent():
                host_opt.zero_grad(set_to_none=True)
                host_model.backward_towers(inputs)
                host_opt.step()
                host_model.invalidate()

            def device():
                model.backward_towers(inputs)
                dev_opt.step()

            def backward_only():
                model.backward_towers(inputs)
            cands = {"parent_sgd_invalidate_ms": parent, "device_solver_ms": device, "backward_towers_ms": backward_only}
            for fn in cands.values():
                for _ in range(2):
                    fn()
            times = {k: [] for k in cands}
            for _ in range(3):
                for k, fn in cands.items():
                    times[k].append(wall_ms(fn))
            out.update({k: round(statistics.median(v), 2) for k, v in times.items()})
            out["device_over_backward"] = round(out["device_solver_ms"] / out["backward_towers_ms"], 3)
            out["parent_over_device"] = round(out["parent_sgd_invalidate_ms"] / out["device_solver_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
