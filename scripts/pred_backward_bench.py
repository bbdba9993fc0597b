"""Kernel time of the prediction layers' weight gradients (dafne_pred_wgrad_hip) at the batch-8, 1024^2 pyramid -- levels 128^2,
64^2, 32^2, 16^2, 8^2 -- against (a) the time to read the three tower maps once at the read rate scripts/bw_probe.py measures
(torch's sum over a bf16 tensor, same machine, same process) and (b) torch's route: torch.nn.grad.conv2d_weight on
channels-last bf16 tensors of the same shapes; and the whole OneStageDetector.backward_prediction_layers step (R50).

Warm-up, then ROUNDS rounds in which the candidates alternate (engine, torch, engine, ...); medians over the rounds.  One JSON
line.    python scripts/pred_backward_bench.py [--rounds 15] [--no-step]
"""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEVELS = [(128, 128), (64, 64), (32, 32), (16, 16), (8, 8)]
N, C = 8, 256
COUTS = {"cls_logits": 15, "corners_ctrness": 9, "center_pred": 2}


def timed(fn, reps=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from dafne_amd import _lib
    from dafne_amd.modeling.dafne.pred_backward import pred_wgrad
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(0)
    calls, gouts, tx, tg = {}, {}, {}, {}
    map_bytes = 0
    for key, cout in COUTS.items():
        maps = []
        for h, w in LEVELS:
            m = torch.zeros(N, h + 2, w + 2, C, dtype=torch.bfloat16, device=d)
            m[:, 1:-1, 1:-1] = torch.randn(N, h, w, C, generator=g, device=d).relu_().to(torch.bfloat16)
            maps.append(m)
        map_bytes += sum(N * h * w * C * 2 for h, w in LEVELS)
        prm = _lib.ConvParams(N, 5, C, cout, 3, 3, 1, 1, 8, None, None, None, None, None, None, None, None, 0.0)
        segs = (_lib.ConvSeg * 5)()
        for i, (m, (h, w)) in enumerate(zip(maps, LEVELS)):
            segs[i] = _lib.ConvSeg(m.data_ptr(), None, None, h, w, h, w)
        calls[key] = types.SimpleNamespace(prm=prm, segs=segs, keep=maps)
        gouts[key] = [torch.randn(N, h, w, cout, generator=g, device=d) * 1e-3 for h, w in LEVELS]
        # torch's route: NCHW-shaped channels-last bf16 views of the same numbers
        tx[key] = [m[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last) for m in maps]
        tg[key] = [t.to(torch.bfloat16).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last) for t in gouts[key]]

    def engine(key):
        return lambda: pred_wgrad(calls[key], gouts[key])

    def engine_all():
        for key in COUTS:
            pred_wgrad(calls[key], gouts[key])

    def torch_all():
        for key, cout in COUTS.items():
            acc = None
            for x, gg in zip(tx[key], tg[key]):
                w = torch.nn.grad.conv2d_weight(x, (cout, C, 3, 3), gg, padding=1)
                acc = w.float() if acc is None else acc + w.float()

    probe = torch.empty(256 * 1024 * 1024 // 2, dtype=torch.bfloat16, device=d).normal_()

    def read_probe():
        probe.sum()
    cands = {"engine_all": engine_all, "torch_all": torch_all, "read_256MB": read_probe}
    cands.update({"engine_" + k: engine(k) for k in COUTS})
    for fn in cands.values():                      # warm-up: kernels loaded, workspaces cached by the allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():                # alternating order inside every round
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    read_tbs = 256 * 1.048576 / med["read_256MB"]          # MB / us = TB/s
    floor_us = map_bytes / 1e6 / read_tbs
    out = {"levels": LEVELS, "batch": N, "map_MB": round(map_bytes / 1e6, 1), "read_TBps": round(read_tbs, 3),
           "read_once_us": round(floor_us, 1), "us": {k: round(v, 1) for k, v in med.items()},
           "min_us": {k: round(min(v), 1) for k, v in times.items()},
           "engine_over_read_floor": round(med["engine_all"] / floor_us, 2),
           "engine_over_torch": round(med["engine_all"] / med["torch_all"], 3), "rounds": args.rounds}
    if not args.no_step:
        import bench
        import dafne_amd.modeling  # noqa: F401
        from dafne_amd.config import load_cfg
        from dafne_amd.data.targets import make_gt_instances
        from dafne_amd.registry import build_model
        cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
        model = build_model(cfg)
        model.load_state_dict(bench.seeded_state_dict(model, 0))
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
        for _ in range(3):
            model.backward_prediction_layers(inputs)
            model.validation_losses(inputs)
        torch.cuda.synchronize()
        st, vt = [], []
        for _ in range(args.rounds):
            st.append(timed(lambda: model.backward_prediction_layers(inputs), reps=2))
            vt.append(timed(lambda: model.validation_losses(inputs), reps=2))
        out["step_us"] = round(statistics.median(st), 1)
        out["validation_losses_us"] = round(statistics.median(vt), 1)
        # a fine-tune step also needs invalidate() (the whole model is re-packed from the fp32 parameters and the plan rebuilt at
        # the next call): host wall time of backward + SGD step + invalidate, device idle at both ends
        import time
        opt = torch.optim.SGD(model.prediction_parameters(), lr=0.0)
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            model.backward_prediction_layers(inputs)
            opt.step()
            model.invalidate()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out["step_with_invalidate_ms"] = round(statistics.median(wall), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
