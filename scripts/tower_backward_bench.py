"""Kernel time of one tower layer's backward -- dafne_tower_wgrad_hip and dafne_tower_dgrad_gn_hip (DESIGN row F13) -- at the
batch-8, 1024^2 pyramid (levels 128^2, 64^2, 32^2, 16^2, 8^2; GN_INPUT), against two baselines on the same tensors in the same
process:
  (a) the only route the weight gradient had before: 16 dafne_pred_wgrad_hip launches over 16-channel slices of g (pixel stride 256);
  (b) torch's conv2d_weight / conv2d_input on channels-last bf16 operands (ONE bf16 product where the kernels here feed g as a
      hi + lo pair, twice the matrix work; torch's data gradient also stops at ga: no ReLU mask, no GroupNorm backward).

Warm-up, then ROUNDS rounds in which the candidates alternate; medians over the rounds.  One JSON line.  Reports, does not gate.
    python scripts/tower_backward_bench.py [--rounds 9]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEVELS = [(128, 128), (64, 64), (32, 32), (16, 16), (8, 8)]
N, C = 8, 256


def timed(fn, reps=3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    from dafne_amd import _lib, engine
    from dafne_amd.modeling.dafne.pred_backward import pred_wgrad
    from dafne_amd.modeling.dafne.tower_backward import tower_dgrad_gn, tower_wgrad
    d = torch.device("cuda", 0)
    g = torch.Generator(device=d).manual_seed(0)
    maps = []
    for h, w in LEVELS:
        m = torch.zeros(N, h + 2, w + 2, C, dtype=torch.bfloat16, device=d)
        m[:, 1:-1, 1:-1] = torch.randn(N, h, w, C, generator=g, device=d).to(torch.bfloat16)
        maps.append(m)
    stats = torch.zeros(5, N, C // 8, 2, device=d)
    stats[..., 1] = 1.0                             # mean 0, rstd 1: the maps are standard normal
    gamma, beta = torch.rand(C, generator=g, device=d) + 0.5, torch.randn(C, generator=g, device=d) * 0.3

    def call(cout, flags):
        prm = _lib.ConvParams(N, 5, C, cout, 3, 3, 1, 1, flags, None, None, None, stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                              None, None, 0.0)
        segs = (_lib.ConvSeg * 5)()
        for i, (m, (h, w)) in enumerate(zip(maps, LEVELS)):
            segs[i] = _lib.ConvSeg(m.data_ptr(), None, None, h, w, h, w)
        return types.SimpleNamespace(prm=prm, segs=segs, keep=(maps, stats, gamma, beta))
    tower, pred16 = call(C, 16 | 32), call(16, 8 | 32)
    gouts = [torch.randn(N, h, w, C, generator=g, device=d) * 1e-3 for h, w in LEVELS]
    wgt = torch.randn(C, C, 3, 3, generator=g, device=d) * 0.03
    wp = engine.pack_conv(wgt, None, d)[0]
    # torch's route: NCHW-shaped channels-last bf16 views of the numbers the kernels multiply
    tx = [torch.relu((m[:, 1:-1, 1:-1].float() * gamma + beta)).to(torch.bfloat16).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
          for m in maps]
    tg = [t.to(torch.bfloat16).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last) for t in gouts]
    tw = wgt.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def wgrad_16_launches():
        for k in range(16):
            pred_wgrad(pred16, [t[..., 16 * k:16 * k + 16] for t in gouts], ps=C)

    def torch_wgrad():
        acc = None
        for x, gg in zip(tx, tg):
            w = torch.nn.grad.conv2d_weight(x, (C, C, 3, 3), gg, padding=1)
            acc = w.float() if acc is None else acc + w.float()

    def torch_dgrad():
        for x, gg in zip(tx, tg):
            torch.nn.grad.conv2d_input(x.shape, tw, gg, padding=1)
    cands = {"tower_wgrad": lambda: tower_wgrad(tower, gouts), "pred_wgrad_x16": wgrad_16_launches, "torch_conv2d_weight_bf16": torch_wgrad,
             "tower_dgrad_gn": lambda: tower_dgrad_gn(tower, wp, gouts), "torch_conv2d_input_bf16": torch_dgrad}
    for fn in cands.values():                      # warm-up: kernels loaded, workspaces cached by the allocator
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():                # alternating order inside every round
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    pixels = sum(N * h * w for h, w in LEVELS)
    flop = 2.0 * pixels * C * C * 9                # one bf16 product; the hi + lo kernels do twice this
    print(json.dumps({"levels": LEVELS, "batch": N, "pixels": pixels, "us": {k: round(v, 1) for k, v in med.items()},
                      "min_us": {k: round(min(v), 1) for k, v in times.items()},
                      "tower_wgrad_over_16_launches": round(med["tower_wgrad"] / med["pred_wgrad_x16"], 3),
                      "tower_wgrad_over_torch": round(med["tower_wgrad"] / med["torch_conv2d_weight_bf16"], 3),
                      "tower_dgrad_over_torch": round(med["tower_dgrad_gn"] / med["torch_conv2d_input_bf16"], 3),
                      "tower_wgrad_hi_lo_TFLOPs": round(2 * flop / med["tower_wgrad"] / 1e6, 1),
                      "tower_dgrad_hi_lo_TFLOPs": round(2 * flop / med["tower_dgrad_gn"] / 1e6, 1), "rounds": args.rounds}))


if __name__ == "__main__":
    main()
