#!/usr/bin/env python3
"""Fine-tune the head's prediction layers (cls_logits, corners_pred, ctrness, center_pred, scales) of a checkpoint on labelled
scenes, every step on the device; backbone, FPN and towers stay frozen (DESIGN row F11).

    python tools/finetune_pred.py --config-file configs/dota-1.0_r50.yaml --weights model.pth \\
        --scene-dir scenes/images --scene-labels scenes/labelTxt --steps 100 --lr 0.001 --out finetuned.pth

Every step: one augmented batch of tiles (data.train_views.scene_train_batches: the flips, sizes and quarter turns of the
reference's training loader, drawn from --seed), OneStageDetector.backward_prediction_layers, torch.optim.SGD with
SOLVER.MOMENTUM (and --weight-decay), model.invalidate().  One JSON line per step with the four losses; the result is written
with checkpoint.save_checkpoint (tools/eval_net.py --weights loads it).

--tail: also each complete tower's last GroupNorm affine and last convolution bias (cls_tower / corners_tower .10.weight, .10.bias,
.9.bias; DESIGN row F12): OneStageDetector.tail_parameters through backward_head_tail.
--towers (implies --tail): the whole of cls_tower and corners_tower, four convolutions and four GroupNorms each (DESIGN row F13):
OneStageDetector.tower_parameters through backward_towers.  center_tower, the FPN and the backbone stay frozen.
--device-solver: the step itself runs on the device as well (DESIGN row F14): dafne_amd.solver.DeviceSGD.from_cfg -- the
reference's per-parameter rule over SOLVER.* (BASE_LR, BIAS_LR_FACTOR, WEIGHT_DECAY, WEIGHT_DECAY_NORM, WEIGHT_DECAY_BIAS, MOMENTUM;
--lr / --weight-decay override BASE_LR / WEIGHT_DECAY) -- updates the parameters AND their packed copies in one launch, so the loop
has no model.invalidate().  --lr-schedule: every step's learning rate from dafne_amd.solver.warmup_multistep_lr (SOLVER.STEPS,
GAMMA, WARMUP_FACTOR, WARMUP_ITERS; BASE_LR, or --lr when given).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--weights", default="", help="checkpoint to start from (default MODEL.WEIGHTS; none: seeded random weights)")
    ap.add_argument("--scene-dir", required=True, help="directory of scene images")
    ap.add_argument("--scene-labels", required=True, help="directory of the scenes' DOTA labelTxt files")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--lr", type=float, default=None, help="learning rate (default 0.001; with --device-solver: SOLVER.BASE_LR)")
    ap.add_argument("--weight-decay", type=float, default=None, help="weight decay (default 0; with --device-solver: SOLVER.WEIGHT_DECAY)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8, help="tiles per step")
    ap.add_argument("--patch-size", type=int, default=1024)
    ap.add_argument("--overlap", type=int, default=200)
    ap.add_argument("--tail", action="store_true", help="also train the last GroupNorm affine and last convolution bias of "
                                                        "cls_tower and corners_tower (backward_head_tail)")
    ap.add_argument("--towers", action="store_true", help="also train every convolution and GroupNorm of cls_tower and corners_tower "
                                                          "(backward_towers; implies --tail)")
    ap.add_argument("--device-solver", action="store_true", help="step on the device and update the packed weights in place "
                                                                 "(solver.DeviceSGD.from_cfg); no invalidate() in the loop")
    ap.add_argument("--lr-schedule", action="store_true", help="each step's learning rate from solver.warmup_multistep_lr")
    ap.add_argument("--out", required=True, help="checkpoint to write")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE config overrides")
    args = ap.parse_args(argv)

    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.checkpoint import load_weights, save_checkpoint
    from dafne_amd.config import load_cfg
    from dafne_amd.data import list_image_records
    from dafne_amd.data.loader import read_image
    from dafne_amd.data.train_views import scene_train_batches
    from dafne_amd.evaluation import dota_evaluation as de
    from dafne_amd.evaluation.scene_eval import load_scene_labels
    from dafne_amd.registry import build_model

    cfg = load_cfg(args.config_file, args.opts)
    if not torch.cuda.is_available():
        raise SystemExit("finetune_pred.py needs an MI355X: the HIP path has no CPU fallback")
    dev = torch.device("cuda", 0)
    model = build_model(cfg)
    if args.weights or cfg.MODEL.WEIGHTS:
        missing, unexpected = load_weights(model, args.weights or cfg.MODEL.WEIGHTS)
        print("loaded weights: %d missing, %d unexpected keys" % (len(missing), len(unexpected)))
    else:
        import bench
        model.load_state_dict(bench.seeded_state_dict(model, args.seed))
    model.to(dev)
    model.invalidate()
    records = list_image_records(args.scene_dir)
    if not records:
        raise SystemExit("--scene-dir %s holds no image files" % args.scene_dir)
    scenes = [torch.from_numpy(read_image(r["file_name"], cfg.INPUT.FORMAT)).to(dev) for r in records]
    names = [r["image_id"] for r in records]
    classnames = (list(de.CLASSNAMES_DOTA_1_0) + ["container-crane"])[:cfg.MODEL.DAFNE.NUM_CLASSES]
    labels = load_scene_labels(args.scene_labels, names, classnames)
    # SOLVER.MOMENTUM; a config that does not set it gets detectron2's default (0.9)
    if args.towers:
        params, backward = model.tower_parameters(), model.backward_towers
    elif args.tail:
        params, backward = model.tail_parameters(), model.backward_head_tail
    else:
        params, backward = model.prediction_parameters(), model.backward_prediction_layers
    from dafne_amd.solver import DeviceSGD, warmup_multistep_lr
    if args.device_solver:
        opt = DeviceSGD.from_cfg(model, params, cfg, lr=args.lr, weight_decay=args.weight_decay)
    else:
        opt = torch.optim.SGD(params, lr=0.001 if args.lr is None else args.lr, momentum=float(cfg.SOLVER.get("MOMENTUM", 0.9)),
                              weight_decay=0.0 if args.weight_decay is None else args.weight_decay)
    sched_cfg = cfg
    if args.lr_schedule and args.lr is not None:
        sched_cfg = cfg.clone()
        sched_cfg.SOLVER.BASE_LR = args.lr
    stream = scene_train_batches(cfg, scenes, labels, batch=args.batch, seed=args.seed, patch_size=args.patch_size,
                                 overlap=args.overlap, device=dev)
    with torch.cuda.device(dev):
        for step, tb in enumerate(stream):
            if step >= args.steps:
                break
            lr = warmup_multistep_lr(sched_cfg, step) if args.lr_schedule else None
            if args.device_solver:
                losses = backward(tb)
                opt.step(lr=lr)             # zeroes the gradients in the same pass
            else:
                if lr is not None:
                    for g in opt.param_groups:
                        g["lr"] = lr
                opt.zero_grad(set_to_none=True)
                losses = backward(tb)
                opt.step()
                model.invalidate()
            print(json.dumps(dict({"step": step, "tiles": len(tb)}, **{k: float(v) for k, v in sorted(losses.items())})))
    save_checkpoint(model, args.out)
    print("wrote %s" % args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
