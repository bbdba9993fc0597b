"""CPU: the oracle of the device SGD step (tests/_solver_np.py) against torch.optim.SGD bit for bit on the inputs the GPU test
uses; DeviceSGD.from_cfg's per-parameter groups against the reference's rule; warmup_multistep_lr against hand-worked values;
the construction-time refusals of dafne_amd/solver.py."""
import os

import numpy as np
import pytest
import torch

import _solver_np as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("foreach", [False, True])
@pytest.mark.parametrize("wd", S.SYNTHETIC_WD)
def test_oracle_equals_torch_sgd_bit_for_bit(wd, foreach):
    params = {n: torch.nn.Parameter(v.clone()) for n, v in S.synthetic_params().items()}
    groups = [{"params": [params[n]], "lr": S.SYNTHETIC_LR * f, "weight_decay": wd} for n, _, f in S.SYNTHETIC]
    assert any(f == 2.0 for _, _, f in S.SYNTHETIC)            # the bias group with lr_factor 2
    opt = torch.optim.SGD(groups, lr=S.SYNTHETIC_LR, momentum=S.SYNTHETIC_MOMENTUM, foreach=foreach)
    want = S.oracle_run(wd, S.SYNTHETIC_STEPS)
    for k in range(S.SYNTHETIC_STEPS):
        gr = S.synthetic_grads(k)
        for n, p in params.items():
            p.grad = gr[n].clone()
        opt.step()
        for n, p in params.items():
            wp, wb = want[k][n]
            assert np.array_equal(S.bits(p.detach().numpy()), S.bits(wp)), (k, n, "parameter")
            assert np.array_equal(S.bits(opt.state[p]["momentum_buffer"].numpy()), S.bits(wb)), (k, n, "momentum buffer")
    assert not np.array_equal(want[0]["w2"][0], want[1]["w2"][0])


def _reference_groups(model, cfg_solver):
    """tools/plain_train_net.py:94-123 restated: {parameter name: (lr, weight_decay)} over every parameter of the model.  The
    reference's towers hold torch.nn.GroupNorm at indices 1 / 4 / 7 / 10; here those layers are params.AffineParams."""
    from dafne_amd.modeling.params import AffineParams
    norm_types = (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d, torch.nn.SyncBatchNorm, torch.nn.GroupNorm,
                  torch.nn.InstanceNorm1d, torch.nn.InstanceNorm2d, torch.nn.InstanceNorm3d, torch.nn.LayerNorm,
                  torch.nn.LocalResponseNorm, AffineParams)
    names = {id(p): n for n, p in model.named_parameters()}
    out = {}
    for module in model.modules():
        for key, value in module.named_parameters(recurse=False):
            lr, wd = cfg_solver["BASE_LR"], cfg_solver["WEIGHT_DECAY"]
            if isinstance(module, norm_types):
                wd = cfg_solver["WEIGHT_DECAY_NORM"]
            elif key == "bias":
                lr, wd = cfg_solver["BASE_LR"] * cfg_solver["BIAS_LR_FACTOR"], cfg_solver["WEIGHT_DECAY_BIAS"]
            out[names[id(value)]] = (lr, wd)
    return out


@pytest.mark.parametrize("strategy,centerness", [("center-to-corner", "oriented"), ("offset", "plain")])
def test_from_cfg_groups_follow_the_reference_rule(strategy, centerness):
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from dafne_amd.solver import DeviceSGD
    solver = {"BASE_LR": 0.004, "BIAS_LR_FACTOR": 2.0, "WEIGHT_DECAY": 0.0002, "WEIGHT_DECAY_NORM": 0.00005,
              "WEIGHT_DECAY_BIAS": 0.0003, "MOMENTUM": 0.8}
    opts = ["MODEL.DAFNE.CORNER_PREDICTION", strategy]
    if strategy != "center-to-corner":
        opts += ["MODEL.DAFNE.CENTERNESS", centerness]
    for k, v in solver.items():
        opts += ["SOLVER." + k, str(v)]
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), opts)
    model = build_model(cfg)
    params = model.tower_parameters()
    opt = DeviceSGD.from_cfg(model, params, cfg)
    want = _reference_groups(model, solver)
    assert opt.momentum == 0.8 and opt.lr == 0.004 and len(opt.groups) == len(params)
    kinds = set()
    for g in opt.groups:
        lr, wd = want[g["name"]]
        assert opt.lr * g["lr_factor"] == lr and g["weight_decay"] == wd, g
        kinds.add((g["lr_factor"], g["weight_decay"]))
    assert kinds == {(1.0, 0.0002), (1.0, 0.00005), (2.0, 0.0003)}
    # .grad are views of ONE arena, in place for the backward's accumulation
    assert all(p.grad is not None and p.grad.shape == p.shape for p in params)
    lo, hi = opt.grad_arena.data_ptr(), opt.grad_arena.data_ptr() + 4 * opt.grad_arena.numel()
    assert all(lo <= p.grad.data_ptr() and p.grad.data_ptr() + 4 * p.numel() <= hi for p in params)
    # detectron2's defaults where the config is silent: WEIGHT_DECAY 1e-4 (bias too), norm 0, BIAS_LR_FACTOR 1, momentum 0.9
    plain = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), opts[:2] + (opts[2:4] if strategy != "center-to-corner" else []))
    for k in ("BASE_LR", "BIAS_LR_FACTOR", "WEIGHT_DECAY", "WEIGHT_DECAY_NORM", "WEIGHT_DECAY_BIAS", "MOMENTUM"):
        plain.SOLVER.pop(k, None)
    m2 = build_model(plain)
    o2 = DeviceSGD.from_cfg(m2, m2.prediction_parameters(), plain)
    assert o2.lr == 0.001 and o2.momentum == 0.9
    assert all(g["lr_factor"] == 1.0 and g["weight_decay"] == 0.0001 for g in o2.groups)
    # a CPU model has no device step
    from dafne_amd import _lib
    with pytest.raises(_lib.DafneHipError):
        o2.step()
    m2.zero_grad(set_to_none=True)


def test_warmup_multistep_lr_by_hand():
    from dafne_amd.config import load_cfg
    from dafne_amd.solver import warmup_multistep_lr
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"),
                   ["SOLVER.BASE_LR", "0.01", "SOLVER.GAMMA", "0.1", "SOLVER.STEPS", "[100, 200]", "SOLVER.WARMUP_FACTOR", "0.001",
                    "SOLVER.WARMUP_ITERS", "50", "SOLVER.WARMUP_METHOD", "linear"])
    # iteration 0: factor 0.001 exactly; iteration 49: 0.001 * (1 - 49/50) + 49/50 = 0.00002 + 0.98 = 0.98002; 50: warm-up over
    assert warmup_multistep_lr(cfg, 0) == pytest.approx(0.01 * 0.001, rel=1e-12)
    assert warmup_multistep_lr(cfg, 49) == pytest.approx(0.01 * 0.98002, rel=1e-12)
    assert warmup_multistep_lr(cfg, 50) == pytest.approx(0.01, rel=1e-12)
    # the milestones: the rate drops AT the step (bisect_right), not one later
    assert warmup_multistep_lr(cfg, 99) == pytest.approx(0.01, rel=1e-12)
    assert warmup_multistep_lr(cfg, 100) == pytest.approx(0.001, rel=1e-12)
    assert warmup_multistep_lr(cfg, 199) == pytest.approx(0.001, rel=1e-12)
    assert warmup_multistep_lr(cfg, 200) == pytest.approx(0.0001, rel=1e-12)
    # detectron2's defaults: 1000 warm-up iterations from 1/1000, one drop by 0.1 at 30000, BASE_LR 0.001
    plain = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"))
    for k in ("BASE_LR", "GAMMA", "STEPS", "WARMUP_FACTOR", "WARMUP_ITERS", "WARMUP_METHOD"):
        plain.SOLVER.pop(k, None)
    assert warmup_multistep_lr(plain, 500) == pytest.approx(0.001 * (0.001 * 0.5 + 0.5), rel=1e-12)
    assert warmup_multistep_lr(plain, 29999) == pytest.approx(0.001, rel=1e-12)
    assert warmup_multistep_lr(plain, 30000) == pytest.approx(0.0001, rel=1e-12)


def test_construction_refusals():
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from dafne_amd.solver import DeviceSGD
    path = os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")
    cfg = load_cfg(path)
    model = build_model(cfg)
    head = model.proposal_generator.dafne_head
    # parameters without a packed copy the step could write: named in the message
    for p, frag in ((head.center_tower[0].weight, "center_tower.0.weight"),
                    (next(p for n, p in model.named_parameters() if n.startswith("backbone.")), "backbone.")):
        with pytest.raises(ValueError, match=frag.replace(".", r"\.")):
            DeviceSGD(model, model.prediction_parameters() + [p], lr=0.01)
    assert all(p.grad is None for p in model.parameters()), "a refused construction must not attach gradients"
    for opts in (["SOLVER.NESTEROV", "True"], ["SOLVER.OPTIMIZER", "adam"], ["SOLVER.CLIP_GRADIENTS.ENABLED", "True"]):
        with pytest.raises(NotImplementedError):
            DeviceSGD.from_cfg(model, model.prediction_parameters(), load_cfg(path, opts))
    with pytest.raises(NotImplementedError):
        m8 = build_model(load_cfg(path, ["ENGINE.WEIGHT_DTYPE", "fp8_e4m3"]))
        DeviceSGD(m8, m8.prediction_parameters(), lr=0.01)
    it = build_model(load_cfg(path, ["MODEL.DAFNE.CORNER_PREDICTION", "iterative", "MODEL.DAFNE.CENTERNESS", "plain"]))
    with pytest.raises(NotImplementedError):
        DeviceSGD(it, [it.proposal_generator.dafne_head.cls_logits.weight], lr=0.01)
    # the state round trip: momentum by parameter name, step count, hyper-parameters
    a = DeviceSGD(model, model.tail_parameters(), lr=0.02, momentum=0.7, weight_decay=1e-4)
    a.momentum_arena.copy_(torch.arange(a.momentum_arena.numel(), dtype=torch.float32))
    a.steps = 5
    sd = a.state_dict()
    assert sorted(sd["momentum"]) == sorted(a.names) and sd["steps"] == 5
    model.zero_grad(set_to_none=True)
    b = DeviceSGD(model, model.tail_parameters(), lr=0.5)
    b.load_state_dict(sd)
    assert b.steps == 5 and b.lr == 0.02 and b.momentum == 0.7 and b.groups == a.groups
    for n in a.names:
        assert torch.equal(b.state_dict()["momentum"][n], sd["momentum"][n])
    with pytest.raises(ValueError):
        DeviceSGD(model, model.prediction_parameters(), lr=0.5).load_state_dict(sd)
    model.zero_grad(set_to_none=True)
