"""SGD on the device that updates the packed weights in place (DESIGN row F14).

    DeviceSGD(model, params, lr, momentum=0.9, weight_decay=0.0, groups=None)
    DeviceSGD.from_cfg(model, params, cfg)      the reference's per-parameter rule (tools/plain_train_net.py:94-123)
    warmup_multistep_lr(cfg, it)                detectron2's WarmupMultiStepLR, linear warm-up: the learning rate of iteration `it`

`params` is what OneStageDetector.prediction_parameters / tail_parameters / tower_parameters return.  step() is ONE launch of
dafne_sgd_step_hip (csrc/solver_kernels.h: torch.optim.SGD's arithmetic bit for bit) over a table built once: every trained master
parameter, its gradient and momentum buffer (two fp32 arenas owned here; p.grad are views, so the backward's _accumulate adds in
place) and the compute copies in model._packed the plans' launches point at -- pack_conv's bf16 matrix and fp32 bias, the
GroupNorm affines, the fragment-major forms (".frag", ".frag16", ".wr") a plan has packed so far.  Nothing is re-packed and no
plan is rebuilt: there is no invalidate() in the loop.  The five level scales are Python floats in the list P["scales"] the plans
share; step() reads the new values back (20 bytes, its only host read) and writes them into that list.
"""
import bisect
import ctypes

import torch

from . import _lib

HEAD = "proposal_generator.dafne_head."
FORMS = ("frag", "frag16", "wr")            # the derived weight forms a packed key may have: key + "." + form
_ALIGN = 64                                 # arena slots in floats (256 bytes)


def _solver_get(cfg, key, default):
    v = cfg.SOLVER.get(key, default) if "SOLVER" in cfg else default
    return default if v is None else v


def check_cfg(cfg):
    """Refuse the solver settings the device step does not implement."""
    if bool(_solver_get(cfg, "NESTEROV", False)):
        raise NotImplementedError("DeviceSGD: SOLVER.NESTEROV is not implemented")
    if str(_solver_get(cfg, "OPTIMIZER", "sgd")).lower() != "sgd":
        raise NotImplementedError("DeviceSGD: SOLVER.OPTIMIZER %r (sgd only)" % (cfg.SOLVER.OPTIMIZER,))
    clip = _solver_get(cfg, "CLIP_GRADIENTS", None)
    if clip is not None and bool(clip.get("ENABLED", False)):
        raise NotImplementedError("DeviceSGD: SOLVER.CLIP_GRADIENTS is not implemented")


def warmup_multistep_lr(cfg, it):
    """detectron2's WarmupMultiStepLR (WARMUP_METHOD linear) at iteration `it`: BASE_LR * warm-up factor * GAMMA ** (number of
    SOLVER.STEPS that are <= it); the warm-up factor is WARMUP_FACTOR * (1 - it / WARMUP_ITERS) + it / WARMUP_ITERS below
    WARMUP_ITERS and 1 from there on.  detectron2's defaults where a key is absent."""
    base = float(_solver_get(cfg, "BASE_LR", 0.001))
    gamma = float(_solver_get(cfg, "GAMMA", 0.1))
    steps = [int(s) for s in _solver_get(cfg, "STEPS", (30000,))]
    wf = float(_solver_get(cfg, "WARMUP_FACTOR", 1.0 / 1000))
    wi = int(_solver_get(cfg, "WARMUP_ITERS", 1000))
    method = str(_solver_get(cfg, "WARMUP_METHOD", "linear"))
    if method != "linear":
        raise NotImplementedError("warmup_multistep_lr: SOLVER.WARMUP_METHOD %r (linear only)" % (method,))
    warm = 1.0
    if it < wi:
        alpha = it / wi
        warm = wf * (1 - alpha) + alpha
    return base * warm * gamma ** bisect.bisect_right(sorted(steps), it)


def _param_names(model, params):
    by_id = {id(p): n for n, p in model.named_parameters()}
    names = []
    for p in params:
        if id(p) not in by_id:
            raise ValueError("DeviceSGD: a parameter of shape %s does not belong to the model" % (tuple(p.shape),))
        names.append(by_id[id(p)])
    if len(set(names)) != len(names):
        raise ValueError("DeviceSGD: a parameter is listed twice")
    return names


def packed_place(name, head_mode):
    """Where the compute copy of parameter `name` lives in the packed weights -> (kind, key, index, row0):
    ("scale", None, level, 0) | ("conv", key, 0, row0): P[key][0] | ("bias", key, 1, row0): P[key][1] | ("gn", key, 0 or 1, 0).
    Raises ValueError, with the name, for a parameter without such a place (backbone, FPN, center_tower, ...)."""
    bad = ValueError("DeviceSGD: no packed copy to update for parameter %r (the backbone, the FPN and center_tower are "
                     "not trained on the device)" % (name,))
    if not name.startswith(HEAD):
        raise bad
    parts = name[len(HEAD):].split(".")
    strategy, has_ctr = head_mode
    if len(parts) == 3 and parts[0] == "scales" and parts[2] == "scale" and parts[1].isdigit() and int(parts[1]) < 5:
        return ("scale", None, int(parts[1]), 0)
    if len(parts) == 2 and parts[1] in ("weight", "bias"):
        mod = parts[0]
        key, row0 = {"cls_logits": ("cls_logits", 0), "corners_pred": ("corners_ctrness", 0),
                     "ctrness": ("corners_ctrness", 8), "center_pred": ("center_pred", 0)}.get(mod, (None, 0))
        if key is None or strategy == "iterative" or (mod == "ctrness" and not has_ctr) or \
                (mod == "center_pred" and strategy != "center-to-corner"):
            raise bad
        return ("conv" if parts[1] == "weight" else "bias", key, 0 if parts[1] == "weight" else 1, row0)
    if len(parts) == 3 and parts[0] in ("cls_tower", "corners_tower") and parts[1].isdigit() and parts[2] in ("weight", "bias"):
        i = int(parts[1])
        if i < 12 and i % 3 == 0:
            return ("conv" if parts[2] == "weight" else "bias", "%s.%d" % (parts[0], i), 0 if parts[2] == "weight" else 1, 0)
        if i < 12 and i % 3 == 1:
            return ("gn", "%s.%d.gn" % (parts[0], i), 0 if parts[2] == "weight" else 1, 0)
    raise bad


def _is_norm_param(model, name):
    """Does `name` belong to a normalisation layer?  The head's GroupNorm layers are held by params.AffineParams."""
    from .modeling.params import AffineParams
    mod = model
    for part in name.split(".")[:-1]:
        mod = getattr(mod, part)
    return isinstance(mod, (AffineParams, torch.nn.modules.batchnorm._BatchNorm, torch.nn.GroupNorm, torch.nn.LayerNorm,
                            torch.nn.LocalResponseNorm, torch.nn.modules.instancenorm._InstanceNorm))


class DeviceSGD:
    """torch.optim.SGD (momentum, dampening 0, no Nesterov) for the head parameters the device backward differentiates.

    groups: None, or one {"lr_factor": f, "weight_decay": wd} per parameter (missing keys: 1.0 and `weight_decay`): parameter i
    is stepped with the learning rate fp32(lr * f) and the weight decay wd.  self.groups holds the resolved list, with "name"."""

    def __init__(self, model, params, lr, momentum=0.9, weight_decay=0.0, groups=None):
        import torch.distributed as dist
        params = list(params)
        head = model.proposal_generator.dafne_head
        if model.cfg.ENGINE.WEIGHT_DTYPE == "fp8_e4m3":
            raise NotImplementedError("DeviceSGD needs bf16 compute weights (ENGINE.WEIGHT_DTYPE fp8_e4m3 serves a quantised "
                                      "model; fine-tune the bf16 one)")
        if head.head_mode[0] == "iterative":
            raise NotImplementedError("DeviceSGD does not cover CORNER_PREDICTION iterative: the corner chain has no backward")
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("DeviceSGD is single-process: no gradient all-reduce (DDP is out of scope)")
        if not params:
            raise ValueError("DeviceSGD: no parameters")
        if groups is not None and len(groups) != len(params):
            raise ValueError("DeviceSGD: %d groups for %d parameters" % (len(groups), len(params)))
        if not (lr >= 0.0 and momentum >= 0.0 and weight_decay >= 0.0):
            raise ValueError("DeviceSGD: lr %r, momentum %r, weight_decay %r" % (lr, momentum, weight_decay))
        self.model = model
        self.params = params
        self.names = _param_names(model, params)
        self.places = [packed_place(n, head.head_mode) for n in self.names]     # raises on a parameter without a packed copy
        self.lr, self.momentum = float(lr), float(momentum)
        self.groups = []
        for i, n in enumerate(self.names):
            g = dict(groups[i]) if groups is not None else {}
            self.groups.append({"name": n, "lr_factor": float(g.get("lr_factor", 1.0)),
                                "weight_decay": float(g.get("weight_decay", weight_decay))})
        self.steps = 0
        dev = params[0].device
        for n, p in zip(self.names, params):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError("DeviceSGD: parameter %r must be a contiguous fp32 tensor on %s" % (n, dev))
        # the two arenas: every tensor at a 256-byte slot
        self._off, total = [], 0
        for p in params:
            self._off.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.grad_arena = torch.zeros(total, dtype=torch.float32, device=dev)
        self.momentum_arena = torch.zeros(total, dtype=torch.float32, device=dev)
        for p, o in zip(params, self._off):
            view = self.grad_arena[o:o + p.numel()].view(p.shape)
            if p.grad is not None:
                view.copy_(p.grad)
            p.grad = view
        self._grad_ptrs = [p.grad.data_ptr() for p in params]
        self._scales_out = None         # device fp32 [5]: the scales' compute copy, read back by step()
        self._table = None              # (descriptors, device image, its bytes, the keys of P it was built from, id(P))

    @classmethod
    def from_cfg(cls, model, params, cfg, lr=None, weight_decay=None):
        """The reference's optimiser (tools/plain_train_net.py:94-123, detectron2's defaults where a key is absent): norm layers
        get WEIGHT_DECAY_NORM, parameters named `bias` BASE_LR * BIAS_LR_FACTOR and WEIGHT_DECAY_BIAS, everything else BASE_LR and
        WEIGHT_DECAY; SOLVER.MOMENTUM.  lr / weight_decay: override BASE_LR / WEIGHT_DECAY (the bias decay follows only when the
        config does not set WEIGHT_DECAY_BIAS)."""
        check_cfg(cfg)
        params = list(params)
        base = float(_solver_get(cfg, "BASE_LR", 0.001)) if lr is None else float(lr)
        wd = float(_solver_get(cfg, "WEIGHT_DECAY", 0.0001)) if weight_decay is None else float(weight_decay)
        wd_norm = float(_solver_get(cfg, "WEIGHT_DECAY_NORM", 0.0))
        wd_bias = float(_solver_get(cfg, "WEIGHT_DECAY_BIAS", wd))
        bias_f = float(_solver_get(cfg, "BIAS_LR_FACTOR", 1.0))
        groups = []
        for n in _param_names(model, params):
            if _is_norm_param(model, n):
                groups.append({"lr_factor": 1.0, "weight_decay": wd_norm})
            elif n.split(".")[-1] == "bias":
                groups.append({"lr_factor": bias_f, "weight_decay": wd_bias})
            else:
                groups.append({"lr_factor": 1.0, "weight_decay": wd})
        return cls(model, params, base, momentum=float(_solver_get(cfg, "MOMENTUM", 0.9)), weight_decay=wd, groups=groups)

    # ------------------------------------------------------------ the table
    def _view(self, arena, i):
        o = self._off[i]
        return arena[o:o + self.params[i].numel()]

    def _build_table(self, P):
        L = _lib.load()
        dev = self.grad_arena.device
        head = self.model.proposal_generator.dafne_head
        trained = sorted(set(k for _, k, _, _ in self.places if k is not None))
        for k in P:
            for t in trained:
                if k.startswith(t + ".") and k[len(t) + 1:] not in FORMS:
                    raise RuntimeError("DeviceSGD: the packed weights hold %r, a copy of the trained %r in a form the device "
                                       "step does not write" % (k, t))
        if self._scales_out is None:
            self._scales_out = torch.tensor([float(v) for v in P["scales"]], dtype=torch.float32, device=dev)
        n = len(self.params)
        desc = (_lib.SgdTensor * n)()
        keep = [self._scales_out]
        for i, (p, name, (kind, key, idx, row0)) in enumerate(zip(self.params, self.names, self.places)):
            d = desc[i]
            d.d_p, d.d_g, d.d_buf = p.data_ptr(), self._grad_ptrs[i], self._view(self.momentum_arena, i).data_ptr()
            d.n = p.numel()
            d.lr_factor, d.weight_decay = self.groups[i]["lr_factor"], self.groups[i]["weight_decay"]
            if kind == "scale":
                d.form = _lib.SGD_F32
                d.d_copy = self._scales_out.data_ptr() + 4 * idx
                if p.numel() != 1:
                    raise RuntimeError("DeviceSGD: %s has %d elements" % (name, p.numel()))
                continue
            t = P[key][idx]
            keep.append(t)
            if kind == "gn":
                if t.dtype != torch.float32 or t.numel() != p.numel() or not t.is_contiguous():
                    raise RuntimeError("DeviceSGD: packed GroupNorm affine %r does not match %s" % (key, name))
                d.form, d.d_copy = _lib.SGD_F32, t.data_ptr()
            elif kind == "bias":
                if t.dtype != torch.float32 or t.dim() != 1 or row0 + p.numel() > t.numel() or not t.is_contiguous():
                    raise RuntimeError("DeviceSGD: packed bias of %r does not hold rows %d..+%d (%s)" % (key, row0, p.numel(), name))
                d.form, d.d_copy = _lib.SGD_F32, t.data_ptr() + 4 * row0
                if key == "corners_ctrness" and row0 == 0 and head.head_mode[0] == "offset":
                    base = head.base_corners            # folded into the packed bias (engine.pack_head_weights): copy = bias + base
                    if base.dtype != torch.float32 or base.numel() != p.numel() or not base.is_contiguous() or base.device != dev:
                        raise RuntimeError("DeviceSGD: base_corners must be 8 contiguous fp32 on %s" % (dev,))
                    keep.append(base)
                    d.d_addend = base.data_ptr()
            else:
                cout, cin, kh, kw = p.shape
                rows = t.shape[0]
                if t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape[1] != cin * kh * kw or row0 + cout > rows or not t.is_contiguous():
                    raise RuntimeError("DeviceSGD: packed weight %r %s does not hold %s at row %d" % (key, tuple(t.shape), name, row0))
                d.form, d.d_plain = _lib.SGD_CONV, t.data_ptr()
                d.Cout, d.Cin, d.KH, d.KW, d.row0, d.rows = cout, cin, kh, kw, row0, rows
                for form, field in (("frag", "d_frag"), ("frag16", "d_frag16"), ("wr", "d_wr")):
                    f = P.get(key + "." + form)
                    if f is None:
                        continue
                    if f.dtype != torch.bfloat16 or f.numel() != t.numel() or not f.is_contiguous():
                        raise RuntimeError("DeviceSGD: %r is not a fragment-major form of %r" % (key + "." + form, key))
                    keep.append(f)
                    setattr(d, field, f.data_ptr())
        nbytes = L.dafne_sgd_table_bytes(desc, n)
        if nbytes == 0:
            _lib.check(_lib.load().dafne_sgd_table_build(desc, n, None, 0), "dafne_sgd_table_build")
        host = torch.empty(nbytes, dtype=torch.uint8)
        _lib.check(L.dafne_sgd_table_build(desc, n, ctypes.c_void_p(host.data_ptr()), nbytes), "dafne_sgd_table_build")
        self._table = {"desc": desc, "dev": host.to(dev), "bytes": nbytes, "keys": set(P), "P": P, "keep": keep}

    # ------------------------------------------------------------ the step
    def step(self, lr=None, zero_grad=True):
        """One SGD step with learning rate `lr` (default: the constructor's; a schedule passes warmup_multistep_lr(cfg, it)):
        one launch on the current stream, then the 20-byte read of the new scales.  zero_grad: the gradients are zeroed in the same
        pass (p.grad stays the arena view the table points at).  No invalidate(): model._packed, the plans and every packed
        tensor stay the objects they were.  The one other packed copy of these parameters, the stand-alone head module's own
        (DAFNeHead._packed / _plans, used by DAFNeHead.forward / run_raw), is dropped and re-packed lazily at its next use."""
        model = self.model
        dev = self.grad_arena.device
        if dev.type != "cuda":
            raise _lib.DafneHipError("DeviceSGD.step: the MI355X engine has no CPU path (the parameters live on %s)" % (dev,))
        for i, p in enumerate(self.params):
            if p.grad is None or p.grad.data_ptr() != self._grad_ptrs[i]:
                raise RuntimeError("DeviceSGD.step: .grad of %s is no longer the solver's gradient buffer (zero_grad(set_to_none="
                                   "True) or an assignment replaced it; use DeviceSGD.zero_grad() or step(zero_grad=True))"
                                   % (self.names[i],))
        lr = self.lr if lr is None else float(lr)
        with torch.cuda.device(dev):
            P = model._weights()
            if self._table is None or self._table["P"] is not P or self._table["keys"] != set(P):
                self._build_table(P)        # first step; a plan built since has packed another form; the model was re-packed
            tb = self._table
            _lib.check(_lib.load().dafne_sgd_step_hip(tb["desc"], len(self.params), _lib.ptr(tb["dev"]), tb["bytes"], lr, self.momentum,
                                                      int(self.steps == 0), int(bool(zero_grad)), _lib.current_stream()),
                       "dafne_sgd_step_hip")
            self.steps += 1
            # the stand-alone head module (DAFNeHead.forward / run_raw, DAFNe.forward) keeps a packed copy and plans of its OWN,
            # packed from the same parameters; the parent's loop dropped them at every step through model.invalidate().  They
            # are not in the table: drop them, so that the next call there packs the new parameters (model._packed and
            # model._plans are not touched)
            head = model.proposal_generator.dafne_head
            if head._packed is not None or head._plans:
                head.invalidate()
            if any(kind == "scale" for kind, _, _, _ in self.places):
                vals = self._scales_out.cpu()           # the step's only host read: 5 floats
                scales = P["scales"]                    # the list the plans hold: written element by element, never replaced
                for kind, _, l, _ in self.places:
                    if kind == "scale":
                        scales[l] = float(vals[l])

    def zero_grad(self):
        """Zero the gradient arena (step(zero_grad=True) already does, in its own pass) and re-attach the views as .grad."""
        self.grad_arena.zero_()
        for p, o in zip(self.params, self._off):
            if p.grad is None or p.grad.data_ptr() != self.grad_arena.data_ptr() + 4 * o:
                p.grad = self.grad_arena[o:o + p.numel()].view(p.shape)

    # ------------------------------------------------------------ state
    def state_dict(self):
        """{"momentum": {parameter name: buffer}, "steps", "lr", "momentum_factor", "groups"}: what a resumed fine-tune needs."""
        return {"momentum": {n: self._view(self.momentum_arena, i).view(p.shape).detach().clone()
                             for i, (n, p) in enumerate(zip(self.names, self.params))},
                "steps": self.steps, "lr": self.lr, "momentum_factor": self.momentum,
                "groups": [dict(g) for g in self.groups]}

    def load_state_dict(self, sd):
        names = set(sd["momentum"])
        if names != set(self.names):
            raise ValueError("DeviceSGD.load_state_dict: momentum buffers for other parameters (missing %s, unknown %s)"
                             % (sorted(set(self.names) - names)[:4], sorted(names - set(self.names))[:4]))
        by_name = {g["name"]: g for g in sd["groups"]}
        if set(by_name) != set(self.names):
            raise ValueError("DeviceSGD.load_state_dict: groups for other parameters")
        for i, (n, p) in enumerate(zip(self.names, self.params)):
            b = sd["momentum"][n]
            if tuple(b.shape) != tuple(p.shape):
                raise ValueError("DeviceSGD.load_state_dict: momentum buffer of %s has shape %s" % (n, tuple(b.shape)))
            self._view(self.momentum_arena, i).copy_(b.reshape(-1).to(self.momentum_arena.device, torch.float32))
        self.steps = int(sd["steps"])
        self.lr, self.momentum = float(sd["lr"]), float(sd["momentum_factor"])
        self.groups = [dict(by_name[n]) for n in self.names]
        self._table = None                  # the descriptors carry lr_factor / weight_decay
