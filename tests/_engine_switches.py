"""What tests/test_gpu_engine_switches.py records of a model under one EngineOptions record, and how two such records are compared:
the environment of a record, the launch lists and their flag / aliasing signature, the 16x16x32 execution count, and the message of
a mismatch (first tensor that moved in execution order, element count, unified diff of the launch lists).  Nothing here runs a
kernel; the plan-side functions work on plans built on any device."""
import ctypes
import dataclasses
import difflib

import torch

from dafne_amd import engine, _lib
from dafne_amd.engine_options import EngineOptions
from test_gpu_res2_tail import _head_tensors, _same_rows, same_bits

FIELDS = [f.name for f in dataclasses.fields(EngineOptions)]
ENV = {f.name: f.metadata["env"] for f in dataclasses.fields(EngineOptions)}
DEFAULT = EngineOptions()
PLAIN = EngineOptions(**{f: False for f in FIELDS})       # every fusion and special kernel off: generic launches only
FLAG_MASK = engine.F_EXCL | engine.F_GNIN | engine.F_GNFIN | engine.F_FRAG16
# execution order of what a plan leaves behind: the FPN runs top-down (P5, P4, P3), then P6, P7; the prediction layers run
# cls_logits, center_pred, corners_ctrness, corner chain
FPN_ORDER = (2, 1, 0, 3, 4)
HEAD_ORDER = ("logits", "center", "delta_ctr", "corners")


def environment(opt):
    """Every variable of the record, explicitly: "1" / "0" mean on / off for both kinds of switch."""
    return {ENV[f]: "1" if getattr(opt, f) else "0" for f in FIELDS}


def flip(opt, name):
    return dataclasses.replace(opt, **{name: not getattr(opt, name)})


def describe(opt):
    """The fields of `opt` that are not at their default, as text."""
    d = ["%s=%d" % (f, getattr(opt, f)) for f in FIELDS if getattr(opt, f) != getattr(DEFAULT, f)]
    return "defaults" if not d else ("plain" + "".join(" +" + f for f in FIELDS if getattr(opt, f)) if len(d) > 12 else " ".join(d))


# ---------------------------------------------------------------------------------------------------------------- plans
def _halves(c):
    return (c.a, c.b) if isinstance(c, engine.ConvPairCall) else (c,)


def names(plan):
    return [c.kernel_name() for c in plan.calls]


def signature(plan):
    """Per launch: kernel name, the F_EXCL / F_GNIN / F_GNFIN / F_FRAG16 bits of its parameter block(s), and whether an output
    is written over an operand (ConvSeg d_out == d_res; two equal pointer arguments of a whole-block kernel)."""
    sig = []
    for c in plan.calls:
        flags, alias = [], False
        for h in _halves(c):
            if hasattr(h, "prm"):
                flags.append(int(h.prm.flags) & FLAG_MASK)
                alias = alias or any(s.d_res is not None and s.d_out == s.d_res for s in h.segs)
        if isinstance(c, engine.FnCall):
            ptrs = [a.value for a in c.args if isinstance(a, ctypes.c_void_p) and a.value]
            alias = len(set(ptrs)) != len(ptrs)
        sig.append((c.kernel_name(), tuple(flags), alias))
    return sig


def frag16_executions(plan):
    """Layer executions in the 16x16x32 form: resident-patch calls with F_FRAG16 (both halves of a pair) and conv_bneck's
    dafne_bottleneck_body16_hip launches."""
    body16 = _lib.load().dafne_bottleneck_body16_hip
    k = 0
    for c in plan.calls:
        for h in _halves(c):
            if isinstance(h, engine.ConvCall) and (int(h.prm.flags) & engine.F_FRAG16):
                k += 1
        if isinstance(c, engine.FnCall) and c.fn is body16:
            k += 1
    return k


def gn_buffers(plan):
    """The fp32 GroupNorm partial / statistics buffers of a plan's launches (not the int32 arrival counters)."""
    out = {}
    for c in plan.calls:
        for h in _halves(c):
            cand = []
            if isinstance(h, engine.ConvCall):
                cand = [h.keep[2]] + (list(h.keep[6][:1]) if h.keep[6] is not None else [])
            elif isinstance(h, engine.FnCall) and h.name in ("groupnorm", "groupnorm_finalize"):
                cand = list(h.keep[1:3])
            for t in cand:
                if t is not None:
                    assert t.dtype == torch.float32
                    out[t.data_ptr()] = t
    return list(out.values())


def head_tensors(head):
    """_head_tensors' clones, in execution order."""
    return sorted(_head_tensors(head), key=lambda e: (HEAD_ORDER.index(e[0]), e[1]))


# ------------------------------------------------------------------------------------------------------------- comparing
def _count(a, b):
    if a.shape != b.shape:
        return "shapes %s / %s" % (tuple(a.shape), tuple(b.shape))
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    elif a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return "%d of %d elements differ" % (int((a != b).sum()), a.numel())


def launch_diff(base, other):
    """Unified diff of the launch lists: the one-stream plan, then every sub-batch plan."""
    lines = []
    for tag, a, b in [("plan", base["names"], other["names"])] + [("sub-batch %d" % k, a, b) for k, (a, b) in
                                                                  enumerate(zip(base["sub_names"], other["sub_names"]))]:
        d = list(difflib.unified_diff(a, b, "base " + tag, "flipped " + tag, lineterm="", n=1))
        lines += d if d else ["(%s: same %d launches)" % (tag, len(a))]
    return "\n".join(lines)


def first_difference(base, other):
    """-> None, or (what moved first in execution order, how much): FPN maps, head tensors, then the same of the sub-batch
    plans, then the detections."""
    for run in ("", "pipelined "):
        fa, fb = base[run + "feats"], other[run + "feats"]
        for k in range(len(fa)):              # (the pipelined run has one set of FPN maps per sub-batch plan)
            for l in FPN_ORDER:
                if not same_bits(fa[k][l], fb[k][l]):
                    return "%sFPN level %d (P%d)%s" % (run, l, l + 3, " of sub-batch %d" % k if run else ""), _count(fa[k][l], fb[k][l])
        ha, hb = base[run + "head"], other[run + "head"]
        assert [(n, l) for n, l, _ in ha] == [(n, l) for n, l, _ in hb]
        for (n, l, ta), (_, _, tb) in zip(ha, hb):
            if not same_bits(ta, tb):
                return "%shead tensor %s level %d" % (run, n, l), _count(ta, tb)
    for run in ("serial", "pipelined"):
        try:
            _same_rows(other[run], base[run], run)
        except AssertionError as e:
            return "%s detections (rows, counts)" % run, str(e)[:200]
    return None


def mismatch_message(switch, shape, base, other):
    d = first_difference(base, other)
    if d is None:
        return None
    return ("switch %s at shape %s: the first recorded tensor that differs is %s (%s)\n%s"
            % (switch, shape, d[0], d[1], launch_diff(base, other)))
