"""CPU: the launch lists of DensePlan, pinned against the commit tests/golden/plan_launch_lists.json names.

A plan builds on torch.device("cpu") without a GPU (nothing runs a kernel here).  For every plan of the matrix below the test
records, per entry of plan.calls in order: class, kernel_name(), flops, bytes; for an FnCall the library symbol and every argument
(ints and floats verbatim, ctypes struct arrays field by field); for a ConvCall every field of its parameter block and segments
(both halves of a ConvPairCall, the convolution inside a WrCall); for an AmaxProbe its key; and the set of tensors reachable from
`keep`.  Per plan: flops, head_start, the feature / stage / stem / head-output buffers, the pool's free lists and the keys of the
packed weights after the build (the lazily packed fragments).  Every pointer is replaced by the index of its first appearance in the
plan, so the dump is the same in every process -- unless an argument points at a tensor nothing keeps.

The fixture holds, per plan, the kernel names and the sha256 of the dump.  It is written from the commit BEFORE a change to the
plan builders, never from the changed code:

    PYTHONPATH=<checkout of that commit, built> python tests/test_plan_launch_lists_cpu.py --write
    python tests/test_plan_launch_lists_cpu.py --dump DIR        (one text file per plan: diff two trees' directories)

The weights are packed once per model and shared by the plans of all option records (a shallow copy with P["options"] replaced:
pack_backbone_weights / pack_head_weights only store the record); every plan gets its own copy, so the lazily packed keys it
leaves are its own."""
import ctypes
import dataclasses
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_launch_lists.json")
CPU = torch.device("cpu")
MODELS = [(50, (2, 64, 96)), (50, (1, 544, 544)), (50, (3, 128, 160)), (101, (2, 64, 96))]      # the switch tests' shapes
SMALL = [(50, (2, 64, 96)), (101, (2, 64, 96))]
NUM_CLASSES = 15


# ------------------------------------------------------------------------------------------------------------ fingerprint
class _Ids:
    """Pointer -> index of its first appearance in the plan."""

    def __init__(self):
        self.ids = {}

    def __call__(self, p):
        if isinstance(p, ctypes.c_void_p):
            p = p.value
        if not p:
            return "NULL"
        return "p%d" % self.ids.setdefault(int(p), len(self.ids))


def _struct(s, ids):
    out = []
    for name, typ in s._fields_:
        v = getattr(s, name)
        out.append("%s=%s" % (name, ids(v) if typ is ctypes.c_void_p else repr(v)))
    return "{" + " ".join(out) + "}"


def _arg(a, ids):
    if a is None or isinstance(a, ctypes.c_void_p):
        return ids(a)
    if isinstance(a, ctypes.Array) and issubclass(a._type_, ctypes.Structure):
        return "[" + ", ".join(_struct(s, ids) for s in a) + "]"
    if isinstance(a, ctypes.Structure):
        return _struct(a, ids)
    if isinstance(a, (ctypes.c_float, ctypes.c_double, ctypes.c_int)):
        return "%s(%r)" % (type(a).__name__, a.value)
    assert isinstance(a, (int, float)), type(a)
    return repr(a)


def _tensors(obj, out):
    """Every tensor reachable from a keep list (Act -> its tensor; lists / tuples / dicts walked)."""
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif hasattr(obj, "t") and isinstance(getattr(obj, "t"), torch.Tensor):
        out.append(obj.t)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _tensors(o, out)
    elif isinstance(obj, dict):
        for o in obj.values():
            _tensors(o, out)
    return out


def _tdesc(t, ids):
    return "%s %s%s" % (ids(t.data_ptr()), str(t.dtype).replace("torch.", ""), list(t.shape))


def _kept(keep, ids):
    ts = _tensors(keep, [])
    known = [t for t in ts if int(t.data_ptr()) in ids.ids]
    # (a kept tensor no argument named: numbered in an order that does not depend on the keep list's)
    new = sorted((t for t in ts if int(t.data_ptr()) not in ids.ids), key=lambda t: (str(t.dtype), list(t.shape)))
    return sorted(set(_tdesc(t, ids) for t in known + new))


def _conv(c, ids):
    lines = ["  prm " + _struct(c.prm, ids)]
    lines += ["  seg " + _struct(s, ids) for s in c.segs]
    if c.fp8 is not None:
        lines.append("  fp8 oscale=%s in_qscale=%r" % (ids(c.fp8[0].data_ptr()), float(c.fp8[1])))
    if c.wfrag is not None:
        lines.append("  wfrag " + _tdesc(c.wfrag, ids))
    lines.append("  keep " + "; ".join(_kept(c.keep, ids)))
    return lines


def _call(c, ids, engine):
    lines = ["%s %s flops=%d bytes=%d" % (type(c).__name__, c.kernel_name(), c.flops, c.bytes)]
    if isinstance(c, engine.FnCall):
        lines.append("  fn " + c.fn.__name__)
        lines.append("  args " + ", ".join(_arg(a, ids) for a in c.args))
        lines.append("  keep " + "; ".join(_kept(c.keep, ids)))
    elif isinstance(c, engine.ConvCall):
        lines += _conv(c, ids)
    elif isinstance(c, engine.ConvPairCall):
        lines += _conv(c.a, ids) + _conv(c.b, ids)
    elif isinstance(c, engine.WrCall):
        lines += _conv(c.conv, ids)
        lines.append("  wr wfrag=%s splits=%d" % (_tdesc(c.wfrag, ids), c.splits))
    elif isinstance(c, engine.AmaxProbe):
        lines.append("  key %s acts %s" % (c.key, "; ".join(_tdesc(a.t, ids) for a in c.acts)))
    else:
        raise AssertionError("unknown launch class %s" % type(c).__name__)
    return lines


def _pdesc(v):
    if isinstance(v, torch.Tensor):
        return "%s%s" % (str(v.dtype).replace("torch.", ""), list(v.shape))
    if isinstance(v, (list, tuple)):
        return "(" + ", ".join(_pdesc(x) for x in v) + ")"
    if isinstance(v, dict):
        return "{" + ", ".join("%s: %s" % (k, _pdesc(v[k])) for k in sorted(v)) + "}"
    return repr(v)


def fingerprint(plan, P):
    """-> (kernel names, full dump as text)."""
    from dafne_amd import engine
    ids = _Ids()
    lines = []
    for i, c in enumerate(plan.calls):
        body = _call(c, ids, engine)
        lines += ["[%d] %s" % (i, body[0])] + body[1:]
    lines.append("flops=%d head_start=%d calls=%d" % (plan.flops, plan.head_start, len(plan.calls)))
    lines.append("features " + "; ".join(_tdesc(a.t, ids) for a in plan.features))
    lines.append("stage_feats " + "; ".join("%s=%s" % (k, _tdesc(a.t, ids)) for k, a in sorted(plan.stage_feats.items())))
    lines.append("stem_in " + _tdesc(plan.stem_in, ids))
    if plan.head is not None:
        for name in ("logits", "center", "delta_ctr", "corners"):
            v = getattr(plan.head, name)
            lines.append("head.%s %s" % (name, "None" if v is None else "; ".join(_tdesc(t, ids) for t in v)))
        lines.append("head.scales %r" % (list(plan.head.scales),))
    lines.append("wr_ws bytes=%d allocated=%s" % (plan.wr_ws.bytes, plan.wr_ws.t is not None))
    lines.append("pool bytes=%d" % plan.pool.bytes)
    for shape in sorted(plan.pool.free):
        lines.append("pool.free %s: %s" % (list(shape), "; ".join(ids(a.t.data_ptr()) for a in plan.pool.free[shape])))
    for k in sorted(P):
        lines.append("P[%s] %s" % (k, _pdesc(P[k])))
    return [c.kernel_name() for c in plan.calls], "\n".join(lines) + "\n"


# ----------------------------------------------------------------------------------------------------------------- matrix
_BASE = {}


def _released_weights(depth, fp8):
    from dafne_amd import engine
    from dafne_amd.engine_options import EngineOptions
    from oracle.model import make_params
    key = (depth, fp8)
    if key not in _BASE:
        sd = make_params(depth, NUM_CLASSES, seed=0)
        P = engine.pack_backbone_weights(sd, depth, CPU, fp8=fp8, options=EngineOptions())
        P.update(engine.pack_head_weights(sd, CPU, fp8=fp8, options=EngineOptions()))
        _BASE[key] = P
    return _BASE[key]


def _ablation_weights(strategy, centerness):
    """The trunk of oracle.model.make_params with an ablation head's parameters by name (tests/test_gpu_ablation_head.py's
    ablation_model, without the device)."""
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd import engine
    from dafne_amd.config import load_cfg
    from dafne_amd.engine_options import EngineOptions
    from dafne_amd.registry import build_model
    from oracle.model import fill_params, make_params
    key = (strategy, centerness)
    if key not in _BASE:
        cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"),
                       ["MODEL.DAFNE.CORNER_PREDICTION", strategy, "MODEL.DAFNE.CENTERNESS", centerness])
        m = build_model(cfg)
        fill_params(m.proposal_generator.dafne_head, seed=5)
        sd = m.state_dict()
        sd.update({k: v for k, v in make_params(50, NUM_CLASSES, seed=5).items() if k.startswith("backbone.")})
        P = engine.pack_backbone_weights(sd, 50, CPU, options=EngineOptions())
        P.update(engine.pack_head_weights(sd, CPU, options=EngineOptions()))
        _BASE[key] = P
    return _BASE[key]


def _options():
    """-> [(name, EngineOptions)]: the defaults, every field off, every single-field flip from each of the two."""
    from dafne_amd.engine_options import EngineOptions
    names = [f.name for f in dataclasses.fields(EngineOptions)]
    default = EngineOptions()
    plain = EngineOptions(**{f: False for f in names})
    out = [("default", default), ("plain", plain)]
    for f in names:
        out.append(("default^" + f, dataclasses.replace(default, **{f: not getattr(default, f)})))
        out.append(("plain^" + f, dataclasses.replace(plain, **{f: not getattr(plain, f)})))
    return out


def _tag(depth, shape):
    return "r%d-%dx%dx%d" % ((depth,) + tuple(shape))


def matrix():
    """-> [(plan name, build)]; build() -> (plan, P)."""
    from dafne_amd import engine
    from dafne_amd.engine_options import EngineOptions
    default = EngineOptions()
    plain = EngineOptions(**{f.name: False for f in dataclasses.fields(EngineOptions)})
    cases = []

    def add(name, base, depth, shape, opt, act_q8=None, outputs=None, **kw):
        def build():
            P = dict(base())
            P["options"] = opt
            if act_q8 is not None:
                P["act_q8"] = act_q8()
            if outputs is not None:
                kw["head_outputs"] = outputs(P)
            return engine.DensePlan(P, shape[0], shape[1], shape[2], depth, NUM_CLASSES, CPU, **kw), P
        assert name not in [c[0] for c in cases], name
        cases.append((name, build))

    for depth, shape in MODELS:
        t = _tag(depth, shape)
        rel = (lambda d: lambda: _released_weights(d, False))(depth)
        for oname, opt in _options():
            add("%s/%s" % (t, oname), rel, depth, shape, opt)
        add(t + "/c64-no-blk-narrow", rel, depth, shape, dataclasses.replace(default, conv_c64=True, fuse_blk_narrow=False))
        add(t + "/shared", rel, depth, shape, default, shared_gpu=True)
        add(t + "/shared-excl", rel, depth, shape, dataclasses.replace(default, shared_excl=True), shared_gpu=True)
        add(t + "/no-head", rel, depth, shape, default, with_head=False)
    # a sub-batch plan as the pipelined step builds it: images 1..2 of a batch of 3, writing into the whole batch's head outputs
    add("r50-sub-batch-1:3-of-3x128x160/shared", lambda: _released_weights(50, False), 50, (2, 128, 160), default, shared_gpu=True,
        outputs=lambda P: engine.HeadOutputs(3, 128, 160, NUM_CLASSES, P["scales"], CPU, head_mode=P["head_mode"]).views(1, 3))
    # the fp8 model: its calibration plan, then a plan with a scale for every layer the calibration plan probed
    for depth, shape in SMALL + [(50, (1, 544, 544))]:
        t = _tag(depth, shape)
        fp8w = (lambda d: lambda: _released_weights(d, True))(depth)
        for oname, opt in (("default", default), ("plain", plain)):
            def probed(fp8w=fp8w, depth=depth, shape=shape, opt=opt):
                P = dict(fp8w())
                P["options"] = opt
                plan = engine.DensePlan(P, shape[0], shape[1], shape[2], depth, NUM_CLASSES, CPU, calib={})
                return {c.key: 0.5 for c in plan.calls if isinstance(c, engine.AmaxProbe)}
            add("%s/fp8-calib-%s" % (t, oname), fp8w, depth, shape, opt, calib={})
            add("%s/fp8-q8-%s" % (t, oname), fp8w, depth, shape, opt, act_q8=probed)
    for strategy, centerness in (("direct", "none"), ("iterative", "plain")):
        ab = (lambda s, c: lambda: _ablation_weights(s, c))(strategy, centerness)
        for oname, opt in (("default", default), ("plain", plain)):
            add("r50-2x64x96/head-%s-%s-%s" % (strategy, centerness, oname), ab, 50, (2, 64, 96), opt)
    return cases


def dumps():
    """name -> (kernel names, dump) of the whole matrix."""
    from dafne_amd import build
    build.build()
    out = {}
    for name, make in matrix():
        plan, P = make()
        out[name] = fingerprint(plan, P)
    return out


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.fixture(scope="module")
def recorded():
    return dumps()          # (the matrix names every switch itself: the environment's DAFNE_* variables are not read)


def test_the_fixture_names_its_commit_and_every_plan(recorded):
    fx = json.load(open(FIXTURE))
    assert len(fx["commit"]) == 40 and "dirty" not in fx["commit"]
    assert sorted(fx["plans"]) == sorted(recorded)
    assert len(recorded) >= 148


def test_launch_lists_equal_the_fixtures(recorded):
    fx = json.load(open(FIXTURE))["plans"]
    bad = []
    for name in sorted(recorded):
        kernels, text = recorded[name]
        if kernels != fx[name]["kernels"]:
            k = next((i for i, (a, b) in enumerate(zip(kernels, fx[name]["kernels"])) if a != b), min(len(kernels), len(fx[name]["kernels"])))
            bad.append("%s: launch %d is %s, recorded %s (%d / %d launches)"
                       % (name, k, (kernels + ["-"])[k], (fx[name]["kernels"] + ["-"])[k], len(kernels), len(fx[name]["kernels"])))
        elif _sha(text) != fx[name]["sha256"]:
            bad.append("%s: same %d kernels, another argument / keep / buffer / weight-key dump" % (name, len(kernels)))
    assert not bad, ("%d of %d plans differ from commit %s (python tests/test_plan_launch_lists_cpu.py --dump DIR on both trees, "
                     "then diff):\n" % (len(bad), len(recorded), json.load(open(FIXTURE))["commit"][:12]) + "\n".join(bad[:20]))


def test_every_pointer_argument_of_an_fncall_is_kept(recorded):
    """What makes the dump reproducible: a pointer argument whose tensor the call does not keep belongs to nobody."""
    for name, (_, text) in recorded.items():
        lines = text.split("\n")
        for i, l in enumerate(lines):
            if l.startswith("  args "):
                kept = set(d.split(" ")[0] for d in lines[i + 1][len("  keep "):].split("; "))
                ptrs = set(a for a in l[len("  args "):].replace("[", " ").replace("]", " ").replace("{", " ").replace("}", " ")
                           .replace(",", " ").replace("=", " ").split() if a[:1] == "p" and a[1:].isdigit())
                assert ptrs <= kept, (name, lines[i - 2], sorted(ptrs - kept))


# ------------------------------------------------------------------------------------------------------------------ script
def _source_commit():
    import subprocess
    import dafne_amd
    tree = os.path.dirname(os.path.dirname(os.path.abspath(dafne_amd.__file__)))
    sha = subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    dirty = subprocess.run(["git", "-C", tree, "status", "--porcelain", "--", "dafne_amd", "oracle", "include"],
                           stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    return sha + ("+dirty" if dirty else "")


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.append(ROOT)            # (behind PYTHONPATH: --write runs against the checkout named there)
    d = dumps()
    if "--write" in sys.argv:
        fx = {"commit": _source_commit(), "plans": {n: {"kernels": k, "sha256": _sha(t)} for n, (k, t) in sorted(d.items())}}
        with open(FIXTURE, "w") as f:             # one plan per line
            f.write('{"commit": %s,\n"plans": {\n' % json.dumps(fx["commit"]))
            f.write(",\n".join("%s: %s" % (json.dumps(n), json.dumps(p, sort_keys=True, separators=(",", ":")))
                               for n, p in fx["plans"].items()))
            f.write("\n}}\n")
        print("wrote %d plans from commit %s to %s" % (len(d), fx["commit"], FIXTURE))
    elif "--dump" in sys.argv:
        out = sys.argv[sys.argv.index("--dump") + 1]
        os.makedirs(out, exist_ok=True)
        for n, (k, t) in d.items():
            with open(os.path.join(out, n.replace("/", "__").replace("^", "~").replace(":", "_") + ".txt"), "w") as f:
                f.write(t)
        print("dumped %d plans to %s" % (len(d), out))
    else:
        for n, (k, t) in sorted(d.items()):
            print(_sha(t)[:16], len(k), n)
