"""GPU: the device SGD step (dafne_sgd_step_hip, csrc/solver_kernels.h; dafne_amd/solver.py DeviceSGD) -- (a) the kernel alone on
synthetic tensors against the NumPy oracle of tests/_solver_np.py and the engine's own pack functions, every bit; (b) the model
route, backward_towers + DeviceSGD.step() against the same backward + the oracle on the host + invalidate(), every bit of the
losses, the parameters, the scales and the detections, with the packed weights, plans and pointers left in place; (c) the
guards; (d) tools/finetune_pred.py --device-solver --lr-schedule.  tests/test_solver_cpu.py pins the oracle to torch.optim.SGD on
the same synthetic inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _solver_np as S
import _targets_np as tn
from test_gpu_tail_backward import ROOT, dev, labelled_batch, released_model

pytestmark = pytest.mark.gpu


def _eq(a, b):
    return bool(torch.equal(S.bits(a), S.bits(b)))


# ------------------------------------------------------------------------------------------------ (a) the kernel alone
class Synthetic:
    """The synthetic tensors on the device with their packed destinations, and the descriptor table over them."""

    def __init__(self, wd):
        from dafne_amd import _lib
        self.L = _lib.load()
        d = dev()
        self.wd = wd
        p0 = S.synthetic_params()
        self.p = {n: v.to(d) for n, v in p0.items()}
        self.g = {n: torch.zeros_like(v) for n, v in self.p.items()}
        self.buf = {n: torch.full_like(v, float("nan")) for n, v in self.p.items()}        # never read on the first step
        self.addend = S.synthetic_addend().to(d)
        self.scales_out = torch.zeros(5, device=d)
        self.dst = {}
        self.dst.update(self.expected(p0))
        self.dst = {k: v.to(d).contiguous() for k, v in self.dst.items()}
        self.desc = (_lib.SgdTensor * len(S.SYNTHETIC))()
        for i, (n, shape, f) in enumerate(S.SYNTHETIC):
            t = self.desc[i]
            t.d_p, t.d_g, t.d_buf, t.n = self.p[n].data_ptr(), self.g[n].data_ptr(), self.buf[n].data_ptr(), self.p[n].numel()
            t.lr_factor, t.weight_decay = f, wd
            if n.startswith("scale"):
                t.form, t.d_copy = _lib.SGD_F32, self.scales_out.data_ptr() + 4 * int(n[5:])
            elif n == "gn_w":
                t.form, t.d_copy = _lib.SGD_F32, self.dst["gn_w"].data_ptr()
            elif n == "gn_b":
                t.form, t.d_copy, t.d_addend = _lib.SGD_F32, self.dst["gn_b"].data_ptr(), self.addend.data_ptr()
            elif n == "bias15":
                t.form, t.d_copy = _lib.SGD_F32, self.dst["m15.bias"].data_ptr()
            else:
                key, row0 = {"w15": ("m15", 0), "w8": ("m9", 0), "w1": ("m9", 8), "w2": ("m2", 0), "w256_frag": ("ma", 0),
                             "w256_frag16": ("mb", 0)}[n]
                t.form, t.d_plain = _lib.SGD_CONV, self.dst[key].data_ptr()
                t.Cout, t.Cin, t.KH, t.KW, t.row0, t.rows = shape[0], shape[1], shape[2], shape[3], row0, self.dst[key].shape[0]
                if n == "w256_frag":
                    t.d_frag = self.dst["ma.frag"].data_ptr()
                if n == "w256_frag16":
                    t.d_frag16 = self.dst["mb.frag16"].data_ptr()
        nb = self.L.dafne_sgd_table_bytes(self.desc, len(self.desc))
        assert nb > 0, self.L.dafne_last_error()
        host = torch.empty(nb, dtype=torch.uint8)
        _lib.check(self.L.dafne_sgd_table_build(self.desc, len(self.desc), ctypes.c_void_p(host.data_ptr()), nb), "table")
        self.table, self.nbytes = host.to(d), nb

    def expected(self, p):
        """{destination: tensor} the packed copies must equal for the masters p ({name: CPU tensor or array})."""
        p = {n: torch.as_tensor(np.asarray(v)) for n, v in p.items()}
        out = {"gn_w": p["gn_w"].clone(), "gn_b": p["gn_b"] + S.synthetic_addend()}
        out["m15"], out["m15.bias"] = S.packed_plain([p["w15"]], p["bias15"])
        out["m9"], _ = S.packed_plain([p["w8"], p["w1"]])
        out["m2"], _ = S.packed_plain([p["w2"]])
        out["ma"], _ = S.packed_plain([p["w256_frag"]])
        out["mb"], _ = S.packed_plain([p["w256_frag16"]])
        out["ma.frag"] = S.packed_form(out["ma"], "frag")
        out["mb.frag16"] = S.packed_form(out["mb"], "frag16")
        return out

    def step(self, k, zero_grad):
        from dafne_amd import _lib
        for n, g in S.synthetic_grads(k).items():
            self.g[n].copy_(g)
        _lib.check(self.L.dafne_sgd_step_hip(self.desc, len(self.desc), _lib.ptr(self.table), self.nbytes, S.SYNTHETIC_LR,
                                             S.SYNTHETIC_MOMENTUM, int(k == 0), int(zero_grad), _lib.current_stream()), "step")
        torch.cuda.synchronize()


@pytest.mark.parametrize("wd,zero_grad", [(S.SYNTHETIC_WD[0], True), (S.SYNTHETIC_WD[1], False)])
def test_kernel_two_steps_equal_the_oracle_and_the_pack_functions(wd, zero_grad):
    with torch.cuda.device(dev()):
        s = Synthetic(wd)
        assert s.dst["m15"].shape[0] > 15, "the padded rows are part of the test"
        want = S.oracle_run(wd, 2)
        for k in range(2):
            s.step(k, zero_grad)
            grads = S.synthetic_grads(k)
            for n, _, _ in S.SYNTHETIC:
                wp, wb = want[k][n]
                assert _eq(s.p[n], torch.from_numpy(wp)), (k, n, "p")
                assert _eq(s.buf[n], torch.from_numpy(wb)), (k, n, "buf")
                assert _eq(s.g[n], torch.zeros_like(grads[n]) if zero_grad else grads[n]), (k, n, "g")
            exp = s.expected({n: want[k][n][0] for n, _, _ in S.SYNTHETIC})
            for key, t in exp.items():
                assert _eq(s.dst[key], t), (k, key)
            assert not bool(s.dst["m15"][15:].any()) and not bool(s.dst["m15.bias"][15:].any()), "padding rows must stay 0"
            assert not bool(s.dst["m9"][9:].any()) and not bool(s.dst["m2"][2:].any())
            assert _eq(s.scales_out, torch.from_numpy(np.concatenate([want[k]["scale%d" % l][0] for l in range(5)])))


def test_bf16_rounding_ties_and_specials():
    from dafne_amd import _lib
    L = _lib.load()
    special = np.array([0x3F808000,      # 1 + 2^-8: a tie, down to even (0x3F80)
                        0x3F818000,      # 1 + 3 * 2^-8: a tie, up to even (0x3F82)
                        0x3F7FFFFF,      # carries into the exponent: 1.0
                        0x00000000, 0x80000000, 0x00012345, 0x7F800000, 0xFF800000, 0x7FC00001,
                        0x3F808001, 0x3F807FFF, 0x7F7FFFFF], dtype=np.uint32).view(np.float32)
    rng = np.random.default_rng(3)
    vals = np.concatenate([special, rng.standard_normal(64 - special.size).astype(np.float32)])
    with torch.cuda.device(dev()):
        p = torch.from_numpy(vals.copy()).reshape(1, 64, 1, 1).to(dev())
        g, buf = torch.zeros_like(p), torch.zeros_like(p)
        plain = torch.zeros(1, 64, dtype=torch.bfloat16, device=dev())
        desc = (_lib.SgdTensor * 1)()
        t = desc[0]
        t.d_p, t.d_g, t.d_buf, t.n, t.lr_factor, t.weight_decay = p.data_ptr(), g.data_ptr(), buf.data_ptr(), 64, 1.0, 0.0
        t.form, t.d_plain, t.Cout, t.Cin, t.KH, t.KW, t.row0, t.rows = _lib.SGD_CONV, plain.data_ptr(), 1, 64, 1, 1, 0, 1
        nb = L.dafne_sgd_table_bytes(desc, 1)
        host = torch.empty(nb, dtype=torch.uint8)
        _lib.check(L.dafne_sgd_table_build(desc, 1, ctypes.c_void_p(host.data_ptr()), nb), "table")
        table = host.to(dev())
        _lib.check(L.dafne_sgd_step_hip(desc, 1, _lib.ptr(table), nb, 0.0, 0.9, 1, 0, _lib.current_stream()), "step")
        torch.cuda.synchronize()
    got_p = p.cpu().numpy().reshape(-1)
    nan = np.isnan(vals)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got_p), nan)
    assert np.array_equal(got_p.view(np.uint32)[~nan], vals.view(np.uint32)[~nan]), "gradient 0 and lr 0 leave p as it was"
    want = torch.from_numpy(vals).to(torch.bfloat16)
    got = plain.cpu().reshape(-1)
    assert np.array_equal(torch.isnan(got.float()).numpy(), nan)
    keep = torch.from_numpy(~nan)
    assert torch.equal(got.view(torch.int16)[keep], want.view(torch.int16)[keep])
    assert [int(v) & 0xFFFF for v in got.view(torch.int16)[:3]] == [0x3F80, 0x3F82, 0x3F80]


def test_a_bad_descriptor_is_an_error_and_changes_nothing():
    from dafne_amd import _lib
    L = _lib.load()
    with torch.cuda.device(dev()):
        p = torch.randn(4, 64, 3, 3, device=dev())
        g, buf = torch.randn_like(p), torch.randn_like(p)
        plain = torch.ones(16, 576, dtype=torch.bfloat16, device=dev())
        copy = torch.ones(4 * 64 * 9, device=dev())
        table = torch.zeros(4096, dtype=torch.uint8, device=dev())
        before = [t.clone() for t in (p, g, buf, plain, copy)]

        def desc(**kw):
            d = (_lib.SgdTensor * 1)()
            t = d[0]
            t.d_p, t.d_g, t.d_buf, t.n, t.lr_factor, t.weight_decay = p.data_ptr(), g.data_ptr(), buf.data_ptr(), p.numel(), 1.0, 0.0
            t.form, t.d_plain, t.Cout, t.Cin, t.KH, t.KW, t.row0, t.rows = _lib.SGD_CONV, plain.data_ptr(), 4, 64, 3, 3, 0, 16
            for k, v in kw.items():
                setattr(t, k, v)
            return d
        assert L.dafne_sgd_table_bytes(desc(), 1) == 128 + 16          # (the good descriptor is served: one chunk)
        cases = {"Cin % 64": desc(Cin=32, n=4 * 32 * 9), "unknown form": desc(form=7), "null d_plain": desc(d_plain=None),
                 "F32 without d_copy": desc(form=_lib.SGD_F32), "null gradient": desc(d_g=None),
                 "rows outside the matrix": desc(row0=13), "fragment form on 16 rows": desc(d_frag=plain.data_ptr()),
                 "misaligned": desc(d_p=p.data_ptr() + 4), "5x5 taps": desc(KH=5, KW=5, n=4 * 64 * 25)}
        for what, d in cases.items():
            assert L.dafne_sgd_table_bytes(d, 1) == 0 and L.dafne_sgd_num_chunks(d, 1) == -1, what
            rc = L.dafne_sgd_step_hip(d, 1, _lib.ptr(table), 4096, 0.1, 0.9, 1, 1, _lib.current_stream())
            msg = L.dafne_last_error().decode()
            assert rc != 0 and "sgd: tensor 0" in msg, (what, rc, msg)
        torch.cuda.synchronize()
        for t, b in zip((p, g, buf, plain, copy), before):
            assert _eq(t, b)


# ------------------------------------------------------------------------------------------------ (b) the model route
def _twin(cfg, m):
    """A second model with m's weights."""
    from dafne_amd.registry import build_model
    t = build_model(cfg)
    t.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    t.to(dev())
    t.invalidate()
    return t


def _images(inputs):
    return torch.stack([x["image"] for x in inputs]).to(dev())


class HostSGD:
    """Route B: the oracle on the host, then invalidate()."""

    def __init__(self, model, params, lr, momentum, groups):
        self.model, self.params, self.lr, self.momentum, self.groups = model, params, lr, momentum, groups
        self.buf = [None] * len(params)
        self.steps = 0

    def step(self):
        for i, p in enumerate(self.params):
            new_p, self.buf[i] = S.sgd_step(p.detach().cpu().numpy(), p.grad.detach().cpu().numpy(), self.buf[i], self.lr, self.momentum,
                                            self.steps == 0, lr_factor=self.groups[i]["lr_factor"], wd=self.groups[i]["weight_decay"])
            p.data.copy_(torch.from_numpy(new_p))
        self.steps += 1
        self.model.zero_grad(set_to_none=True)
        self.model.invalidate()


def _head_keys(P):
    return [k for k in P if k.split(".")[0] in ("cls_tower", "corners_tower", "center_tower", "cls_logits", "center_pred",
                                                "corners_ctrness")]


def _tensors(v):
    return [t for t in (v if isinstance(v, (tuple, list)) else (v,)) if torch.is_tensor(t)]


def _assert_packed_like_fresh(m):
    """Every head entry of a fresh pack of the parameters equals the model's packed tensors, the derived forms included."""
    from dafne_amd import engine
    P = m._packed
    fresh = engine.pack_model_weights(m.state_dict(), m.depth, m.device, weight_dtype=m.cfg.ENGINE.WEIGHT_DTYPE,
                                      fp8_kernel=m.cfg.ENGINE.FP8_CONV3X3_KERNEL)
    assert fresh["scales"] == P["scales"]
    for k in _head_keys(fresh):
        got, want = _tensors(P[k]), _tensors(fresh[k])
        assert len(got) == len(want) and all(_eq(a, b) for a, b in zip(got, want)), k
    derived = [k for k in _head_keys(P) if k not in fresh]
    for k in derived:
        base, form = k.rsplit(".", 1)
        assert _eq(P[k], S.packed_form(fresh[base][0], form)), k
    return derived


def _head_alone(m, feats):
    """The stand-alone head module on FPN-shaped maps (DAFNeHead.run_raw: its OWN packed copy and plans) -> clones of its raw
    outputs and its scales."""
    hp = m.proposal_generator.dafne_head.run_raw(feats)
    outs = [t.clone() for t in hp.logits + hp.delta_ctr + (hp.center if hp.center is not None else [])]
    torch.cuda.synchronize()
    return outs, list(hp.scales)


def _run_routes(cfg, ma, params_of, backward_of, steps, lr, momentum, wd, mid_detect=None):
    """mid_detect: (n, h, w) of a detect_packed on route A between the first and the second step, at a shape whose plan packs a
    fragment-major form of a trained layer that no plan needed before: the next step rebuilds and uploads its table."""
    from dafne_amd.solver import DeviceSGD
    inputs = labelled_batch()
    mb = _twin(cfg, ma)
    g = torch.Generator().manual_seed(6)
    feats = [torch.randn(1, 256, h, w, generator=g).to(dev()) for h, w in ((8, 12), (4, 6), (2, 3), (1, 2), (1, 1))]
    head_a0, scales_a0 = _head_alone(ma, feats)             # the head module holds a packed copy of its own from here on
    head_b0, scales_b0 = _head_alone(mb, feats)
    assert scales_a0 == scales_b0 and all(_eq(a, b) for a, b in zip(head_a0, head_b0))
    ma.zero_grad(set_to_none=True)
    pa, pb = params_of(ma), params_of(mb)
    # the plans and every lazily packed form exist before the first step: one forward + backward that is thrown away
    backward_of(ma)(inputs)
    ma.zero_grad(set_to_none=True)
    opt_a = DeviceSGD(ma, pa, lr=lr, momentum=momentum, weight_decay=wd)
    opt_b = HostSGD(mb, pb, lr, momentum, opt_a.groups)
    packed = ma._packed
    plans = dict(ma._plans)
    ptrs = {k: [t.data_ptr() for t in _tensors(v)] for k, v in packed.items()}
    scales_list = packed["scales"]
    trunk = {k: [t.clone() for t in _tensors(v)] for k, v in packed.items() if k not in _head_keys(packed)}
    assert plans and any(k.startswith("res") for k in trunk) and any(k.startswith("fpn_") for k in trunk)
    start = [p.detach().clone() for p in pa]
    for k in range(steps):
        la = backward_of(ma)(inputs)
        opt_a.step()
        lb = backward_of(mb)(inputs)
        opt_b.step()
        torch.cuda.synchronize()
        assert sorted(la) == sorted(lb)
        for key in la:
            assert _eq(la[key], lb[key]), (k, key)
        for n, a, b in zip(opt_a.names, pa, pb):
            assert _eq(a, b), (k, n)
        assert ma._packed["scales"] == mb._weights()["scales"], k
        assert all(not bool(p.grad.any()) for p in pa), "step() zeroes the gradient arena"
        # the head module run on its own serves the new parameters too, as a freshly packed twin does
        head_a, scales_a = _head_alone(ma, feats)
        head_b, scales_b = _head_alone(mb, feats)
        assert scales_a == scales_b == ma._packed["scales"], k
        assert all(_eq(a, b) for a, b in zip(head_a, head_b)), (k, "DAFNeHead.run_raw after a step")
        assert not all(_eq(a, b) for a, b in zip(head_a, head_a0)), (k, "the head module still serves the old weights")
        if mid_detect is not None and k == 0:
            keys0 = set(ma._packed)
            n, h, w = mid_detect
            ma.detect_packed(torch.randint(0, 256, (n, 3, h, w), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).to(dev()))
            torch.cuda.synchronize()
            gained = set(ma._packed) - keys0
            trained = set(key for _, key, _, _ in opt_a.places if key is not None)
            assert any(key.rsplit(".", 1)[0] in trained for key in gained), ("no new form of a trained layer was packed", gained)
            table0 = opt_a._table
    assert all(not _eq(p, s) for p, s in zip(pa, start)), "a parameter did not move"
    ims = _images(inputs)
    ra, ca = ma.detect_packed(ims)
    rb, cb = mb.detect_packed(ims)
    torch.cuda.synchronize()
    assert _eq(ca, cb) and int(ca.min()) > 0
    for i, c in enumerate(ca.tolist()):                     # (rows past an image's count are not written)
        assert _eq(ra[i, :c], rb[i, :c]), i
    # nothing was rebuilt
    assert ma._packed is packed and packed["scales"] is scales_list
    assert all(ma._plans.get(k) is v for k, v in plans.items())
    for k, v in ptrs.items():
        assert [t.data_ptr() for t in _tensors(packed[k])] == v, k
    for k, v in trunk.items():
        assert all(_eq(a, b) for a, b in zip(_tensors(packed[k]), v)), k
    derived = _assert_packed_like_fresh(ma)
    if mid_detect is not None:
        assert opt_a._table is not table0 and gained <= opt_a._table["keys"], "the table was rebuilt over the new forms"
        assert gained <= set(derived), "the forms packed between two steps are compared with a fresh pack"
    ma.zero_grad(set_to_none=True)
    return opt_a, derived


def test_three_tower_steps_equal_the_host_route_bit_for_bit():
    cfg, m = released_model()
    with torch.cuda.device(dev()):
        opt, derived = _run_routes(cfg, m, lambda x: x.tower_parameters(), lambda x: x.backward_towers, 3, 0.01, 0.9, 1e-4,
                                   mid_detect=(4, 512, 640))
    assert len(opt.params) == 45 and opt.steps == 3
    assert any(k.endswith(".frag") or k.endswith(".frag16") for k in derived), "the tower layers run on a fragment-major form"
    # state: a resumed solver continues with the same momentum
    sd = opt.state_dict()
    assert sd["steps"] == 3 and sorted(sd["momentum"]) == sorted(opt.names)
    assert all(bool(v.abs().sum() > 0) for v in sd["momentum"].values())


@pytest.mark.parametrize("strategy,centerness", [("offset", "plain"), ("direct", "plain"), ("center-to-corner", "none")])
def test_one_prediction_step_on_the_other_heads(strategy, centerness):
    from test_gpu_ablation_head import ablation_model
    cfg, m = ablation_model(strategy, centerness)
    saved = {k: v.detach().clone() for k, v in m.state_dict().items()}
    try:
        with torch.cuda.device(dev()):
            opt, _ = _run_routes(cfg, m, lambda x: x.prediction_parameters(), lambda x: x.backward_prediction_layers, 1, 0.01, 0.9,
                                 1e-4)
            P = m._packed
            head = m.proposal_generator.dafne_head
            w, b = P["corners_ctrness"]
            if centerness == "none":
                assert not any("ctrness" in n for n in opt.names) and not bool(w[8:].any()) and not bool(b[8:].any())
            if strategy == "offset":
                want = head.corners_pred.bias.detach().float().cpu() + head.base_corners.detach().float().cpu().reshape(8)
                assert _eq(b[:8], want), "the packed bias is bias + base_corners"
    finally:
        m.zero_grad(set_to_none=True)
        m.load_state_dict(saved)


# ------------------------------------------------------------------------------------------------ (c) guards
def test_guards():
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from dafne_amd.solver import DeviceSGD
    from test_gpu_ablation_head import ablation_model
    cfg, m = released_model()
    inputs = labelled_batch()
    with torch.cuda.device(dev()):
        opt = DeviceSGD(m, m.prediction_parameters(), lr=0.01)
        m.backward_prediction_layers(inputs)
        before = [p.detach().clone() for p in opt.params]
        m.zero_grad(set_to_none=True)                       # replaces every .grad
        with pytest.raises(RuntimeError, match=r"\.grad"):
            opt.step()
        opt.zero_grad()                                     # the solver's own: the views are back
        m.backward_prediction_layers(inputs)
        m._weights()["cls_logits.bogus"] = torch.zeros(1, device=dev())
        with pytest.raises(RuntimeError, match="cls_logits.bogus"):
            opt.step()
        torch.cuda.synchronize()
        assert all(_eq(p, b) for p, b in zip(opt.params, before)), "a refused step changes nothing"
        del m._weights()["cls_logits.bogus"]
        opt.step()
        torch.cuda.synchronize()
        assert not _eq(opt.params[0], before[0]) and not _eq(opt.params[1], before[1]), "cls_logits did not move"
        m.zero_grad(set_to_none=True)
        m.invalidate()
    _, it = ablation_model("iterative", "plain")
    with pytest.raises(NotImplementedError):
        DeviceSGD(it, [it.proposal_generator.dafne_head.cls_logits.weight], lr=0.01)
    m8 = build_model(load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), ["ENGINE.WEIGHT_DTYPE", "fp8_e4m3"]))
    with pytest.raises(NotImplementedError):
        DeviceSGD(m8, m8.prediction_parameters(), lr=0.01)


# ------------------------------------------------------------------------------------------------ (d) the tool
def test_finetune_tool_with_the_device_solver_runs_on_a_scene_directory(tmp_path, capsys):
    """tools/finetune_pred.py --towers --device-solver --lr-schedule on the scene directory of tests/test_gpu_tower_backward.py's
    tool test: two steps, finite losses, a checkpoint that loads completely into a fresh model and in which the trained layers
    moved and nothing else did."""
    import json
    import sys
    from PIL import Image
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.checkpoint import load_weights, save_checkpoint
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    cfg, m = released_model()
    start = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    save_checkpoint(m, str(tmp_path / "start.pth"))
    rng = np.random.default_rng(4)
    sd, ld = tmp_path / "scenes", tmp_path / "labelTxt"
    sd.mkdir()
    ld.mkdir()
    classes = ["plane", "ship", "harbor"]
    for name, (h, w) in (("P0001", (200, 260)), ("P0002", (180, 150))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(sd / (name + ".png"))
        rows = ["imagesource:GoogleEarth", "gsd:0.146"]
        for q in tn.random_quads(10, rng, h, w, lo=16.0, hi=48.0):
            rows.append(" ".join("%.1f" % v for v in q) + " %s 0" % classes[int(rng.integers(0, 3))])
        (ld / (name + ".txt")).write_text("\n".join(rows) + "\n")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import finetune_pred
    finally:
        sys.path.pop(0)
    out = tmp_path / "tuned.pth"
    capsys.readouterr()
    rc = finetune_pred.main(["--config-file", os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"), "--weights", str(tmp_path / "start.pth"),
                             "--scene-dir", str(sd), "--scene-labels", str(ld), "--steps", "2", "--batch", "2", "--patch-size", "128",
                             "--overlap", "32", "--lr", "0.003", "--seed", "1", "--towers", "--device-solver", "--lr-schedule",
                             "--out", str(out), "INPUT.MIN_SIZE_TRAIN", "[96, 128, 160]", "INPUT.MAX_SIZE_TRAIN", "192",
                             "SOLVER.WARMUP_ITERS", "2", "SOLVER.WARMUP_FACTOR", "0.5"])
    torch.cuda.synchronize()
    assert rc == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [0, 1]
    for l in lines:
        assert all(np.isfinite(l[k]) for k in l if k.startswith("loss/")) and l["loss/total"] > 0
    fresh = build_model(load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml")))
    missing, unexpected = load_weights(fresh, str(out))
    assert missing == [] and unexpected == []
    tuned = fresh.state_dict()
    allowed = ["cls_logits.", "corners_pred.", "ctrness.", "center_pred.", "scales.", "cls_tower.", "corners_tower."]
    moved = [k for k in tuned if not torch.equal(tuned[k].cpu(), start[k])]
    assert moved and all(any(("dafne_head." + p) in k for p in allowed) for k in moved), moved[:5]
    for t in ("cls_tower", "corners_tower"):
        for i in range(4):
            for k in ("%d.weight" % (3 * i), "%d.bias" % (3 * i), "%d.weight" % (3 * i + 1), "%d.bias" % (3 * i + 1)):
                assert any(k2.endswith("dafne_head.%s.%s" % (t, k)) for k2 in moved), (t, k)
