"""CPU: the gradient of the DAFNe losses with respect to the head outputs.

  * the numpy restatement (tests/_targets_grad_np.py) against the reference's own autograd in fp64
    (tests/golden/dafne_targets_grad.npz).  The two differ only through the centerness target (the engine takes the
    reference's fp32 ratio and raises it in fp64), one fp32 rounding of a weight -- the size of the reference's own fp32
    rounding.  The bound is therefore 4 x the largest |fp32 - fp64| the fixture's maker saw in that tensor (4 x covers the
    ratio's three fp32 operations), not a number chosen here.  Measured: the largest ratio is 0.47 (profiles/NOTES_targets.md).
  * which elements are exactly zero equals the reference's, element for element
  * the autograd plumbing of DAFNeOutputs.losses() with the kernels replaced by the restatement
  * the ABI
"""
import os

import numpy as np
import pytest
import torch

import _targets_np as tn
import _targets_grad_np as gn

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dafne_targets_grad.npz")
TENSORS = ("logits", "corners", "center", "ctr")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def small():
    return gn.small_grad_case()


def compare(got, want, maxdiff, tag, ratios):
    """got: the restatement; want: the reference in fp64; maxdiff: the reference's own max |fp32 - fp64| of this tensor."""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got == 0, want == 0), (tag, "zero pattern", np.argwhere((got == 0) != (want == 0))[:5])
    err = float(np.abs(got - want).max()) if got.size else 0.0
    ratio = err / maxdiff if maxdiff > 0 else (0.0 if err == 0 else np.inf)
    ratios.append(ratio)
    print(tag, "max |restatement - fp64| %.3e, reference's max |fp32 - fp64| %.3e, ratio %.3f" % (err, maxdiff, ratio))
    assert err <= 4.0 * maxdiff, (tag, err, maxdiff)


def test_restatement_small_case(gold, small):
    _, _, tg, preds = small
    pos = gold["s_pos"]
    assert np.array_equal(pos, np.nonzero(tg["labels"] != 15)[0])
    keys = list(gold["s_logit_keys"])
    assert len(keys) == 3
    ratios = []
    for name, Lc in tn.loss_configs():
        g = gn.grads(preds[0], preds[1], preds[2], preds[3], tg, Lc)
        md = gold["s_%s_maxdiff" % name]
        compare(g["logits"], gold["s_logits_%d" % keys.index(gn.lam_cls_key(Lc))], md[0], (name, "logits"), ratios)
        for i, k in enumerate(TENSORS[1:], 1):
            if g[k] is None:
                assert "s_%s_%s" % (name, k) not in gold.files
                continue
            rest = np.ones(g[k].shape[0], bool)
            rest[pos] = False
            assert not g[k][rest].any(), (name, k, "a gradient at a non-positive")
            compare(g[k][pos].reshape(len(pos), -1), gold["s_%s_%s" % (name, k)].reshape(len(pos), -1), md[i], (name, k), ratios)
    print("largest ratio over the small case: %.3f" % max(ratios))


def test_restatement_handmade(gold):
    th, hp, where = gn.handmade_grad_case()
    ratios = []
    for name, Lc in gn.handmade_configs():
        g = gn.grads(hp[0], hp[1], hp[2], hp[3], th, Lc)
        md = gold["h_%s_maxdiff" % name]
        for i, k in enumerate(TENSORS):
            compare(g[k], gold["h_%s_%s" % (name, k)], md[i], (name, k), ratios)
        gc = g["corners"].reshape(-1, 4, 2)
        assert not g["corners"][where["n_zero"]].any() and not g["center"][where["n_zero"]].any()
        if Lc["sort_corners"]:      # [0,0, 1,1, 2,2, 3,3]: the sorted output is all zeros, only the leftmost corner is an input
            assert gc[where["collinear"], 0].all() and not gc[where["collinear"], 1:].any()
            assert not gc[where["all_equal"], 1:].any()
            assert (gc[where["three_collinear"]] == 0).all(1).any(), "three collinear points: a corner without a gradient"
        else:
            assert gc[where["collinear"]].all()
    print("largest ratio over the handmade cases: %.3f" % max(ratios))


@pytest.mark.parametrize("kind", ["zero_ctr", "nan_ctr"])
@pytest.mark.parametrize("mode", ["oriented", "plain"])
def test_restatement_handmade_centerness(gold, kind, mode):
    tz = tn.handmade_targets(kind)
    pz = tn.case_b_predictions(tz, seed=23)
    g = gn.grads(pz[0], pz[1], pz[2], pz[3], tz, dict(tn.LOSS_RELEASED, ctr_mode=mode))
    md = gold["z_%s_%s_maxdiff" % (kind, mode)]
    for i, k in enumerate(TENSORS):
        compare(g[k], gold["z_%s_%s_%s" % (kind, mode, k)], md[i], (kind, mode, k), [])


def test_restatement_no_positives(gold):
    th, hp, _ = gn.handmade_grad_case()
    t0 = dict(th, labels=np.full(64, 15, np.int64))
    g = gn.grads(hp[0], hp[1], hp[2], hp[3], t0, tn.LOSS_RELEASED)
    for i, k in enumerate(TENSORS):
        compare(g[k], gold["n_%s" % k], gold["n_maxdiff"][i], ("nopos", k), [])
        if k != "logits":
            assert not g[k].any()


def test_sort_sources_agree_with_the_sort():
    from dafne_amd.data.targets import sort_quadrilateral_np
    rng = np.random.default_rng(4)
    q = tn.random_quads(500, rng, 100, 100)
    q[:6] = [[0, 0, 1, 1, 2, 2, 3, 3], [1, 1, 1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 2, 2, 1, 5], [1, 4, 1, 0, 5, 0.5, 4, 5],
             [3, 3, 2, 2, 1, 1, 0, 0], [0, 0, 0, 1, 0, 2, 0, 3]]
    s, src = gn.sort_with_sources(q)
    assert np.array_equal(s.view(np.uint32), sort_quadrilateral_np(q).view(np.uint32))
    q4 = q.reshape(-1, 4, 2)
    for j in range(4):
        ok = src[:, j] >= 0
        assert np.array_equal(s.reshape(-1, 4, 2)[ok, j], q4[ok, src[ok, j]])
        assert not s.reshape(-1, 4, 2)[~ok, j].any()
    assert (src[0] == [0, -1, -1, -1]).all() and (src[1] == [0, -1, -1, -1]).all() and (src[4] == [3, -1, -1, -1]).all()
    live = (src >= 0).all(1)
    assert live[6:].all() and (np.sort(src[live], axis=1) == np.arange(4)).all()


# ------------------------------------------------------------------------------------------------ autograd plumbing
class _FakeTargets:
    def __init__(self, tg, n, shapes):
        self.np, self.n_images, self.shapes = tg, n, [tuple(s) for s in shapes]
        self.P = tg["labels"].shape[0]
        self.labels = torch.from_numpy(tg["labels"].astype(np.int32))
        self.corners, self.ltrb, self.abcd = (torch.from_numpy(tg[k]) for k in ("corners", "ltrb", "abcd"))


def _flat(levels, attr):
    ts = [getattr(lv, attr) for lv in levels]
    if ts[0] is None:
        return None
    return np.concatenate([t.reshape(-1, t.shape[3]).numpy() for t in ts])


@pytest.fixture()
def stubbed(monkeypatch, small):
    """DAFNeOutputs whose three device calls are the numpy restatements, on CPU tensors."""
    from test_gpu_targets import make_outputs
    from dafne_amd.modeling.dafne import loss_function as lf
    _, shapes, tg, preds = small
    Lc = tn.LOSS_RELEASED
    outs = make_outputs(Lc=Lc)
    calls = {"forward": 0, "backward": 0}

    def assign_targets(shp, gt_instances, device):
        assert [tuple(s) for s in shp] == [tuple(s) for s in shapes]
        return _FakeTargets(tg, 2, shapes)

    def dafne_losses_packed(levels, targets, cooked=False, want_ctr_targets=False, _call=None):
        assert cooked
        calls["forward"] += 1
        ctr = _flat(levels, "ctrness")
        e = tn.losses(_flat(levels, "logits"), _flat(levels, "delta"), _flat(levels, "center"), ctr[:, 0], targets.np, Lc)
        row = torch.tensor([e["cls"], e["corners"], e["center"], e["ctr"], e["num_pos"], e["loss_denorm"]], dtype=torch.float64)
        r32 = row.to(torch.float32)
        if _call is not None:
            _call.update(prm=None, descs=None, ws=None, ws_bytes=0)
        return ({"loss_denorm": r32[5], "num_pos": r32[4], "values_f64": row},
                {"loss/cls": r32[0], "loss/corners": r32[1], "loss/center": r32[2], "loss/ctr": r32[3]})

    def backward_call(call, levels, targets, grad4, grads):
        calls["backward"] += 1
        assert grad4.dtype == torch.float64 and grad4.shape == (4,)
        g = gn.grads(_flat(levels, "logits"), _flat(levels, "delta"), _flat(levels, "center"), _flat(levels, "ctrness")[:, 0],
                     targets.np, Lc, upstream=grad4.tolist())
        for col, k in enumerate(TENSORS):
            parts = tn.split_levels(g[k].reshape(targets.P, -1), 2, shapes)
            for l, part in enumerate(parts):
                if grads[l][col] is not None:
                    grads[l][col].copy_(torch.from_numpy(part.astype(np.float32)))

    monkeypatch.setattr(outs, "_require_device", lambda ts: None)
    monkeypatch.setattr(outs, "assign_targets", assign_targets)
    monkeypatch.setattr(outs, "dafne_losses_packed", dafne_losses_packed)
    monkeypatch.setattr(lf, "_backward_call", backward_call)
    return outs, calls, shapes, tg, preds, Lc


def _nchw_inputs(preds, shapes, requires=(True, True, True, True), dtypes=None):
    out = []
    for i, a in enumerate(preds):
        a = a if a.ndim == 2 else a[:, None]
        lv = [torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))) for x in tn.split_levels(a, 2, shapes)]
        if dtypes:
            lv = [t.to(dtypes[i]) for t in lv]
        out.append([t.requires_grad_(requires[i]) for t in lv])
    return out


def _flat_grads(ts):
    return np.concatenate([t.grad.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).float().numpy() for t in ts])


def test_autograd_nchw_in_nchw_out(stubbed):
    outs, calls, shapes, tg, preds, Lc = stubbed
    lg, co, ce, ct = _nchw_inputs(preds, shapes)
    extras, losses = outs.losses(lg, co, ce, None, ct, None, [None, None])
    assert sorted(losses) == ["loss/center", "loss/cls", "loss/corners", "loss/ctr"]
    assert all(v.grad_fn is not None and v.dim() == 0 and v.dtype == torch.float32 for v in losses.values())
    assert sorted(extras) == ["loss_denorm", "num_pos", "values_f64"]
    e = tn.losses(preds[0], preds[1], preds[2], preds[3], tg, Lc)
    assert float(losses["loss/corners"].detach()) == float(np.float32(e["corners"]))
    sum(losses.values()).backward()
    assert calls == {"forward": 1, "backward": 1}
    want = gn.grads(preds[0], preds[1], preds[2], preds[3], tg, Lc)
    for ts, k in zip((lg, co, ce, ct), TENSORS):
        for t in ts:
            assert t.grad.shape == t.shape and t.grad.dtype == t.dtype
        assert np.array_equal(_flat_grads(ts), want[k].reshape(len(tg["labels"]), -1).astype(np.float32)), k


def test_autograd_none_for_inputs_without_grad(stubbed):
    outs, calls, shapes, tg, preds, Lc = stubbed
    lg, co, ce, ct = _nchw_inputs(preds, shapes, requires=(False, True, False, True))
    ct[1].requires_grad_(False)          # one level of a group that is otherwise wanted
    _, losses = outs.losses(lg, co, ce, None, ct, None, [None, None])
    sum(losses.values()).backward()
    assert all(t.grad is None for t in lg + ce) and ct[1].grad is None
    assert all(t.grad is not None for t in co) and all(t.grad is not None for i, t in enumerate(ct) if i != 1)


def test_autograd_upstream_factors(stubbed):
    outs, calls, shapes, tg, preds, Lc = stubbed
    lg, co, ce, ct = _nchw_inputs(preds, shapes)
    _, losses = outs.losses(lg, co, ce, None, ct, None, [None, None])
    (2.0 * losses["loss/cls"] + 0.0 * losses["loss/corners"] + 0.5 * losses["loss/center"] + losses["loss/ctr"]).backward()
    want = gn.grads(preds[0], preds[1], preds[2], preds[3], tg, Lc, upstream=(2.0, 0.0, 0.5, 1.0))
    one = gn.grads(preds[0], preds[1], preds[2], preds[3], tg, Lc)
    P = len(tg["labels"])
    for ts, k in zip((lg, co, ce, ct), TENSORS):
        assert np.array_equal(_flat_grads(ts), want[k].reshape(P, -1).astype(np.float32)), k
    assert not _flat_grads(co).any()
    assert np.allclose(_flat_grads(lg), 2.0 * one["logits"], rtol=1e-6, atol=0) and np.allclose(_flat_grads(ce), 0.5 * one["center"], rtol=1e-6, atol=0)


def test_autograd_low_precision_inputs(stubbed):
    """bf16 / fp16 head outputs (autocast): the kernel sees .float() copies, the gradients come back in the inputs' dtype."""
    outs, calls, shapes, tg, preds, Lc = stubbed
    lg, co, ce, ct = _nchw_inputs(preds, shapes, dtypes=(torch.bfloat16, torch.float16, torch.float32, torch.bfloat16))
    _, losses = outs.losses(lg, co, ce, None, ct, None, [None, None])
    sum(losses.values()).backward()
    for ts, dt in ((lg, torch.bfloat16), (co, torch.float16), (ce, torch.float32), (ct, torch.bfloat16)):
        assert all(t.grad.dtype == dt and t.grad.shape == t.shape for t in ts)


def test_no_grad_inputs_take_the_old_path(stubbed, monkeypatch):
    outs, calls, shapes, tg, preds, Lc = stubbed
    from dafne_amd.modeling.dafne import loss_function as lf
    monkeypatch.setattr(lf, "losses_with_grad", lambda *a, **k: pytest.fail("the autograd path ran without an input that requires grad"))
    lg, co, ce, ct = _nchw_inputs(preds, shapes, requires=(False, False, False, False))
    _, losses = outs.losses(lg, co, ce, None, ct, None, [None, None])
    assert all(v.grad_fn is None and not v.requires_grad for v in losses.values())
    lg, co, ce, ct = _nchw_inputs(preds, shapes)
    with torch.no_grad():
        _, losses = outs.losses(lg, co, ce, None, ct, None, [None, None])
    assert all(v.grad_fn is None for v in losses.values())


def test_world_size_above_one_is_refused_in_both_paths(monkeypatch, small):
    import torch.distributed as dist
    from test_gpu_targets import make_outputs
    _, shapes, tg, preds = small
    outs = make_outputs()
    monkeypatch.setattr(outs, "_require_device", lambda ts: None)
    monkeypatch.setattr(outs, "assign_targets", lambda shp, gt, device: _FakeTargets(tg, 2, shapes))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    for req in (True, False):
        lg, co, ce, ct = _nchw_inputs(preds, shapes, requires=(req,) * 4)
        with pytest.raises(NotImplementedError):
            outs.losses(lg, co, ce, None, ct, None, [None, None])


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_has_the_backward():
    from dafne_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.dafne_abi_version() >= 152
    for sym in ("dafne_losses_backward_workspace_bytes", "dafne_losses_backward_hip"):
        assert sym in _lib.SIGNATURES and hasattr(L, sym)
    # argument checks that need no device: a null parameter block, and the workspace size of a real level table
    assert L.dafne_losses_backward_workspace_bytes(None, None) == 0
    assert L.dafne_losses_backward_hip(None, None, None, None, None, None, None, 0, None, None, None, 0, None) == 1
