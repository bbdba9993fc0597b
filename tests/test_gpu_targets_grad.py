"""GPU: loss_grad_kernel (csrc/targets_kernels.h) behind dafne_losses_backward_hip and DAFNeOutputs.losses()' autograd path.

  * kernel against the restatement (tests/_targets_grad_np.py): every fp32 output within 1 ulp of the restatement's fp64 value
    rounded to fp32.  Both are roundings of fp64 values that differ by a few fp64 ulps (exp / pow / log1p and the order of the
    partial sums); neither focal term cancels against the other; so the two fp32 values are equal or neighbours.  Exact zeros
    are exactly zero.  Measured on an MI355X: see profiles/NOTES_targets.md.
  * two runs give equal bits; the raw (not COOKED) form is refused with DAFNE_E_UNSUPPORTED
  * losses() end to end: .grad of NCHW leaves, values bit-equal to the no_grad call, accumulation over two backward passes
  * the forward's d_out6 and a detect_packed call are unchanged by a backward
"""
import numpy as np
import pytest
import torch

import _targets_np as tn
import _targets_grad_np as gn
from test_gpu_targets import cooked_levels, dev, gt_instances, make_outputs, upload_targets

pytestmark = pytest.mark.gpu
TENSORS = ("logits", "corners", "center", "ctr")
SEEN = {"max_ulp": 0, "differ": 0, "elements": 0}


def ordered(a):
    """fp32 -> int64 that counts representable values: the difference of two is their distance in ulps."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def check(got, want64, tag):
    """got: the kernel's fp32; want64: the restatement's fp64."""
    want = want64.astype(np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), tag
    zero = want64 == 0
    assert not got[zero].any(), (tag, "an exact zero is not zero", np.argwhere(zero & (got != 0))[:5])
    d = np.abs(ordered(got) - ordered(want))
    SEEN["max_ulp"] = max(SEEN["max_ulp"], int(d.max()) if d.size else 0)
    SEEN["differ"] += int((d > 0).sum())
    SEEN["elements"] += d.size
    print(tag, "largest ulp distance", int(d.max()) if d.size else 0, "share that differs %.2e" % ((d > 0).mean() if d.size else 0.0))
    bad = np.argwhere(d > 1)
    assert bad.size == 0, (tag, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def device_grads(outs, levels, tg, upstream=(1.0, 1.0, 1.0, 1.0), cooked=True, only=None):
    """One forward and one dafne_losses_backward_hip call -> ({name: flat fp32 numpy}, forward row, raw torch buffers)."""
    from dafne_amd.modeling.dafne import loss_function as lf
    call = {}
    extras, _ = outs.dafne_losses_packed(levels, tg, cooked=cooked, _call=call)
    grads = []
    for lv in levels:
        bufs = []
        for k, t in zip(TENSORS, (lv.logits, lv.delta, lv.center, lv.ctrness)):
            keep = t is not None and (only is None or k in only)
            bufs.append(torch.full_like(t, float("nan")) if keep else None)      # every element must be written
        grads.append(tuple(bufs))
    grad4 = torch.tensor(upstream, dtype=torch.float64, device=dev())
    lf._backward_call(call, levels, tg, grad4, grads)
    torch.cuda.synchronize()
    out = {}
    for col, k in enumerate(TENSORS):
        if grads[0][col] is not None:
            out[k] = np.concatenate([g[col].reshape(-1, g[col].shape[3]).cpu().numpy() for g in grads])
    return out, extras["values_f64"], grads


def run_case(tg_np, preds, n, shapes, Lc, tag, upstream=(1.0, 1.0, 1.0, 1.0)):
    outs = make_outputs(T=tn.assign_config("released", num_classes=Lc["num_classes"]), Lc=Lc)
    outs.strides = list(tn.STRIDES[:len(shapes)])
    tg = upload_targets(tg_np, n, shapes)
    levels = cooked_levels(preds, n, shapes, Lc)
    got, _, _ = device_grads(outs, levels, tg, upstream)
    want = gn.grads(preds[0], preds[1], preds[2], preds[3], tg_np, Lc, upstream=upstream)
    P = tg_np["labels"].shape[0]
    assert sorted(got) == sorted(k for k in TENSORS if want[k] is not None), tag
    for k in got:
        check(got[k], want[k].reshape(P, -1), (tag, k))
    return got


@pytest.fixture(scope="module")
def small():
    return gn.small_grad_case()


@pytest.fixture(scope="module", autouse=True)
def report():
    """After the module: what its checks saw (the figures of profiles/NOTES_targets.md)."""
    yield
    print("\nlargest ulp distance %d, %d of %d elements differ (%.3e)" % (
        SEEN["max_ulp"], SEEN["differ"], SEEN["elements"], SEEN["differ"] / max(SEEN["elements"], 1)))


@pytest.mark.parametrize("name", [n for n, _ in tn.loss_configs()])
def test_kernel_small_case_every_configuration(small, name):
    _, shapes, tg, preds = small
    run_case(tg, preds, 2, shapes, dict(tn.loss_configs())[name], name)


@pytest.mark.parametrize("name", [n for n, _ in gn.handmade_configs()])
def test_kernel_handmade(name):
    th, hp, where = gn.handmade_grad_case()
    Lc = dict(gn.handmade_configs())[name]
    got = run_case(th, hp, 1, [(8, 8)], Lc, name)
    gc = got["corners"].reshape(-1, 4, 2)
    if Lc["sort_corners"]:
        assert gc[where["collinear"], 0].all() and not gc[where["collinear"], 1:].any()


@pytest.mark.parametrize("kind", ["zero_ctr", "nan_ctr"])
@pytest.mark.parametrize("mode", ["oriented", "plain"])
def test_kernel_handmade_centerness(kind, mode):
    tz = tn.handmade_targets(kind)
    run_case(tz, tn.case_b_predictions(tz, seed=23), 1, [(8, 8)], dict(tn.LOSS_RELEASED, ctr_mode=mode), (kind, mode))


def test_kernel_no_positives():
    th, hp, _ = gn.handmade_grad_case()
    got = run_case(dict(th, labels=np.full(64, 15, np.int64)), hp, 1, [(8, 8)], tn.LOSS_RELEASED, "nopos")
    assert got["logits"].all() and not got["corners"].any() and not got["center"].any() and not got["ctr"].any()


# 64 x 96: levels 8 x 12, 4 x 6, 2 x 3, 1 x 2, 1 x 1 (129 positions per image); 200 x 250: 25 x 32 .. 2 x 2 (1084 per image: a last
# workgroup that is not full, levels that start inside a workgroup)
@pytest.mark.parametrize("seed", [7, 46, 107, 151])
@pytest.mark.parametrize("n_images", [1, 2])
def test_kernel_odd_shapes(seed, n_images):
    gts, shapes, T = tn.small_case(seed)
    assert shapes in ([(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)], [(25, 32), (13, 16), (7, 8), (4, 4), (2, 2)])
    gts = gts[-n_images:]
    tg = tn.assign(gts, shapes, T)
    run_case(tg, tn.case_b_predictions(tg, seed=seed), n_images, shapes, tn.LOSS_RELEASED, ("seed", seed, n_images),
             upstream=(1.0, 0.5, 2.0, 3.0))


@pytest.mark.parametrize("C", [1, 15, 16])
def test_kernel_class_counts(C):
    gts, shapes, T = tn.small_case(46)
    for g in gts:
        g["cls"] = g["cls"] % C
    T = dict(T, num_classes=C)
    tg = tn.assign(gts, shapes, T)
    assert (tg["labels"] != C).sum() > 0
    Lc = dict(tn.LOSS_RELEASED, num_classes=C)
    run_case(tg, tn.case_b_predictions(tg, seed=5, num_classes=C), 2, shapes, Lc, ("C", C))


def test_kernel_alpha_off_and_gamma_zero(small):
    """alpha < 0 (no class weight) and gamma = 0 (the second focal term is exactly 0), gamma = 1.5 (a power that is not an integer)."""
    _, shapes, tg, preds = small
    for a, g in ((-1.0, 2.0), (0.25, 0.0), (0.5, 1.5)):
        run_case(tg, preds, 2, shapes, dict(tn.LOSS_RELEASED, alpha=a, gamma=g), ("alpha", a, "gamma", g))


def test_leaving_gradients_out(small):
    """A gradient pointer that is NULL in every level is not computed; the others have the same bits."""
    _, shapes, tg_np, preds = small
    Lc = tn.LOSS_RELEASED
    outs = make_outputs(Lc=Lc)
    tg = upload_targets(tg_np, 2, shapes)
    levels = cooked_levels(preds, 2, shapes, Lc)
    full, _, _ = device_grads(outs, levels, tg)
    part, _, _ = device_grads(outs, levels, tg, only=("corners", "ctr"))
    assert sorted(part) == ["corners", "ctr"]
    for k in part:
        assert np.array_equal(part[k].view(np.uint32), full[k].view(np.uint32))


def test_run_to_run(small):
    _, shapes, tg_np, preds = small
    outs = make_outputs()
    tg = upload_targets(tg_np, 2, shapes)
    levels = cooked_levels(preds, 2, shapes, tn.LOSS_RELEASED)
    a, _, _ = device_grads(outs, levels, tg)
    b, _, _ = device_grads(outs, levels, tg)
    for k in TENSORS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_raw_form_is_unsupported(small):
    from dafne_amd import _lib
    _, shapes, tg_np, preds = small
    outs = make_outputs()
    tg = upload_targets(tg_np, 2, shapes)
    levels = cooked_levels(preds, 2, shapes, tn.LOSS_RELEASED)
    with pytest.raises(_lib.DafneHipError, match=r"code 4.*COOKED"):
        device_grads(outs, levels, tg, cooked=False)


# ------------------------------------------------------------------------------------------------ losses() end to end
def nchw_leaves(preds, n, shapes):
    out = []
    for a in preds:
        a = a if a.ndim == 2 else a[:, None]
        out.append([torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2))).to(dev()).requires_grad_(True)
                    for x in tn.split_levels(a, n, shapes)])
    return out


def flat_grad(ts):
    return np.concatenate([t.grad.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).cpu().numpy() for t in ts])


def test_losses_end_to_end(small):
    gts, shapes, tg_np, preds = small
    Lc = tn.LOSS_RELEASED
    outs = make_outputs(Lc=Lc)
    inst = gt_instances(gts, gn.SMALL_HW)
    lg, co, ce, ct = nchw_leaves(preds, 2, shapes)
    with torch.no_grad():
        extras0, plain = outs.losses(lg, co, ce, None, ct, None, inst)
    assert all(v.grad_fn is None for v in plain.values())
    extras, losses = outs.losses(lg, co, ce, None, ct, None, inst)
    assert sorted(losses) == sorted(plain) and sorted(extras) == sorted(extras0)
    assert all(v.grad_fn is not None for v in losses.values())
    for k in plain:
        assert torch.equal(losses[k].detach().view(torch.int32), plain[k].view(torch.int32)), k
    assert torch.equal(extras["values_f64"].view(torch.int64), extras0["values_f64"].view(torch.int64))
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    want = gn.grads(preds[0], preds[1], preds[2], preds[3], tg_np, Lc)
    P = tg_np["labels"].shape[0]
    first = {}
    for ts, k in zip((lg, co, ce, ct), TENSORS):
        assert all(t.grad.shape == t.shape and t.grad.dtype == torch.float32 for t in ts)
        first[k] = flat_grad(ts)
        check(first[k], want[k].reshape(P, -1), ("end to end", k))
    # the same bits as the kernel called directly on the same values
    direct, _, _ = device_grads(outs, cooked_levels(preds, 2, shapes, Lc), upload_targets(tg_np, 2, shapes))
    for k in TENSORS:
        assert np.array_equal(first[k].view(np.uint32), direct[k].view(np.uint32)), k
    # a second forward / backward accumulates
    _, losses = outs.losses(lg, co, ce, None, ct, None, inst)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    for ts, k in zip((lg, co, ce, ct), TENSORS):
        assert np.array_equal(flat_grad(ts), first[k] + first[k]), k


def test_losses_partial_requires_grad_and_low_precision(small):
    gts, shapes, tg_np, preds = small
    outs = make_outputs()
    inst = gt_instances(gts, gn.SMALL_HW)
    lg, co, ce, ct = nchw_leaves(preds, 2, shapes)
    lg = [t.detach() for t in lg]
    co = [t.detach().to(torch.bfloat16).requires_grad_(True) for t in co]
    _, losses = outs.losses(lg, co, ce, None, ct, None, inst)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert all(t.grad is None for t in lg)
    assert all(t.grad is not None and t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape for t in co)
    assert all(t.grad is not None for t in ce + ct)


def test_nothing_else_moved(small):
    """d_out6 with and without a following backward, and a detect_packed call before and after one."""
    import os
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    from oracle import model as om
    _, shapes, tg_np, preds = small
    outs = make_outputs()
    tg = upload_targets(tg_np, 2, shapes)
    levels = cooked_levels(preds, 2, shapes, tn.LOSS_RELEASED)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = build_model(load_cfg(os.path.join(root, "configs", "dota-1.0_r50.yaml")))
    m.load_state_dict(om.make_params(50, 15, seed=5))
    m.to(dev())
    m.invalidate()
    ims = torch.randint(0, 256, (2, 3, 128, 160), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(dev())

    def detections():
        rows, counts = m.detect_packed(ims)
        torch.cuda.synchronize()
        return rows.clone(), counts.clone()
    before = detections()
    extras, _ = outs.dafne_losses_packed(levels, tg, cooked=True)
    torch.cuda.synchronize()
    alone = extras["values_f64"].clone()
    _, row, _ = device_grads(outs, levels, tg)
    assert torch.equal(row.view(torch.int64), alone.view(torch.int64))
    after = detections()
    assert torch.equal(before[1], after[1]) and int(before[1].sum()) > 0
    for i, c in enumerate(before[1].tolist()):          # the rows past an image's count are unwritten memory
        assert torch.equal(before[0][i, :c].view(torch.int32), after[0][i, :c].view(torch.int32)), i
