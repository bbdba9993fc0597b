"""CPU: the fp64 restatement of a tower layer's backward (tests/_tower_backward_np.py) against torch autograd in fp64 on a two-layer
chain conv -> GroupNorm(32) -> ReLU -> conv (256 channels, 2 images of 3 x 5), the ReLU mask taken from the forward; and the
wrappers of modeling/dafne/tower_backward.py refuse CPU tensors."""
import types

import numpy as np
import pytest
import torch

import _tower_backward_np as R

C = 256


def _chain():
    g = torch.Generator().manual_seed(11)
    f64 = torch.float64
    x0 = torch.randn(2, C, 3, 5, generator=g, dtype=f64)
    w1 = (torch.randn(C, C, 3, 3, generator=g, dtype=f64) * 0.03).requires_grad_()
    b1 = (torch.randn(C, generator=g, dtype=f64) * 0.1).requires_grad_()
    gamma = ((torch.rand(C, generator=g, dtype=f64) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)).requires_grad_()
    beta = (torch.randn(C, generator=g, dtype=f64) * 0.3).requires_grad_()
    w2 = (torch.randn(C, C, 3, 3, generator=g, dtype=f64) * 0.03).requires_grad_()
    gout = torch.randn(2, C, 3, 5, generator=g, dtype=f64) * torch.exp(torch.rand(2, C, 3, 5, generator=g, dtype=f64) * 8 - 6)
    z = torch.nn.functional.conv2d(x0, w1, b1, padding=1)
    z.retain_grad()
    a = torch.relu(torch.nn.functional.group_norm(z, 32, gamma, beta, eps=1e-5))
    out = torch.nn.functional.conv2d(a, w2, None, padding=1)
    (out * gout).sum().backward()
    return x0, w1, b1, gamma, beta, w2, gout, z, a


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def close(name, got, want):
    want = np.asarray(want)
    scale = float(np.abs(want).max())
    assert scale > 0, name
    err = float(np.abs(np.asarray(got).reshape(want.shape) - want).max())
    assert err <= 1e-10 * scale, "%s: %.3g of %.3g" % (name, err, scale)


def test_restatement_agrees_with_autograd_on_a_two_layer_chain():
    x0, w1, b1, gamma, beta, w2, gout, z, a = _chain()
    zn = nhwc(z)
    grp = zn.reshape(2, 15, 32, 8)
    mean = grp.mean((1, 3))
    rstd = 1.0 / np.sqrt(grp.var((1, 3)) + 1e-5)
    stats = np.stack((mean, rstd), -1)                              # [N, 32, 2]
    mask = nhwc(a) > 0                                              # the forward's own
    assert 0.2 < mask.mean() < 0.8
    # layer 2: weight gradient on the map it multiplied; data gradient back to the raw output of layer 1
    dw2, _, _, _, n = R.wgrad([nhwc(a)], [nhwc(gout)])
    assert n == 30
    close("dW2", dw2, w2.grad.numpy())
    ref = R.layer_backward([zn], [stats], gamma.detach().numpy(), beta.detach().numpy(), w2.detach().numpy(), [nhwc(gout)], [mask])
    close("gx", ref["gx"][0], nhwc(z.grad))
    close("dgamma", ref["dgamma"], gamma.grad.numpy())
    close("dbeta", ref["dbeta"], beta.grad.numpy())
    close("dbias", ref["dbias"], b1.grad.numpy())
    # layer 1: its weight gradient from the restated gx
    dw1, db1, _, _, _ = R.wgrad([nhwc(x0)], [ref["gx"][0]])
    close("dW1", dw1, w1.grad.numpy())
    close("db1", db1, b1.grad.numpy())
    # the magnitude sums dominate the values they stand behind
    assert (ref["gx_abs"][0] >= np.abs(ref["gx"][0]) * (1 - 1e-12)).all()


def test_applied_is_the_forward_mask():
    rng = np.random.default_rng(3)
    x = R.PB.bf16_round(rng.normal(0.3, 1.0, (1, 2, 3, C)).astype(np.float32))
    st = np.stack((rng.normal(0.3, 0.1, (1, 32)), rng.uniform(0.5, 1.5, (1, 32))), -1).astype(np.float32)
    gamma = rng.normal(0, 1, C).astype(np.float32)
    beta = rng.normal(0, 0.3, C).astype(np.float32)
    a = R.applied(x, st, gamma, beta)
    assert a.dtype == np.float32 and (a >= 0).all() and (R.PB.bf16_round(a) == a).all()
    y = (x.astype(np.float64) - np.repeat(st[:, :, 0], 8, 1)[:, None, None]) * np.repeat(st[:, :, 1], 8, 1)[:, None, None] * gamma + beta
    assert np.abs(a - np.maximum(y, 0)).max() <= 2.0 ** -8 * np.abs(y).max() + 1e-6


def test_bounds_are_the_documented_constants():
    assert R.C_PIXEL == 2.0 ** -16 + (4608 + 46) * 2.0 ** -24
    assert R.wgrad_bound(1.0, 100) == 2.0 ** -16 + 100 * 2.0 ** -24
    # one tile, one workgroup: 8 pixels per lane in pass 1; pass 2 adds one pixel per thread and level
    assert R.lane_pixels([(1, 1)], 1, 256) == 8
    # 522 tiles on 256 CUs: three tiles per workgroup
    assert R.lane_pixels([(1041, 1)], 2, 256) == 24


def test_wrappers_refuse_cpu_tensors():
    from dafne_amd import _lib
    from dafne_amd.modeling.dafne.tower_backward import tower_dgrad_gn, tower_wgrad
    prm = _lib.ConvParams(1, 1, C, C, 3, 3, 1, 1, 32, None, None, None, None, None, None, None, None, 0.0)
    segs = (_lib.ConvSeg * 1)()
    segs[0] = _lib.ConvSeg(None, None, None, 2, 3, 2, 3)
    call = types.SimpleNamespace(prm=prm, segs=segs)
    g = [torch.zeros(1, 2, 3, C)]
    with pytest.raises(_lib.DafneHipError):
        tower_wgrad(call, g)
    with pytest.raises(_lib.DafneHipError):
        tower_dgrad_gn(call, torch.zeros(C * 2304, dtype=torch.bfloat16), g)
    assert _lib.load().dafne_abi_version() >= 156
