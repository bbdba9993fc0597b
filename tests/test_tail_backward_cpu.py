"""CPU: the fp64 restatement of the head-tail backward (tests/_tail_backward_np.py) against torch autograd, the parameter list of
OneStageDetector.tail_parameters, and the C ABI of dafne_pred_dgrad_gn_hip without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _tail_backward_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 7), (3, 4), (1, 2)]


@pytest.mark.parametrize("cout", [1, 9, 16])
def test_restatement_against_autograd(cout):
    """conv2d(relu(group_norm(x))) in fp64 with exact statistics and no bf16 rounding: x.grad, the GroupNorm affine gradients and
    the bias gradient of the convolution that wrote x (the per-channel sum of x.grad), summed over three levels that share the
    parameters."""
    rng = np.random.default_rng(cout)
    n, C, eps = 2, 256, 1e-5
    gamma = torch.tensor(rng.normal(1.0, 0.5, C), requires_grad=True)
    beta = torch.tensor(rng.normal(0.0, 0.5, C), requires_grad=True)
    W = torch.tensor(rng.normal(0, 0.1, (cout, C, 3, 3)))
    xs = [torch.tensor(rng.normal(0.2, 1.5, (n, C, h, w)), requires_grad=True) for h, w in SHAPES]
    gs = [torch.tensor(rng.normal(0, 1, (n, cout, h, w)) * np.exp(rng.uniform(-6, 2, (n, cout, h, w)))) for h, w in SHAPES]
    loss, masks, stats = 0.0, [], []
    for x, g in zip(xs, gs):
        z = torch.nn.functional.group_norm(x, 32, gamma, beta, eps)
        loss = loss + (torch.nn.functional.conv2d(torch.relu(z), W, padding=1) * g).sum()
        masks.append((z > 0).permute(0, 2, 3, 1).numpy())
        xg = x.detach().reshape(n, 32, -1)
        stats.append(torch.stack((xg.mean(2), 1.0 / torch.sqrt(xg.var(2, unbiased=False) + eps)), -1).numpy())
    loss.backward()
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).numpy()
    got = R.tail_backward([nhwc(x) for x in xs], stats, gamma.detach().numpy(), beta.detach().numpy(), W.numpy(),
                          [nhwc(g) for g in gs], masks)

    def close(a, b, what):
        scale = max(np.abs(b).max(), 1e-300)
        assert np.abs(a - b).max() <= 1e-11 * scale, (what, np.abs(a - b).max() / scale)
    dbias = np.zeros(C)
    for l, x in enumerate(xs):
        close(got["gx"][l], nhwc(x.grad), "gx[%d]" % l)
        dbias += x.grad.sum((0, 2, 3)).numpy()
        assert (got["gx_abs"][l] >= np.abs(got["gx"][l]) * (1 - 1e-12)).all()
    close(got["dgamma"], gamma.grad.numpy(), "dgamma")
    close(got["dbeta"], beta.grad.numpy(), "dbeta")
    # (the group sums of x.grad cancel to rounding: compared on the scale of the gradient itself)
    assert np.abs(got["dbias"] - dbias).max() <= 1e-11 * max(np.abs(nhwc(x.grad)).max() for x in xs) * sum(n * h * w for h, w in SHAPES)
    for k in ("dgamma", "dbeta", "dbias"):
        assert (got[k + "_abs"] >= np.abs(got[k]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("centerness", ["plain", "none"])
@pytest.mark.parametrize("strategy", ["center-to-corner", "direct", "offset", "iterative"])
def test_tail_parameters(strategy, centerness):
    import dafne_amd.modeling  # noqa: F401
    from dafne_amd.config import load_cfg
    from dafne_amd.registry import build_model
    cfg = load_cfg(os.path.join(ROOT, "configs", "dota-1.0_r50.yaml"),
                   ["MODEL.DAFNE.CORNER_PREDICTION", strategy, "MODEL.DAFNE.CENTERNESS", centerness])
    m = build_model(cfg)
    if strategy == "iterative":
        with pytest.raises(NotImplementedError):
            m.tail_parameters()
        return
    names = {id(p): k for k, p in m.named_parameters()}
    got = [names[id(p)] for p in m.tail_parameters()]
    hp = "proposal_generator.dafne_head."
    want = [hp + "cls_logits.weight", hp + "cls_logits.bias", hp + "corners_pred.weight", hp + "corners_pred.bias"]
    if centerness != "none":
        want += [hp + "ctrness.weight", hp + "ctrness.bias"]
    if strategy == "center-to-corner":
        want += [hp + "center_pred.weight", hp + "center_pred.bias"]
    want += [hp + "scales.%d.scale" % l for l in range(5)]
    assert got[:len(want)] == want == [names[id(p)] for p in m.prediction_parameters()]
    tail = [hp + "%s.%s" % (t, k) for t in ("cls_tower", "corners_tower") for k in ("9.bias", "10.weight", "10.bias")]
    assert got[len(want):] == tail
    assert not any("center_tower" in k for k in got)
    assert len(set(got)) == len(got)


def test_abi_and_refusals_without_a_device():
    from dafne_amd import _lib, build
    build.build()
    L = _lib.load()
    assert L.dafne_abi_version() >= 155
    assert "dafne_pred_dgrad_gn_hip" in _lib.SIGNATURES and "dafne_pred_dgrad_gn_workspace_bytes" in _lib.SIGNATURES
    seg = (_lib.ConvSeg * 1)(_lib.ConvSeg(8, None, None, 2, 3, 2, 3))
    ptrs = (ctypes.c_void_p * 1)(8)
    P8 = ctypes.c_void_p(8)

    def prm(**kw):
        p = _lib.ConvParams(1, 1, 256, 9, 3, 3, 1, 1, 8 | 32, None, None, None, 8, 8, 8, None, None, 0.0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(p, ps=9, g=ptrs, gx=ptrs, w=P8):
        return L.dafne_pred_dgrad_gn_hip(ctypes.byref(p), seg, w, g, ps, gx, P8, P8, P8, P8, 1 << 30, None)
    assert call(prm(Cin=128)) == 4 and call(prm(Cout=17), ps=17) == 4 and call(prm(Cout=0)) == 4
    assert call(prm(KH=1, KW=1, pad=0)) == 4 and call(prm(stride=2)) == 4
    assert call(prm(), ps=8) == 1 and call(prm(n_segs=6)) == 1 and call(prm(n_segs=0)) == 1
    assert call(prm(), g=None) == 1 and call(prm(), gx=None) == 1 and call(prm(), w=None) == 1
    assert call(prm(flags=8)) == 1                                         # no GroupNorm on load: no raw map
    assert call(prm(d_in_gn_stats=None)) == 1                              # GN input without statistics
    assert call(prm(flags=8 | 32 | 1)) == 1                                # unknown flag
    assert b"pred_dgrad_gn" in L.dafne_last_error()
    assert L.dafne_pred_dgrad_gn_workspace_bytes(ctypes.byref(prm(Cin=128)), seg) == 0
    assert L.dafne_pred_dgrad_gn_workspace_bytes(ctypes.byref(prm(flags=8)), seg) == 0
