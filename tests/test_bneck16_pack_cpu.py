"""CPU: engine.pack_bneck16 (the weights of dafne_bottleneck_body16_hip, conv_bneck.hip's 16x16x32 form) against the layout
include/dafne_amd.h spells out, element by element, and engine.bneck_weights, the plans' one-form-per-model cache.  No kernel runs."""
import pytest
import torch

BF = torch.bfloat16


def _weights():
    g = torch.Generator().manual_seed(11)
    w2 = torch.randn(256, 2304, generator=g).to(BF)
    w3 = torch.randn(1024, 256, generator=g).to(BF)
    w1 = torch.randn(256, 1024, generator=g).to(BF)
    return w2, w3, w1


def _perm16(p):
    cb, a, i = p >> 4, (p >> 2) & 3, p & 3
    return 8 * a + 4 * cb + i


def test_row_order_makes_a_lanes_eight_values_one_run_of_channels():
    from dafne_amd import engine
    perm = engine._bneck_row_perm16("cpu").tolist()
    assert sorted(perm) == list(range(32)) and perm == [_perm16(p) for p in range(32)]
    for a in range(4):            # a lane (lane >> 4 == a) holds rows 4a .. 4a + 3 of fragment 0, then of fragment 1
        assert [perm[16 * cb + 4 * a + i] for cb in range(2) for i in range(4)] == list(range(8 * a, 8 * a + 8))


def test_pack_bneck16_is_the_documented_layout():
    from dafne_amd import engine
    w2, w3, w1 = _weights()
    wf = engine.pack_bneck16(w2, w3, w1)
    assert wf.dtype == BF and wf.shape == engine.pack_bneck(w2, w3, w1).shape == (8 * 144 * 512 + 8 * 8 * 16 * 512,)
    a = wf[:8 * 144 * 512].reshape(8, 144, 64, 8)                   # conv2: [wave][fragment][lane][8]
    b = wf[8 * 144 * 512:].reshape(8, 8, 16, 64, 8)                 # [GEMM][wave][fragment][lane][8]
    g = torch.Generator().manual_seed(5)
    for _ in range(400):
        wave, frag, lane = (int(torch.randint(0, n, (1,), generator=g)) for n in (8, 144, 64))
        m, cb = frag >> 1, frag & 1
        row, k0 = wave * 32 + _perm16(16 * cb + (lane & 15)), 32 * m + 8 * (lane >> 4)
        assert torch.equal(a[wave, frag, lane], w2[row, k0:k0 + 8])
        c, frag = int(torch.randint(0, 4, (1,), generator=g)), frag % 16
        m, k0 = frag >> 1, 32 * (frag >> 1) + 8 * (lane >> 4)
        assert torch.equal(b[2 * c, wave, frag, lane], w3[c * 256 + row, k0:k0 + 8])
        assert torch.equal(b[2 * c + 1, wave, frag, lane], w1[row, c * 256 + k0:c * 256 + k0 + 8])


def test_one_conv_bneck_form_per_packed_weights():
    from dafne_amd import engine
    from dafne_amd.engine_options import EngineOptions
    w2, w3, w1 = _weights()
    P = {"options": EngineOptions()}
    wf, m16 = engine.bneck_weights(P, "res4.1.", w2, w3, w1)
    assert m16 is True and torch.equal(wf, engine.pack_bneck16(w2, w3, w1)) and engine.bneck_weights(P, "res4.1.", w2, w3, w1)[0] is wf
    assert [k for k in P if k != "options"] == ["res4.1.bneck16"]
    P = {"options": EngineOptions(rp_mfma16=False)}
    wf, m16 = engine.bneck_weights(P, "res4.1.", w2, w3, w1)
    assert m16 is False and torch.equal(wf, engine.pack_bneck(w2, w3, w1)) and [k for k in P if k != "options"] == ["res4.1.bneck"]
    P["res4.1.bneck16"] = wf
    with pytest.raises(AssertionError):
        engine.bneck_weights(P, "res4.1.", w2, w3, w1)
