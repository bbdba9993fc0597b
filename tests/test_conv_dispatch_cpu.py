"""CPU: which kernel of csrc/conv.hip the library picks for every case of tests/_conv_cases.py, under the DEFAULT dispatch (this
module sets no DAFNE_CONV_* variable: the library reads most of them once per process), and the rejection of launches whose
32-bit input / residual offsets would wrap.  dafne_conv2d_kernel_id never touches a device, so dummy pointers do."""
import collections
import ctypes
import os

import pytest

from _conv_cases import CASES, LIMIT_CASES, exact_bound, probe


@pytest.fixture(scope="module")
def built():
    from dafne_amd import build
    assert not [k for k in os.environ if k.startswith(("DAFNE_CONV_", "DAFNE_WS_"))], "this module tests the default dispatch"
    return build.build()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_runs_on_the_kernel_it_was_written_for(built, case):
    from dafne_amd.engine import ConvCall
    assert case.kernel in ConvCall.KERNEL_NAMES and case.why
    kid, tiles, msg = probe(case.cin, case.cout, case.k, case.stride, case.sizes, case.n, case.flags, case.bias)
    assert kid >= 0, msg
    assert ConvCall.KERNEL_NAMES[kid] == case.kernel, (case.name, "now runs on", ConvCall.KERNEL_NAMES[kid])
    assert tiles > 0
    # precondition of the exact-data regime of tests/test_gpu_conv_matrix.py: every partial sum is an integer below 2^24
    assert exact_bound(case) < 2 ** 24


def test_every_kernel_has_cases(built):
    from dafne_amd.engine import ConvCall
    assert len(set(c.name for c in CASES)) == len(CASES)
    n = collections.Counter(c.kernel for c in CASES)
    for name in ConvCall.KERNEL_NAMES:
        need = 1 if name in ("conv3x3_pred16", "conv3x3_slab", "conv3x3_patch") else 3
        assert n[name] >= need, (name, n[name])
    # conv_ws: six template instantiations (Cin 64 / 128 / 256, with and without the residual tile)
    for cin in (64, 128, 256):
        for res in (False, True):
            assert [c for c in CASES if c.kernel == "conv_ws" and c.cin == cin and ("RES" in c.flags) == res], (cin, res)
    assert any(c.kernel == "conv_stream" and "RES" in c.flags for c in CASES)
    for name in ConvCall.KERNEL_NAMES[:4]:
        assert any(c.kernel == name and "F32" in c.flags for c in CASES), name          # fp32 epilogue of every igemm tile
    for name in ("conv_igemm<2,2,2,2>", "conv_igemm<4,2,2,4>", "conv_stream", "conv_ws"):
        assert any(c.kernel == name and len(c.sizes) > 1 for c in CASES), name         # several segments


@pytest.mark.parametrize("cin,cout,k,size,n_ok,n_bad", LIMIT_CASES)
def test_input_beyond_32bit_offsets_is_rejected(built, cin, cout, k, size, n_ok, n_bad):
    kid, tiles, msg = probe(cin, cout, k, 1, [size], n_ok)
    assert kid >= 0 and tiles > 0, msg
    assert n_ok * (size[0] + 2) * (size[1] + 2) * cin * 2 <= 0xffffffff
    for n in n_bad:
        nbytes = n * (size[0] + 2) * (size[1] + 2) * cin * 2
        assert nbytes > 0xffffffff
        kid, tiles, msg = probe(cin, cout, k, 1, [size], n)
        assert kid == -1 and tiles == -1
        assert str(nbytes) in msg and "32-bit" in msg, msg
    # one oversized segment among small ones is enough
    kid, _, msg = probe(cin, cout, k, 1, [(8, 8), size], n_bad[0])
    assert kid == -1 and "segment 1" in msg, msg


def test_stream_residual_beyond_32bit_offsets_is_rejected(built):
    """conv_stream_kernel forms the residual offset in 32 bits too: with Cout > Cin the residual map passes 2^32 bytes before the
    input does.  320 -> 640 channels at 510 x 510: 2^18 haloed pixels x 1280 B = 2^26 * 5 B per image."""
    from dafne_amd.engine import ConvCall
    per_img = 512 * 512 * 640 * 2
    n_ok, n_bad = 0xffffffff // per_img, 0xffffffff // per_img + 1
    kid, _, msg = probe(320, 640, 1, 1, [(510, 510)], n_ok, ("RES",))
    assert kid >= 0 and ConvCall.KERNEL_NAMES[kid] == "conv_stream", msg
    kid, _, msg = probe(320, 640, 1, 1, [(510, 510)], n_bad, ("RES",))
    assert kid == -1 and str(n_bad * per_img) in msg and "residual" in msg, msg
    assert n_bad * 512 * 512 * 320 * 2 <= 0xffffffff            # (the input alone would still have passed)
    kid, _, msg = probe(320, 640, 1, 1, [(510, 510)], n_bad)    # no residual: nothing 32-bit is out of range
    assert kid >= 0, msg


def test_refused_call_has_no_kernel_name(built):
    """engine.ConvCall.kernel_name() of a call the library refuses raises the library's message; it used to index
    KERNEL_NAMES[-1] and answer 'conv3x3_pred16'."""
    from dafne_amd import _lib, engine

    class T:                                    # what ConvCall needs of a tensor: an address (never dereferenced on the host)
        def data_ptr(self):
            return 0x1000

        def numel(self):
            return 0

        def element_size(self):
            return 2

    t = T()
    c = engine.ConvCall(t, t, 256, 128, 1, 1, 0, 0, [(t, t, None, 254, 254, 254, 254)], 129)
    assert c.kernel_id() == -1 and c.num_tiles() == -1
    with pytest.raises(_lib.DafneHipError, match="4328521728 bytes"):
        c.kernel_name()
    with pytest.raises(_lib.DafneHipError, match="4328521728 bytes"):
        c(ctypes.c_void_p(0))                  # the launch entry point refuses before it touches the device
    ok = engine.ConvCall(t, t, 256, 128, 1, 1, 0, 0, [(t, t, None, 254, 254, 254, 254)], 127)
    assert ok.kernel_name() == "conv_ws"
