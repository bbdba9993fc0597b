"""NumPy oracle of the device SGD step (dafne_amd/csrc/solver_kernels.h, include/dafne_amd.h): torch.optim.SGD with momentum,
dampening 0, no Nesterov, in fp32 with the two fused operations torch's CPU kernels have --

    g'  = wd == 0 ? g : fma(wd, p, g)
    buf = first ? g' : (m * buf) + g'          two roundings
    p   = fma(-lr_t, buf, p)                   lr_t = fp32(lr * lr_factor), the product in double

fma(a, b, c) is float32(float64(a) * float64(b) + float64(c)): the fp64 product of two fp32 values is exact, the sum rounds once
to fp64 and once more to fp32, so a double rounding is possible in principle; tests/test_solver_cpu.py pins the oracle to
torch.optim.SGD bit for bit on exactly the inputs the GPU test uses (synthetic_* below).

The packed destinations are restated with the engine's own pack functions on the new masters (packed_*).
"""
import numpy as np
import torch


def fma32(a, b, c):
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def sgd_step(p, g, buf, lr, momentum, first, lr_factor=1.0, wd=0.0):
    """p, g, buf: float32 arrays (buf is ignored when first) -> (new p, new buf)."""
    p, g = np.asarray(p, np.float32), np.asarray(g, np.float32)
    lr_t = np.float32(float(lr) * float(lr_factor))
    with np.errstate(all="ignore"):
        g1 = g if wd == 0 else fma32(np.float32(wd), p, g)
        if first:
            nb = g1.copy()
        else:
            mb = (np.float32(momentum) * np.asarray(buf, np.float32)).astype(np.float32)
            nb = (mb + g1).astype(np.float32)
        return fma32(-lr_t, nb, p), nb


# ---------------------------------------------------------------- the synthetic tensors of the kernel test
# (name, shape, lr_factor, is a bias / norm group with its own weight decay)
SYNTHETIC = [("scale%d" % l, (1,), 1.0) for l in range(5)] + [
    ("gn_w", (256,), 1.0), ("gn_b", (256,), 1.0), ("bias15", (15,), 2.0), ("w15", (15, 256, 3, 3), 1.0),
    ("w8", (8, 256, 3, 3), 1.0), ("w1", (1, 256, 3, 3), 1.0), ("w2", (2, 256, 3, 3), 1.0),
    ("w256_frag", (256, 256, 3, 3), 1.0), ("w256_frag16", (256, 256, 3, 3), 1.0)]
SYNTHETIC_LR, SYNTHETIC_MOMENTUM, SYNTHETIC_STEPS = 0.0125, 0.9, 3
SYNTHETIC_WD = (0.0, 1e-4)


def synthetic_params(seed=20):
    g = torch.Generator().manual_seed(seed)
    return {n: (torch.randn(*s, generator=g) * 0.05 + (1.0 if n.startswith("scale") or n == "gn_w" else 0.0)).float()
            for n, s, _ in SYNTHETIC}


def synthetic_grads(step, seed=20):
    """The gradients of step `step`: another draw per step."""
    g = torch.Generator().manual_seed(1000 * seed + step)
    return {n: (torch.randn(*s, generator=g) * 0.02).float() for n, s, _ in SYNTHETIC}


def synthetic_addend(seed=20):
    g = torch.Generator().manual_seed(seed + 7)
    return torch.randn(256, generator=g).float()


def oracle_run(wd, steps, seed=20):
    """-> per step {name: (p, buf)} of the synthetic tensors under the oracle."""
    p = {n: v.numpy().copy() for n, v in synthetic_params(seed).items()}
    buf = {n: None for n in p}
    out = []
    for k in range(steps):
        gr = synthetic_grads(k, seed)
        for n, _, f in SYNTHETIC:
            p[n], buf[n] = sgd_step(p[n], gr[n].numpy(), buf[n], SYNTHETIC_LR, SYNTHETIC_MOMENTUM, k == 0, lr_factor=f, wd=wd)
        out.append({n: (p[n].copy(), buf[n].copy()) for n in p})
    return out


# ---------------------------------------------------------------- packed destinations, by the engine's own functions
def packed_plain(weights, bias=None):
    """engine.pack_conv of the row-wise concatenation of OIHW fp32 weights (numpy or torch) -> (bf16 [Cout_pad, K], fp32 [Cout_pad])
    on the CPU."""
    from dafne_amd import engine
    w = torch.cat([torch.as_tensor(np.asarray(x)) for x in weights], 0)
    b = None if bias is None else torch.as_tensor(np.asarray(bias))
    return engine.pack_conv(w, b, "cpu")


def packed_form(plain, form):
    from dafne_amd import engine
    return {"frag": engine.pack_conv3x3_frag, "frag16": engine.pack_conv3x3_frag16, "wr": engine.pack_conv_frag}[form](plain)


def bits(t):
    """The bit pattern of a float32 / bfloat16 tensor or array as integers (NaNs compare by their bits)."""
    if isinstance(t, np.ndarray):
        return t.view(np.uint32) if t.dtype == np.float32 else t
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
