"""Reference of the guarded optimiser step (pf_adam_step_guarded), written once and evaluated in fp64 or in fp32 (numpy).

The options arrive at the C ABI as fp32 numbers, so both evaluations first round them to fp32: what is compared is the
arithmetic, not the representation of 0.999.  tests/test_optim_host.py holds the fp64 evaluation against
torch.nn.utils.clip_grad_norm_ / clip_grad_value_ followed by torch.optim.Adam on split tensors."""
from types import SimpleNamespace

import numpy as np

CLIP_NONE, CLIP_NORM, CLIP_VALUE = 0, 1, 2


def grad_norm64(g):
    """sqrt(sum g^2) in fp64 (non-finite iff some g is)"""
    with np.errstate(over="ignore", invalid="ignore"):
        g = np.asarray(g, np.float64)
        return float(np.sqrt(np.sum(g * g)))


def guarded_step(p, g, m, v, ema=None, *, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0,
                 clip_mode=CLIP_NONE, clip=0.0, ema_decay=0.0, dtype=np.float64):
    """One guarded step on flat vectors; ``step`` is the APPLIED step this call would be (bias corrections 1 - beta^step).
    Returns a namespace p, m, v, ema (new arrays of ``dtype``; the inputs when the step is skipped), norm (of the scaled gradient),
    coef, finite."""
    f = np.dtype(dtype).type
    o = {k: f(np.float32(x)) for k, x in dict(lr=lr, b1=betas[0], b2=betas[1], eps=eps, wd=weight_decay, scale=grad_scale,
                                              clip=clip, d=ema_decay).items()}
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    ema = None if ema is None else np.asarray(ema, dtype)
    # the norm: fp64 accumulation in every evaluation (the kernel's contract), rounded to fp32, as the state block holds it
    norm = np.float32(grad_norm64(g))
    one = f(1)
    with np.errstate(over="ignore", invalid="ignore"):
        ns = f(np.float32(o["scale"]) * norm) if dtype == np.float32 else f(norm) * o["scale"]
    if not np.isfinite(norm):
        return SimpleNamespace(p=p, m=m, v=v, ema=ema, norm=float(ns), coef=0.0, finite=False)
    coef = min(one, o["clip"] / (ns + f(np.float32(1e-6)))) if clip_mode == CLIP_NORM else one
    gi = (g * o["scale"]) * coef
    if clip_mode == CLIP_VALUE:
        gi = np.clip(gi, -o["clip"], o["clip"])
    if o["wd"] != 0:
        gi = gi + o["wd"] * p
    mi = m + (one - o["b1"]) * (gi - m)
    vi = o["b2"] * v + ((one - o["b2"]) * gi) * gi
    bc1 = f(1.0 - float(np.float32(betas[0])) ** step)
    bc2_sqrt = f(np.sqrt(1.0 - float(np.float32(betas[1])) ** step))
    denom = np.sqrt(vi) / bc2_sqrt + o["eps"]
    pn = p - (o["lr"] / bc1) * (mi / denom)
    en = None if ema is None else ema + (one - o["d"]) * (pn - ema)
    return SimpleNamespace(p=pn.astype(dtype), m=mi.astype(dtype), v=vi.astype(dtype), ema=None if en is None else en.astype(dtype),
                           norm=float(ns), coef=float(coef), finite=True)


def six_decades(n, seed):
    """(p, g, m, v, ema) as fp32 arrays: seeded, the gradient's magnitudes spread over six decades"""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4.0, 2.0, n)).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    m = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v = (0.01 * rng.random(n) + 1e-6).astype(np.float32)
    ema = (p + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return p, g, m, v, ema
