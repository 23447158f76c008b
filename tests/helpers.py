"""Shared helpers for the test-suite (CPU side)."""
import functools
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import pf_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fiub" and z[k].ndim > 0 else z[k]) for k in z.files}


def batch_from(z, prefix="b_"):
    return O.PocketBatch(z[prefix + "prot_x"], z[prefix + "prot_h"], z[prefix + "prot_ptr"].long(),
                         z[prefix + "pharm_ptr"].long(), z[prefix + "pp_src"].long(), z[prefix + "pp_dst"].long())


def edge_set(src, dst):
    return set(zip(src.tolist(), dst.tolist()))


# dynamics goldens: file -> config that generated it (tests/golden/make_golden.py:main)
DYN_CASES = {
    "dynamics_c1.npz": O.DynamicsConfig(),
    "dynamics_ragged.npz": O.DynamicsConfig(),
    "dynamics_radius.npz": O.DynamicsConfig(n_convs=3, n_noise_gvps=3, message_norm=10, pf_k=0, ff_k=0),
    "dynamics_knnff.npz": O.DynamicsConfig(ff_k=2, pf_k=3, message_norm=1),
    # message_norm = 0 (per-graph normalisers, gvp.py:504-507): radius pf edges / kNN pf edges (the reference's
    # dynamics_gvp.py:220 bookkeeping, reproduced), ragged pockets
    "dynamics_gnorm_radius.npz": O.DynamicsConfig(message_norm=0, pf_k=0),
    "dynamics_gnorm_knn.npz": O.DynamicsConfig(message_norm=0, pf_k=5),
}


# training goldens (reference in train() mode, with the dropout draws recorded)
GRAD_CASES = {
    "train_grads.npz": O.DynamicsConfig(),
    "train_grads_radius.npz": O.DynamicsConfig(n_convs=3, n_noise_gvps=3, message_norm=10, pf_k=0, ff_k=0),
}


def dropout_from(z, cfg):
    """conv_layer-style mask dicts (one per layer) from a train_grads golden."""
    return [{nt: tuple(z[f"drop_{i}_{nt}_{w}_{c}"] for w in ("msg", "res") for c in ("s", "v"))
             for nt in ("pharm", "prot")} for i in range(cfg.n_convs)]


def head_wu_key(cfg):
    """The last GVP of the noise head has identity vector gating (dynamics_gvp.py:33), so eps_x is linear in its Wu [V, 1]."""
    return f"dynamics.noise_predictor.noise_predictor.gvps.{cfg.n_noise_gvps - 1}.Wu"


def live_head(sd, cfg, eps_x_ref):
    """(sd_live, k): a copy of ``sd`` whose last head Wu is multiplied by 2**k, k the integer that puts
    max|eps_x_ref| * 2**k in [0.5, 1) -- ``eps_x_ref`` being the reference's eps_x for ``sd`` (a golden or the oracle).
    A power of two scales every product and partial sum exactly, so the reference output for sd_live is eps_x_ref * 2**k
    bit for bit and eps_h is unchanged: with seeded random weights eps_x is ~1e-5, below every absolute tolerance of the
    suite; under sd_live it is of order one and the same tolerances bite."""
    m = float(torch.as_tensor(eps_x_ref).abs().max())
    assert m > 0 and math.isfinite(m)
    k = -math.frexp(m)[1]
    out = dict(sd)
    out[head_wu_key(cfg)] = sd[head_wu_key(cfg)] * (2.0 ** k)
    return out, k


BUDGET_FACTOR, BUDGET_FLOOR = 8.0, 2.0 ** -22


def within_budget(got, ref32, ref64, what=""):
    """The error budget of one output tensor, relative to m = max|ref64|: e32 = max|ref32 - ref64| / m is the rounding
    noise of ONE fp32 evaluation of this graph (the fp32 oracle against the fp64 oracle, same inputs, same edges),
    e = max|got - ref64| / m the kernel's.  Asserts e <= 8 * max(e32, 2**-22) and returns (e, e32).  The factor: another
    summation order (MFMA k-order, partial rows, fixed-point scatter) is an independent draw of the same noise -- over a
    few dozen entries the max of one draw rarely exceeds three times that of another --, the hardware exp / rcp / rsq at
    about an ulp each can add as much again, the rest is headroom.  The floor (a quarter ulp of the tensor's max) keeps a
    lucky e32 from setting an unreachable bound."""
    ref64 = torch.as_tensor(ref64).double()
    got = torch.as_tensor(got).detach().cpu().double()
    ref32 = torch.as_tensor(ref32).double()
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref32.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), what
    m = float(ref64.abs().max())
    e32 = float((ref32 - ref64).abs().max()) / m
    e = float((got - ref64).abs().max()) / m
    bound = BUDGET_FACTOR * max(e32, BUDGET_FLOOR)
    print(f"fp64 budget {what}: e {e:.3e} e32 {e32:.3e} ratio {e / max(e32, BUDGET_FLOOR):.2f}")
    assert e <= bound, f"{what}: error against fp64 {e:.3e} of the max > {BUDGET_FACTOR:g} x max(e32 = {e32:.3e}, 2**-22)"
    return e, e32


HEADS = ("recorded", "live")


def with_head(values):
    """parametrize values for ("<arg>,head"): the `recorded` leg keeps the test id it had before the head parameter existed"""
    import pytest
    return [pytest.param(v, h, id=str(v) if h == "recorded" else f"{v}+live") for v in values for h in HEADS]


def live_reference(sd, cfg, batch, prot_x, x_t, h_t, t, eps_x_ref=None):
    """The references of a `live` leg for one dynamics call: sd (live head), k, the fp32 oracle's outputs on it (oh, ox) and the
    fp64 oracle's (h64, x64).  eps_x_ref: the reference's eps_x for ``sd`` (a golden); default: the fp32 oracle's."""
    if eps_x_ref is None:
        eps_x_ref = O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, t)[1]
    sd_live, k = live_head(sd, cfg, eps_x_ref)
    oh, ox = O.dynamics_forward(sd_live, cfg, batch, prot_x, x_t, h_t, t)
    h64, x64 = O.dynamics_forward64(sd_live, cfg, batch, prot_x, x_t, h_t, t)
    return SimpleNamespace(sd=sd_live, k=k, oh=oh, ox=ox, h64=h64, x64=x64)


@functools.lru_cache(maxsize=None)
def golden_live(name):
    """live_reference of a DYN_CASES golden, computed once per session and left unchanged"""
    z, cfg = load(name), DYN_CASES[name]
    return live_reference(O.make_state_dict(cfg, int(z["wseed"])), cfg, batch_from(z), z["prot_x"], z["x_t"], z["h_t"], z["t"],
                          eps_x_ref=z["eps_x"])


def check_live(eps_h, eps_x, live, what, rtol, atol, z=None):
    """A `live` leg's assertions: eps_x (now of order one) and eps_h against the fp32 oracle on the live weights -- and, with a
    golden ``z``, against the reference's recorded output times 2**k, which is its output for those weights -- at the tolerance
    the `recorded` leg uses; then both outputs inside the fp64 error budget (within_budget).  Returns the two (e, e32)."""
    eps_h, eps_x = eps_h.detach().cpu(), eps_x.detach().cpu()
    torch.testing.assert_close(eps_h, live.oh, rtol=rtol, atol=atol)
    torch.testing.assert_close(eps_x, live.ox, rtol=rtol, atol=atol)
    if z is not None:
        torch.testing.assert_close(eps_h, z["eps_h"], rtol=rtol, atol=atol)
        torch.testing.assert_close(eps_x, z["eps_x"] * 2.0 ** live.k, rtol=rtol, atol=atol)
    return (within_budget(eps_h, live.oh, live.h64, what + " eps_h"), within_budget(eps_x, live.ox, live.x64, what + " eps_x"))


def frames_within_budget(got, ref64, e32, what):
    """Every frame of a trajectory within 8 * max(e32, 2**-22 * max|frame|) of the fp64 frames; e32: the fp32 oracle's worst
    absolute deviation from them over all frames.  Returns the worst ratio err / max(e32, floor)."""
    got, ref64 = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref64).double()
    assert got.shape == ref64.shape and bool(torch.isfinite(got).all()), what
    n = ref64.shape[0]
    err = (got - ref64).abs().reshape(n, -1).max(dim=1).values
    unit = torch.clamp(BUDGET_FLOOR * ref64.abs().reshape(n, -1).max(dim=1).values, min=float(e32))
    ratio = err / unit
    worst = int(ratio.argmax())
    print(f"fp64 budget {what}: worst frame {worst} err {float(err[worst]):.3e} e32 {float(e32):.3e} ratio {float(ratio[worst]):.2f}")
    assert float(ratio[worst]) <= BUDGET_FACTOR, f"{what}: frame {worst} is {float(err[worst]):.3e} from fp64, e32 {float(e32):.3e}"
    return float(ratio[worst])


def sampler_live_head(sd, cfg, batch, T, precision, noise):
    """live_head for a sampling run: k from the fp32 oracle's eps_x of the run's first dynamics call (x_T = noise[0], t = 1)"""
    prot_x = batch.prot_x - O.segment_mean(batch.prot_x, batch.prot_ptr)[batch.batch_idxs()["prot"]]
    t = O.step_coefficients(O.gamma_table(T, precision), T)["t"][T - 1].expand(batch.batch_size).contiguous()
    nf = cfg.pharm_nf
    _, ex = O.dynamics_forward(sd, cfg, batch, prot_x, noise[0][:, :3], noise[0][:, 3:3 + nf], t)
    return live_head(sd, cfg, ex)
