"""The reference of a few-step run: a CPU composition of the oracle's own functions (dynamics_forward, segment_mean, gamma_table,
alpha, sigma), in fp32 and -- ``double=True`` -- in fp64 on the fp32 weights, batch, noise and coefficients.  It is
seeded_ref.seeded_reference's loop (the same begin, seeded or not) over a list of ops of two kinds:

    ("first", s, t, eta)        z_s = z_t / a_ts - var * eps + sigma * noise     (or  ep_zt * z_t + ep_pred * pred  per endpoint block)
    ("ms", prev, t, s)          z_s = (cz * z_t + c0 * o_t) + c1 * o_prev        prev None: first order, c1 = 0

each followed by the removal of the COM of the graph's centers from centers and protein.  The coefficient formulas are written
out here from the gamma table, independently of pharmacoforge_amd.schedule: eta = 1 is the oracle's sigma_and_alpha_t_given_s
composition at a general (s, t) in fp32; eta < 1 and the multistep triples are float64 numpy expressions through lambda =
log(alpha / sigma), cast to fp32.  A first-order op consumes the next noise row; a multistep op consumes none."""
import functools
import math

import numpy as np
import torch

from oracle import pf_oracle as O
from resample_ref import PREC, T, case
from seeded_ref import seed_coef, seeded_begin

TOL = 5e-3                       # the project's whole-run tolerance (test_gpu_seeded.check)


# ---- plans, written out independently of schedule.level_plan (these are the plans the GPU tests run) ----
def uniform_plan(top, n):
    """round(top (1 - i / n)): no collisions for the (top, n) used here"""
    lv = [int(round(top * (1.0 - i / n))) for i in range(n + 1)]
    assert lv[0] == top and lv[-1] == 0 and all(a > b for a, b in zip(lv, lv[1:]))
    return lv


# ---- coefficients from the gamma table ----
def _g(gamma, n_t, level):
    return O.gamma_lookup(gamma, torch.tensor(level).float() / n_t, n_t)


def _alpha_sigma64(gamma, n_t, level):
    g = float(_g(gamma, n_t, level))
    return math.sqrt(1.0 / (1.0 + math.exp(g))), math.sqrt(1.0 / (1.0 + math.exp(-g)))


def first_coef(gamma, n_t, s, t, eta):
    """(a_ts, var, sigma, ep_zt, ep_pred) of the step t -> s, fp32 scalars"""
    if eta == 1.0:
        g_s, g_t = _g(gamma, n_t, s), _g(gamma, n_t, t)
        s2_ts, s_ts, a_ts, a_s = O.sigma_and_alpha_t_given_s(g_t, g_s)
        sig_s, sig_t = O.sigma(g_s), O.sigma(g_t)
        return a_ts, s2_ts / a_ts / sig_t, s_ts * sig_s / sig_t, a_ts * (sig_s ** 2) / (sig_t ** 2), a_s * s2_ts / (sig_t ** 2)
    (al_s, sg_s), (al_t, sg_t) = _alpha_sigma64(gamma, n_t, s), _alpha_sigma64(gamma, n_t, t)
    a_ts = al_t / al_s
    s2_ts = sg_t ** 2 - (a_ts * sg_s) ** 2              # sigma_t^2 = alpha_{t|s}^2 sigma_s^2 + sigma_{t|s}^2
    s_eta = eta * math.sqrt(max(s2_ts, 0.0)) * sg_s / sg_t
    k = math.sqrt(sg_s ** 2 - s_eta ** 2)
    vals = (a_ts, sg_t / a_ts - k, s_eta, k / sg_t, al_s - k * al_t / sg_t)
    return tuple(torch.tensor(np.float32(v)) for v in vals)


def ms_coef(gamma, n_t, prev, t, s, endpoint):
    """(cz, c0, c1) of one block, fp32 scalars; prev None (or s == 0): first order"""
    (al_s, sg_s), (al_t, sg_t) = _alpha_sigma64(gamma, n_t, s), _alpha_sigma64(gamma, n_t, t)
    lam_s, lam_t = math.log(al_s / sg_s), math.log(al_t / sg_t)
    h = lam_s - lam_t
    w = 0.0
    if prev is not None and s != 0:
        al_p, sg_p = _alpha_sigma64(gamma, n_t, prev)
        w = 0.5 * h / (lam_t - math.log(al_p / sg_p))   # 1 / (2 r)
    if endpoint:
        base = al_s * math.expm1(-h)
        vals = (sg_s / sg_t, -base * (1.0 + w), base * w)
    else:
        base = sg_s * math.expm1(h)
        vals = (al_s / al_t, -base * (1.0 + w), base * w)
    return tuple(torch.tensor(np.float32(v + 0.0)) for v in vals)


# ---- op lists ----
def first_ops(levels, eta=1.0):
    return [("first", s, t, float(eta)) for t, s in zip(levels[:-1], levels[1:])]


def ms_ops(levels, history=False):
    """the multistep steps of a plan; history: the step in front of levels[0] was a multistep step too (never here: a run's first
    multistep step, and the first after a plain step, is first order)"""
    return [("ms", levels[i - 1] if i else None, levels[i], levels[i + 1]) for i in range(len(levels) - 1)]


def fewstep_reference(sd, cfg, batch, n_t, precision, ops, noise, init_pharm_com, seed=None, level=None, fnorm=1.0, ep=(False, False),
                      double=False, wrong=None):
    """ops: see the module's docstring.  seed: (seed_x, seed_h) with ``level``, or None.  ep = (ep_coord, ep_feat).
    wrong: None, or the name of a wrong neighbour -- "c1_zero" (every multistep c1 forced to 0), "unit_stride" (a first-order op
    takes the coefficients of (t - 1, t) in place of (s, t)), "eta1" (eta = 1 in place of the op's).
    Returns x_0, h_0, frames x [n_ops + 1], frames h [n_ops + 1]."""
    dt = torch.float64 if double else torch.float32
    if double:
        sd, batch, noise, init_pharm_com = O.state_dict64(sd), O.batch64(batch), noise.double(), init_pharm_com.double()
        seed = None if seed is None else (seed[0].double(), seed[1].double())
    bidx, B = batch.batch_idxs(), batch.batch_size
    gamma = O.gamma_table(n_t, precision)
    c_init = O.segment_mean(batch.prot_x, batch.prot_ptr)
    prot_x = batch.prot_x - init_pharm_com[bidx["prot"]]
    if seed is None:
        x_t, h_t = noise[0][:, :3].clone(), noise[0][:, 3:].clone()
    else:
        prot_x, x_t, h_t = seeded_begin(batch, bidx, c_init, prot_x, *seed_coef(gamma, n_t, level), seed[0], seed[1], noise[0], fnorm)

    def frame(p, x, h):
        return x + (c_init - O.segment_mean(p, batch.prot_ptr))[bidx["pharm"]], h * fnorm
    a, b = frame(prot_x, x_t, h_t)
    fx, fh = [a], [b]
    row, prev_x, prev_h = 1, None, None
    for op in ops:
        t_lvl = op[2]
        t = (torch.tensor(t_lvl).float() / n_t).expand(B).contiguous()
        pred_h, pred_x = O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, t.double() if double else t)
        if op[0] == "first":
            s, eta = op[1], op[3]
            if wrong == "unit_stride":
                s = t_lvl - 1
            if wrong == "eta1":
                eta = 1.0
            a_ts, var, sig, ep_zt, ep_pred = (c.to(dt) for c in first_coef(gamma, n_t, s, t_lvl, eta))
            nz = noise[row]
            row += 1
            mu_x = ep_zt * x_t + ep_pred * pred_x if ep[0] else x_t / a_ts - var * pred_x
            mu_h = ep_zt * h_t + ep_pred * pred_h if ep[1] else h_t / a_ts - var * pred_h
            x_s, h_s = mu_x + sig * nz[:, :3], mu_h + sig * nz[:, 3:]
            prev_x = prev_h = None
        else:
            prev = op[1] if prev_x is not None else None
            cx = [c.to(dt) for c in ms_coef(gamma, n_t, prev, t_lvl, op[3], ep[0])]
            ch = [c.to(dt) for c in ms_coef(gamma, n_t, prev, t_lvl, op[3], ep[1])]
            x_s, h_s = cx[0] * x_t + cx[1] * pred_x, ch[0] * h_t + ch[1] * pred_h
            if prev is not None and op[3] != 0 and wrong != "c1_zero":
                x_s, h_s = x_s + cx[2] * prev_x, h_s + ch[2] * prev_h
            prev_x, prev_h = pred_x, pred_h
        com = O.segment_mean(x_s, batch.pharm_ptr)
        x_t, h_t, prot_x = x_s - com[bidx["pharm"]], h_s, prot_x - com[bidx["prot"]]
        a, b = frame(prot_x, x_t, h_t)
        fx.append(a); fh.append(b)
    x_0 = x_t - O.segment_mean(prot_x, batch.prot_ptr)[bidx["pharm"]] + c_init[bidx["pharm"]]      # (O.sample_given_receptor's order)
    h_0 = h_t * fnorm
    fh[-1] = h_0
    return x_0, h_0, torch.stack(fx), torch.stack(fh)


def worst_center_gap(ref, other):
    """the largest distance between the two compositions' x_0 over the centers, and the same for the h_0 rows"""
    return float((ref[0] - other[0]).abs().max()), float((ref[1] - other[1]).abs().max())


@functools.lru_cache(maxsize=None)
def reference(ops, ep=(False, False), double=False, seeded=False, level=None, wrong=None, live=True):
    """the composition of resample_ref.case() for a tuple of ops, computed once per session and left unchanged; live: with the
    scaled head of resample_ref.live_sd (eps_x of order one, so that the previous output's term counts in the coordinates)"""
    cfg, sd, batch, plan, noise, pins, com = case()
    if live:
        from resample_ref import live_sd
        sd = live_sd()[0]
    seed = (pins[1], pins[2]) if seeded else None
    return fewstep_reference(sd, cfg, batch, T, PREC, list(ops), noise, com, seed=seed, level=level, ep=ep, double=double, wrong=wrong)
