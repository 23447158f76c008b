"""The reference of a seeded run (pf_sample_seed_next): a CPU composition of the oracle's own functions.  It is
resample_ref.resampled_reference's loop with the begin lines of include/pfdyn.h ("seeded sampling") in front -- in place of
"state := noise0", for every graph g and center f

    D[g]  = c_init[g] - (mean of the graph's current protein rows)
    x[f]  = alpha_a * (seed_x[f] - D[g])              + sigma_a * noise0_x[f]
    h[f]  = alpha_a * (seed_h[f] / feat_norm_constant) + sigma_a * noise0_h[f]
    then the COM of all centers of the graph is removed from centers and protein

and a plan over the levels below a: ("denoise", s) / ("renoise", b, a') tuples, D(a-1) ... D(0) for a run without resampling.
With ``restraints`` the denoise op is guidance_ref's guided step.  ``seed=None`` gives the unseeded run of the same ops (the
initial draw as it is), which is what a seed that was NOT applied looks like.  ``double=True`` evaluates the same composition in
fp64 on the fp32 weights, batch, noise, seed and pins (O.sample_given_receptor64's rules)."""
import functools

import torch

from oracle import pf_oracle as O
from resample_ref import PREC, T, case, plan_of, renoise_coef, renoise_op

LEVELS = (1, 4, 9, 16, 24)
NOISE_SEED = 42


def steps_of(a):
    """the plan of a seeded run without resampling: D(a-1) ... D(0)"""
    return [("denoise", s) for s in reversed(range(a))]


def seed_coef(gamma, n_t, a):
    """(alpha_a, sigma_a), fp32: alpha / sigma(gamma(a / T))"""
    g_a = O.gamma_lookup(gamma, torch.tensor(a).float() / n_t, n_t)
    return O.alpha(g_a), O.sigma(g_a)


def seeded_begin(batch, bidx, c_init, prot_x, al, sg, seed_x, seed_h, nz0, fnorm):
    """the begin lines: returns (prot_x, x, h)"""
    D = (c_init - O.segment_mean(prot_x, batch.prot_ptr))[bidx["pharm"]]
    x = al * (seed_x - D) + sg * nz0[:, :3]
    h = al * (seed_h / fnorm) + sg * nz0[:, 3:]
    com = O.segment_mean(x, batch.pharm_ptr)
    return prot_x - com[bidx["prot"]], x - com[bidx["pharm"]], h


def seeded_reference(sd, cfg, batch, n_t, precision, level, plan, noise, seed, pins, init_pharm_com, fnorm=1.0, ep=False,
                     double=False, restraints=None, scale=1.0):
    """seed: (seed_x [Nf,3] caller's frame, seed_h [Nf,nf] raw rows) or None; pins: (flags, pin_x, pin_h) or None (nothing pinned).
    Returns x_0, h_0, frames x [n_ops + 1], frames h [n_ops + 1]."""
    batch32 = batch
    Nf = int(batch.pharm_ptr[-1])
    flags, pin_x, pin_h = pins if pins is not None else (torch.zeros(Nf, dtype=torch.int32), torch.zeros(Nf, 3),
                                                         torch.zeros(Nf, cfg.pharm_nf))
    dt = torch.float64 if double else torch.float32
    if double:
        sd, batch, noise = O.state_dict64(sd), O.batch64(batch), noise.double()
        pin_x, pin_h, init_pharm_com = pin_x.double(), pin_h.double(), init_pharm_com.double()
        seed = None if seed is None else (seed[0].double(), seed[1].double())
    rt = None
    if restraints is not None:
        import guidance_ref as G
        rt = G.restraint_tensors(restraints, dt)
        scale_t = torch.tensor(float(scale), dtype=torch.float32).to(dt)
    bidx, B = batch.batch_idxs(), batch.batch_size
    gamma = O.gamma_table(n_t, precision)
    coef = O.step_coefficients(gamma, n_t)
    px, ph = ((flags & 1) != 0)[:, None], ((flags & 2) != 0)[:, None]
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
    for it, op in enumerate(plan):
        nz = noise[1 + it]
        if op[0] == "renoise":
            prot_x, x_t, h_t = renoise_op(batch, bidx, *renoise_coef(gamma, n_t, op[1], op[2]), nz, prot_x, x_t, h_t)
        else:
            s = op[1]
            D = (c_init - O.segment_mean(prot_x, batch.prot_ptr))[bidx["pharm"]]          # before this step's shift
            t = coef["t"][s].expand(B).contiguous()
            t = t.double() if double else t
            if rt is not None:
                pred_h, pred_x, J = G.dynamics_vjp(sd, cfg, batch32, batch, prot_x, x_t, h_t, t)
            else:
                pred_h, pred_x = O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, t)
            a_ts, var, sig = coef["alpha_t_given_s"][s], coef["var_terms"][s], coef["sigma"][s]
            mu_x = coef["ep_zt"][s] * x_t + coef["ep_pred"][s] * pred_x if ep else x_t / a_ts - var * pred_x
            mu_h = coef["ep_zt"][s] * h_t + coef["ep_pred"][s] * pred_h if ep else h_t / a_ts - var * pred_h
            x_s, h_s = mu_x + sig * nz[:, :3], mu_h + sig * nz[:, 3:]
            if rt is not None:                          # guidance_ref.guided_reference's step (no clip)
                g_t = O.gamma_lookup(gamma, coef["t"][s], n_t)
                al_t, sg_t = O.alpha(g_t), O.sigma(g_t)
                x0_hat = pred_x if ep else (x_t - sg_t * pred_x) / al_t
                g0, _ = G.energy_and_g0(rt, batch.pharm_ptr, x0_hat + D)
                Jg = J(g0)
                grad = Jg if ep else g0 / al_t - (sg_t / al_t) * Jg
                x_s = x_s - (scale_t * (sig * sig)) * grad
            g_s = O.gamma_lookup(gamma, coef["s"][s], n_t)
            al, sg = O.alpha(g_s), O.sigma(g_s)
            x_s = torch.where(px, al * (pin_x - D) + sg * nz[:, :3], x_s)
            h_s = torch.where(ph, al * (pin_h / fnorm) + sg * nz[:, 3:], h_s)
            com = O.segment_mean(x_s, batch.pharm_ptr)
            x_t, h_t, prot_x = x_s - com[bidx["pharm"]], h_s, prot_x - com[bidx["prot"]]
        a, b = frame(prot_x, x_t, h_t)
        fx.append(a); fh.append(b)
    x_0 = x_t - O.segment_mean(prot_x, batch.prot_ptr)[bidx["pharm"]] + c_init[bidx["pharm"]]      # (O.sample_given_receptor's order)
    x_0, h_0 = torch.where(px, pin_x, x_0), torch.where(ph, pin_h, h_t * fnorm)
    fx[-1], fh[-1] = torch.where(px, pin_x, fx[-1]), h_0
    return x_0, h_0, torch.stack(fx), torch.stack(fh)


@functools.lru_cache(maxsize=None)
def seeded_case():
    """resample_ref.case() -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms with 3 / 8 / 5 / 1 / 6 centers, T = 24, precision
    0.25, init_pharm_com = pocket mean + 0.5 -- with the seed of test_gpu_pinned.pins_for: positions = pocket COM + 1.5 * randn,
    rows = random one-hots.  The case's pin arrays ARE such a draw for every center, so they serve as the seed; the pins of a
    seeded pinned run are the same values under resample_ref's flags (the seed rides on the pin arrays, as at model level).
    Returns (cfg, sd, batch, noise, seed, pins, com)."""
    cfg, sd, batch, plan, noise, pins, com = case()
    flags, pin_x, pin_h = pins
    return cfg, sd, batch, noise, (pin_x, pin_h), pins, com


@functools.lru_cache(maxsize=None)
def live_sd():
    """the case's weights with the scaled head (helpers.live_head); k from the unseeded run's first dynamics call, as in
    resample_ref.live_sd -- one scale for every level"""
    from resample_ref import live_sd as base
    return base()


@functools.lru_cache(maxsize=None)
def reference(level, ep=False, live=False, double=False, seeded=True, pinned=False, plan=None):
    """the composition of the case at seed level ``level``, computed once per session and left unchanged; plan: None (the plain
    steps) or a tuple of ops"""
    cfg, sd, batch, noise, seed, pins, com = seeded_case()
    if live:
        sd = live_sd()[0]
    ops = steps_of(level) if plan is None else list(plan)
    return seeded_reference(sd, cfg, batch, T, PREC, level, ops, noise[:len(ops) + 1], seed if seeded else None,
                            pins if pinned else None, com, ep=ep, double=double)
