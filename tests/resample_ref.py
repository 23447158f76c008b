"""The reference of a pinned run with resampling jumps (pf_sample_pinned_resampled / pf_renoise_step): a CPU composition of the
oracle's own functions.  It is test_gpu_pinned.py's `pinned_reference` loop opened up to a plan (schedule.resample_plan's
("denoise", s) / ("renoise", b, a) tuples), with one more branch for R(b -> a):

    z_a = alpha_{a|b} * z_b + sigma_{a|b} * noise      every center, coordinates and feature rows alike
    then the COM of all centers of the graph is removed from centers and protein

With resamples = 1 the plan is D(T-1) ... D(0) and the outputs are `pinned_reference`'s, bit for bit (asserted in
test_resample_host.py).  ``double=True`` evaluates the same composition in fp64 on the fp32 weights, batch, noise and pins
(O.sample_given_receptor64's rules: the fp32 coefficient tables promote, every step's edges are decided in fp32 on the
rounded coordinates)."""
import functools

import torch

from oracle import pf_oracle as O

T, PREC, JUMP, RESAMPLES = 24, 0.25, 5, 3
NOISE_SEED = 42


def plan_of(n_t, jump, resamples):
    """The op list of include/pfdyn.h, written out independently of schedule.resample_plan."""
    plan, a = [], n_t
    while a > 0:
        b = max(a - jump, 0)
        for rep in range(resamples):
            if rep:
                plan.append(("renoise", b, a))
            plan.extend(("denoise", s) for s in reversed(range(b, a)))
        a = b
    return plan


def renoise_coef(gamma, n_t, b, a):
    """(alpha_{a|b}, sigma_{a|b}), fp32: O.sigma_and_alpha_t_given_s(gamma(a / T), gamma(b / T))"""
    g_a = O.gamma_lookup(gamma, torch.tensor(a).float() / n_t, n_t)
    g_b = O.gamma_lookup(gamma, torch.tensor(b).float() / n_t, n_t)
    _, s_ab, a_ab, _ = O.sigma_and_alpha_t_given_s(g_a, g_b)
    return a_ab, s_ab


def renoise_op(batch, bidx, a_ab, s_ab, nz, prot_x, x_t, h_t):
    """R(b -> a) on the sampler state: returns (prot_x, x, h)"""
    x_a, h_a = a_ab * x_t + s_ab * nz[:, :3], a_ab * h_t + s_ab * nz[:, 3:]
    com = O.segment_mean(x_a, batch.pharm_ptr)
    return prot_x - com[bidx["prot"]], x_a - com[bidx["pharm"]], h_a


def resampled_reference(sd, cfg, batch, n_t, precision, plan, noise, flags, pin_x, pin_h, init_pharm_com, fnorm=1.0, ep=False,
                        double=False, return_state=False):
    """Returns x_0, h_0, frames x [n_ops + 1], frames h [n_ops + 1] (+ the sampler state (prot_x, x_t, h_t) behind the last op)."""
    if double:
        sd, batch, noise = O.state_dict64(sd), O.batch64(batch), noise.double()
        pin_x, pin_h, init_pharm_com = pin_x.double(), pin_h.double(), init_pharm_com.double()
    bidx, B = batch.batch_idxs(), batch.batch_size
    gamma = O.gamma_table(n_t, precision)
    coef = O.step_coefficients(gamma, n_t)
    px, ph = ((flags & 1) != 0)[:, None], ((flags & 2) != 0)[:, None]
    c_init = O.segment_mean(batch.prot_x, batch.prot_ptr)
    prot_x = batch.prot_x - init_pharm_com[bidx["prot"]]
    x_t, h_t = noise[0][:, :3].clone(), noise[0][:, 3:].clone()

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
            pred_h, pred_x = O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, t.double() if double else t)
            a_ts, var, sig = coef["alpha_t_given_s"][s], coef["var_terms"][s], coef["sigma"][s]
            mu_x = coef["ep_zt"][s] * x_t + coef["ep_pred"][s] * pred_x if ep else x_t / a_ts - var * pred_x
            mu_h = coef["ep_zt"][s] * h_t + coef["ep_pred"][s] * pred_h if ep else h_t / a_ts - var * pred_h
            x_s, h_s = mu_x + sig * nz[:, :3], mu_h + sig * nz[:, 3:]
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
    out = (x_0, h_0, torch.stack(fx), torch.stack(fh))
    return out + ((prot_x, x_t, h_t),) if return_state else out


@functools.lru_cache(maxsize=None)
def case():
    """test_gpu_pinned.py's shape -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms with 3 / 8 / 5 / 1 / 6 centers, the same
    flags, pins and initial COM -- with the noise of a resampled run: T = 24, jump 5, resamples 3 -> 82 ops, 83 rows"""
    from test_gpu_pinned import pins_for
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    batch = O.synthetic_batch([31, 32, 33, 34, 35], [48, 300, 40, 64, 32], [3, 8, 5, 1, 6], cfg)
    Nf = int(batch.pharm_ptr[-1])
    plan = plan_of(T, JUMP, RESAMPLES)
    assert Nf == 23 and len(plan) == 82
    noise = torch.randn(len(plan) + 1, Nf, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(NOISE_SEED))
    #        graph 0 | graph 1: 0, 1 both, 2 position, 3 row | graph 2: all | graph 3 | graph 4: the last
    flags = [0, 0, 0] + [3, 3, 1, 2, 0, 0, 0, 0] + [3] * 5 + [3] + [0, 0, 0, 0, 0, 3]
    pins = pins_for(batch, cfg, flags)
    com = O.segment_mean(batch.prot_x, batch.prot_ptr) + 0.5
    return cfg, sd, batch, plan, noise, pins, com


@functools.lru_cache(maxsize=None)
def live_sd():
    """the case's weights with the scaled head (helpers.live_head), k from the run's first dynamics call"""
    from helpers import sampler_live_head
    cfg, sd, batch, plan, noise, pins, com = case()
    return sampler_live_head(sd, cfg, batch, T, PREC, noise)


@functools.lru_cache(maxsize=None)
def reference(ep=False, live=False, double=False):
    """the composition of the case, computed once per session and left unchanged"""
    cfg, sd, batch, plan, noise, pins, com = case()
    if live:
        sd = live_sd()[0]
    return resampled_reference(sd, cfg, batch, T, PREC, plan, noise, *pins, com, ep=ep, double=double)


OP_ALONE_PLAN = [("renoise", 4, 9), ("renoise", 4, 9), ("denoise", 8)]


@functools.lru_cache(maxsize=None)
def op_alone_reference(double=False):
    """The op alone: the state of sample_begin (the initial draw, the protein shifted by the initial COM), then R(4 -> 9) of T = 24
    twice and D(8), with noise rows 1, 2 and 3.  Returns (frames x [4], frames h [4], the sampler state (prot_x, x, h) behind the
    two R ops, the state behind D(8)); frames 1 and 2 follow the R ops (frame 3 carries the given values)."""
    cfg, sd, batch, plan, noise, pins, com = case()
    kw = dict(double=double, return_state=True)
    _, _, fx, fh, st_d = resampled_reference(sd, cfg, batch, T, PREC, OP_ALONE_PLAN, noise, *pins, com, **kw)
    st_rr = resampled_reference(sd, cfg, batch, T, PREC, OP_ALONE_PLAN[:2], noise, *pins, com, **kw)[4]
    return fx, fh, st_rr, st_d
