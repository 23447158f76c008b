"""The reference of a guided run with pair guidance (pf_guide_pairs_next): guidance_ref.guided_reference -- with a field or type
guidance present, type_guidance_ref.types_reference -- with the lines of include/pfdyn.h ("pair guidance") inserted: distance
restraints between two centers of one graph on the predicted clean centers, a position-pinned center standing at its given
position and taking no gradient, added into g0 and E behind every other energy.  Without pairs it is
guidance_ref.guided_reference bit for bit (asserted in test_pair_guidance_host.py).

The sums follow k_guide_pairs (pf_pairs.hip): per center the covered partners b, restraints ascending and partners ascending
within a restraint, in four partial sums by (b & 3) that meet as (s0 + s1) + (s2 + s3); E_pair = sum_f e_f, f ascending.

``double=True``: the same composition in fp64 on the fp32 inputs (guidance_ref's rules).  The teeth of the GPU tests:
``use_pairs=False`` ignores the arming; ``pin_rule=False`` uses x0_hat + D for a position-pinned center and gives it its gradient
(what a kernel that forgot the pin flags would compute)."""
import functools
import math
from types import SimpleNamespace

import torch

import guidance_ref as G
import pocket_field_ref as F
import type_guidance_ref as TG
from oracle import pf_oracle as O

T, PREC, TOL, GUIDE_SCALE = G.T, G.PREC, G.TOL, G.GUIDE_SCALE
INF = math.inf


def make_pairs(restraints):
    """Pair restraints as the library receives them: one list or None per graph of (i, j, lo, hi, w) -- None / '*' / a negative
    index: every center -- with the values rounded to fp32"""
    f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
    idx = lambda c: -1 if c is None or c == "*" or int(c) < 0 else int(c)
    return [[(idx(i), idx(j), f32(lo), f32(hi), f32(w)) for i, j, lo, hi, w in (rows or [])] for rows in restraints]


def covered(i, j, n):
    """[n, n] bool: entry (a, b) is set when the restraint (i, j) covers the pair {a, b}"""
    M = torch.zeros(n, n, dtype=torch.bool)
    if i >= 0 and j >= 0:
        M[i, j] = M[j, i] = True
    elif i >= 0 or j >= 0:
        c0 = i if i >= 0 else j
        M[c0, :] = True
        M[:, c0] = True
    else:
        M[:, :] = True
    M.fill_diagonal_(False)
    return M


def pair_terms(pt, pharm_ptr, y, px=None, pin_x=None, pin_rule=True):
    """(g_pair [Nf, 3], E_pair [B], stats) of the pair restraints ``pt`` (make_pairs) on the points y [Nf, 3] = x0_hat + D, in y's
    dtype.  px [Nf] bool / pin_x [Nf, 3]: the position-pinned centers and their given positions.  stats: over all restraints the
    covered unordered pairs, and those whose lower / upper hinge is open."""
    dt = y.dtype
    B = len(pharm_ptr) - 1
    g_pair, E_pair = torch.zeros_like(y), torch.zeros(B, dtype=dt)
    stats = dict(covered=0, lo_open=0, hi_open=0)
    if px is not None and pin_rule:
        y = torch.where(px[:, None], pin_x.to(dt), y)
    for g, rows in enumerate(pt):
        f0, f1 = int(pharm_ptr[g]), int(pharm_ptr[g + 1])
        n = f1 - f0
        if n < 2 or not rows:
            continue
        Y = y[f0:f1]
        d = Y[:, None, :] - Y[None, :, :]                   # [c, b]: y_c - y_b
        rho = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        safe = torch.where(rho > 0, rho, torch.ones_like(rho))
        upper = torch.arange(n)[:, None] < torch.arange(n)[None, :]
        acc = [torch.zeros(n, 3, dtype=dt) for _ in range(4)]
        en = [torch.zeros(n, dtype=dt) for _ in range(4)]
        for i, j, lo, hi, w in rows:
            lo, hi, w = lo.to(dt), hi.to(dt), w.to(dt)
            M = covered(i, j, n)
            m_lo, m_hi = torch.clamp(lo - rho, min=0), torch.clamp(rho - hi, min=0)
            cf = torch.where(rho > 0, ((2.0 * w) * (m_hi - m_lo)) / safe, torch.zeros_like(rho))
            Tm = cf[..., None] * d
            Em = w * (m_lo * m_lo + m_hi * m_hi)
            stats["covered"] += int((M & upper).sum())
            stats["lo_open"] += int((M & upper & (m_lo > 0)).sum())
            stats["hi_open"] += int((M & upper & (m_hi > 0)).sum())
            for b in range(n):
                col = M[:, b]
                if not bool(col.any()):
                    continue
                acc[b & 3] = acc[b & 3] + torch.where(col[:, None], Tm[:, b], torch.zeros_like(Tm[:, b]))
                en[b & 3] = en[b & 3] + torch.where(col & upper[:, b], Em[:, b], torch.zeros_like(Em[:, b]))
        gp = (acc[0] + acc[1]) + (acc[2] + acc[3])
        if px is not None and pin_rule:
            gp = torch.where(px[f0:f1, None], torch.zeros_like(gp), gp)
        g_pair[f0:f1] = gp
        ef = (en[0] + en[1]) + (en[2] + en[3])
        tot = torch.zeros((), dtype=dt)
        for f in range(n):
            tot = tot + ef[f]
        E_pair[g] = tot
    return g_pair, E_pair, stats


def pairs_reference(sd, cfg, batch, n_t, precision, noise, flags, pin_x, pin_h, init_pharm_com, restraints, field=None, types=None,
                    pairs=None, scale=1.0, clip=0.0, fnorm=1.0, ep=False, double=False, n_steps=None, use_pairs=True, pin_rule=True):
    """type_guidance_ref.types_reference's namespace plus g_pair [n_steps, Nf, 3], E_pair [n_steps, B] and stats (one dict per
    step); pairs: one list or None per graph of (i, j, lo, hi, w), or None"""
    batch32 = batch
    dt = torch.float64 if double else torch.float32
    if double:
        sd, batch, noise = O.state_dict64(sd), O.batch64(batch), noise.double()
        pin_x, pin_h, init_pharm_com = pin_x.double(), pin_h.double(), init_pharm_com.double()
    rt = G.restraint_tensors(restraints, dt) if restraints is not None else [[] for _ in range(batch.batch_size)]
    fd, tg = field, types
    pt = make_pairs(pairs) if pairs is not None and use_pairs else None
    guided = any(len(rs) for rs in rt) or fd is not None or tg is not None or (pt is not None and any(len(r) for r in pt))
    scale_t, clip_t = torch.tensor(float(scale), dtype=torch.float32).to(dt), torch.tensor(float(clip), dtype=torch.float32).to(dt)
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
    fx, fh, Es, g0s, grads, shifts, E3s = [a], [b], [], [], [], [], []
    Ets, g0hs, gradhs, shifths, gps, Eps, stats = [], [], [], [], [], [], []
    order = list(reversed(range(n_t)))[:n_steps]
    for it, s in enumerate(order):
        nz = noise[1 + it]
        D = (c_init - O.segment_mean(prot_x, batch.prot_ptr))[bidx["pharm"]]          # before this step's shift
        t = coef["t"][s].expand(B).contiguous()
        t = t.double() if double else t
        if guided and tg is not None:
            pred_h, pred_x, J2 = TG.dynamics_vjp2(sd, cfg, batch32, batch, prot_x, x_t, h_t, t)
        elif guided:
            pred_h, pred_x, J = G.dynamics_vjp(sd, cfg, batch32, batch, prot_x, x_t, h_t, t)
        else:
            pred_h, pred_x = O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, t)
        a_ts, var, sig = coef["alpha_t_given_s"][s], coef["var_terms"][s], coef["sigma"][s]
        mu_x = coef["ep_zt"][s] * x_t + coef["ep_pred"][s] * pred_x if ep else x_t / a_ts - var * pred_x
        mu_h = coef["ep_zt"][s] * h_t + coef["ep_pred"][s] * pred_h if ep else h_t / a_ts - var * pred_h
        x_s, h_s = mu_x + sig * nz[:, :3], mu_h + sig * nz[:, 3:]
        if guided:
            g_t = O.gamma_lookup(gamma, coef["t"][s], n_t)
            al_t, sg_t = O.alpha(g_t), O.sigma(g_t)
            x0_hat = pred_x if ep else (x_t - sg_t * pred_x) / al_t
            g0, E = G.energy_and_g0(rt, batch.pharm_ptr, x0_hat + D)
            h0_hat = pred_h if ep else (h_t - sg_t * pred_h) / al_t
            if fd is not None:                  # the pocket field's lines
                g_cl, g_co, E_cl, E_co = F.field_terms(fd, batch, prot_x, x0_hat, D, h0_hat)
                E3s.append(torch.stack([E, E_cl, E_co], dim=1))
                g0, E = (g0 + g_cl) + g_co, (E + E_cl) + E_co
            if tg is not None:                  # type guidance's lines, in front of the pairs: they add into g0 and E too
                g0_h, gy, E_type = TG.type_restraint_terms(tg, batch.pharm_ptr, x0_hat + D, h0_hat)
                if tg.comp and fd is not None and fd.ph_ptr is not None and float(fd.w_comp) > 0 and fd.ph_ptr[-1] > 0:
                    gc_h, E_un = TG.comp_type_terms(fd, tg, batch, x0_hat, D, h0_hat)
                    g0_h, E_type = g0_h + gc_h, E_type + E_un
                g0, E = g0 + gy, E + E_type
            if pt is not None and any(len(r) for r in pt):       # pair guidance's lines: the last energy in front of the VJP
                g_pair, E_pair, st = pair_terms(pt, batch.pharm_ptr, x0_hat + D, px[:, 0], pin_x, pin_rule)
                g0, E = g0 + g_pair, E + E_pair
                gps.append(g_pair); Eps.append(E_pair); stats.append(st)
            if tg is not None:
                phi_x = torch.ones((), dtype=dt) if ep else -(sg_t / al_t)
                phi_h = phi_x
                Jg, Jh = J2(g0, (phi_h / phi_x) * g0_h)
                grad_h = phi_x * Jh if ep else g0_h / al_t + phi_x * Jh
                shift_h = (tg.scale.to(dt) * (sig * sig)) * grad_h
                if float(tg.clip) > 0:
                    nh = torch.sqrt((shift_h * shift_h).sum(dim=1))
                    over = nh > tg.clip.to(dt)
                    shift_h = torch.where(over[:, None], shift_h * (tg.clip.to(dt) / torch.where(over, nh, torch.ones_like(nh)))[:, None], shift_h)
                h_s = h_s - shift_h
                Ets.append(E_type); g0hs.append(g0_h); gradhs.append(grad_h); shifths.append(shift_h)
            else:
                Jg = J(g0)
            grad = Jg if ep else g0 / al_t - (sg_t / al_t) * Jg
            shift = (scale_t * (sig * sig)) * grad
            n = torch.sqrt((shift[:, 0] * shift[:, 0] + shift[:, 1] * shift[:, 1]) + shift[:, 2] * shift[:, 2])
            if float(clip) > 0:
                over = n > clip_t
                shift = torch.where(over[:, None], shift * (clip_t / torch.where(over, n, torch.ones_like(n)))[:, None], shift)
            x_s = x_s - shift
            Es.append(E); g0s.append(g0); grads.append(grad); shifts.append(shift)
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
    stack = lambda v, shape: torch.stack(v) if v else torch.zeros(shape, dtype=dt)
    Nf, nf = x_t.shape[0], h_t.shape[1]
    return SimpleNamespace(x0=x_0, h0=h_0, fx=torch.stack(fx), fh=torch.stack(fh), E=stack(Es, (0, B)), g0=stack(g0s, (0, Nf, 3)),
                           grad=stack(grads, (0, Nf, 3)), shift=stack(shifts, (0, Nf, 3)), E3=stack(E3s, (0, B, 3)),
                           E_type=stack(Ets, (0, B)), g0_h=stack(g0hs, (0, Nf, nf)), grad_h=stack(gradhs, (0, Nf, nf)),
                           shift_h=stack(shifths, (0, Nf, nf)), g_pair=stack(gps, (0, Nf, 3)), E_pair=stack(Eps, (0, B)), stats=stats)


def final_pair_energy(pairs, batch, x0):
    """E_pair [B] of the pair restraints on final centers x0 (caller's frame), fp64"""
    return pair_terms(make_pairs(pairs), batch.pharm_ptr, x0.double())[1]


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------
# The minimum separations weigh 0.125: at 1 the fp32 composition of the endpoint parameterisation ends 1.6 A from its fp64 self (its
# frames part from step 14 on: energies of 250 on eight centers), at 0.125 it stays within 4e-5 and the noise one within 4e-6
W_SEP = 0.125
PAIRS = [None,
         [(None, None, 4.0, INF, W_SEP), (0, 5, 0.0, 6.0, 1.0)],
         [(1, 3, 5.0, 7.0, 2.0), (2, None, 3.0, INF, 0.5)],
         [(None, None, 4.0, INF, W_SEP)],
         [(None, None, 4.0, INF, W_SEP)]]


@functools.lru_cache(maxsize=None)
def case():
    """guidance_ref.case() -- five ragged pockets with 3 / 8 / 5 / 1 / 6 centers, graph 1's centers 0 and 1 position-pinned, its
    spatial restraints, T = 24, live head -- with pair restraints:
      graph 0  none
      graph 1  a minimum separation of 4 between all centers (weight W_SEP here and below), and an upper bound of 6 between the pinned center 0 and the free 5
      graph 2  centers 1 and 3 five to seven apart (weight 2), center 2 at least 3 from every other (weight 0.5)
      graph 3  (the single-center graph) a minimum separation: no pairs, exact zeros
      graph 4  a minimum separation of 4 between all centers
    Returns guidance_ref.case()'s tuple with the pair restraints appended."""
    return G.case() + (PAIRS,)


@functools.lru_cache(maxsize=None)
def reference(ep=False, double=False, use_pairs=True, pin_rule=True):
    """the composition of the case, computed once per session and left unchanged"""
    cfg, sd, k, batch, noise, pins, com, restraints, pairs = case()
    return pairs_reference(sd, cfg, batch, T, PREC, noise, *pins, com, restraints, pairs=pairs, scale=GUIDE_SCALE, ep=ep, double=double,
                           use_pairs=use_pairs, pin_rule=pin_rule)


WIDE_PAIRS = [[(None, None, 4.0, INF, 1.0)], [(None, None, 4.0, INF, 1.0)]]


@functools.lru_cache(maxsize=None)
def wide_reference(use_pairs=True):
    """guidance_ref.wide_case() at (64, 32), T = 12, feat_norm 2, with a minimum separation of 4 on each graph"""
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    return pairs_reference(sd, cfg, batch, G.WIDE_T, PREC, noise, *pins, com, restraints, pairs=WIDE_PAIRS, scale=GUIDE_SCALE, fnorm=2.0,
                           use_pairs=use_pairs)


@functools.lru_cache(maxsize=None)
def shapes_case():
    """One step's batch of the shapes at which the kernel can go wrong: graphs of 1, 2, 5, 3 and 64 centers (the last:
    pocket_field_ref.tall_case()'s size, sixteen partners per quarter).
      graph 0  (one center) a minimum separation: no pairs, exact zeros
      graph 1  (two centers, both pinned to the same point: rho == 0) a window of 2 .. 3: E = w lo^2, a zero gradient
      graph 2  (five centers) a restraint naming the last center twice over: (4, *) and (0, 4)
      graph 3  (three centers) no pair restraint, between two graphs that have some
      graph 4  (64 centers) the cap of 256: a minimum separation, the pair {62, 63}, and 254 more of every form
    Returns (cfg, sd, k, batch, noise, pins, com, pairs)."""
    from helpers import sampler_live_head
    from test_gpu_pinned import pins_for
    cfg = O.DynamicsConfig()
    sizes = [1, 2, 5, 3, 64]
    batch = O.synthetic_batch([71, 72, 73, 74, 77], [40, 48, 56, 32, 600], sizes, cfg)
    Nf = sum(sizes)
    noise = torch.randn(2, Nf, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(G.NOISE_SEED))
    sd, k = sampler_live_head(O.make_state_dict(cfg, 0), cfg, batch, T, PREC, noise)
    flags = [0] * Nf
    flags[1] = flags[2] = 1
    pins = pins_for(batch, cfg, flags)
    pins[1][2] = pins[1][1]                     # both pinned centers of graph 1 at one point
    com = O.segment_mean(batch.prot_x, batch.prot_ptr) + 0.5
    gen = torch.Generator().manual_seed(3)
    many = [(None, None, 3.0, INF, 0.25), (62, 63, 2.0, 5.0, 1.0)]
    while len(many) < 256:
        i, j = (int(v) for v in torch.randint(0, 64, (2,), generator=gen))
        lo = float(torch.rand((), generator=gen)) * 6.0
        form = len(many) % 4
        if i == j:
            continue
        many.append([(i, j, lo, lo + 2.0, 0.5), (i, None, lo, INF, 0.125), (None, j, 0.0, lo + 1.0, 0.125), (j, i, lo, lo, 0.5)][form])
    pairs = [[(None, None, 4.0, INF, 1.0)], [(0, 1, 2.0, 3.0, 1.5)], [(4, None, 5.0, INF, 1.0), (0, 4, 1.0, 2.0, 2.0)], None, many]
    return cfg, sd, k, batch, noise, pins, com, pairs
