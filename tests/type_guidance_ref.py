"""The reference of a guided run with type guidance (pf_guide_types_next): pocket_field_ref.field_reference with the lines of
include/pfdyn.h ("type guidance") inserted -- typed restraints on the predicted clean feature rows (a compact C1 window in the
caller's frame times the cross-entropy of the soft type assignment), the complementarity energy's gradient w.r.t. those rows, the
VJP of the dynamics with g_eps_h = (phi_h / phi_x) g0_h next to g_eps_x = g0, and the feature shift in front of the type-pin
select.  Without type guidance it is pocket_field_ref.field_reference bit for bit (asserted in test_type_guidance_host.py).

``double=True``: the same composition in fp64 on the fp32 inputs (guidance_ref's rules).  The teeth of the GPU tests:
``use_jh=False`` drops J_h from grad_h (what a step end that forgot the VJP's feature output would compute), ``zero_geps_h=True``
hands the VJP a zero g_eps_h (what a step that kept the stored zeros would compute), ``use_types=False`` ignores the arming."""
import functools
from types import SimpleNamespace

import torch

import guidance_ref as G
import pocket_field_ref as F
from oracle import pf_oracle as O

T, PREC, TOL, GUIDE_SCALE = G.T, G.PREC, G.TOL, G.GUIDE_SCALE
SHARP = F.SHARP
FEAT_SCALE, UNMATCHED = 4.0, 1.5
WIDE_FEAT_SCALE = 1.0             # (64, 32) with feat_norm 2: at 4 the fp32 composition is 4e-3 from its fp64 self, at 1 5e-4


def make_types(restraints=None, scale=1.0, clip=0.0, sharpness=0.0, complementarity=False, unmatched=0.0):
    """Type guidance as the library receives it: every value rounded to fp32.  The arguments are PfEngine.types_next's;
    restraints: one list or None per graph of (type index, center or None, point, radius, weight)."""
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float32)
    rs = None
    if restraints is not None:
        rs = [[(int(t), -1 if c is None or c == "*" else int(c), f32([float(v) for v in p]), f32(float(r)), f32(float(w)))
               for t, c, p, r, w in (rows or [])] for rows in restraints]
    return SimpleNamespace(restraints=rs, raw=restraints, scale=f32(scale), clip=f32(clip), sharp=f32(sharpness),
                           comp=bool(complementarity), unmatched=f32(unmatched))


def types_kwargs(tg):
    """the dict PfEngine.sample(types=...) takes"""
    return dict(restraints=tg.raw, scale=float(tg.scale), clip=float(tg.clip), sharpness=float(tg.sharp), complementarity=tg.comp,
                unmatched=float(tg.unmatched))


def type_restraint_terms(tg, pharm_ptr, y, h0_hat):
    """(g0_h [Nf, nf], gy [Nf, 3], E [B]) of the type restraints, in y's dtype; j ascending per center, E over (f, j) ascending"""
    dt = y.dtype
    B = len(pharm_ptr) - 1
    g0h, gy, E = torch.zeros_like(h0_hat), torch.zeros_like(y), torch.zeros(B, dtype=dt)
    if tg.restraints is None:
        return g0h, gy, E
    s = tg.sharp.to(dt)
    v = s * h0_hat
    mx = v.max(dim=1).values
    Z = torch.exp(v - mx[:, None]).sum(dim=1)
    p = torch.exp(v - mx[:, None]) / Z[:, None]
    lse = torch.log(Z) + mx
    for g, rows in enumerate(tg.restraints):
        f0, f1 = int(pharm_ptr[g]), int(pharm_ptr[g + 1])
        for f in range(f0, f1):
            for t, center, pt, r, w in rows:
                if center >= 0 and center != f - f0:
                    continue
                pt, r, w = pt.to(dt), r.to(dt), w.to(dt)
                CE = lse[f] - v[f, t]
                omega = torch.ones((), dtype=dt)
                if float(r) > 0:
                    d = y[f] - pt
                    rho2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                    r2 = r * r
                    q = torch.clamp(1.0 - rho2 / r2, min=0)
                    omega = q * q
                    if float(q) > 0:
                        gy[f] = gy[f] + ((w * CE) * (2.0 * q)) * ((-2.0 * d) / r2)
                wo = w * omega
                E[g] = E[g] + wo * CE
                onehot = torch.zeros_like(p[f])
                onehot[t] = 1.0
                g0h[f] = g0h[f] + (wo * s) * (p[f] - onehot)
    return g0h, gy, E


def comp_type_terms(fd, tg, batch, x0_hat, D, h0_hat):
    """(g0_h [Nf, nf], E_unmatched [B]) of the complementarity energy with a type gradient: m_t the field's hinge where S_t is
    non-empty in the graph, ``unmatched`` where it is empty (a graph without features: every type)"""
    dt = x0_hat.dtype
    B = batch.batch_size
    g0h, E_un = torch.zeros_like(h0_hat), torch.zeros(B, dtype=dt)
    w, kappa, s, u = fd.w_comp.to(dt), fd.kappa.to(dt), fd.sharp.to(dt), tg.unmatched.to(dt)
    nt = h0_hat.shape[1]
    for g in range(B):
        f0, f1 = int(batch.pharm_ptr[g]), int(batch.pharm_ptr[g + 1])
        if f1 == f0:
            continue
        j0, j1 = fd.ph_ptr[g], fd.ph_ptr[g + 1]
        y = x0_hat[f0:f1] + D[f0:f1]
        p = torch.softmax(s * h0_hat[f0:f1], dim=1)
        m2 = torch.zeros(f1 - f0, nt, dtype=dt)
        ut = fd.ph_type[j0:j1]
        d = y[:, None, :] - fd.ph_x[j0:j1].to(dt)[None]
        rho = F._rho(d)
        for t in range(nt):
            S = fd.match[t][ut] != 0
            if not bool(S.any()):
                m2[:, t] = u * u
                E_un[g] = E_un[g] + ((w * p[:, t]) * (u * u)).sum()
                continue
            rs = rho[:, S]
            mn = rs.min(dim=1).values
            Z = torch.exp(-(kappa * (rs - mn[:, None]))).sum(dim=1)
            m = torch.clamp((mn - torch.log(Z) / kappa) - fd.dist[t].to(dt), min=0)
            m2[:, t] = m * m
        mean = (p * m2).sum(dim=1)
        g0h[f0:f1] = ((w * s) * p) * (m2 - mean[:, None])
    return g0h, E_un


def dynamics_vjp2(sd, cfg, batch32, batch, prot_x, x_t, h_t, t):
    """(eps_h, eps_x, J) with J(u_x, u_h) = d(sum eps_x . u_x + sum eps_h . u_h) / d(x_t, h_t) on the edge set decided in fp32"""
    edges = O.build_dynamic_edges(cfg, batch32, prot_x.float(), x_t.float())
    x = x_t.detach().clone().requires_grad_(True)
    h = h_t.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        oh, ox = O.dynamics_forward(sd, cfg, batch, prot_x, x, h, t, edges=edges)

    def J(ux, uh):
        gx, gh = torch.autograd.grad((ox * ux).sum() + (oh * uh).sum(), (x, h), retain_graph=True, allow_unused=True)
        return (torch.zeros_like(x_t) if gx is None else gx.detach(), torch.zeros_like(h_t) if gh is None else gh.detach())
    return oh.detach(), ox.detach(), J


def types_reference(sd, cfg, batch, n_t, precision, noise, flags, pin_x, pin_h, init_pharm_com, restraints, field=None, types=None,
                    scale=1.0, clip=0.0, fnorm=1.0, ep=False, double=False, use_vjp=True, n_steps=None, use_field=True, use_types=True,
                    use_jh=True, zero_geps_h=False):
    """pocket_field_ref.field_reference's namespace plus E_type [n_steps, B] and g0_h / grad_h / shift_h [n_steps, Nf, nf]"""
    batch32 = batch
    dt = torch.float64 if double else torch.float32
    if double:
        sd, batch, noise = O.state_dict64(sd), O.batch64(batch), noise.double()
        pin_x, pin_h, init_pharm_com = pin_x.double(), pin_h.double(), init_pharm_com.double()
    rt = G.restraint_tensors(restraints, dt) if restraints is not None else [[] for _ in range(batch.batch_size)]
    fd = field if use_field else None
    tg = types if use_types else None
    guided = any(len(rs) for rs in rt) or fd is not None or tg is not None
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
    Ets, g0hs, gradhs, shifths = [], [], [], []
    order = list(reversed(range(n_t)))[:n_steps]
    for it, s in enumerate(order):
        nz = noise[1 + it]
        D = (c_init - O.segment_mean(prot_x, batch.prot_ptr))[bidx["pharm"]]          # before this step's shift
        t = coef["t"][s].expand(B).contiguous()
        t = t.double() if double else t
        if guided and tg is not None:
            pred_h, pred_x, J2 = dynamics_vjp2(sd, cfg, batch32, batch, prot_x, x_t, h_t, t)
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
            if tg is not None:                  # type guidance's lines
                g0_h, gy, E_type = type_restraint_terms(tg, batch.pharm_ptr, x0_hat + D, h0_hat)
                if tg.comp and fd is not None and fd.ph_ptr is not None and float(fd.w_comp) > 0 and fd.ph_ptr[-1] > 0:
                    gc_h, E_un = comp_type_terms(fd, tg, batch, x0_hat, D, h0_hat)
                    g0_h, E_type = g0_h + gc_h, E_type + E_un
                g0, E = g0 + gy, E + E_type
                phi_x = torch.ones((), dtype=dt) if ep else -(sg_t / al_t)
                phi_h = phi_x
                ge_h = torch.zeros_like(g0_h) if zero_geps_h else (phi_h / phi_x) * g0_h
                Jg, Jh = J2(g0, ge_h) if use_vjp else (torch.zeros_like(g0), torch.zeros_like(g0_h))
                if not use_jh:
                    Jh = torch.zeros_like(Jh)
                grad_h = phi_x * Jh if ep else g0_h / al_t + phi_x * Jh
                shift_h = (tg.scale.to(dt) * (sig * sig)) * grad_h
                if float(tg.clip) > 0:
                    nh = torch.sqrt((shift_h * shift_h).sum(dim=1))
                    over = nh > tg.clip.to(dt)
                    shift_h = torch.where(over[:, None], shift_h * (tg.clip.to(dt) / torch.where(over, nh, torch.ones_like(nh)))[:, None], shift_h)
                h_s = h_s - shift_h
                Ets.append(E_type); g0hs.append(g0_h); gradhs.append(grad_h); shifths.append(shift_h)
            else:
                Jg = J(g0) if use_vjp else torch.zeros_like(g0)
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
                           shift_h=stack(shifths, (0, Nf, nf)))


def final_type_energy(tg, batch, x0, h0, fnorm=1.0):
    """E [B] of the type restraints on final centers x0 (caller's frame) / features h0, fp64"""
    t64 = make_types(tg.raw, sharpness=float(tg.sharp))
    return type_restraint_terms(t64, batch.pharm_ptr, x0.double(), h0.double() / fnorm)[2]


# ---- the case of the GPU tests --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case():
    """pocket_field_ref.case() -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms with 3 / 8 / 5 / 1 / 6 centers, graph 1 with a
    type-pinned center, T = 24, live head, the field with 0 / 70 / 5 / 1 / 3 receptor features -- with type guidance:
      graph 0  no type restraint (and no receptor feature: no complementarity term either)
      graph 1  (center 0 is pinned in position and type, center 1 in position) a restraint without a window on every center: the
               pinned center's shift must be ignored, the free ones take theirs
      graph 2  a windowed restraint on every center, centred where the run without type guidance puts center 0 and asking for
               another type than that center ends with
      graph 3  (the single-center graph) a restraint without a window (r = 0) on center 0
      graph 4  none: complementarity with a type gradient only
    Returns pocket_field_ref.case()'s tuple with the type guidance appended."""
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    plain = F.reference()
    ptr = batch.pharm_ptr.tolist()
    nf = cfg.pharm_nf
    other = lambda f: int((plain.h0[f].argmax() + 2) % nf)
    tr = [None,
          [(other(ptr[1] + 3), None, (0.0, 0.0, 0.0), 0.0, 1.0)],
          [(other(ptr[2]), None, plain.x0[ptr[2]].tolist(), 6.0, 2.0)],
          [(other(ptr[3]), 0, (0.0, 0.0, 0.0), 0.0, 2.0)],
          None]
    tg = make_types(tr, scale=FEAT_SCALE, clip=0.0, sharpness=SHARP, complementarity=True, unmatched=UNMATCHED)
    return cfg, sd, k, batch, noise, pins, com, restraints, fd, tg


@functools.lru_cache(maxsize=None)
def reference(ep=False, double=False, use_types=True, use_jh=True, zero_geps_h=False):
    """the composition of the case, computed once per session and left unchanged"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = case()
    return types_reference(sd, cfg, batch, T, PREC, noise, *pins, com, restraints, fd, tg, scale=GUIDE_SCALE, ep=ep, double=double,
                           use_types=use_types, use_jh=use_jh, zero_geps_h=zero_geps_h)


@functools.lru_cache(maxsize=None)
def wide_case():
    """pocket_field_ref.wide_case() at (64, 32), T = 12, feat_norm 2, with type guidance: a windowless restraint on center 1 of
    graph 0 and a windowed one on every center of graph 1 (which has the type-pinned center 2); feat_scale 1"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.wide_case()
    pcom = O.segment_mean(batch.prot_x, batch.prot_ptr)
    tr = [[(2, 1, (0.0, 0.0, 0.0), 0.0, 1.0)], [(4, None, pcom[1].tolist(), 30.0, 1.0)]]
    tg = make_types(tr, scale=WIDE_FEAT_SCALE, sharpness=SHARP, complementarity=True, unmatched=UNMATCHED)
    return cfg, sd, k, batch, noise, pins, com, restraints, fd, tg


@functools.lru_cache(maxsize=None)
def wide_reference(use_types=True):
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = wide_case()
    return types_reference(sd, cfg, batch, G.WIDE_T, PREC, noise, *pins, com, restraints, fd, tg, scale=GUIDE_SCALE, fnorm=2.0,
                           use_types=use_types)
