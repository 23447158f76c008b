"""The reference of a guided run with a pocket field (pf_guide_field_next): guidance_ref.guided_reference with the field's lines
of include/pfdyn.h ("pocket field") inserted -- the clash energy of the predicted clean centers against the current protein rows
(sampler's frame), the complementarity energy against receptor features (caller's frame, type weights from the predicted clean
features as constants), their gradients added to the restraints' g0 in front of the VJP.  Without a field it is
guidance_ref.guided_reference bit for bit (asserted in test_pocket_field_host.py).

``double=True``: the same composition in fp64 on the fp32 inputs (guidance_ref's rules).  ``use_field=False`` drops the field and
keeps the restraints: what a library that ignored the arming would compute (the teeth of the GPU tests)."""
import functools
from types import SimpleNamespace

import torch

import guidance_ref as G
from oracle import pf_oracle as O

T, PREC, TOL, GUIDE_SCALE = G.T, G.PREC, G.TOL, G.GUIDE_SCALE
W_CLASH, W_COMP, KAPPA, SHARP = 1.0, 0.25, 4.0, 4.0
N_FEATURES = [0, 70, 5, 1, 3]
FEATURE_SEED = 7


def make_field(atom_r=None, w_clash=0.0, ph=None, match=None, dist=None, w_comp=0.0, kappa=4.0, type_sharpness=0.0):
    """A field as the library receives it: every value rounded to fp32.  The arguments are PfEngine.field_next's."""
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float32)
    return SimpleNamespace(atom_r=None if atom_r is None else f32(atom_r).reshape(-1), w_clash=f32(w_clash),
                           ph_ptr=None if ph is None else [int(v) for v in ph[0]],
                           ph_x=None if ph is None else f32(ph[1]).reshape(-1, 3),
                           ph_type=None if ph is None else torch.as_tensor(ph[2]).long().reshape(-1),
                           match=None if match is None else torch.as_tensor(match).long(),
                           dist=None if dist is None else f32(dist), w_comp=f32(w_comp), kappa=f32(kappa), sharp=f32(type_sharpness))


def field_kwargs(fd):
    """the dict PfEngine.sample(field=...) takes"""
    ph = None if fd.ph_ptr is None else (fd.ph_ptr, fd.ph_x, fd.ph_type)
    return dict(atom_r=fd.atom_r, w_clash=float(fd.w_clash), ph=ph, match=fd.match, dist=fd.dist, w_comp=float(fd.w_comp),
                kappa=float(fd.kappa), type_sharpness=float(fd.sharp))


def _rho(d):
    return torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def field_terms(fd, batch, prot_x, x0_hat, D, h0_hat):
    """(g_clash, g_comp [Nf, 3], E_clash, E_comp [B]) in x0_hat's dtype.  prot_x: the current protein rows (sampler's frame);
    D [Nf, 3]: the frame offset per center; h0_hat [Nf, pharm_nf]: the predicted clean features (no gradient flows through them)."""
    dt = x0_hat.dtype
    B = batch.batch_size
    g_cl, g_co = torch.zeros_like(x0_hat), torch.zeros_like(x0_hat)
    E_cl, E_co = torch.zeros(B, dtype=dt), torch.zeros(B, dtype=dt)
    one = torch.ones((), dtype=dt)
    for g in range(B):
        f0, f1 = int(batch.pharm_ptr[g]), int(batch.pharm_ptr[g + 1])
        p0, p1 = int(batch.prot_ptr[g]), int(batch.prot_ptr[g + 1])
        x = x0_hat[f0:f1]
        if fd.atom_r is not None and f1 > f0:
            w = fd.w_clash.to(dt)
            d = x[:, None, :] - prot_x[p0:p1][None]
            rho = _rho(d)
            m = torch.clamp(fd.atom_r[p0:p1].to(dt)[None] - rho, min=0)
            live = (rho > 0) & (m > 0)
            c = torch.where(live, ((2.0 * w) * m) / torch.where(live, rho, one), torch.zeros_like(rho))
            g_cl[f0:f1] = -(c[..., None] * d).sum(dim=1)
            E_cl[g] = (w * (m * m)).sum()
        if fd.ph_ptr is None or f1 == f0:
            continue
        j0, j1 = fd.ph_ptr[g], fd.ph_ptr[g + 1]
        if j1 == j0:
            continue
        w, kappa = fd.w_comp.to(dt), fd.kappa.to(dt)
        y = x + D[f0:f1]
        p = torch.softmax(fd.sharp.to(dt) * h0_hat[f0:f1].detach(), dim=1)
        u = fd.ph_type[j0:j1]
        d = y[:, None, :] - fd.ph_x[j0:j1].to(dt)[None]
        rho = _rho(d)
        for t in range(fd.match.shape[0]):
            S = fd.match[t][u] != 0
            if not bool(S.any()):
                continue
            rs, ds = rho[:, S], d[:, S]
            mn = rs.min(dim=1).values
            wj = torch.exp(-(kappa * (rs - mn[:, None])))
            Z = wj.sum(dim=1)
            soft = mn - torch.log(Z) / kappa
            m = torch.clamp(soft - fd.dist[t].to(dt), min=0)
            wp = w * p[:, t]
            E_co[g] = E_co[g] + (wp * (m * m)).sum()
            c = torch.where(rs > 0, wj / torch.where(rs > 0, rs, one), torch.zeros_like(rs))
            V = (c[..., None] * ds).sum(dim=1)
            g_co[f0:f1] = g_co[f0:f1] + ((wp * (2.0 * m)) / Z)[:, None] * V
    return g_cl, g_co, E_cl, E_co


def field_reference(sd, cfg, batch, n_t, precision, noise, flags, pin_x, pin_h, init_pharm_com, restraints, field=None, scale=1.0,
                    clip=0.0, fnorm=1.0, ep=False, double=False, use_vjp=True, n_steps=None, use_field=True):
    """guidance_ref.guided_reference's namespace plus E3 [n_steps, B, 3] (restraints, clash, complementarity)."""
    batch32 = batch
    dt = torch.float64 if double else torch.float32
    if double:
        sd, batch, noise = O.state_dict64(sd), O.batch64(batch), noise.double()
        pin_x, pin_h, init_pharm_com = pin_x.double(), pin_h.double(), init_pharm_com.double()
    rt = G.restraint_tensors(restraints, dt) if restraints is not None else [[] for _ in range(batch.batch_size)]
    fd = field if use_field else None
    guided = any(len(rs) for rs in rt) or fd is not None
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
    order = list(reversed(range(n_t)))[:n_steps]
    for it, s in enumerate(order):
        nz = noise[1 + it]
        D = (c_init - O.segment_mean(prot_x, batch.prot_ptr))[bidx["pharm"]]          # before this step's shift
        t = coef["t"][s].expand(B).contiguous()
        t = t.double() if double else t
        if guided:
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
            if fd is not None:                  # the pocket field's lines
                h0_hat = pred_h if ep else (h_t - sg_t * pred_h) / al_t
                g_cl, g_co, E_cl, E_co = field_terms(fd, batch, prot_x, x0_hat, D, h0_hat)
                E3s.append(torch.stack([E, E_cl, E_co], dim=1))
                g0, E = (g0 + g_cl) + g_co, (E + E_cl) + E_co
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
    Nf = x_t.shape[0]
    return SimpleNamespace(x0=x_0, h0=h_0, fx=torch.stack(fx), fh=torch.stack(fh), E=stack(Es, (0, B)), g0=stack(g0s, (0, Nf, 3)),
                           grad=stack(grads, (0, Nf, 3)), shift=stack(shifts, (0, Nf, 3)), E3=stack(E3s, (0, B, 3)))


def final_energies(fd, batch, x0, h0, fnorm=1.0):
    """(E_clash, E_comp [B], clashing pairs [B]) of final centers x0 / features h0 in the caller's frame, fp64: the field on the
    pocket as given (the distances are those of the sampler's frame)."""
    b64 = O.batch64(batch)
    x, h = x0.double(), h0.double() / fnorm
    _, _, E_cl, E_co = field_terms(fd, b64, b64.prot_x, x, torch.zeros_like(x), h)
    pairs = torch.zeros(batch.batch_size, dtype=torch.long)
    if fd.atom_r is not None:
        for g in range(batch.batch_size):
            f0, f1 = int(batch.pharm_ptr[g]), int(batch.pharm_ptr[g + 1])
            p0, p1 = int(batch.prot_ptr[g]), int(batch.prot_ptr[g + 1])
            rho = _rho(x[f0:f1, None, :] - b64.prot_x[p0:p1][None])
            pairs[g] = int((rho < fd.atom_r[p0:p1].double()[None]).sum())
    return E_cl, E_co, pairs


def synthetic_features(batch, counts, seed, nt, spread=4.0):
    """seeded receptor features around each pocket's centre, caller's frame: (ph_ptr, ph_x [n, 3], ph_type [n])"""
    gen = torch.Generator().manual_seed(seed)
    pcom = O.segment_mean(batch.prot_x, batch.prot_ptr)
    ptr, xs, ty = [0], [], []
    for g, n in enumerate(counts):
        xs.append(pcom[g][None] + spread * torch.randn(n, 3, generator=gen))
        ty.append(torch.randint(0, nt, (n,), generator=gen))
        ptr.append(ptr[-1] + n)
    return ptr, torch.cat(xs).float(), torch.cat(ty)


def tables():
    from pharmacoforge_amd import analysis
    return analysis.complementarity_tables()


@functools.lru_cache(maxsize=None)
def case(clash=True, comp=True):
    """guidance_ref.case() -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms with 3 / 8 / 5 / 1 / 6 centers, graph 1 with pins,
    T = 24, live head -- with a field: radii of 2.0 with every seventh atom inert, 0 / 70 / 5 / 1 / 3 receptor features (none; more
    than a wave; few; a single one, so that most types have an empty set there).  Only graph 2 keeps its restraints: there all
    three terms add.  Returns guidance_ref.case()'s tuple with the field appended."""
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    Np = int(batch.prot_ptr[-1])
    atom_r = torch.full((Np,), 2.0)
    atom_r[::7] = 0.0
    match, dist = tables()
    ph = synthetic_features(batch, N_FEATURES, FEATURE_SEED, cfg.pharm_nf)
    fd = make_field(atom_r=atom_r if clash else None, w_clash=W_CLASH if clash else 0.0, ph=ph if comp else None,
                    match=match if comp else None, dist=dist if comp else None, w_comp=W_COMP if comp else 0.0, kappa=KAPPA,
                    type_sharpness=SHARP)
    restraints = [None, None, restraints[2], None, None]
    return cfg, sd, k, batch, noise, pins, com, restraints, fd


@functools.lru_cache(maxsize=None)
def reference(ep=False, double=False, use_field=True, clash=True, comp=True, with_restraints=True):
    """the composition of the case, computed once per session and left unchanged"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd = case(clash, comp)
    return field_reference(sd, cfg, batch, T, PREC, noise, *pins, com, restraints if with_restraints else None, fd, scale=GUIDE_SCALE,
                           ep=ep, double=double, use_field=use_field)


@functools.lru_cache(maxsize=None)
def wide_case():
    """guidance_ref.wide_case() at (64, 32), T = 12, feat_norm 2, with a field: 0 / 9 features, every fifth atom inert"""
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    atom_r = torch.full((int(batch.prot_ptr[-1]),), 2.0)
    atom_r[::5] = 0.0
    match, dist = tables()
    fd = make_field(atom_r=atom_r, w_clash=W_CLASH, ph=synthetic_features(batch, [0, 9], FEATURE_SEED + 1, cfg.pharm_nf), match=match,
                    dist=dist, w_comp=W_COMP, kappa=KAPPA, type_sharpness=SHARP)
    return cfg, sd, k, batch, noise, pins, com, restraints, fd


@functools.lru_cache(maxsize=None)
def wide_reference(use_field=True):
    cfg, sd, k, batch, noise, pins, com, restraints, fd = wide_case()
    return field_reference(sd, cfg, batch, G.WIDE_T, PREC, noise, *pins, com, restraints, fd, scale=GUIDE_SCALE, fnorm=2.0,
                           use_field=use_field)


@functools.lru_cache(maxsize=None)
def tall_case():
    """one graph of 600 atoms, 64 centers and 130 receptor features: atoms beyond the rows a lane keeps, sixteen centers per wave,
    features beyond two waves.  T = 24; one step of it is what the GPU test reads back."""
    from helpers import sampler_live_head
    cfg = O.DynamicsConfig()
    batch = O.synthetic_batch([77], [600], [64], cfg)
    noise = torch.randn(2, 64, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(G.NOISE_SEED))
    sd, k = sampler_live_head(O.make_state_dict(cfg, 0), cfg, batch, T, PREC, noise)
    atom_r = torch.full((600,), 2.0)
    atom_r[::7] = 0.0
    match, dist = tables()
    fd = make_field(atom_r=atom_r, w_clash=W_CLASH, ph=synthetic_features(batch, [130], FEATURE_SEED + 2, cfg.pharm_nf, spread=6.0),
                    match=match, dist=dist, w_comp=W_COMP, kappa=KAPPA, type_sharpness=SHARP)
    pins = (torch.zeros(64, dtype=torch.int32), torch.zeros(64, 3), torch.zeros(64, cfg.pharm_nf))
    com = O.segment_mean(batch.prot_x, batch.prot_ptr) + 0.5
    return cfg, sd, k, batch, noise, pins, com, fd
