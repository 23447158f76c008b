"""The reference of a guided run (pf_sample_guided / pf_denoise_step_guided): resample_ref.resampled_reference's denoise branch
with the lines of include/pfdyn.h ("guided sampling") inserted -- restraint energies on the predicted clean centers in the
caller's frame, their gradient pulled back to x_t through the dynamics by the oracle's autograd on the edge set decided in fp32
(input_grad_ref.oracle_input_gradients' rule), the shift of the posterior mean and its clip -- in front of the pin selects and the
COM removal.  With no restraints it is test_gpu_pinned.pinned_reference bit for bit (asserted in test_guidance_host.py).

``double=True`` evaluates the same composition in fp64 on the fp32 weights, batch, noise, pins and restraints (resample_ref's
rules: the fp32 coefficient tables promote, every step's edges are decided in fp32 on the rounded coordinates).
``use_vjp=False`` drops the J(g0) term: what a kernel that forgot the VJP would compute (the teeth of the GPU tests)."""
import functools
from types import SimpleNamespace

import torch

from oracle import pf_oracle as O

T, PREC = 24, 0.25
NOISE_SEED = 42
GUIDE_SCALE = 4.0
TOL = 5e-3                       # the project's trajectory tolerance


def restraint_terms(kind, p, r, w, y):
    """(E [n], dE/dy [n, 3]) of one restraint on the rows y [n, 3]; p [3], r, w: tensors of y's dtype.  The operation order of
    pf_restraint (pf_kernels.hip)."""
    d = y - p
    rho = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    m = torch.clamp(r - rho if kind else rho - r, min=0)
    c = torch.where(rho > 0, ((2.0 * w) * m) / torch.where(rho > 0, rho, torch.ones_like(rho)), torch.zeros_like(rho))
    if kind:
        c = -c
    return w * (m * m), c[:, None] * d


def restraint_tensors(restraints, dtype):
    """per graph [(kind, center or -1, p, r, w)] with the values rounded to fp32 (what the library receives), then in ``dtype``"""
    out = []
    for rs in restraints:
        out.append([(1 if k in ("repel", 1) else 0, -1 if c is None or c == "*" else int(c),
                     torch.tensor([float(v) for v in p], dtype=torch.float32).to(dtype),
                     torch.tensor(float(r), dtype=torch.float32).to(dtype), torch.tensor(float(w), dtype=torch.float32).to(dtype))
                    for k, c, p, r, w in (rs or [])])
    return out


def energy_and_g0(rt, pharm_ptr, y):
    """g0 [Nf, 3] (per center: the restraints that apply, j ascending) and E [B] (f ascending, j ascending), in y's dtype"""
    g0, E = torch.zeros_like(y), torch.zeros(len(rt), dtype=y.dtype)
    for g, rs in enumerate(rt):
        f0, f1 = int(pharm_ptr[g]), int(pharm_ptr[g + 1])
        terms = []
        for kind, center, p, r, w in rs:
            rows = slice(f0, f1) if center < 0 else slice(f0 + center, f0 + center + 1)
            e, dy = restraint_terms(kind, p, r, w, y[rows])
            g0[rows] = g0[rows] + dy
            full = torch.full((f1 - f0,), float("nan"), dtype=y.dtype)
            full[rows.start - f0:rows.stop - f0] = e
            terms.append(full)
        acc = torch.zeros((), dtype=y.dtype)
        for f in range(f1 - f0):
            for full in terms:
                if not torch.isnan(full[f]):
                    acc = acc + full[f]
        E[g] = acc
    return g0, E


def dynamics_vjp(sd, cfg, batch32, batch, prot_x, x_t, h_t, t):
    """(eps_h, eps_x, J) with J(u) = d(sum eps_x . u)/d x_t on the edge set decided in fp32"""
    edges = O.build_dynamic_edges(cfg, batch32, prot_x.float(), x_t.float())
    x = x_t.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        oh, ox = O.dynamics_forward(sd, cfg, batch, prot_x, x, h_t, t, edges=edges)

    def J(u):
        (gx,) = torch.autograd.grad((ox * u).sum(), x, retain_graph=True, allow_unused=True)
        return torch.zeros_like(x_t) if gx is None else gx.detach()
    return oh.detach(), ox.detach(), J


def guided_reference(sd, cfg, batch, n_t, precision, noise, flags, pin_x, pin_h, init_pharm_com, restraints, scale=1.0, clip=0.0,
                     fnorm=1.0, ep=False, double=False, use_vjp=True, n_steps=None):
    """Returns a namespace: x0, h0, fx / fh (frames [n_steps + 1]), E [n_steps, B], and per step g0 / grad / shift [n_steps, Nf, 3]."""
    batch32 = batch
    dt = torch.float64 if double else torch.float32
    if double:
        sd, batch, noise = O.state_dict64(sd), O.batch64(batch), noise.double()
        pin_x, pin_h, init_pharm_com = pin_x.double(), pin_h.double(), init_pharm_com.double()
    rt = restraint_tensors(restraints, dt) if restraints is not None else [[] for _ in range(batch.batch_size)]
    guided = any(len(rs) for rs in rt)
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
    fx, fh, Es, g0s, grads, shifts = [a], [b], [], [], [], []
    order = list(reversed(range(n_t)))[:n_steps]
    for it, s in enumerate(order):
        nz = noise[1 + it]
        D = (c_init - O.segment_mean(prot_x, batch.prot_ptr))[bidx["pharm"]]          # before this step's shift
        t = coef["t"][s].expand(B).contiguous()
        t = t.double() if double else t
        if guided:
            pred_h, pred_x, J = dynamics_vjp(sd, cfg, batch32, batch, prot_x, x_t, h_t, t)
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
            g0, E = energy_and_g0(rt, batch.pharm_ptr, x0_hat + D)
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
                           grad=stack(grads, (0, Nf, 3)), shift=stack(shifts, (0, Nf, 3)))


def final_energy(restraints, batch, x0):
    """E [B] of the restraints on final centers x0 (caller's frame), fp64"""
    return energy_and_g0(restraint_tensors(restraints, torch.float64), batch.pharm_ptr, x0.double())[1]


# ---- the case of the GPU tests --------------------------------------------------------------------------------------------
#        graph 0: free | graph 1: center 0 both, 1 position, the rest free | graph 2: free | graph 3: free | graph 4: free
FLAGS = [0, 0, 0] + [3, 1, 0, 0, 0, 0, 0, 0] + [0] * 5 + [0] + [0] * 6


@functools.lru_cache(maxsize=None)
def case():
    """The five ragged pockets of resample_ref.case() (48 / 300 / 40 / 64 / 32 atoms, 3 / 8 / 5 / 1 / 6 centers), T = 24 at precision
    0.25, the scaled head of helpers.sampler_live_head.  Restraints (caller's frame):
      graph 0  none
      graph 1  (a pinned center next to restraints) an attract on center 5 with r = 0, and a repel sphere on all centers far from
               everything: its hinge never opens, it contributes exact zeros
      graph 2  an attract on center 1 plus a repel sphere around the pocket's COM on all centers
      graph 3  (the single-center graph) an attract
      graph 4  a repel sphere on all centers, placed where the unguided run puts center 0
    Returns (cfg, sd_live, k, batch, noise, pins, com, restraints)."""
    from helpers import sampler_live_head
    from test_gpu_pinned import pins_for
    cfg = O.DynamicsConfig()
    batch = O.synthetic_batch([31, 32, 33, 34, 35], [48, 300, 40, 64, 32], [3, 8, 5, 1, 6], cfg)
    Nf = int(batch.pharm_ptr[-1])
    assert Nf == 23 and len(FLAGS) == Nf
    noise = torch.randn(T + 1, Nf, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(NOISE_SEED))
    sd, k = sampler_live_head(O.make_state_dict(cfg, 0), cfg, batch, T, PREC, noise)
    pins = pins_for(batch, cfg, FLAGS)
    pcom = O.segment_mean(batch.prot_x, batch.prot_ptr)
    com = pcom + 0.5
    plain = guided_reference(sd, cfg, batch, T, PREC, noise, *pins, com, None)
    ptr = batch.pharm_ptr.tolist()
    off = lambda g, v: (pcom[g] + torch.tensor(v)).tolist()
    restraints = [
        None,
        [("attract", 5, off(1, [2.0, -1.0, 1.5]), 0.0, 1.0), ("repel", None, off(1, [60.0, 60.0, 60.0]), 3.0, 2.0)],
        [("attract", 1, off(2, [-2.5, 1.0, 2.0]), 1.5, 1.0), ("repel", None, off(2, [0.0, 0.0, 0.0]), 3.0, 1.0)],
        [("attract", 0, off(3, [3.0, 2.0, -2.0]), 1.0, 1.0)],
        [("repel", None, plain.x0[ptr[4]].tolist(), 2.5, 1.0)],
    ]
    return cfg, sd, k, batch, noise, pins, com, restraints


@functools.lru_cache(maxsize=None)
def reference(ep=False, double=False, guided=True, use_vjp=True):
    """the composition of the case, computed once per session and left unchanged"""
    cfg, sd, k, batch, noise, pins, com, restraints = case()
    return guided_reference(sd, cfg, batch, T, PREC, noise, *pins, com, restraints if guided else None, scale=GUIDE_SCALE, ep=ep,
                            double=double, use_vjp=use_vjp)


WIDE_T = 12


@functools.lru_cache(maxsize=None)
def wide_case():
    """the smaller leg at (64, 32): two pockets of 40 / 56 atoms with 3 / 5 centers, T = 12, one pinned center, feat_norm 2"""
    from helpers import sampler_live_head
    from test_gpu_pinned import pins_for
    cfg = O.DynamicsConfig(n_hidden_scalars=64, vector_size=32)
    batch = O.synthetic_batch([0, 1], [40, 56], [3, 5], cfg)
    noise = torch.randn(WIDE_T + 1, 8, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(NOISE_SEED))
    sd, k = sampler_live_head(O.make_state_dict(cfg, 0), cfg, batch, WIDE_T, PREC, noise)
    pins = pins_for(batch, cfg, [3, 0, 0] + [0, 0, 3, 0, 0])
    pcom = O.segment_mean(batch.prot_x, batch.prot_ptr)
    com = pcom + 0.5
    restraints = [[("repel", None, pcom[0].tolist(), 3.0, 1.0)],
                  [("attract", 1, (pcom[1] + torch.tensor([2.0, 2.0, -1.0])).tolist(), 1.0, 1.0)]]
    return cfg, sd, k, batch, noise, pins, com, restraints


@functools.lru_cache(maxsize=None)
def wide_reference(double=False):
    cfg, sd, k, batch, noise, pins, com, restraints = wide_case()
    return guided_reference(sd, cfg, batch, WIDE_T, PREC, noise, *pins, com, restraints, scale=GUIDE_SCALE, fnorm=2.0, double=double)
