"""Noise schedule and per-step scalar algebra of the diffusion wrapper (host logic, tiny B-length
vector work that the reference also does with torch ops): pharmacoforge/models/pharmacodiff.py
:140-160 (sigma, alpha, sigma_and_alpha_t_given_s), :387-420 (per-step terms), :582-668 (schedules)."""
from typing import Dict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def cosine_beta_schedule(timesteps, s=0.008, raise_to_power: float = 1):
    """pharmacodiff.py:582-599 (kept for API completeness; the model hard-wires 'polynomial_2')."""
    steps = timesteps + 2
    x = np.linspace(0, steps, steps)
    ac = np.cos(((x / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    ac = ac / ac[0]
    betas = np.clip(1 - (ac[1:] / ac[:-1]), a_min=0, a_max=0.999)
    ac = np.cumprod(1. - betas, axis=0)
    return np.power(ac, raise_to_power) if raise_to_power != 1 else ac


def clip_noise_schedule(alphas2, clip_value=0.001):
    """pharmacodiff.py:602-615: clip alpha_t / alpha_{t-1} for sampling stability."""
    a2 = np.concatenate([np.ones(1), alphas2], axis=0)
    step = np.clip(a2[1:] / a2[:-1], a_min=clip_value, a_max=1.)
    return np.cumprod(step, axis=0)


def polynomial_schedule(timesteps: int, s=1e-4, power=3.):
    """pharmacodiff.py:618-632: alpha^2 = (1 - (x/steps)^power)^2, clipped, then squeezed by s."""
    steps = timesteps + 1
    x = np.linspace(0, steps, steps)
    a2 = clip_noise_schedule((1 - np.power(x / steps, power)) ** 2, clip_value=0.001)
    return (1 - 2 * s) * a2 + s


class PredefinedNoiseSchedule(nn.Module):
    """Lookup table gamma[t] = -(log alpha_t^2 - log sigma_t^2)  (pharmacodiff.py:636-668)."""

    def __init__(self, noise_schedule, timesteps, precision):
        super().__init__()
        self.timesteps = timesteps
        if noise_schedule == 'cosine':
            alphas2 = cosine_beta_schedule(timesteps)
        elif 'polynomial' in noise_schedule:
            splits = noise_schedule.split('_')
            assert len(splits) == 2
            alphas2 = polynomial_schedule(timesteps, s=precision, power=float(splits[1]))
        else:
            raise ValueError(noise_schedule)
        sigmas2 = 1 - alphas2
        self.gamma = nn.Parameter(torch.from_numpy(-(np.log(alphas2) - np.log(sigmas2))).float(), requires_grad=False)

    def forward(self, t):
        return self.gamma[torch.round(t * self.timesteps).long()]


def sigma(gamma):
    return torch.sqrt(torch.sigmoid(gamma))


def alpha(gamma):
    return torch.sqrt(torch.sigmoid(-gamma))


def sigma_and_alpha_t_given_s(gamma_t, gamma_s):
    sigma2_t_given_s = -torch.expm1(F.softplus(gamma_s) - F.softplus(gamma_t))
    log_alpha2_t = F.logsigmoid(-gamma_t)
    log_alpha2_s = F.logsigmoid(-gamma_s)
    alpha_t_given_s = torch.exp(0.5 * (log_alpha2_t - log_alpha2_s))
    alpha_s = torch.exp(0.5 * log_alpha2_s)
    return sigma2_t_given_s, torch.sqrt(sigma2_t_given_s), alpha_t_given_s, alpha_s


def step_coefficients(gamma_table: torch.Tensor, timesteps: int) -> Dict[str, torch.Tensor]:
    """Everything sample_p_zs_given_zt derives from (s, t=s+1) for all s at once, in fp32 on the host,
    with the reference's op order (pharmacodiff.py:387-400, 413-420).  Index = s."""
    g = gamma_table.detach().float().cpu()
    s_int = torch.arange(timesteps)
    s = s_int.float() / timesteps
    t = (s_int + 1).float() / timesteps
    g_s = g[torch.round(s * timesteps).long()]
    g_t = g[torch.round(t * timesteps).long()]
    s2_ts, s_ts, a_ts, a_s = sigma_and_alpha_t_given_s(g_t, g_s)
    sig_s, sig_t = sigma(g_s), sigma(g_t)
    return {"t": t, "s": s, "alpha_t_given_s": a_ts, "var_terms": s2_ts / a_ts / sig_t, "sigma": s_ts * sig_s / sig_t,
            "ep_zt": a_ts * (sig_s ** 2) / (sig_t ** 2), "ep_pred": a_s * s2_ts / (sig_t ** 2)}


def pin_coefficients(gamma_table: torch.Tensor, timesteps: int, levels=None) -> Dict[str, torch.Tensor]:
    """Noise level of z_s for all s at once (index = s), fp32 on the host: alpha_s = alpha(gamma(s / T)) and
    sigma_s = sigma(gamma(s / T)) -- what a pinned run noises its given centers with (pf_denoise_step_pinned).
    levels (a plan, level_plan): the same table selected at the plan's steps -- index = step i, s = l_{i+1}."""
    g = gamma_table.detach().float().cpu()
    s_int = torch.arange(timesteps) if levels is None else torch.tensor(_plan_levels(timesteps, levels)[1:], dtype=torch.long)
    s = s_int.float() / timesteps
    g_s = g[torch.round(s * timesteps).long()]
    return {"alpha_s": alpha(g_s), "sigma_s": sigma(g_s)}


def guide_coefficients(gamma_table: torch.Tensor, timesteps: int, levels=None) -> Dict[str, torch.Tensor]:
    """Noise level of z_t, t = s + 1, for all s at once (index = s), fp32 on the host: alpha_t = alpha(gamma((s + 1) / T)) and
    sigma_t = sigma(gamma((s + 1) / T)) -- what a guided step predicts the clean centers with, x0_hat = (x_t - sigma_t eps_x) /
    alpha_t (pf_denoise_step_guided, pf_guide_coef).
    levels (a plan, level_plan): the same table selected at the plan's steps -- index = step i, t = l_i."""
    g = gamma_table.detach().float().cpu()
    t_int = torch.arange(timesteps) + 1 if levels is None else torch.tensor(_plan_levels(timesteps, levels)[:-1], dtype=torch.long)
    t = t_int.float() / timesteps
    g_t = g[torch.round(t * timesteps).long()]
    return {"alpha_t": alpha(g_t), "sigma_t": sigma(g_t)}


def seed_coefficients(gamma_table: torch.Tensor, timesteps: int, level: int) -> Dict[str, torch.Tensor]:
    """Noise level a = ``level`` of a seeded run's first state, fp32 on the host: alpha_a = alpha(gamma(a / T)) and sigma_a =
    sigma(gamma(a / T)) -- what a seeded begin noises the given pharmacophore with, z_a = alpha_a seed + sigma_a noise0
    (pf_sample_seed_next, pf_seed_coef).  The run then makes the steps s = a-1 .. 0."""
    level = int(level)
    if not 1 <= level <= timesteps:
        raise ValueError(f"a seed level must satisfy 1 <= level <= {timesteps}, got {level}")
    g = gamma_table.detach().float().cpu()
    a = torch.tensor(level).float() / timesteps
    g_a = g[torch.round(a * timesteps).long()]
    return {"alpha_a": alpha(g_a), "sigma_a": sigma(g_a)}


def resample_plan(timesteps: int, jump: int, resamples: int):
    """The op list of a pinned run with resampling jumps (include/pfdyn.h, "pinned runs with resampling jumps"): levels run
    T -> 0 in segments (a, b) of length ``jump`` (the last one possibly shorter); every segment is denoised, D(a-1) ... D(b), and
    then ``resamples`` - 1 times re-noised from b back up to a and denoised again.  Returns ("denoise", s) and
    ("renoise", b, a) tuples; resamples = 1 gives D(T-1) ... D(0)."""
    if jump < 1:
        raise ValueError(f"jump must be at least 1, got {jump}")
    if resamples < 1:
        raise ValueError(f"resamples must be at least 1, got {resamples}")
    plan, a = [], int(timesteps)
    while a > 0:
        b = max(a - int(jump), 0)
        down = [("denoise", s) for s in range(a - 1, b - 1, -1)]
        plan += down
        for _ in range(int(resamples) - 1):
            plan.append(("renoise", b, a))
            plan += down
        a = b
    return plan


def renoise_coefficients(gamma_table: torch.Tensor, timesteps: int, pairs) -> Dict[str, torch.Tensor]:
    """alpha_{a|b} and sigma_{a|b} of the forward jump from level b up to level a > b, for every (b, a) of ``pairs`` (index =
    position in pairs), fp32 on the host: sigma_and_alpha_t_given_s(gamma(a / T), gamma(b / T)) -- what pf_renoise_step moves the
    whole state with, z_a = alpha_{a|b} z_b + sigma_{a|b} noise."""
    g = gamma_table.detach().float().cpu()
    pairs = [(int(b), int(a)) for b, a in pairs]
    for b, a in pairs:
        if not 0 <= b < a <= timesteps:
            raise ValueError(f"a re-noise pair must satisfy 0 <= b < a <= {timesteps}, got ({b}, {a})")
    b_int = torch.tensor([p[0] for p in pairs], dtype=torch.long)
    a_int = torch.tensor([p[1] for p in pairs], dtype=torch.long)
    g_b = g[torch.round(b_int.float() / timesteps * timesteps).long()]
    g_a = g[torch.round(a_int.float() / timesteps * timesteps).long()]
    _, s_ab, a_ab, _ = sigma_and_alpha_t_given_s(g_a, g_b)
    return {"alpha_t_given_s": a_ab, "sigma_t_given_s": s_ab}


def score_levels(timesteps: int, n=None):
    """The noise levels a scoring call visits (PharmacophoreDiff.score, pf_score): every level 1 .. T without ``n``; with it, n
    levels stratified evenly over 1 .. T -- level i lies in the i-th of n equal parts of (0, T]: its middle rounded up, or the
    part's last integer where that falls outside --, deterministic, ascending, without repeats; n = T gives every level."""
    T = int(timesteps)
    if T < 1:
        raise ValueError(f"score_levels: timesteps must be at least 1, got {timesteps}")
    if n is None:
        return list(range(1, T + 1))
    n = int(n)
    if not 1 <= n <= T:
        raise ValueError(f"score_levels: n must satisfy 1 <= n <= {T}, got {n}")
    return [min(-((-(2 * i + 1) * T) // (2 * n)), ((i + 1) * T) // n) for i in range(n)]


def score_weights(gamma_table: torch.Tensor, timesteps: int, levels, kind: str = "uniform", ep_coord: bool = False, ep_feat: bool = False):
    """(w_pos, w_feat): the weight of every level's position and feature term in a score, fp32 arrays of len(levels), computed in
    float64 from the gamma table.
    'uniform': 1 / len(levels) -- the score estimates the per-graph training loss (sum over centers, mean over levels); valid for
    all four parameterisations.
    'vlb': the diffusion terms of the variational bound times T / len(levels), so that a subset of the levels estimates the full
    sum.  With s = t - 1: 0.5 * expm1(gamma_t - gamma_s) for a noise-parameterised output (0.5 * (SNR(s) / SNR(t) - 1) on the noise
    error), 0.5 * (exp(-gamma_s) - exp(-gamma_t)) for the endpoint coordinate output (0.5 * (SNR(s) - SNR(t)) on the error of the
    predicted clean center).  A cross-entropy has no such weight (ep_feat) and level 0 has no s: ValueError."""
    lv = np.asarray([int(t) for t in levels], dtype=np.int64)
    if lv.size == 0:
        raise ValueError("score_weights: at least one level")
    T = int(timesteps)
    if lv.min() < 0 or lv.max() > T:
        raise ValueError(f"score_weights: levels must lie in 0..{T}")
    if kind == "uniform":
        w = np.full(lv.size, 1.0 / lv.size, dtype=np.float64)
        return w.astype(np.float32), w.astype(np.float32)
    if kind != "vlb":
        raise ValueError(f"score_weights: kind must be 'uniform' or 'vlb', got {kind!r}")
    if ep_feat:
        raise ValueError("score_weights: 'vlb' has no weight for an endpoint feature output (a cross-entropy); use 'uniform'")
    if lv.min() < 1:
        raise ValueError("score_weights: 'vlb' weights need levels >= 1 (level 0 has no s = t - 1)")
    g = gamma_table.detach().cpu().double().numpy()
    g_t, g_s = g[lv], g[lv - 1]
    scale = float(T) / lv.size
    noise = 0.5 * np.expm1(g_t - g_s) * scale
    w_pos = 0.5 * (np.exp(-g_s) - np.exp(-g_t)) * scale if ep_coord else noise
    return w_pos.astype(np.float32), noise.astype(np.float32)


# ---- few-step sampling: a plan of levels, first-order coefficients for any pair of levels, second-order multistep coefficients ----
def _plan_levels(timesteps: int, levels):
    """``levels`` as a list of ints, checked: timesteps >= l_0 > l_1 > ... > l_N >= 0 with N >= 1."""
    lv = [int(l) for l in levels]
    if len(lv) < 2:
        raise ValueError("a plan has at least two levels")
    if lv[0] > int(timesteps) or lv[-1] < 0 or any(a <= b for a, b in zip(lv[:-1], lv[1:])):
        raise ValueError(f"a plan's levels must descend strictly inside {int(timesteps)}..0, got {lv}")
    return lv


def level_plan(timesteps: int, n_steps: int, spacing: str = "uniform", top=None, gamma_table=None):
    """The levels a few-step run visits: integers top = l_0 > l_1 > ... > l_N = 0 with N = n_steps; step i goes from l_i to l_{i+1}.
    top defaults to T (a seeded run passes its seed level).  spacing: 'uniform' in the level index; 'quadratic', l = top (1 - i/N)^2,
    denser near 0; 'logsnr', uniform in lambda = -gamma / 2 between the two ends (needs gamma_table), each target taken to the level
    whose lambda is nearest.  Rounding collisions are resolved the same way every time: one pass down from l_0 (no level at or above
    its predecessor), one pass up from l_N = 0 (no level at or below its successor); 1 <= N <= top leaves room for both.  N = top
    gives every level."""
    T = int(timesteps)
    top = T if top is None else int(top)
    if not 1 <= top <= T:
        raise ValueError(f"level_plan: top must satisfy 1 <= top <= {T}, got {top}")
    N = int(n_steps)
    if not 1 <= N <= top:
        raise ValueError(f"level_plan: n_steps must satisfy 1 <= n_steps <= {top}, got {n_steps}")
    u = np.arange(N + 1, dtype=np.float64) / N
    if spacing == "uniform":
        lv = np.rint(top * (1.0 - u))
    elif spacing == "quadratic":
        lv = np.rint(top * (1.0 - u) ** 2)
    elif spacing == "logsnr":
        if gamma_table is None:
            raise ValueError("level_plan: spacing 'logsnr' needs gamma_table")
        lam = -0.5 * gamma_table.detach().cpu().double().numpy()[:top + 1]
        target = lam[top] + (lam[0] - lam[top]) * u
        lv = np.array([int(np.argmin(np.abs(lam - x))) for x in target], dtype=np.float64)   # (the first of equals: the lowest level)
    else:
        raise ValueError(f"level_plan: spacing must be 'uniform', 'quadratic' or 'logsnr', got {spacing!r}")
    lv = [int(x) for x in lv]
    lv[0], lv[-1] = top, 0
    for i in range(1, N):
        lv[i] = min(lv[i], lv[i - 1] - 1)
    for i in range(N - 1, 0, -1):
        lv[i] = max(lv[i], lv[i + 1] + 1)
    return lv


def strided_coefficients(gamma_table: torch.Tensor, timesteps: int, levels, eta: float = 1.0) -> Dict[str, torch.Tensor]:
    """The fields of step_coefficients for the steps of a plan: entry i is the pair (s, t) = (l_{i+1}, l_i), t = l_i / T.
    eta = 1: the reference's posterior evaluated at (s, t) (pharmacodiff.py:387-420 with a general s), fp32 in its op order -- a
    unit-stride plan gives step_coefficients' arrays bit for bit.  0 <= eta < 1: the DDIM family on the SAME struct, float64 cast to
    fp32: with s_eta = eta sigma_{t|s} sigma_s / sigma_t and k = sqrt(sigma_s^2 - s_eta^2), alpha_t_given_s = alpha_t / alpha_s,
    var_terms = sigma_t / alpha_{t|s} - k, sigma = s_eta, ep_zt = k / sigma_t, ep_pred = alpha_s - k alpha_t / sigma_t (at eta = 1
    these are the posterior's expressions)."""
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"strided_coefficients: eta must lie in [0, 1], got {eta}")
    lv = _plan_levels(timesteps, levels)
    g = gamma_table.detach().float().cpu()
    s_int, t_int = torch.tensor(lv[1:], dtype=torch.long), torch.tensor(lv[:-1], dtype=torch.long)
    s = s_int.float() / timesteps
    t = t_int.float() / timesteps
    if eta == 1.0:
        # torch's vectorised kernels may round an element differently in a vector's body and in its scalar tail (softplus does), so
        # "the same expression" is bit for bit the same only at the same position of a tensor of the same length: every pair is
        # evaluated at position s of step_coefficients' own T-long tensors, with t = s + 1 wherever the plan does not say otherwise
        t_of = torch.arange(timesteps) + 1
        t_of[s_int] = t_int
        t_all = t_of.float() / timesteps
        g_s = g[torch.round(torch.arange(timesteps).float() / timesteps * timesteps).long()]
        g_t = g[torch.round(t_all * timesteps).long()]
        s2_ts, s_ts, a_ts, a_s = sigma_and_alpha_t_given_s(g_t, g_s)
        sig_s, sig_t = sigma(g_s), sigma(g_t)
        full = {"alpha_t_given_s": a_ts, "var_terms": s2_ts / a_ts / sig_t, "sigma": s_ts * sig_s / sig_t,
                "ep_zt": a_ts * (sig_s ** 2) / (sig_t ** 2), "ep_pred": a_s * s2_ts / (sig_t ** 2)}
        out = {name: v[s_int] for name, v in full.items()}
        out.update(t=t, s=s)
        return out
    g_s, g_t = g[torch.round(s * timesteps).long()].double(), g[torch.round(t * timesteps).long()].double()
    _, s_ts, a_ts, a_s = sigma_and_alpha_t_given_s(g_t, g_s)
    sig_s, sig_t, a_t = sigma(g_s), sigma(g_t), alpha(g_t)
    s_eta = eta * s_ts * sig_s / sig_t
    k = torch.sqrt(sig_s ** 2 - s_eta ** 2)
    out = {"alpha_t_given_s": a_t / a_s, "var_terms": sig_t / a_ts - k, "sigma": s_eta, "ep_zt": k / sig_t, "ep_pred": a_s - k * a_t / sig_t}
    out = {name: v.float() for name, v in out.items()}
    out.update(t=t, s=s)
    return out


def multistep_coefficients(gamma_table: torch.Tensor, timesteps: int, levels, ep_coord: bool = False, ep_feat: bool = False) -> Dict[str, torch.Tensor]:
    """Per step i of a plan (t = l_i, s = l_{i+1}, prev = l_{i-1}) and per block -- x: coordinates, h: features -- the triple of the
    linear move z_s = cz z_t + c0 o_t + c1 o_prev (pf_ms_coef), o the network's output for the block as it is.  With lambda =
    -gamma / 2, h = lambda_s - lambda_t, r = (lambda_t - lambda_prev) / h:
      noise block:                       cz = alpha_s / alpha_t, c0 = -sigma_s expm1(h) (1 + 1/(2r)),  c1 = sigma_s expm1(h) / (2r)
      endpoint block (DPM-Solver++ 2M):  cz = sigma_s / sigma_t, c0 = -alpha_s expm1(-h) (1 + 1/(2r)), c1 = alpha_s expm1(-h) / (2r)
    The first step (no history) and the last (to level 0) are first-order: the 1/(2r) terms dropped, c1 = 0 exactly.  float64 cast
    to fp32; all solver knowledge is here, the device knows the linear form only."""
    lv = _plan_levels(timesteps, levels)
    n = len(lv) - 1
    g = gamma_table.detach().float().cpu().double()[torch.tensor(lv, dtype=torch.long)]
    lam, al, sg = -0.5 * g, alpha(g), sigma(g)
    h = lam[1:] - lam[:-1]
    inv2r = torch.zeros(n, dtype=torch.float64)
    for i in range(1, n - 1):
        inv2r[i] = 0.5 * float(h[i]) / float(lam[i] - lam[i - 1])
    a_t, a_s, s_t, s_s = al[:-1], al[1:], sg[:-1], sg[1:]
    eps_blk = (a_s / a_t, -s_s * torch.expm1(h) * (1.0 + inv2r), s_s * torch.expm1(h) * inv2r)
    end_blk = (s_s / s_t, -a_s * torch.expm1(-h) * (1.0 + inv2r), a_s * torch.expm1(-h) * inv2r)
    out = {"t": torch.tensor(lv[:-1], dtype=torch.long).float() / timesteps}
    for blk, ep in (("x", ep_coord), ("h", ep_feat)):
        for name, v in zip(("cz", "c0", "c1"), end_blk if ep else eps_blk):
            out[f"{name}_{blk}"] = (v + 0.0).float()          # (+ 0.0: a dropped term is +0, never -0)
    return out
