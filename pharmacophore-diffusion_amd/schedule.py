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


def pin_coefficients(gamma_table: torch.Tensor, timesteps: int) -> Dict[str, torch.Tensor]:
    """Noise level of z_s for all s at once (index = s), fp32 on the host: alpha_s = alpha(gamma(s / T)) and
    sigma_s = sigma(gamma(s / T)) -- what a pinned run noises its given centers with (pf_denoise_step_pinned)."""
    g = gamma_table.detach().float().cpu()
    s_int = torch.arange(timesteps)
    s = s_int.float() / timesteps
    g_s = g[torch.round(s * timesteps).long()]
    return {"alpha_s": alpha(g_s), "sigma_s": sigma(g_s)}


def guide_coefficients(gamma_table: torch.Tensor, timesteps: int) -> Dict[str, torch.Tensor]:
    """Noise level of z_t, t = s + 1, for all s at once (index = s), fp32 on the host: alpha_t = alpha(gamma((s + 1) / T)) and
    sigma_t = sigma(gamma((s + 1) / T)) -- what a guided step predicts the clean centers with, x0_hat = (x_t - sigma_t eps_x) /
    alpha_t (pf_denoise_step_guided, pf_guide_coef)."""
    g = gamma_table.detach().float().cpu()
    t = (torch.arange(timesteps) + 1).float() / timesteps
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
