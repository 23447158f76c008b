#!/usr/bin/env python3
"""tests/golden/traj_live_c1_T500.npz: the bounded T = 500 trajectory with a LIVE noise head, evaluated in fp64.

With the suite's seeded random weights eps_x is ~4e-5, so the eps_x term of the sampler update moves a trajectory by less
than its tolerances.  The last GVP of the noise head has identity vector gating, so eps_x is linear in that GVP's Wu:
multiplying it by 2**k scales eps_x by 2**k exactly (helpers.live_head).  This script runs the oracle -- nothing from the
reference tree -- on the batch, schedule precision, weight seed and noise (fair_noise: all but a few steps' draws) of traj_c1_T500_bounded.npz with
such a head:
once in fp64 (every step's edges decided in fp32 on the rounded coordinates: the fixture) and once in fp32 (whose worst
deviation from the fp64 frames is the rounding noise an fp32 implementation is granted: e32_pos, e32_feat).

It asserts, on the reference alone, what makes the comparison fair: the centers stay inside the pocket at every step, every
ordered pair of centers is an ff edge over the last 100 steps, and at every step no edge decision is within 1e-3 (relative,
in d^2) of flipping -- the k-th and (k+1)-th pf neighbour of every center, every ff pair against the cutoff -- so no fp32
implementation can legitimately build another edge set.

    python tests/golden/make_golden_live.py          # writes the fixture next to this file
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))            # tests/ (helpers)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import pf_oracle as O                    # noqa: E402
from helpers import batch_from, load, sampler_live_head      # noqa: E402

SOURCE, NAME = "traj_c1_T500_bounded.npz", "traj_live_c1_T500.npz"
MARGIN = 1e-3


def setup():
    """(z, cfg, batch, sd_live, k, T, precision): k from the oracle's eps_x of the trajectory's first dynamics call."""
    z = load(SOURCE)
    cfg = O.DynamicsConfig()
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    T, prec = int(z["T"]), float(z["precision"])
    sd_live, k = sampler_live_head(sd, cfg, batch, T, prec, z["noise"])
    return z, cfg, batch, sd_live, k, T, prec


def run(sd, cfg, batch, T, prec, noise, n_steps=None, double=True):
    """(pos_frames, feat_frames, x0, h0) of the oracle's sampler, stacked."""
    f = O.sample_given_receptor64 if double else O.sample_given_receptor
    x0, h0, frames = f(sd, cfg, batch, T, prec, noise, return_traj=True, n_steps=n_steps)
    return torch.stack([p for p, _ in frames]), torch.stack([h for _, h in frames]), x0, h0


def check_fair(cfg, batch, pos, tail=True):
    """The conditions of the module docstring on the frames ``pos`` [n, Nf, 3] (the caller's frame: the pocket's own)."""
    assert batch.batch_size == 1
    n_prot = int(batch.prot_ptr[-1])
    com = batch.prot_x.double().mean(dim=0)
    radius = (3.0 * n_prot / (4.0 * math.pi * 0.05)) ** (1.0 / 3.0)           # O.synthetic_pocket's ball
    far = float((pos - com).norm(dim=-1).max())
    assert far < radius, (far, radius)
    if tail:
        assert float(torch.cdist(pos[-100:], pos[-100:]).max()) < cfg.cutoff_ff
    d2 = (pos[:, :, None, :] - batch.prot_x.double()[None, None]).square().sum(-1)          # [n, Nf, Np]
    srt = d2.sort(dim=-1).values
    pf_gap = float(((srt[..., cfg.pf_k] - srt[..., cfg.pf_k - 1]) / srt[..., cfg.pf_k]).min())
    assert pf_gap > MARGIN, pf_gap
    nf = pos.shape[1]
    ff = (pos[:, :, None, :] - pos[:, None, :, :]).square().sum(-1)[:, ~torch.eye(nf, dtype=torch.bool)]
    ff_gap = float((ff / cfg.cutoff_ff ** 2 - 1.0).abs().min())
    assert ff_gap > MARGIN, ff_gap
    return far, pf_gap, ff_gap


def fair_noise(z, cfg, batch, sd_live, T, prec):
    """The noise of the fixture: the reference's recorded draw of every step where the frame it leads to meets check_fair's
    margins, otherwise the first redraw that does (torch's generator seeded with 1000 * step + attempt) -- over 501 frames
    of 4 centers some edge decision of a wholly random draw always comes within 1e-3 of flipping.  Steps the fp64 sampler by
    hand (O.sample_step, as O.sample_given_receptor does); returns (noise [T + 1, Nf, 9] fp32, steps redrawn)."""
    sd64, b64 = O.state_dict64(sd_live), O.batch64(batch)
    coef = O.step_coefficients(O.gamma_table(T, prec), T)
    com0 = O.segment_mean(b64.prot_x, b64.prot_ptr)

    def fair(px, xt):
        try:
            check_fair(cfg, batch, (xt + (com0 - O.segment_mean(px, b64.prot_ptr)))[None], tail=False)
            return True
        except AssertionError:
            return False

    noise = z["noise"].clone()
    prot_x = b64.prot_x - com0
    redrawn = []
    assert fair(prot_x, noise[0][:, :3].double())
    x_t, h_t = noise[0][:, :3].double(), noise[0][:, 3:].double()
    for it, s in enumerate(reversed(range(T))):
        for attempt in range(100):
            nz = noise[1 + it] if attempt == 0 else torch.randn(noise[0].shape, generator=torch.Generator().manual_seed(1000 * it + attempt))
            px, xs, hs = O.sample_step(sd64, cfg, b64, coef, s, prot_x, x_t, h_t, nz[:, :3].double(), nz[:, 3:].double())
            if fair(px, xs):
                break
        else:
            raise SystemExit(f"step {it}: no fair draw")
        if attempt:
            noise[1 + it] = nz
            redrawn.append(it)
        prot_x, x_t, h_t = px, xs, hs
    return noise, redrawn


def main():
    torch.set_num_threads(1)
    z, cfg, batch, sd_live, k, T, prec = setup()
    noise, redrawn = fair_noise(z, cfg, batch, sd_live, T, prec)
    pos, feat, x0, h0 = run(sd_live, cfg, batch, T, prec, noise)
    far, pf_gap, ff_gap = check_fair(cfg, batch, pos)
    p32, f32, x32, h32 = run(sd_live, cfg, batch, T, prec, noise, double=False)
    e32_pos, e32_feat = float((p32.double() - pos).abs().max()), float((f32.double() - feat).abs().max())
    bx0, _ = O.sample_given_receptor(O.make_state_dict(cfg, int(z["wseed"])), cfg, batch, T, prec, noise)
    moved = float((x0 - bx0.double()).abs().max())       # against the recorded head on the same noise
    assert moved > 0.5, moved                            # the eps_x term decides the result
    np.savez_compressed(os.path.join(HERE, NAME), k=np.int64(k), T=np.int64(T), precision=np.float64(prec),
                        wseed=np.int64(int(z["wseed"])), redrawn_steps=np.array(redrawn, dtype=np.int64), noise=noise.numpy(), x0_recorded_head=bx0.numpy(),
                        pos_frames=pos.numpy(), feat_frames=feat.numpy(), x0=x0.numpy(), h0=h0.numpy(),
                        e32_pos=np.float64(e32_pos), e32_feat=np.float64(e32_feat))
    print(f"{NAME}: k {k}, {len(redrawn)} steps redrawn, farthest center {far:.2f} A, pf margin {pf_gap:.2e}, ff margin {ff_gap:.2e}, "
          f"e32_pos {e32_pos:.2e}, e32_feat {e32_feat:.2e}, x0 moved {moved:.2f} A, "
          f"x0 fp32 - fp64 {float((x32.double() - x0).abs().max()):.2e}, h0 {float((h32.double() - h0).abs().max()):.2e}")


if __name__ == "__main__":
    main()
