"""The edge shapes of the sampler's move kernels (csrc/pf_stepmove.h), shared by test_gpu_step_moves.py and test_step_moves_host.py.

One batch of four graphs with 300 / 70 / 33 / 48 atoms and 64 / 1 / 17 / 2 centers: PF_MAXF = 64 centers fill every lane of the
wave that owns a graph's centers; 300 atoms take the frame offset's stride-64 loop four times and the COM removal's stride-256 loop
once; 70 atoms take the stride-64 loop once and no stride-256 pass; 33 and 48 atoms none; one center is the COM of itself.  Set up
as test_gpu_feature_counts.kind_case sets its batch up: flags [3, 1, 2, 0, ...] per graph, test_gpu_pinned.pins_for, COM + 0.5, the
live head of the run's first dynamics call, T = 24 at precision 0.25, noise seed resample_ref.NOISE_SEED.

Kinds: pinned_renoise D(23) D(22) R(22 -> 24) D(23); seeded from level 4; multistep over 24, 18, 12, 6, 0; guided with the pins, four
steps, scale guidance_ref.GUIDE_SCALE, clip 0.5.  Every reference is computed once per session and left unchanged."""
import functools

import torch

import fewstep_ref as F
import guidance_ref as G
import resample_ref as RR
import seeded_ref as SR
from oracle import pf_oracle as O

N_PROT, N_PHARM = (300, 70, 33, 48), (64, 1, 17, 2)
RUN_T, RUN_PREC = RR.T, RR.PREC
PINNED_PLAN = [("denoise", 23), ("denoise", 22), ("renoise", 22, 24), ("denoise", 23)]
SEED_LEVEL = 4
MS_LEVELS = F.uniform_plan(RUN_T, 4)
GUIDED_STEPS, GUIDE_CLIP = 4, 0.5
KINDS = ("pinned_renoise", "seeded", "multistep", "guided")


@functools.lru_cache(maxsize=None)
def case():
    """(nf_case, live weights, noise [5, Nf, 9], pins, init_pharm_com, restraints)"""
    from helpers import sampler_live_head
    from nf_cases import nf_case
    from test_gpu_pinned import pins_for
    c = nf_case(6, 11, n_prot=N_PROT, n_pharm=N_PHARM)
    ptr = c.batch.pharm_ptr.tolist()
    assert MS_LEVELS == [24, 18, 12, 6, 0] and ptr == [0, 64, 65, 82, 84]
    noise = torch.randn(5, ptr[-1], 3 + c.cfg.pharm_nf, generator=torch.Generator().manual_seed(RR.NOISE_SEED))
    flags = []
    for n in N_PHARM:
        flags += ([3, 1, 2] + [0] * n)[:n]
    pins = pins_for(c.batch, c.cfg, flags)
    pcom = O.segment_mean(c.batch.prot_x, c.batch.prot_ptr)
    com = pcom + 0.5
    sd, _ = sampler_live_head(c.sd, c.cfg, c.batch, RUN_T, RUN_PREC, noise)
    off = lambda g, v: (pcom[g] + torch.tensor(v)).tolist()
    # graph 0: an attract on its last center (lane 63) plus a repel sphere on all 64; graph 1 (one center): an attract; graph 2:
    # none; graph 3: a repel sphere on both centers
    restraints = [
        [("attract", 63, off(0, [-2.5, 1.0, 2.0]), 1.5, 1.0), ("repel", None, off(0, [0.0, 0.0, 0.0]), 3.0, 1.0)],
        [("attract", 0, off(1, [3.0, 2.0, -2.0]), 1.0, 1.0)],
        None,
        [("repel", None, off(3, [0.5, -0.5, 0.5]), 2.5, 1.0)],
    ]
    return c, sd, noise, pins, com, restraints


@functools.lru_cache(maxsize=None)
def reference(kind, double=False):
    """pinned_renoise / seeded / multistep: (x_0, h_0, frames x, frames h); guided: guidance_ref.guided_reference's namespace"""
    c, sd, noise, pins, com, restraints = case()
    if kind == "pinned_renoise":
        return RR.resampled_reference(sd, c.cfg, c.batch, RUN_T, RUN_PREC, PINNED_PLAN, noise, *pins, com, double=double)
    if kind == "seeded":
        a = SEED_LEVEL
        return SR.seeded_reference(sd, c.cfg, c.batch, RUN_T, RUN_PREC, a, SR.steps_of(a), noise[:a + 1], (pins[1], pins[2]), None, com,
                                   double=double)
    if kind == "multistep":
        return F.fewstep_reference(sd, c.cfg, c.batch, RUN_T, RUN_PREC, F.ms_ops(MS_LEVELS), noise, com, double=double)
    return G.guided_reference(sd, c.cfg, c.batch, RUN_T, RUN_PREC, noise, *pins, com, restraints, scale=G.GUIDE_SCALE, clip=GUIDE_CLIP,
                              double=double, n_steps=GUIDED_STEPS)
