"""The CPU composition a device score (pf_score) is compared with: the lines of O.training_forward per noise level, keeping the
per-graph sums instead of the batch means, in fp32 and in fp64, for all four parameterisations -- written on the oracle's public
functions only.  And the one case the scoring tests share (computed once per session, left unchanged)."""
import functools
from types import SimpleNamespace

import torch

from oracle import pf_oracle as O
from helpers import live_head

T, PRECISION = 24, 0.25              # alpha^2 runs from 0.75 down to 0.25: no level divides by a tiny alpha
LEVELS = [1, 7, 24]
# the smallest shapes at which the kernels can go wrong: ragged pockets (300 atoms: the strided pocket loop of k_score_prepare),
# one center (it is its own COM: x0c = 0), 64 centers (a full wave, the per-graph limit)
N_PROT, N_PHARM = [48, 300, 40, 64, 32], [3, 8, 5, 1, 64]
POCKET_SEEDS = [11, 12, 13, 14, 15]
CASE_SEED = 498                       # chosen so that every predicted-type margin is clear AND one fp32 evaluation stays within the
                                     # budget's floor of fp64 in every combination (test_score_host.py asserts both)
WIDTHS = {"128x16": {}, "64x32": dict(n_hidden_scalars=64, vector_size=32)}
PARAMS = [(False, False), (False, True), (True, False), (True, True)]        # (ep_coord, ep_feat)


def tables(T_=T, precision=PRECISION):
    """(gamma, alpha, sigma) tables [T + 1], fp32 -- what the caller of pf_score uploads"""
    g = O.gamma_table(T_, precision)
    return g, O.alpha(g), O.sigma(g)


def level_inputs(batch, x0, h0, t_int, eps, T_, feat_norm, remove_com, alpha_tab, sigma_tab, dtype):
    """training_forward's lines up to the dynamics call for ONE level of the whole batch.  eps: [Nf, 3 + nf], x columns first."""
    bidx = batch.batch_idxs()
    x0, h0, eps, prot = x0.to(dtype), h0.to(dtype) / feat_norm, eps.to(dtype), batch.prot_x.to(dtype)
    com = O.segment_mean(x0, batch.pharm_ptr)
    x0c = x0 - com[bidx["pharm"]]
    prot_x = prot - com[bidx["prot"]]
    a, s = alpha_tab[t_int].to(dtype), sigma_tab[t_int].to(dtype)
    x_t = a * x0c + s * eps[:, :3]
    h_t = a * h0 + s * eps[:, 3:]
    com2 = torch.zeros_like(com)
    if remove_com:
        com2 = O.segment_mean(x_t, batch.pharm_ptr)
        x_t = x_t - com2[bidx["pharm"]]
        prot_x = prot_x - com2[bidx["prot"]]
    t = torch.full((batch.batch_size,), t_int, dtype=torch.float32) / T_
    return SimpleNamespace(x0c=x0c, h0=h0, prot_x=prot_x, x_t=x_t, h_t=h_t, com2=com2, a=a, s=s, t=t, eps_x=eps[:, :3], eps_h=eps[:, 3:])


def level_terms(batch, st, dyn_h, dyn_x, ep_coord, ep_feat):
    """[B, 4] = pos, feat, err, hits of one level, each summed over the centers of a graph; and the per-center margin of the
    predicted type (top value minus runner-up, over the row's largest magnitude)."""
    bidx = batch.batch_idxs()["pharm"]
    if ep_coord:
        pos = (dyn_x + st.com2[bidx] - st.x0c).square().sum(dim=1)
        err = pos
    else:
        pos = (st.eps_x - dyn_x).square().sum(dim=1)
        err = ((st.x_t - st.s * dyn_x) / st.a - st.x0c).square().sum(dim=1)
    clean = st.h0.argmax(dim=1)
    if ep_feat:
        feat = torch.logsumexp(dyn_h, dim=1) - dyn_h.gather(1, clean[:, None])[:, 0]
        pred_rows = dyn_h
    else:
        feat = (st.eps_h - dyn_h).square().sum(dim=1)
        pred_rows = (st.h_t - st.s * dyn_h) / st.a
    hit = (pred_rows.argmax(dim=1) == clean).to(pos.dtype)
    if pred_rows.shape[1] >= 2:
        top = pred_rows.topk(2, dim=1).values
        margin = (top[:, 0] - top[:, 1]) / pred_rows.abs().max(dim=1).values
    else:                                   # one type: there is no runner-up, the prediction cannot be another
        margin = torch.ones_like(pos)
    out = torch.zeros(batch.batch_size, 4, dtype=pos.dtype)
    for q, v in enumerate((pos, feat, err, hit)):
        out[:, q].index_add_(0, bidx, v)
    return out, margin


def compose(sd, cfg, batch, x0, h0, levels, noise, T_, alpha_tab, sigma_tab, feat_norm=1.0, remove_com=True, double=False,
            drop_com2=False):
    """{(ep_coord, ep_feat): (terms [L, B, 4], margins [L, Nf])} -- one dynamics call per level serves the four forms.
    drop_com2: a WRONG composition for the discrimination checks (the second COM is removed but not added back / not counted)."""
    dtype = torch.float64 if double else torch.float32
    fwd = O.dynamics_forward64 if double else O.dynamics_forward
    acc = {p: ([], []) for p in PARAMS}
    for l, t_int in enumerate(levels):
        st = level_inputs(batch, x0, h0, int(t_int), noise[l], T_, feat_norm, remove_com, alpha_tab, sigma_tab, dtype)
        dyn_h, dyn_x = fwd(sd, cfg, batch, st.prot_x, st.x_t, st.h_t, st.t)
        if drop_com2:
            st.com2 = torch.zeros_like(st.com2)
        for p in PARAMS:
            tm, mg = level_terms(batch, st, dyn_h.to(dtype), dyn_x.to(dtype), *p)
            acc[p][0].append(tm)
            acc[p][1].append(mg)
    return {p: (torch.stack(v[0]), torch.stack(v[1])) for p, v in acc.items()}


def score_of(terms, w_pos, w_feat):
    """[B, 2]: the weighted sums over levels, added in level order in the dtype of ``terms``"""
    out = torch.zeros(terms.shape[1], 2, dtype=terms.dtype)
    for l in range(terms.shape[0]):
        out[:, 0] += torch.as_tensor(w_pos[l]).to(terms.dtype) * terms[l, :, 0]
        out[:, 1] += torch.as_tensor(w_feat[l]).to(terms.dtype) * terms[l, :, 1]
    return out


@functools.lru_cache(maxsize=None)
def inputs(width="128x16"):
    """the shared case's batch, candidates and noise (one row per entry of LEVELS) and the recorded weights"""
    cfg = O.DynamicsConfig(**WIDTHS[width])
    batch = O.synthetic_batch(POCKET_SEEDS, N_PROT, N_PHARM, cfg)
    gen = torch.Generator().manual_seed(CASE_SEED)
    Nf = int(batch.pharm_ptr[-1])
    x0 = 3.0 * torch.randn(Nf, 3, generator=gen) + torch.tensor([1.5, -2.0, 0.5])       # (a frame in which the COMs are not zero)
    h0 = torch.nn.functional.one_hot(torch.randint(0, cfg.pharm_nf, (Nf,), generator=gen), cfg.pharm_nf).float()
    noise = torch.randn(len(LEVELS), Nf, 3 + cfg.pharm_nf, generator=gen)
    return SimpleNamespace(cfg=cfg, batch=batch, x0=x0, h0=h0, noise=noise, sd=O.make_state_dict(cfg, 0))


@functools.lru_cache(maxsize=None)
def weights(width, head):
    """the recorded weights, or the live head's (helpers.live_head: eps_x of order one, scaled by a power of two from the fp32
    oracle's eps_x of the case's first level)"""
    c = inputs(width)
    if head == "recorded":
        return c.sd
    _, al, sg = tables()
    st = level_inputs(c.batch, c.x0, c.h0, LEVELS[0], c.noise[0], T, 1.0, True, al, sg, torch.float32)
    _, ex = O.dynamics_forward(c.sd, c.cfg, c.batch, st.prot_x, st.x_t, st.h_t, st.t)
    return live_head(c.sd, c.cfg, ex)[0]


@functools.lru_cache(maxsize=None)
def reference(width, head, remove_com, double):
    """compose() of the shared case: {(ep_coord, ep_feat): (terms [3, B, 4], margins [3, Nf])}"""
    c = inputs(width)
    _, al, sg = tables()
    return compose(weights(width, head), c.cfg, c.batch, c.x0, c.h0, LEVELS, c.noise, T, al, sg, remove_com=remove_com, double=double)
