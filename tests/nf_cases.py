"""Inputs at feature counts other than the shipped pharm_nf = 6 / rec_nf = 11, for tests/test_oracle_feature_counts.py (CPU) and
tests/test_gpu_feature_counts.py.

O.synthetic_pocket draws element one-hots from columns 0..3 only, whatever rec_nf is: an encoder column, a type-table row or a
stride that is only right for the first four types goes unseen.  nf_case places the types so that every column counts: the
atoms that are sources of the call's pf edges come first, and the type is the rank modulo rec_nf.
tests/test_oracle_feature_counts.py proves on the oracle that zeroing any one encoder column then moves an output by ten error
budgets or more."""
import functools
from types import SimpleNamespace

import torch

from oracle import pf_oracle as O
from helpers import live_reference

# (pharm_nf, rec_nf) -> (atoms per graph, centers per graph, config fields): what the GPU tests and the knock-out test share.
# Why each pair is here: tests/test_gpu_feature_counts.py.
NF_DESIGNS = {
    (1, 1): ((40, 33), (3, 2), {}),
    (7, 5): ((40, 33, 37), (5, 1, 6), {}),
    (8, 16): ((48, 41), (5, 4), {}),
    (15, 17): ((40, 33), (5, 4), {}),
    (16, 40): ((48, 41, 37), (6, 5, 7), {}),
    (6, 127): ((150, 140, 130), (8, 6, 7), {"pf_k": 16}),
    (6, 130): ((150, 140, 130), (8, 6, 7), {"pf_k": 16}),
    (9, 11): ((40, 33), (4, 3), {}),
    (7, 33): ((64, 56), (4, 3), {"pf_k": 0}),
}
POCKET_SEEDS = (91, 92, 93, 94)


def ranked_types(cfg, batch, prot_x, x_t):
    """[Np] type of every atom: the distinct sources of the call's pf edges first (in order of appearance in the edge list), the
    other atoms behind them in index order, type = rank % rec_nf."""
    src = O.build_dynamic_edges(cfg, batch, prot_x, x_t)["pf"][0].tolist()
    order = list(dict.fromkeys(src))
    seen = set(order)
    order += [a for a in range(int(batch.prot_ptr[-1])) if a not in seen]
    types = torch.empty(len(order), dtype=torch.int64)
    types[torch.tensor(order)] = torch.arange(len(order)) % cfg.rec_nf
    return types, len(seen)


@functools.lru_cache(maxsize=None)
def _nf_case(pharm_nf, rec_nf, n_prot, n_pharm, features, fields, wseed, iseed):
    cfg = O.DynamicsConfig(pharm_nf=pharm_nf, rec_nf=rec_nf, **dict(fields))
    geo = O.synthetic_batch(POCKET_SEEDS[:len(n_prot)], list(n_prot), list(n_pharm),
                            O.DynamicsConfig(**{**cfg.__dict__, "rec_nf": max(rec_nf, 4)}))
    Np, Nf, B = int(geo.prot_ptr[-1]), int(geo.pharm_ptr[-1]), geo.batch_size
    g = torch.Generator().manual_seed(iseed)
    com = O.segment_mean(geo.prot_x, geo.prot_ptr)
    x_t = com[geo.batch_idxs()["pharm"]] + 3.0 * torch.randn(Nf, 3, generator=g)
    h_t = torch.randn(Nf, pharm_nf, generator=g)
    t = torch.rand(B, generator=g)
    w_h, w_x = torch.randn(Nf, pharm_nf, generator=g), torch.randn(Nf, 3, generator=g)
    types, n_src = None, 0
    if features == "onehot":
        types, n_src = ranked_types(cfg, geo, geo.prot_x, x_t)
        prot_h = torch.zeros(Np, rec_nf)
        prot_h[torch.arange(Np), types] = 1.0
    elif features == "dense":
        prot_h = torch.randn(Np, rec_nf, generator=g)
    else:
        raise ValueError(features)
    batch = O.PocketBatch(geo.prot_x, prot_h, geo.prot_ptr, geo.pharm_ptr, geo.pp_src, geo.pp_dst)
    sd = O.make_state_dict(cfg, wseed)
    live = live_reference(sd, cfg, batch, batch.prot_x, x_t, h_t, t)
    return SimpleNamespace(cfg=cfg, batch=batch, prot_x=batch.prot_x, x_t=x_t, h_t=h_t, t=t, w_h=w_h, w_x=w_x, sd=sd, live=live,
                           types=types, n_sources=n_src, features=features)


def nf_case(pharm_nf, rec_nf, n_prot=None, n_pharm=None, features="onehot", wseed=3, iseed=0, **cfg_fields):
    """One dynamics call at (pharm_nf, rec_nf): .cfg, .batch (synthetic_batch geometry built at max(rec_nf, 4), prot_h replaced:
    `onehot` ranked_types, `dense` randn rows), .prot_x (= batch.prot_x), .x_t (pocket COM + 3 randn), .h_t (randn), .t (rand per
    graph) as test_gpu_wide.inputs draws them, .w_h / .w_x (upstream weights for gradients), .sd (seeded weights) and .live
    (helpers.live_reference).  n_prot / n_pharm / config fields default to NF_DESIGNS.  Computed once per argument set; callers
    leave it unchanged."""
    d_prot, d_pharm, d_fields = NF_DESIGNS.get((pharm_nf, rec_nf), ((40, 33), (5, 4), {}))
    fields = {**d_fields, **cfg_fields}
    n_prot = d_prot if n_prot is None else n_prot
    n_pharm = d_pharm if n_pharm is None else n_pharm
    return _nf_case(pharm_nf, rec_nf, tuple(n_prot), tuple(n_pharm), features, tuple(sorted(fields.items())), wseed, iseed)


SCORE_SEEDS = {(8, 16): 5, (1, 1): 5}


@functools.lru_cache(maxsize=None)
def score_case(pharm_nf, rec_nf):
    """Candidates for pf_score on nf_case's batch, drawn as score_ref.inputs draws them (a frame in which the COMs are not zero,
    one-hot rows, one noise row per entry of score_ref.LEVELS); .sd: the case's weights with the live head, k from the first
    level's dynamics call as in score_ref.weights."""
    import score_ref as R
    from helpers import live_head
    c = nf_case(pharm_nf, rec_nf)
    gen = torch.Generator().manual_seed(SCORE_SEEDS[(pharm_nf, rec_nf)])
    Nf = int(c.batch.pharm_ptr[-1])
    x0 = 3.0 * torch.randn(Nf, 3, generator=gen) + torch.tensor([1.5, -2.0, 0.5])
    h0 = torch.nn.functional.one_hot(torch.randint(0, pharm_nf, (Nf,), generator=gen), pharm_nf).float()
    noise = torch.randn(len(R.LEVELS), Nf, 3 + pharm_nf, generator=gen)
    _, al, sg = R.tables()
    st = R.level_inputs(c.batch, x0, h0, R.LEVELS[0], noise[0], R.T, 1.0, True, al, sg, torch.float32)
    _, ex = O.dynamics_forward(c.sd, c.cfg, c.batch, st.prot_x, st.x_t, st.h_t, st.t)
    return SimpleNamespace(cfg=c.cfg, batch=c.batch, x0=x0, h0=h0, noise=noise, sd=live_head(c.sd, c.cfg, ex)[0])


@functools.lru_cache(maxsize=None)
def score_reference(pharm_nf, rec_nf, double):
    """score_ref.compose of score_case: {(ep_coord, ep_feat): (terms [L, B, 4], margins [L, Nf])}"""
    import score_ref as R
    s = score_case(pharm_nf, rec_nf)
    _, al, sg = R.tables()
    return R.compose(s.sd, s.cfg, s.batch, s.x0, s.h0, R.LEVELS, s.noise, R.T, al, sg, double=double)


def edge_margins(cfg, batch, prot_x, x_t):
    """What makes an edge set the same in any correct implementation: {name: value} with `ties` the number of exact distance ties
    that decide membership (kNN: the k-th and (k+1)-th nearest at the same squared distance; radius: none can, the comparison is
    strict, so the count is of squared distances equal to the squared cutoff) and `cap_reached` the number of rows whose
    neighbour count reaches the cap of the radius searches (100 pf, 200 ff, 100 pp)."""
    ties = caps = 0
    r2 = lambda r: torch.tensor(r, dtype=torch.float32) ** 2
    for g in range(batch.batch_size):
        p0, p1 = int(batch.prot_ptr[g]), int(batch.prot_ptr[g + 1])
        f0, f1 = int(batch.pharm_ptr[g]), int(batch.pharm_ptr[g + 1])
        px, fx = prot_x[p0:p1], x_t[f0:f1]
        if f1 > f0 and p1 > p0:
            d = O._d2(fx, px)
            if cfg.pf_k > 0:
                k = min(cfg.pf_k, p1 - p0)
                s = torch.sort(d, dim=1).values
                if k < p1 - p0:
                    ties += int((s[:, k] == s[:, k - 1]).sum())
            else:
                ties += int((d == r2(cfg.cutoff_pf)).sum())
                caps += int(((d < r2(cfg.cutoff_pf)).sum(dim=0) >= 100).sum())
        if f1 - f0 >= 2:
            d = O._d2(fx, fx)
            d.fill_diagonal_(float("inf"))
            if cfg.ff_k > 0:
                k = min(cfg.ff_k, f1 - f0 - 1)
                s = torch.sort(d, dim=1).values
                if k < f1 - f0 - 1:
                    ties += int((s[:, k] == s[:, k - 1]).sum())
            else:
                ties += int((d == r2(cfg.cutoff_ff)).sum())
                caps += int(((d < r2(cfg.cutoff_ff)).sum(dim=1) >= 200).sum())
        if p1 - p0 >= 2:
            d = O._d2(px, px)
            d.fill_diagonal_(float("inf"))
            ties += int((d == r2(cfg.cutoff_pp)).sum())
            caps += int(((d < r2(cfg.cutoff_pp)).sum(dim=1) >= 100).sum())
    return {"ties": ties, "cap_reached": caps}
