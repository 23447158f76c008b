"""Gradients w.r.t. the center coordinates and features (pf_train_backward_inputs) held to the fp64 oracle per center row.

The yardstick is the oracle's autograd with x_t and h_t as leaves, on the edge set decided in fp32 (the edge set is piecewise
constant in x and carries no gradient), exactly as grad_budget.oracle_gradients does for the parameters.  The noise unit is
grad_budget's, per center row:

    unit[row] = max(max over K = 4 fp32 oracle draws of max|draw - g64| on that row, 2**-22 max|g64[row]|)

the draws being grad_budget.permuted_case seeds 0..3 with the input gradients mapped back through the center permutation, the
bound helpers.BUDGET_FACTOR (8) units per row of g_x and per row of g_h, a row whose unit is zero exactly zero.  Per row: in the
twin cases the planted rows are 1e5 times the ordinary ones and a whole-tensor tolerance would be blind to every ordinary row.
tests/test_input_grad_host.py calibrates the unit on the reference alone and shows that it has teeth."""
import functools

import torch

from oracle import pf_oracle as O
import grad_budget as G
from helpers import BUDGET_FACTOR, BUDGET_FLOOR

# name -> (builder, live head); the widths are the two vector widths of the wide family and one odd scalar width
CASES = {
    "train_grads 128/16": (lambda: G.build_case("train_grads.npz", 128, 16), True),
    "train_grads 64/32": (lambda: G.build_case("train_grads.npz", 64, 32), True),
    "twin_dev 128/16": (lambda: _twin(128), False),
    "twin 64/32": (lambda: _twin(64), False),
    "per_graph_norm_knn 128/16": (lambda: G.build_case("per_graph_norm_knn", 128, 16), True),
    "single_layer_single_center 96/32": (lambda: G.build_case("single_layer_single_center", 96, 32), True),
    "deep 64/32": (lambda: G.build_case("deep", 64, 32), True),
}


def _twin(S):
    from test_oracle_norm_floor import twin_case
    if S == 128:
        return twin_case("dev")
    from test_gpu_norm_floor import _wide_twin
    return _wide_twin()


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][0]()


def center_permutation(c, seed):
    """the permutation of the centers permuted_case(c, seed) applies: new position i holds old center perm[i]"""
    if seed == 0:
        return torch.arange(int(c.batch.pharm_ptr[-1]))
    gen = torch.Generator().manual_seed(1000 + seed)
    G._perm_within(c.batch.prot_ptr, gen)
    return G._perm_within(c.batch.pharm_ptr, gen)


def oracle_input_gradients(c, drop, fp64=False):
    """(g_x [Nf, 3], g_h [Nf, pharm_nf], eps_h, eps_x) of sum(eps_h * w_h) + sum(eps_x * w_x) w.r.t. x_t and h_t by the oracle's
    autograd under the masks ``drop``, in fp32 or -- on the edge set decided in fp32 -- in fp64"""
    dt = torch.float64 if fp64 else torch.float32
    sd = {k: v.detach().to(dt) for k, v in c.sd.items()}
    batch = O.batch64(c.batch) if fp64 else c.batch
    if drop is not None:
        drop = [{nt: tuple(m.to(dt) for m in d[nt]) for nt in d} for d in drop]
    edges = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)
    x = c.x_t.detach().to(dt).clone().requires_grad_(True)
    h = c.h_t.detach().to(dt).clone().requires_grad_(True)
    with torch.enable_grad():
        oh, ox = O.dynamics_forward(sd, c.cfg, batch, c.prot_x.to(dt), x, h, c.t.to(dt), dropout=drop, edges=edges)
        ((oh * c.w_h.to(dt)).sum() + (ox * c.w_x.to(dt)).sum()).backward()
    zero = lambda leaf: torch.zeros_like(leaf) if leaf.grad is None else leaf.grad.detach()
    return zero(x), zero(h), oh.detach(), ox.detach()


def draw(c, drop, seed):
    """(g_x, g_h) of the fp32 oracle on permuted_case(c, seed), the rows back in the unpermuted order"""
    pc, pd = G.permuted_case(c, seed, drop)
    gx, gh, _, _ = oracle_input_gradients(pc, pd)
    perm = center_permutation(c, seed)
    bx, bh = torch.empty_like(gx), torch.empty_like(gh)
    bx[perm], bh[perm] = gx, gh
    return bx, bh


def reference_draws(c, drop, k=G.K_DRAWS):
    """(draws32 [(g_x, g_h)] of seeds 0..k-1, (g_x64, g_h64), (eps_h32, eps_x32))"""
    draws = [draw(c, drop, seed) for seed in range(k)]
    _, _, oh, ox = oracle_input_gradients(c, drop)
    gx64, gh64, _, _ = oracle_input_gradients(c, drop, fp64=True)
    return draws, (gx64, gh64), (oh, ox)


_REFS = {}


def references(name, c, drop):
    """reference_draws of a case under the masks ``drop``, computed once and left unchanged: every engine draws the same masks for
    a case (one hash of seed, layer, site, node, column)"""
    if name not in _REFS:
        _REFS[name] = (drop,) + reference_draws(c, drop)
    ref = _REFS[name]
    for a, b in zip(ref[0], drop):
        for nt in a:
            assert all(torch.equal(p, q) for p, q in zip(a[nt], b[nt])), "the tests of a case must draw the same dropout masks"
    return ref[1:]


def row_ratios(got, draws, g64):
    """per row: (ratio = err / unit with 0 where the unit is zero, dead = unit is zero, err)"""
    g64 = g64.double()
    got = torch.as_tensor(got).detach().cpu().double().reshape(g64.shape)
    assert bool(torch.isfinite(got).all())
    err = (got - g64).abs().amax(dim=1)
    dev = torch.zeros_like(err)
    for d in draws:
        dev = torch.maximum(dev, (d.double() - g64).abs().amax(dim=1))
    unit = torch.maximum(dev, BUDGET_FLOOR * g64.abs().amax(dim=1))
    dead = unit == 0
    return torch.where(dead, torch.zeros_like(err), err / unit.clamp(min=1e-300)), dead, err


def rows_within_budget(got_x, got_h, draws, g64, what, factor=BUDGET_FACTOR, check=True):
    """Every row of g_x and of g_h within ``factor`` units of the fp64 oracle's; a row whose unit is zero exactly zero.  Prints
    the worst ratio per tensor and returns them as (worst g_x, worst g_h); check=False only measures (a dead row that is not
    zero counts as inf)."""
    worst = []
    for i, (got, part) in enumerate(((got_x, "g_x"), (got_h, "g_h"))):
        ratio, dead, err = row_ratios(got, [d[i] for d in draws], g64[i])
        live = bool(dead.any()) and bool((err[dead] > 0).any())
        w = float("inf") if live else (float(ratio.max()) if ratio.numel() else 0.0)
        row = int(ratio.argmax()) if ratio.numel() else -1
        print(f"input gradient budget {what} {part}: worst ratio {w:.2f} (row {row}, err {float(err[row]) if row >= 0 else 0.0:.3e}), "
              f"median {float(ratio.median()) if ratio.numel() else 0.0:.2f}, {int(dead.sum())} dead rows of {ratio.numel()}")
        if check:
            assert not live, f"{what} {part}: rows {torch.nonzero(dead & (err > 0)).flatten().tolist()} must be exactly zero"
            bad = torch.nonzero(ratio > factor).flatten().tolist()
            assert not bad, (f"{what} {part}: rows outside {factor:g} units of the fp64 gradient (row, ratio, err)",
                             [(r, float(ratio[r]), float(err[r])) for r in bad[:8]])
        worst.append(w)
    return tuple(worst)
