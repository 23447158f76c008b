"""Parameter gradients held to the fp64 oracle per 16 x 16 block, with a noise unit that comes from the reference alone.

test_gpu_train.compare holds a gradient tensor to 2e-3 of its own maximum against ONE fp32 oracle evaluation: a thousand times
the kernels' real error, and blind to every block of a tensor whose own maximum is below that (the rbf columns beside the h_src
columns of a message GVP's to_feats_out, the x_hat row of its Wh, the rare element columns of the encoders).  Here:

  * permuted_case / reference_draws: K fp32 oracle gradients of the same mathematics in different summation orders (nodes
    permuted inside every graph, the pp edge order shuffled).  Their spread around the fp64 oracle's gradient, per block, is the
    rounding noise of an fp32 evaluation of that block -- the unit.
  * gradients_within_budget: every block of every tensor within BUDGET_FACTOR units of the fp64 gradient; structurally dead
    blocks exactly zero.

K and the block size are fixed by tests/test_grad_budget_host.py on the reference alone (a held-out draw must pass at half the
factor; profiles/grad_budget/reference_calibration.txt), by nothing a kernel produced."""
from types import SimpleNamespace

import torch

from oracle import pf_oracle as O
from helpers import BUDGET_FACTOR, BUDGET_FLOOR, GRAD_CASES, batch_from, live_head, load

K_DRAWS = 4          # fp32 reference draws that make the unit: draw 0 the identity, draws 1.. permutations
BLOCK = 16           # 16 x 16 tiles of a 2-D tensor, 16-entry segments of a 1-D one (PFT_ROWS, mm16_*)
HELD_OUT = 4         # the seed of the calibration draw: never part of a unit
CALIBRATION_RATIO = BUDGET_FACTOR / 2


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def make_case(cfg, batch, prot_x, x_t, h_t, t, sd, wseed_up, live=True):
    """One training case: inputs, weights (live head: k from the fp32 oracle's eval-mode forward) and random upstream weights."""
    gen = torch.Generator().manual_seed(wseed_up)
    w_h, w_x = torch.randn(h_t.shape, generator=gen), torch.randn(x_t.shape, generator=gen)
    k = 0
    if live:
        sd, k = live_head(sd, cfg, O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, t)[1])
    return SimpleNamespace(cfg=cfg, batch=batch, prot_x=prot_x, x_t=x_t, h_t=h_t, t=t, w_h=w_h, w_x=w_x, sd=sd, k=k)


def widened(cfg, S, V):
    return O.DynamicsConfig(**{**cfg.__dict__, "n_hidden_scalars": S, "vector_size": V})


def golden_case(name, S=128, V=16, live=True):
    """a GRAD_CASES golden's batch and noised inputs (test_gpu_train.noised_inputs), seeded weights at the width asked for"""
    from test_gpu_train import noised_inputs
    z, cfg = load(name), widened(GRAD_CASES[name], S, V)
    batch = batch_from(z)
    x_t, h_t, prot_x, t = noised_inputs(cfg, batch, z, int(z["T"]))
    return make_case(cfg, batch, prot_x, x_t, h_t, t, O.make_state_dict(cfg, int(z["wseed"])), 21, live)


def extra_case(name, S=128, V=16, live=True):
    """a test_gpu_train.EXTRA_CASES shape with the inputs test_gradients_vs_oracle_more_configs draws"""
    from test_gpu_train import EXTRA_CASES
    base, seeds, n_prot, n_pharm = EXTRA_CASES[name]
    cfg = widened(base, S, V)
    batch = O.synthetic_batch(seeds, n_prot, n_pharm, cfg)
    Nf, B = int(batch.pharm_ptr[-1]), batch.batch_size
    gen = torch.Generator().manual_seed(11)
    prot_x = batch.prot_x - O.segment_mean(batch.prot_x, batch.prot_ptr)[batch.batch_idxs()["prot"]]
    x_t = 2.5 * torch.randn(Nf, 3, generator=gen)
    h_t = torch.randn(Nf, cfg.pharm_nf, generator=gen)
    t = torch.rand(B, generator=gen)
    return make_case(cfg, batch, prot_x, x_t, h_t, t, O.make_state_dict(cfg, 3), 22, live)


def build_case(name, S=128, V=16, live=True):
    return golden_case(name, S, V, live) if name in GRAD_CASES else extra_case(name, S, V, live)


# ---- draws of the reference's own rounding noise --------------------------------------------------------------------------------
def _perm_within(ptr, gen):
    """a permutation of 0..ptr[-1] that keeps every graph's index range: new position i holds old node perm[i]"""
    parts = [int(ptr[g]) + torch.randperm(int(ptr[g + 1] - ptr[g]), generator=gen) for g in range(ptr.numel() - 1)]
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64)


def _inverse(perm):
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    return inv


def dynamic_edge_sets(cfg, batch, prot_x, x_t, perm_p=None, perm_f=None):
    """{etype: set of (src, dst)} of build_dynamic_edges, the node ids mapped back through the permutations"""
    edges = O.build_dynamic_edges(cfg, batch, prot_x, x_t)
    ident = lambda n: torch.arange(n)
    perm_p = ident(prot_x.shape[0]) if perm_p is None else perm_p
    perm_f = ident(x_t.shape[0]) if perm_f is None else perm_f
    maps = {"ff": (perm_f, perm_f), "pf": (perm_p, perm_f), "fp": (perm_f, perm_p)}
    out = {}
    for et, (ms, md) in maps.items():
        s, d = edges[et]
        pairs = list(zip(ms[s].tolist(), md[d].tolist()))
        out[et] = set(pairs)
        assert len(out[et]) == len(pairs), et
    return out


def permuted_case(case, seed, drop=None):
    """(case', drop'): the same graphs with the atoms and the centers permuted inside every graph -- pp_src / pp_dst remapped and
    the pp edge order shuffled inside every graph (the edges of a graph stay together: the per-graph edge counts of
    message_norm = 0 are run lengths) --, x_t, h_t, the upstream weights and the dropout masks permuted with their nodes.  Every
    parameter gradient is mathematically invariant under this; in fp32 every scatter sum and every row sum of a weight gradient
    runs in another order.  seed 0 is the identity.  The dynamic edge sets, mapped back, must equal the unpermuted ones (random
    coordinates have no exact distance ties, and no neighbour cap is reached)."""
    if seed == 0:
        return case, drop
    gen = torch.Generator().manual_seed(1000 + seed)
    b = case.batch
    pp, pf = _perm_within(b.prot_ptr, gen), _perm_within(b.pharm_ptr, gen)
    ip = _inverse(pp)
    src, dst = ip[b.pp_src], ip[b.pp_dst]
    gid = torch.searchsorted(b.prot_ptr[1:].contiguous(), dst, right=True)
    assert bool((gid[1:] >= gid[:-1]).all()), "pp edges must be grouped by graph"
    order = torch.argsort(gid.double() + 0.5 * torch.rand(gid.numel(), generator=gen).double())
    batch = O.PocketBatch(b.prot_x[pp], b.prot_h[pp], b.prot_ptr, b.pharm_ptr, src[order], dst[order])
    out = SimpleNamespace(**case.__dict__)
    out.batch, out.prot_x = batch, case.prot_x[pp]
    out.x_t, out.h_t, out.w_h, out.w_x = case.x_t[pf], case.h_t[pf], case.w_h[pf], case.w_x[pf]
    assert (dynamic_edge_sets(case.cfg, batch, out.prot_x, out.x_t, pp, pf)
            == dynamic_edge_sets(case.cfg, b, case.prot_x, case.x_t)), "a permutation changed the dynamic edge set"
    if drop is not None:
        drop = [{"prot": tuple(m[pp] for m in d["prot"]), "pharm": tuple(m[pf] for m in d["pharm"])} for d in drop]
    return out, drop


def oracle_gradients(c, drop, fp64=False, edges=None, w_x=None):
    """({name: gradient}, eps_h, eps_x) of sum(eps_h * w_h) + sum(eps_x * w_x) by the oracle's autograd under the masks ``drop``,
    in fp32 or -- on the edge set decided in fp32 -- in fp64.  edges / w_x: a mutant's replacements."""
    dt = torch.float64 if fp64 else torch.float32
    leaf = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in c.sd.items()}
    batch = O.batch64(c.batch) if fp64 else c.batch
    if drop is not None:
        drop = [{nt: tuple(m.to(dt) for m in d[nt]) for nt in d} for d in drop]
    if edges is None:
        edges = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)
    w_x = c.w_x if w_x is None else w_x
    with torch.enable_grad():
        oh, ox = O.dynamics_forward(leaf, c.cfg, batch, c.prot_x.to(dt), c.x_t.to(dt), c.h_t.to(dt), c.t.to(dt), dropout=drop,
                                    edges=edges)
        ((oh * c.w_h.to(dt)).sum() + (ox * w_x.to(dt)).sum()).backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach()) for k, v in leaf.items()}
    return grads, oh.detach(), ox.detach()


def reference_draws(c, drop, k=K_DRAWS):
    """(draws32, g64, (oh32, ox32), (oh64, ox64)): the K fp32 draws (seeds 0..K-1), the fp64 gradient and the training-forward
    outputs of the unpermuted case in both precisions"""
    draws, out32 = [], None
    for seed in range(k):
        pc, pd = permuted_case(c, seed, drop)
        g, oh, ox = oracle_gradients(pc, pd)
        if seed == 0:
            out32 = (oh, ox)
        draws.append(g)
    g64, h64, x64 = oracle_gradients(c, drop, fp64=True)
    return draws, g64, out32, (h64, x64)


# ---- the check ------------------------------------------------------------------------------------------------------------------
def _block_max(a, block):
    """max over block x block tiles (ragged edges: smaller tiles) of a non-negative 1-D or 2-D tensor, as a 2-D grid"""
    a = a.reshape(a.shape[0], -1) if a.dim() > 1 else a.reshape(-1, 1)
    r, c = a.shape
    R, C = -(-r // block), -(-c // block)
    pad = torch.zeros(R * block, C * block, dtype=a.dtype)
    pad[:r, :c] = a
    return pad.reshape(R, block, C, block).amax(dim=(1, 3))


def block_name(key, shape, i, j, block):
    r = shape[0]
    c = 1
    for s in shape[1:]:
        c *= s
    rows = f"rows {i * block}:{min((i + 1) * block, r)}"
    return f"{key} {rows}" + (f" cols {j * block}:{min((j + 1) * block, c)}" if len(shape) > 1 else "")


def gradients_within_budget(got, draws32, g64, what, block=BLOCK, factor=BUDGET_FACTOR, check=True, extra_unit=None):
    """Every block of every parameter gradient within ``factor`` units of the fp64 oracle's.

    Blocks: a 2-D tensor (state-dict shape) in block x block tiles, a 1-D tensor in block-entry segments, ragged edges as smaller
    blocks, and the whole tensor as one more block.  Per block m = max|g64| and
        unit = max(max_k max|draws32[k] - g64|, BUDGET_FLOOR * m)
    -- the worst of K fp32 evaluations of the same gradient in different summation orders, floored at a quarter ulp of the block's
    largest entry (helpers.within_budget gives the reasoning for the factor 8 and the floor 2**-22; the max over K draws steadies
    the unit a single draw gives).  Asserts max|got - g64| <= factor * unit.  A block whose unit is zero -- g64 and every draw
    identically zero: a structurally dead parameter, whose upstream gradient is exactly zero and everything linear in it -- must
    be exactly zero in ``got``.  extra_unit: None or {name: tensor of the parameter's shape} of absolute terms added to the unit
    elementwise (a derived quantum of the design, never a measured one).

    Prints the worst ratio per tensor.  Returns a SimpleNamespace: ratios (every block with a non-zero unit, as a tensor), worst,
    median, rows [(ratio, err, unit, block name)] sorted worst first, bad (the rows over the bound and the dead blocks that are
    not zero).  check=False only measures."""
    rows, bad, ratios = [], [], []
    for key, r64 in g64.items():
        if r64.numel() == 0:
            continue
        r64 = r64.double()
        g = torch.as_tensor(got[key]).detach().cpu().double().reshape(r64.shape)
        assert bool(torch.isfinite(g).all()), (what, key)
        err = (g - r64).abs()
        dev = torch.zeros_like(r64)
        for d in draws32:
            dev = torch.maximum(dev, (d[key].double().reshape(r64.shape) - r64).abs())
        if extra_unit is not None and key in extra_unit:
            dev = dev + extra_unit[key].double().reshape(r64.shape)
        worst_here = (0.0, 0.0, 0.0, "")
        grids = [(_block_max(err, block), _block_max(dev, block), _block_max(r64.abs(), block), False),
                 (err.max().reshape(1, 1), dev.max().reshape(1, 1), r64.abs().max().reshape(1, 1), True)]
        for e_b, d_b, m_b, whole in grids:
            unit = torch.maximum(d_b, BUDGET_FLOOR * m_b)
            dead = unit == 0
            ratio = torch.where(dead, torch.zeros_like(e_b), e_b / unit.clamp(min=1e-300))
            for i, j in torch.nonzero(dead & (e_b > 0)).tolist():
                name = f"{key} (whole tensor)" if whole else block_name(key, r64.shape, i, j, block)
                bad.append((float("inf"), float(e_b[i, j]), 0.0, name + " [dead block not zero]"))
            ratios.append(ratio[~dead])
            if int((~dead).sum()) == 0:
                continue
            flat = int(torch.where(dead, torch.full_like(ratio, -1.0), ratio).argmax())
            i, j = divmod(flat, ratio.shape[1])
            name = f"{key} (whole tensor)" if whole else block_name(key, r64.shape, i, j, block)
            row = (float(ratio[i, j]), float(e_b[i, j]), float(unit[i, j]), name)
            worst_here = max(worst_here, row)
            for i, j in torch.nonzero(ratio > factor).tolist():
                name = f"{key} (whole tensor)" if whole else block_name(key, r64.shape, i, j, block)
                bad.append((float(ratio[i, j]), float(e_b[i, j]), float(unit[i, j]), name))
        if worst_here[3]:
            rows.append(worst_here)
            print(f"gradient budget {what}: ratio {worst_here[0]:.2f} err {worst_here[1]:.3e} unit {worst_here[2]:.3e} {worst_here[3]}")
    ratios = torch.cat(ratios) if ratios else torch.zeros(0, dtype=torch.float64)
    rows.sort(reverse=True)
    bad.sort(reverse=True)
    res = SimpleNamespace(ratios=ratios, worst=float(ratios.max()) if ratios.numel() else 0.0,
                          median=float(ratios.median()) if ratios.numel() else 0.0, rows=rows, bad=bad,
                          n_blocks=int(ratios.numel()))
    print(f"gradient budget {what}: {res.n_blocks} live blocks, worst ratio {res.worst:.2f}, median {res.median:.2f}, "
          f"{len(bad)} over {factor:g}")
    if check:
        assert not bad, (f"{what}: {len(bad)} blocks outside {factor:g} units of the fp64 gradient (ratio, err, unit, block)",
                         bad[:8])
    return res


UNDERFLOW_ZONE = 2.0 ** -100


def scales_exactly(g64, c):
    """The entries of a gradient for which backward(c w) == c backward(w) can be asked bit for bit in fp32, c a power of two: those
    with min(1, c) |g64| >= 2**-100.  A product or partial sum loses bits to underflow only below the smallest normal, 2**-126; an
    addend that small is under 2**-26 of an entry of 2**-100, a sixteenth of an ulp of it, and does not move its rounding.  Below
    that the entry itself may be built from denormals (the far rbf columns: exp(-(d - mu)**2 / ...) of an edge 10 A from the
    centre of the basis function)."""
    return g64.double().abs() * min(1.0, c) >= UNDERFLOW_ZONE


def worst_blocks(res, n=6):
    """the n worst blocks of a result, tile rows before the per-tensor summary rows they repeat"""
    seen, out = set(), []
    for row in sorted(res.bad + res.rows, reverse=True):
        if row[3] not in seen:
            seen.add(row[3])
            out.append(row)
    return out[:n]
