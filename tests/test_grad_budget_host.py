"""grad_budget.gradients_within_budget calibrated and proved on the CPU oracle alone.

Calibration: a held-out fp32 draw of the reference (a permutation that is in no unit) must sit within HALF the budget factor of
the fp64 gradient in every block of every case -- that fixes K and the block size (grad_budget.K_DRAWS, BLOCK), and nothing
measured on a GPU does.  With PF_GRADIENT_CALIBRATION_FILE naming a file the chosen values and the held-out ratios are written
there (profiles/grad_budget/reference_calibration.txt).

Mutants: four wrong gradients, restated on the oracle, that test_gpu_train.compare at 2e-3 lets through and the new check does
not."""
import functools
import os

import pytest
import torch

from oracle import pf_oracle as O
import grad_budget as G
from helpers import BUDGET_FACTOR
from test_gpu_train import compare

P_DROP, DROP_SEED = 0.1, 5
# the four calibration cases at 128 / 16, and the two other widths the GPU legs run (on the largest case)
CALIBRATION_CASES = [("train_grads.npz", 128, 16), ("large_radius", 128, 16), ("per_graph_norm_knn", 128, 16),
                     ("single_layer_single_center", 128, 16), ("large_radius", 64, 32), ("large_radius", 256, 32)]
CALIBRATION_ROWS = {}
MSG0_OUT = "dynamics.noise_predictor.conv_layers.0.edge_message_fns.prot_pf_pharm.0.to_feats_out.0.weight"


def masks(c):
    return O.dropout_masks(c.cfg, int(c.batch.pharm_ptr[-1]), int(c.batch.prot_ptr[-1]), P_DROP, DROP_SEED)


@functools.lru_cache(maxsize=None)
def refs(name, S=128, V=16, live=True):
    """(case, masks, draws32, g64, the held-out permuted case and its masks): computed once and left unchanged"""
    c = G.build_case(name, S, V, live)
    drop = masks(c)
    draws, g64, _, _ = G.reference_draws(c, drop)
    hc, hd = G.permuted_case(c, G.HELD_OUT, drop)
    return c, drop, draws, g64, hc, hd


@functools.lru_cache(maxsize=None)
def held_out(name, S=128, V=16, live=True):
    c, drop, draws, g64, hc, hd = refs(name, S, V, live)
    return G.oracle_gradients(hc, hd)[0]


# ---- the check itself -----------------------------------------------------------------------------------------------------------
def test_blocks_units_and_dead_blocks():
    g64 = {"w": torch.zeros(20, 33, dtype=torch.float64), "b": torch.zeros(40, dtype=torch.float64), "e": torch.zeros(0)}
    g64["w"][:16, :16] = 1.0
    g64["w"][16:, 32] = 2.0 ** -30          # a ragged 4 x 1 corner block, far below the tensor's max
    g64["b"][:16] = 1.0
    draws = [{k: v.float() for k, v in g64.items()}]
    ok = {k: v.clone() for k, v in g64.items()}
    res = G.gradients_within_budget(ok, draws, g64, "exact")
    assert res.worst == 0.0 and res.n_blocks == 2 + 1 + 1 + 1            # live tiles of w, whole w, b[0:16], whole b
    # within the floor: 8 * 2**-22 of the BLOCK's max
    near = {k: v.clone() for k, v in g64.items()}
    near["w"][17, 32] += 7.9 * 2.0 ** -52
    assert 7.8 < G.gradients_within_budget(near, draws, g64, "near").worst < 8.0
    # one unit more in the small corner: invisible at the tensor's scale, named by rows and columns
    off = {k: v.clone() for k, v in g64.items()}
    off["w"][17, 32] *= 1.0 + 2.0 ** -18
    with pytest.raises(AssertionError, match=r"w rows 16:20 cols 32:33"):
        G.gradients_within_budget(off, draws, g64, "off")
    compare({k: v.float() for k, v in off.items()}, draws[0], 2e-3, "off")
    # a dead block must be exactly zero
    dead = {k: v.clone() for k, v in g64.items()}
    dead["b"][39] = 1e-30
    with pytest.raises(AssertionError, match=r"b rows 32:40 \[dead block not zero\]"):
        G.gradients_within_budget(dead, draws, g64, "dead")
    # the draws make the unit: a block the reference itself cannot pin down is allowed as much
    noisy = [draws[0], {k: v.clone() for k, v in draws[0].items()}]
    noisy[1]["b"][20] = 1e-3
    moved = {k: v.clone() for k, v in g64.items()}
    moved["b"][21] = 7e-3
    assert 6.9 < G.gradients_within_budget(moved, noisy, g64, "noisy").worst < 7.1
    # a derived absolute term widens the unit where it is given, nowhere else
    extra = {"b": torch.full((40,), 1e-30, dtype=torch.float64)}
    assert G.gradients_within_budget(dead, draws, g64, "dead + term", extra_unit=extra).worst == pytest.approx(1.0)


def test_permuted_case_is_the_same_mathematics():
    """seed 0 is the identity; a permuted copy has the graphs' node ranges, the same dynamic edge sets (asserted inside
    permuted_case) and pp edge multiset, and -- in fp64, where summation order no longer matters at this level -- the same
    gradient; in fp32 it is a different draw"""
    c, drop, draws, g64, hc, hd = refs("per_graph_norm_knn")
    same, same_drop = G.permuted_case(c, 0, drop)
    assert same is c and same_drop is drop
    assert torch.equal(hc.batch.prot_ptr, c.batch.prot_ptr) and not torch.equal(hc.x_t, c.x_t)
    assert sorted(hc.x_t.flatten().tolist()) == sorted(c.x_t.flatten().tolist())
    assert hc.batch.pp_src.numel() == c.batch.pp_src.numel()
    d = lambda b: sorted(((b.prot_x[b.pp_src] - b.prot_x[b.pp_dst]).square().sum(1)).tolist())
    assert d(hc.batch) == d(c.batch)
    assert not torch.equal(hc.batch.pp_dst, torch.sort(hc.batch.pp_dst).values)          # the edge order is shuffled too
    p64 = G.oracle_gradients(hc, hd, fp64=True)[0]
    h32 = held_out("per_graph_norm_knn")
    moved = 0
    for k, r in g64.items():
        if r.numel() == 0:
            continue
        m = float(r.abs().max())
        assert float((p64[k] - r).abs().max()) <= 1e-12 * m, k
        moved += int(not torch.equal(h32[k], draws[0][k]))
    assert moved >= 100


# ---- calibration ----------------------------------------------------------------------------------------------------------------
def _write_calibration():
    out = os.environ.get("PF_GRADIENT_CALIBRATION_FILE")
    if not out:
        return
    head = (f"Calibration of tests/grad_budget.py::gradients_within_budget on the reference alone (tests/test_grad_budget_host.py::\n"
            f"test_held_out_reference_draw_is_within_half_the_budget): K = {G.K_DRAWS} fp32 oracle draws make the unit (draw 0 the\n"
            f"identity, draws 1..{G.K_DRAWS - 1} node permutations), blocks of {G.BLOCK} x {G.BLOCK} (1-D: {G.BLOCK}) plus the whole tensor, factor "
            f"{BUDGET_FACTOR:g}, floor 2**-22 of a block's max.\nA held-out fp32 draw (permutation seed {G.HELD_OUT}) against the fp64 "
            f"gradient, dropout {P_DROP}, live head: every block ratio must be <= {G.CALIBRATION_RATIO:g}.\nThe first K and block size "
            f"tried (K = 4, 16 x 16) pass; nothing here was measured on a GPU.\n\n")
    with open(out, "w") as f:
        f.write(head + "\n".join(CALIBRATION_ROWS[k] for k in sorted(CALIBRATION_ROWS)) + "\n")


@pytest.mark.parametrize("name,S,V", CALIBRATION_CASES)
def test_held_out_reference_draw_is_within_half_the_budget(name, S, V):
    """The reference against itself: a fifth fp32 draw, in no unit, inside ratio 4 in every block.  Were it not, K would go up
    (to 8 at most), then the tiles to 32 x 32 and 64 x 64 -- here, never from what a kernel gives."""
    c, drop, draws, g64, hc, hd = refs(name, S, V)
    assert len(draws) == G.K_DRAWS
    res = G.gradients_within_budget(held_out(name, S, V), draws, g64, f"held-out draw {name} {S}/{V}",
                                    factor=G.CALIBRATION_RATIO)
    dead = sum(1 for k, r in g64.items() if r.numel() and float(r.abs().max()) == 0.0
               and all(float(d[k].abs().max()) == 0.0 for d in draws))
    live = sum(1 for r in g64.values() if r.numel()) - dead
    assert res.worst <= G.CALIBRATION_RATIO and live >= 80 and res.n_blocks >= 1000
    lines = [f"{name} {S}/{V}: {live} live tensors, {dead} dead, {res.n_blocks} live blocks, worst ratio {res.worst:.2f}, "
             f"median {res.median:.2f}, blocks over 2: {int((res.ratios > 2).sum())}"]
    lines += [f"    {r:8.2f}  err {e:.3e}  unit {u:.3e}  {b.replace('dynamics.noise_predictor.', '')}"
              for r, e, u, b in G.worst_blocks(res, 3)]
    CALIBRATION_ROWS[f"{name} {S:4d}/{V}"] = "\n".join(lines)
    _write_calibration()


def test_dead_parameters_are_exactly_zero_in_every_draw():
    """about 54 of the 244 tensors of the default architecture have no path to the outputs (the last layer's protein side): the
    reference gives exact zeros for them in fp32, fp64 and under every permutation, so the check may ask for exact zeros"""
    c, drop, draws, g64, hc, hd = refs("train_grads.npz")
    dead = [k for k, r in g64.items() if r.numel() and float(r.abs().max()) == 0.0]
    assert 40 <= len(dead) <= 70 and len(g64) == 244, (len(dead), len(g64))
    for k in dead:
        assert all(float(d[k].abs().max()) == 0.0 for d in draws + [held_out("train_grads.npz")]), k


# ---- mutants --------------------------------------------------------------------------------------------------------------------
# Each is a wrong gradient restated on the oracle side (on the held-out draw, which no unit contains).  Each must fail the new
# check.  (a) and (b) pass test_gpu_train.compare at 2e-3 -- the gap this check closes.  (c) and (d) as the issue states them do
# NOT pass compare on these inputs, by a wide margin, and are not tuned until they do; their docstrings give the figures.
def _fails_new(got, draws, g64, what, expect_block=None):
    res = G.gradients_within_budget(got, draws, g64, what, check=False)
    print(f"mutant {what}: {len(res.bad)} blocks over the bound, worst {res.bad[0] if res.bad else None}")
    assert res.bad, what
    with pytest.raises(AssertionError, match="outside"):
        G.gradients_within_budget(got, draws, g64, what)
    if expect_block is not None:
        assert any(expect_block in b[3] for b in res.bad), (expect_block, res.bad[:4])
    return res


def _compare_verdict(got, ref, what):
    """True where test_gpu_train.compare at 2e-3 sees the mutant"""
    try:
        compare(got, ref, 2e-3, what)
    except AssertionError:
        return True
    return False


def test_mutant_one_small_tile_zeroed():
    """(a) one tile of the 16 x 16 grid lost, in a tensor where that tile's max is below 1e-3 of the tensor's max: of all such
    tiles of the `deep` case the largest (the other calibration cases have none below 1e-3: their smallest tiles, the sh column 160
    of a message GVP 0's to_feats_out and the corner of its 17 x 17 Wh, sit at 1.0e-3 .. 5e-3 of the tensor's max).  compare
    passes; the new check names the tile."""
    c, drop, draws, g64, hc, hd = refs("deep")
    got = {k: v.clone() for k, v in held_out("deep").items()}
    best = (0.0, None)
    for k, r in g64.items():
        if r.dim() != 2 or r.numel() == 0 or float(r.abs().max()) == 0.0:
            continue
        tiles = G._block_max(r.abs(), G.BLOCK)
        small = torch.where(tiles < 1e-3 * r.abs().max(), tiles, torch.zeros_like(tiles))
        if float(small.max()) / float(r.abs().max()) > best[0]:
            i, j = divmod(int(small.argmax()), tiles.shape[1])
            best = (float(small.max()) / float(r.abs().max()), (k, i, j))
    assert best[1] is not None and 0 < best[0] < 1e-3
    k, i, j = best[1]
    B = G.BLOCK
    got[k][B * i:B * i + B, B * j:B * j + B] = 0.0
    name = G.block_name(k, g64[k].shape, i, j, B)
    print(f"mutant (a): {name}, max {best[0]:.3e} of the tensor's")
    compare(got, draws[0], 2e-3, "mutant (a)")                          # the suite's gradient check lets it through
    res = _fails_new(got, draws, g64, "mutant (a) tile zeroed", name)
    assert all(k in b[3] for b in res.bad) and len(res.bad) <= 2          # the tile, and the tensor as a whole at the reference's unit


def test_mutant_rbf_columns_scaled():
    """(b) the rbf columns [S, S + 16) of a message GVP 0 to_feats_out gradient 1 % too large, for every message GVP 0 of the
    large_radius case in turn.  The new check fails on each, in those columns.  compare lets the mutant through exactly where
    0.01 max|rbf columns| <= 2e-3 max|tensor|, i.e. where the rbf columns stay below a fifth of the tensor's max: two of the six
    live tensors here (the others' rbf columns reach 0.20 .. 0.28 of the max, and compare sees 1 % of that)."""
    c, drop, draws, g64, hc, hd = refs("large_radius")
    held = held_out("large_radius")
    S, R = c.cfg.n_hidden_scalars, c.cfg.rbf_dim
    keys = [k for k in g64 if ".edge_message_fns." in k and k.endswith(".0.to_feats_out.0.weight") and float(g64[k].abs().max()) > 0]
    assert len(keys) == 6
    let_through = 0
    for k in keys:
        got = {k: held[k].clone()}
        got[k][:, S:S + R] *= 1.01
        share = float(g64[k][:, S:S + R].abs().max() / g64[k].abs().max())
        res = _fails_new(got, [{k: d[k]} for d in draws], {k: g64[k]}, f"mutant (b) {k}", f"cols {S}:{S + R}")
        assert all(f"cols {S}:{S + R}" in b[3] or "whole tensor" in b[3] for b in res.bad)
        seen = _compare_verdict(got, {k: draws[0][k]}, k)
        print(f"mutant (b) {k}: rbf columns at {share:.3f} of the max, compare {'sees it' if seen else 'lets it through'}")
        assert seen == (share > 0.2) or 0.19 <= share <= 0.21
        let_through += not seen
    assert let_through >= 2


def test_mutant_one_pf_edge_lost():
    """(c) the gradient of a forward that lost one pf edge -- the longest of 1,212, the one a cutoff comparison an ulp off
    loses -- with build_dynamic_edges wrapped.  The new check fails in thousands of blocks.  This mutant does NOT pass compare:
    one message less into a center moves that center's features through two LayerNorms and every gradient with them, the encoders'
    by 9e-2 of their max; 188 tensors are outside 2e-3.  It is kept as stated, not tuned."""
    c, drop, draws, g64, hc, hd = refs("large_radius")
    orig = O.build_dynamic_edges

    def wrapped(cfg, batch, prot_x, pharm_x):
        edges = dict(orig(cfg, batch, prot_x, pharm_x))
        s, d = edges["pf"]
        far = int((prot_x[s] - pharm_x[d]).square().sum(1).argmax())
        keep = torch.arange(s.numel()) != far
        edges["pf"] = (s[keep], d[keep])
        return edges

    O.build_dynamic_edges = wrapped
    try:
        n_before = orig(hc.cfg, hc.batch, hc.prot_x, hc.x_t)["pf"][0].numel()
        assert wrapped(hc.cfg, hc.batch, hc.prot_x, hc.x_t)["pf"][0].numel() == n_before - 1
        got = G.oracle_gradients(hc, hd)[0]
    finally:
        O.build_dynamic_edges = orig
    res = _fails_new(got, draws, g64, f"mutant (c) one of {n_before} pf edges lost")
    print(f"mutant (c): compare at 2e-3 {'sees it' if _compare_verdict(got, draws[0], 'mutant (c)') else 'lets it through'}")
    assert len(res.bad) >= 1000


def test_mutant_vector_head_upstream_dropped():
    """(d) w_x = 0: the backward of the vector head never ran.  Under the live head the new check fails in thousands of blocks by
    factors beyond a hundred budgets.  Under the plain head compare does NOT let it through either on this case (65 tensors
    outside 2e-3: the vector-channel parameters -- Wh, Wu, the gates -- whose gradient through eps_h is as small as the one through
    eps_x), so the plain leg shows no gap here; what it shows is printed."""
    for live in (False, True):
        c, drop, draws, g64, hc, hd = refs("large_radius", 128, 16, live)
        got = G.oracle_gradients(hc, hd, w_x=torch.zeros_like(hc.w_x))[0]
        print(f"mutant (d) {'live' if live else 'plain'} head: compare at 2e-3 "
              f"{'sees it' if _compare_verdict(got, draws[0], 'mutant (d)') else 'lets it through'}")
        if live:
            res = _fails_new(got, draws, g64, "mutant (d) live head")
            assert len(res.bad) >= 1000 and res.bad[0][0] > 100 * BUDGET_FACTOR


# ---- the upstream scale ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2c", [-30, 20])
def test_oracle_gradient_scales_exactly_with_the_upstream(log2c):
    """Every gradient is linear in the upstream ones and a power of two scales every product and partial sum exactly unless
    something underflows.  On the fp32 oracle (one thread: its threaded reductions are not run-to-run deterministic) something
    does, at c = 1 already: the far rbf columns of a message GVP 0's to_feats_out gradient hold entries down to 1e-43.  Outside
    grad_budget.scales_exactly's zone -- entries below 2**-100 after scaling -- backward(c w) equals c backward(w) bit for bit,
    which is what tests/test_gpu_grad_budget.py then asks of the kernels (k_fix_scale); inside it, to 2**-100."""
    c, drop, draws, g64, hc, hd = refs("large_radius")
    s = 2.0 ** log2c
    from types import SimpleNamespace
    scaled = SimpleNamespace(**{**c.__dict__, "w_h": c.w_h * s, "w_x": c.w_x * s})
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        base = G.oracle_gradients(c, drop)[0]
        g = G.oracle_gradients(scaled, drop)[0]
    finally:
        torch.set_num_threads(threads)
    inside = 0
    for k, v in base.items():
        if v.numel() == 0:
            continue
        exact = G.scales_exactly(g64[k], s)
        assert torch.equal(g[k][exact], (v * s)[exact]), k
        assert float((g[k].double() - v.double() * s).abs().max()) <= 2.0 ** -100, k
        inside += int((~exact & (g64[k] != 0)).sum())
    print(f"upstream scale 2**{log2c}: {inside} non-zero entries inside the underflow zone")
    assert 0 < inside < 2000
