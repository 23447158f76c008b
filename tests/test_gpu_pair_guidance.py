"""Pair guidance of a guided run (pf_guide_pairs_next: distance restraints between two centers of one graph; k_guide_pairs behind
k_guide_grad, k_guide_field and k_guide_types) against the CPU composition of tests/pair_guidance_ref.py:
guidance_ref.guided_reference -- type_guidance_ref.types_reference where a field and types are present -- with the lines of
DESIGN 4.25.

Shape: guidance_ref.case() -- five ragged pockets with 3 / 8 / 5 / 1 / 6 centers, graph 1's centers 0 and 1 position-pinned, its
spatial restraints, T = 24, live head -- with minimum separations of 4 on graphs 1, 3 (the single center: exact zeros) and 4, a
pinned - free upper bound on graph 1, a window and a one-wildcard restraint on graph 2.  Whole runs at rtol = atol = 5e-3 in both
parameterisations on the tuned family and at (64, 32), T = 12 on the wide family; the noise run must MISS the references that
ignore the arming or the pin rule.  One step read back against fp64 under helpers.within_budget, also on a batch of 1 / 2 / 5 / 3 /
64 centers with the cap of 256 restraints, rho == 0 between two pinned centers and a graph without pairs between two with some;
that step bitwise equal on a second run.  The minimum separations weigh 0.125 (pair_guidance_ref.W_SEP says why).

Measured on the MI355X, worst |error| over x_0, h_0 and all frames: 2.9e-6 (noise; energies 2.1e-5, the last E_pair 5.9e-8, g_pair
4.8e-7), 8.9e-6 (endpoint; energies 4.3e-5), 2.5e-5 at (64, 32) (energies 9.8e-4 on values of several thousand); the noise run misses
the references without the arming / without the pin rule by 1.90 / 3.67.  One step against the fp64 reference, ratio to
max(e32, 2**-22) of E / g0 / grad / shift / g_pair / E_pair: 0.20 / 0.57 / 1.70 / 1.79 / 1.52 / 0.30 (noise), 0.35 / 1.22 / 3.26 /
3.36 / 1.27 / 0.92 (endpoint), 0.58 / 0.74 / 1.57 / 1.60 / 0.74 / 0.58 (the shapes batch), 0.14 / 1.62 / 0.91 / 0.95 / 1.52 / 0.30
(with field and types); of the allowed 8.

Conditions on the inputs are checked on the CPU by test_pair_guidance_host.py."""
import math

import pytest
import torch

import pharmacoforge_amd as pfa
import guidance_ref as G
import pair_guidance_ref as PG
import pocket_field_ref as F
import type_guidance_ref as TG
from helpers import within_budget
from oracle import pf_oracle as O
from test_gpu_guidance import ERR_ARG, ERR_STATE, arrays, check_run
from test_gpu_pinned import bound, engine_for

pytestmark = pytest.mark.gpu

T = PG.T
INF = math.inf


def run_pairs(eng, n_t, noise, pins, com, restraints, pairs, family="tuned", field=None, types=None, **kw):
    arr, parr, garr = arrays(eng, n_t)
    return eng.sample(arr, n_t, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr,
                      guide_scale=G.GUIDE_SCALE, guide_family=family, pairs=pairs, field=field, types=types, **kw)


# 1. whole runs
@pytest.mark.parametrize("ep", [False, True])
def test_pairs_run_vs_composition(ep):
    cfg, sd, k, batch, noise, pins, com, restraints, pairs = PG.case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_pairs(eng, T, noise, pins, com, restraints, pairs, ep_coord=ep, ep_feat=ep, trajectory=True, energies=True)
    assert eng.train_family() == "tuned" and eng.train_input_grads() is False
    ref = PG.reference(ep)
    check_run(eng, cfg, got, ref, pins, f"pairs, tuned {'ep' if ep else 'noise'} (k = {k})")
    g_pair, e_pair = (t.cpu() for t in eng.last_pair_guidance())
    print("E_pair of the last step, worst |error|: %.3g; g_pair %.3g" % (float((e_pair - ref.E_pair[-1]).abs().max()),
                                                                        float((g_pair - ref.g_pair[-1]).abs().max())))
    torch.testing.assert_close(e_pair, ref.E_pair[-1], rtol=G.TOL, atol=G.TOL)
    torch.testing.assert_close(g_pair, ref.g_pair[-1], rtol=G.TOL, atol=G.TOL)
    if ep:
        return
    # ... and it is no rounding error of a run that ignored the arming or the pin rule
    tx = got[2].cpu()
    for name, un in (("without the arming", PG.reference(ep, False, False)), ("without the pin rule", PG.reference(ep, False, True, False))):
        miss = float((tx - un.fx).abs().max())
        print(f"the reference {name} is missed by {miss:.3g}")
        assert miss >= 10 * G.TOL
        with pytest.raises(AssertionError):
            torch.testing.assert_close(tx, un.fx, rtol=G.TOL, atol=G.TOL)


def test_pairs_run_width_generic_family():
    """(64, 32), T = 12, a pinned center, feat_norm_constant 2, the wide family: a minimum separation on each graph"""
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_pairs(eng, G.WIDE_T, noise, pins, com, restraints, PG.WIDE_PAIRS, family="wide", feat_norm_constant=2.0, trajectory=True,
                    energies=True)
    assert eng.kernel_family(0) == 64
    ref = PG.wide_reference()
    check_run(eng, cfg, got, ref, pins, f"pairs (64, 32) (k = {k})")
    torch.testing.assert_close(eng.last_pair_guidance()[1].cpu(), ref.E_pair[-1], rtol=G.TOL, atol=G.TOL)
    with pytest.raises(AssertionError):
        torch.testing.assert_close(got[2].cpu(), PG.wide_reference(False).fx, rtol=G.TOL, atol=G.TOL)


# 2. one step read back
def one_step(eng, n_t, noise, pins, com, restraints, pairs, ep=False, family="tuned", field=None, types=None):
    arr, parr, garr = arrays(eng, n_t)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family=family,
                     pairs=pairs, field=field, types=types)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1], ep_coord=ep, ep_feat=ep)
    out = tuple(t.cpu() for t in eng.last_guidance()) + tuple(t.cpu() for t in eng.last_pair_guidance())
    if family == "tuned":
        eng.set_train_input_grads(False)
    return out


def budget(got, r32, r64, leg):
    g0, grad, shift, en, g_pair, e_pair = got
    within_budget(en, r32.E[0], r64.E[0], f"{leg} E")
    within_budget(g0, r32.g0[0], r64.g0[0], f"{leg} g0")
    within_budget(grad, r32.grad[0], r64.grad[0], f"{leg} grad")
    within_budget(shift, r32.shift[0], r64.shift[0], f"{leg} shift")
    within_budget(g_pair, r32.g_pair[0], r64.g_pair[0], f"{leg} g_pair")
    within_budget(e_pair, r32.E_pair[0], r64.E_pair[0], f"{leg} E_pair")


@pytest.mark.parametrize("ep", [False, True])
def test_one_step_within_the_fp64_budget(ep):
    leg = "pairs ep" if ep else "pairs noise"
    cfg, sd, k, batch, noise, pins, com, restraints, pairs = PG.case()
    kw = dict(pairs=pairs, scale=G.GUIDE_SCALE, ep=ep, n_steps=1)
    r32 = PG.pairs_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, **kw)
    r64 = PG.pairs_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, double=True, **kw)
    eng = bound(engine_for(cfg, sd), batch)
    got = one_step(eng, T, noise, pins, com, restraints, pairs, ep=ep)
    budget(got, r32, r64, leg)
    ptr = batch.pharm_ptr.tolist()
    g_pair, e_pair = got[4], got[5]
    assert float(g_pair[ptr[1]:ptr[1] + 2].abs().max()) == 0        # the position-pinned centers: exact zeros
    assert float(g_pair[ptr[0]:ptr[1]].abs().max()) == 0 and float(g_pair[ptr[3]].abs().max()) == 0
    assert float(e_pair[0]) == 0 and float(e_pair[3]) == 0 and float(e_pair[1]) > 0


def test_shapes_one_step_and_repeatable():
    """graphs of 1, 2, 5, 3 and 64 centers: no pairs; rho == 0 between two pinned centers; the last center named; a graph without
    pair restraints between two with some; the cap of 256 restraints on the 64-center graph.  Bitwise equal on a second run."""
    cfg, sd, k, batch, noise, pins, com, pairs = PG.shapes_case()
    kw = dict(pairs=pairs, scale=G.GUIDE_SCALE, n_steps=1)
    r32 = PG.pairs_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, None, **kw)
    r64 = PG.pairs_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, None, double=True, **kw)
    st = r64.stats[0]
    assert st["lo_open"] > 0 and st["hi_open"] > 0
    eng = bound(engine_for(cfg, sd), batch)
    first = one_step(eng, T, noise, pins, com, None, pairs)
    budget(first, r32, r64, "pairs shapes")
    g_pair, e_pair = first[4], first[5]
    assert bool(torch.isfinite(g_pair).all()) and bool(torch.isfinite(e_pair).all())
    ptr = batch.pharm_ptr.tolist()
    assert float(e_pair[0]) == 0 and float(g_pair[0].abs().max()) == 0                  # one center: no pairs
    assert float(e_pair[1]) == 1.5 * 2.0 ** 2 and float(g_pair[1:3].abs().max()) == 0   # rho == 0: E = w lo^2, a zero gradient
    assert float(e_pair[3]) == 0 and float(g_pair[ptr[3]:ptr[4]].abs().max()) == 0      # no pair restraint on graph 3
    assert float(g_pair[ptr[3] - 1].abs().max()) > 0 and float(g_pair[ptr[5] - 1].abs().max()) > 0     # the last centers take theirs
    for g in (2, 4):                                    # per graph too: the budget above is set by the largest graph
        s = slice(ptr[g], ptr[g + 1])
        within_budget(g_pair[s], r32.g_pair[0][s], r64.g_pair[0][s], f"pairs shapes g_pair graph {g}")
        within_budget(e_pair[g:g + 1], r32.E_pair[0][g:g + 1], r64.E_pair[0][g:g + 1], f"pairs shapes E_pair graph {g}")
    again = one_step(eng, T, noise, pins, com, None, pairs)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


# 3. composition with a pocket field and type guidance
def test_one_step_with_field_and_types():
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    fkw, tkw = F.field_kwargs(fd), TG.types_kwargs(tg)
    eng = bound(engine_for(cfg, sd), batch)

    def step(pairs):
        arr, parr, garr = arrays(eng, T)
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned",
                         field=fkw, types=tkw, pairs=pairs)
        eng.guided_step(arr[0], parr[0], garr[0], noise[1])
        out = dict(zip(("g0", "grad", "shift", "E"), (t.cpu() for t in eng.last_guidance())), e3=eng.last_field_energies().cpu(),
                   e_type=eng.last_type_guidance()[3].cpu())
        if pairs is not None:
            out["g_pair"], out["e_pair"] = (t.cpu() for t in eng.last_pair_guidance())
        eng.set_train_input_grads(False)
        return out
    without, armed = step(None), step(PG.PAIRS)
    # the field's three components and E_type keep their bits; the total is the documented sum
    assert torch.equal(armed["e3"], without["e3"]) and torch.equal(armed["e_type"], without["e_type"])
    e3 = armed["e3"]
    assert torch.equal((((e3[:, 0] + e3[:, 1]) + e3[:, 2]) + armed["e_type"]) + armed["e_pair"], armed["E"])
    assert torch.equal(without["E"] + armed["e_pair"], armed["E"]) and torch.equal(without["g0"] + armed["g_pair"], armed["g0"])
    kw = dict(pairs=PG.PAIRS, scale=G.GUIDE_SCALE, n_steps=1)
    r32 = PG.pairs_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, fd, tg, **kw)
    r64 = PG.pairs_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, fd, tg, double=True, **kw)
    budget((armed["g0"], armed["grad"], armed["shift"], armed["E"], armed["g_pair"], armed["e_pair"]), r32, r64, "pairs + field + types")


# 4. inert armings
def test_inert_armings_are_the_run_without():
    cfg, sd, k, batch, noise, pins, com, restraints, pairs = PG.case()
    eng = bound(engine_for(cfg, sd), batch)
    mask = 0x1FFF                                       # every kernel class, the gradient classes included
    counts = lambda: ({k_: v[1] for k_, v in eng.profile_read().items()}, {k_: v[1] for k_, v in eng.profile_read_train().items()})
    eng.profile_enable(mask)
    try:
        counts()
        want = run_pairs(eng, T, noise, pins, com, restraints, None, trajectory=True, energies=True)
        n_want = counts()
        assert sum(n_want[0].values()) > 0
        with pytest.raises(pfa.PfError, match=ERR_STATE):
            eng.last_pair_guidance()
        eng.pairs_next(None)                            # ptr = NULL: armed, consumed by the next begin, inert
        got = run_pairs(eng, T, noise, pins, com, restraints, None, trajectory=True, energies=True)
        assert counts() == n_want
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        with pytest.raises(pfa.PfError, match=ERR_STATE):
            eng.last_pair_guidance()
        got = run_pairs(eng, T, noise, pins, com, restraints, [None, [], None, None, []], trajectory=True, energies=True)     # no restraint in any graph
        assert counts() == n_want
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        with pytest.raises(pfa.PfError, match=ERR_STATE):
            eng.last_pair_guidance()
    finally:
        eng.profile_enable(0)
    # all weights zero (the launch alone): zeros are added, the bits stay
    zero_w = [None if r is None else [(i, j, lo, hi, 0.0) for i, j, lo, hi, w in r] for r in pairs]
    got = run_pairs(eng, T, noise, pins, com, restraints, zero_w, trajectory=True, energies=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    g_pair, e_pair = eng.last_pair_guidance()
    assert float(g_pair.abs().max()) == 0 and float(e_pair.abs().max()) == 0
    # a run with pairs in between leaves nothing behind
    mid = run_pairs(eng, T, noise, pins, com, restraints, pairs, trajectory=True, energies=True)
    assert not torch.equal(mid[0], want[0])
    again = run_pairs(eng, T, noise, pins, com, restraints, None, trajectory=True, energies=True)
    for a, b in zip(again, want):
        assert torch.equal(a, b)
    # the step API equals the whole loop bitwise
    arr, parr, garr = arrays(eng, T)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned", pairs=pairs)
    for i in range(T):
        eng.guided_step(arr[i], parr[i], garr[i], noise[1 + i])
    x1, h1 = eng.sample_end()
    eng.set_train_input_grads(False)
    assert torch.equal(x1, mid[0]) and torch.equal(h1, mid[1])
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


# 5. arming, state and argument errors
def test_arming_state_and_argument_errors():
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()     # 3 and 5 centers
    eng = bound(engine_for(cfg, sd), batch)
    eng.set_train_family("wide")
    arr, parr, garr = arrays(eng, G.WIDE_T)
    good = PG.WIDE_PAIRS

    def first_step(**kw):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, **kw)
        eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    first_step()
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_pair_guidance()
    plain_g0 = eng.last_guidance()[0].clone()
    first_step(pairs=good)
    want_pair = [t.clone() for t in eng.last_pair_guidance()]
    assert float(want_pair[1].abs().max()) > 0 and not torch.equal(eng.last_guidance()[0], plain_g0)
    # each refusal is PF_ERR_ARG with a message, and the arming made before it still takes effect in the next run
    one = lambda *row: [[row], None]
    refusals = {"twice": one(1, 1, 1.0, 2.0, 1.0), "names center 3": one(0, 3, 1.0, 2.0, 1.0), "names center 5": [None, [(5, None, 1.0, 2.0, 1.0)]],
                "hi must be >= lo": one(0, 1, 3.0, 2.0, 1.0), "hi must be": one(0, 1, 0.0, -INF, 1.0), "lo must be finite": one(0, 1, float("nan"), 2.0, 1.0),
                "lo must be": one(0, 1, INF, INF, 1.0), "weight": one(0, 1, 1.0, 2.0, -1.0), "the weight": one(0, 1, 1.0, 2.0, INF),
                "at most 256": [[(None, None, 1.0, INF, 0.0)] * 257, None]}
    for what, bad in refusals.items():
        eng.pairs_next(good)
        with pytest.raises(pfa.PfError, match=ERR_ARG + ".*pf_guide_pairs_next.*" + what):
            eng.pairs_next(bad)
        first_step()                                    # (no pairs= here: the arming above is the one the begin consumes)
        for a, b in zip(eng.last_pair_guidance(), want_pair):
            assert torch.equal(a, b)
    import numpy as np                                  # a non-monotone ptr cannot be written as lists: the C entry point itself
    ptr = np.asarray([0, 2, 1], dtype=np.int32)
    col = np.zeros(2, dtype=np.int32)
    val = np.ones(2, dtype=np.float32)
    rc = eng.lib.pf_guide_pairs_next(eng._h, ptr.ctypes.data, col.ctypes.data, (col + 1).ctypes.data, val.ctypes.data, val.ctypes.data, val.ctypes.data)
    assert rc == -1
    # a plain begin while armed is PF_ERR_STATE and drops the arming; the run in progress goes on
    eng.sample_begin(noise[0], init_pharm_com=com)
    eng.denoise_step(arr[0], noise[1])
    state = [t.clone() for t in eng.sample_frame()]
    eng.pairs_next(good)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pair guidance"):
        eng.sample_begin(noise[0], init_pharm_com=com)
    assert all(torch.equal(a, b) for a, b in zip(state, eng.sample_frame()))
    eng.denoise_step(arr[1], noise[2])
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)      # dropped: the pinned begin is accepted
    eng.pairs_next(good)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pair guidance"):
        eng.sample(arr, 2, noise, init_pharm_com=com)
    first_step()                                        # ... and the guided run behind it has no pairs
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_pair_guidance()
    assert torch.equal(eng.last_guidance()[0], plain_g0)
    # a bind drops it silently
    eng.pairs_next(good)
    bound(eng, batch)
    first_step()
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_pair_guidance()
    assert torch.equal(eng.last_guidance()[0], plain_g0)
    # it ends with its run; an arming inside the run is for the NEXT run and leaves this one as it is
    first_step(pairs=good)
    eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    second = [t.clone() for t in eng.last_pair_guidance()] + [eng.last_guidance()[0].clone()]
    first_step(pairs=good)
    eng.pairs_next(None)
    eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    for a, b in zip(list(eng.last_pair_guidance()) + [eng.last_guidance()[0]], second):
        assert torch.equal(a, b)
    first_step()                                        # consumes the inert arming
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_pair_guidance()
    # the Python layer
    with pytest.raises(ValueError, match="multistep"):
        eng.sample(None, 2, noise, ms_coef_arr=[None, None], pairs=good)
    with pytest.raises(ValueError, match="one entry per graph"):
        eng.pairs_next([None])
    with pytest.raises(ValueError, match="is \\(i, j, lo, hi, weight\\)"):
        eng.pairs_next([[(0, 1, 2.0, 3.0)], None])
    assert eng.xchg_timeouts() == 0


# 6. model level
def test_model_level_min_separation(tmp_path):
    """PharmacophoreDiff.sample(min_separation=d) on two pockets with injected noise is sample(pair_restraints=[[(None, None, d, inf,
    w)], ...]) bit for bit and differs from the call without either; the samples carry analysis.pair_restraint_energy of their
    final centers, which scores.tsv writes"""
    from test_gpu_api import graph_from, make_model
    import generate_pharmacophores as cli
    n_t = 12
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[3, 5, 4], [4, 3, 6]]
    gen = torch.Generator().manual_seed(11)
    nz = [torch.randn(n_t + 1, 12, 9, generator=gen), torch.randn(n_t + 1, 13, 9, generator=gen)]
    kw = dict(max_batch_size=3, lanes=2, noise=nz, guide_family="tuned")
    d, w = 2000.0, 1e-3      # (this fixture's seeded random weights throw the centers hundreds of angstroms apart: a separation that reaches them)
    sep = m.sample(pockets, n_pharms, min_separation=d, separation_weight=w, **kw)
    rows = m.sample(pockets, n_pharms, pair_restraints=[[(None, None, d, INF, w)]] * 2, **kw)
    plain = m.sample(pockets, n_pharms, **kw)
    assert [[p.n_ph_centers for p in o] for o in sep] == n_pharms
    for a, b in zip([p for o in sep for p in o], [p for o in rows for p in o]):
        assert torch.equal(a.ph_coords, b.ph_coords) and torch.equal(a.g.pharm_h0, b.g.pharm_h0)
        assert a.pair_energy == b.pair_energy and a.pair_violations == b.pair_violations
    assert any(not torch.equal(a.ph_coords, b.ph_coords) for a, b in zip(sep[0] + sep[1], plain[0] + plain[1]))
    assert all(p.pair_energy is None for o in plain for p in o)
    flat = [p for o in sep for p in o]
    for p in flat:
        e, v = pfa.analysis.pair_restraint_energy(p.ph_coords, [(None, None, d, INF, w)])
        assert p.pair_energy == e and p.pair_violations == v
    # mixed: pair restraints on pocket 0 only -- pocket 1's batch runs the default path's bits; a named center composes with pins
    c0 = pockets[0].prot_x.mean(dim=0).float()
    mixed = m.sample(pockets, n_pharms, pair_restraints=[[(0, 2, 5.0, 7.0, 0.01)], None],
                     pinned=[(c0[None], torch.tensor([2]), None), None], **kw)
    pinned_only = m.sample(pockets, n_pharms, pinned=[(c0[None], torch.tensor([2]), None), None], **kw)
    for a, b in zip(mixed[1], pinned_only[1]):
        assert torch.equal(a.ph_coords, b.ph_coords) and a.pair_energy is None
    assert any(not torch.equal(a.ph_coords, b.ph_coords) for a, b in zip(mixed[0], pinned_only[0]))
    assert all(torch.equal(p.ph_coords[0], c0) for p in mixed[0])
    with pytest.raises(ValueError, match="resampling"):
        m.sample(pockets, n_pharms, min_separation=d, pinned=[(c0[None], torch.tensor([2]), None), None], pin_resamples=2, **kw)
    with pytest.raises(ValueError, match="multistep"):
        m.sample(pockets, n_pharms, min_separation=d, sample_steps=4, sampler="multistep", **kw)
    with pytest.raises(ValueError, match="names center 3 but sizes"):
        m.sample(pockets, n_pharms, pair_restraints=[[(0, 3, 5.0, 7.0, 2.0)], None], **kw)
    # scores.tsv carries the number
    from types import SimpleNamespace
    sc = SimpleNamespace(n_centers=3, total=1.0, per_center=0.5, pos=0.25, feat=0.25, position_error=0.1, type_accuracy=1.0)
    cli.write_scores(tmp_path / "scores.tsv", range(len(flat)), [sc] * len(flat), None, None, [p.pair_energy for p in flat])
    tsv = [l.split("\t") for l in (tmp_path / "scores.tsv").read_text().splitlines()]
    assert tsv[0][-1] == "pair_energy"
    for row, p in zip(tsv[1:], flat):
        assert row[-1] == f"{p.pair_energy:.6g}"
