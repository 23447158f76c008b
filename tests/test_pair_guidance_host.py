"""Host side of pair guidance (pf_guide_pairs_next): the conditions the GPU tests (test_gpu_pair_guidance.py) put on their own
inputs, checked on the reference alone (tests/pair_guidance_ref.py) -- without pairs it is guidance_ref.guided_reference bit for
bit; g_pair is autograd of the fp64 energy with the pinned rows zero; in fp32 and fp64 the composition agrees with itself within
the trajectory tolerance; the references that ignore the arming or the pin rule miss the frames by more than ten times that; the
lower hinge is open for some covered pairs of the first step and closed for others, the upper one opens in some step --, the
parser, analysis.pair_restraint_energy against a brute-force loop, and the argument rules of the model and the two command lines.
The argument validation of the C ABI is test_pairs_host.py's stand-alone checker.  No GPU.

Recorded (fp32 composition, T = 24, guide_scale 4, minimum separations at weight 0.125): fp32 against fp64 over all frames 3.2e-6
(noise) / 3.6e-5 (endpoint); the frames miss the run without pairs by 1.90 and the one without the pin rule by 3.67 (noise), 1.53 /
0.54 (endpoint); of the 49 covered pairs the lower hinge is open for 13 in step 0 and for 4 to 14 later, the upper one in step 7.
With the minimum separations at weight 1 the endpoint composition ends 1.6 from its fp64 self: that is why they weigh 0.125."""
import math
import os
import sys

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import generate_pharmacophores as cli  # noqa: E402
import guidance_ref as G  # noqa: E402
import pair_guidance_ref as PG  # noqa: E402
import type_guidance_ref as TG  # noqa: E402

TOL = G.TOL
INF = math.inf


# ---- the reference, and the conditions the GPU tests rest on ----------------------------------------------------------------
@pytest.mark.parametrize("ep", [False, True])
def test_without_pairs_the_reference_is_guided_reference(ep):
    cfg, sd, k, batch, noise, pins, com, restraints, pairs = PG.case()
    want = G.reference(ep)
    for kw in (dict(pairs=None), dict(pairs=pairs, use_pairs=False), dict(pairs=[None] * 5)):
        got = PG.pairs_reference(sd, cfg, batch, PG.T, PG.PREC, noise, *pins, com, restraints, scale=PG.GUIDE_SCALE, ep=ep, **kw)
        for name in ("x0", "h0", "fx", "fh", "E", "g0", "grad", "shift"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
        assert got.E_pair.shape[0] == 0 and got.g_pair.shape[0] == 0


def test_with_a_field_and_types_and_no_pairs_the_reference_is_types_reference():
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    kw = dict(scale=TG.GUIDE_SCALE, n_steps=2)
    want = TG.types_reference(sd, cfg, batch, TG.T, TG.PREC, noise, *pins, com, restraints, fd, tg, **kw)
    got = PG.pairs_reference(sd, cfg, batch, TG.T, TG.PREC, noise, *pins, com, restraints, fd, tg, **kw)
    for name in ("fx", "fh", "E", "g0", "grad", "shift", "E3", "E_type", "g0_h", "grad_h", "shift_h"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name


def test_the_case_holds_every_kind_of_graph_the_gpu_tests_rely_on():
    cfg, sd, k, batch, noise, pins, com, restraints, pairs = PG.case()
    assert batch.pharm_ptr.diff().tolist() == [3, 8, 5, 1, 6]
    assert [len(r or []) for r in pairs] == [0, 2, 2, 1, 1]
    ptr = batch.pharm_ptr.tolist()
    flags = pins[0]
    assert int(flags[ptr[1]]) & 1 and int(flags[ptr[1] + 1]) & 1 and not bool((flags[ptr[1] + 2:ptr[2]] & 1).any())
    assert pairs[1][1][:2] == (0, 5)                    # a pinned - free upper bound
    ref = PG.reference()
    # the pinned centers take no pair gradient, their free partners do; the single-center graph and graph 0: exact zeros
    assert float(ref.g_pair[:, ptr[1]:ptr[1] + 2].abs().max()) == 0
    assert float(ref.g_pair[0, ptr[1] + 2:ptr[2]].abs().max()) > 0
    assert float(ref.E_pair[:, 0].abs().max()) == 0 and float(ref.E_pair[:, 3].abs().max()) == 0
    assert float(ref.g_pair[:, ptr[0]:ptr[1]].abs().max()) == 0 and float(ref.g_pair[:, ptr[3]].abs().max()) == 0
    assert bool((ref.E_pair[0, [1, 2, 4]] > 0).all()) and bool((ref.E_pair[:, 1] > 0).all())
    # the two pinned centers of graph 1 stand closer than 4: their pair counts in E although neither moves
    d01 = float((pins[1][ptr[1]] - pins[1][ptr[1] + 1]).norm())
    assert d01 < 4.0
    # E is the documented sum: the restraints' energy, then the pairs'
    plain = G.reference()
    assert torch.equal(ref.E[0], plain.E[0] + ref.E_pair[0]) and torch.equal(ref.g0[0], plain.g0[0] + ref.g_pair[0])


def test_hinges_open_and_close_over_the_run():
    ref = PG.reference()
    lo = [s["lo_open"] for s in ref.stats]
    hi = [i for i, s in enumerate(ref.stats) if s["hi_open"]]
    print("covered pairs", ref.stats[0]["covered"], "lower hinge open per step", lo, "upper hinge open in steps", hi)
    assert ref.stats[0]["covered"] == 49
    assert 0 < lo[0] < 49                               # the first step: open for some covered pairs, closed for others
    assert hi                                           # the upper hinge opens in at least one step


@pytest.mark.parametrize("leg", ["noise", "ep"])
def test_fp32_against_fp64_composition(leg):
    r32, r64 = PG.reference(leg == "ep"), PG.reference(leg == "ep", True)
    d = {n: float((getattr(r32, n).double() - getattr(r64, n)).abs().max()) for n in ("x0", "h0", "fx", "fh")}
    dE = float(((r32.E.double() - r64.E).abs() / r64.E.abs().clamp(min=1.0)).max())
    dP = float(((r32.E_pair.double() - r64.E_pair).abs() / r64.E_pair.abs().clamp(min=1.0)).max())
    print(f"{leg}: fp32 against fp64 composition {d}, energies {dE:.3g} / pair energies {dP:.3g} relative")
    assert max(d.values()) <= TOL and dE <= TOL and dP <= TOL


@pytest.mark.parametrize("leg", ["noise", "ep"])
def test_references_that_drop_the_pairs_or_the_pin_rule_miss(leg):
    """the teeth of the GPU test: at least 10 x the tolerance over the trajectory frames"""
    ep = leg == "ep"
    ref = PG.reference(ep)
    for name, other in (("the pairs", PG.reference(ep, False, False)), ("the pin rule", PG.reference(ep, False, True, False))):
        miss = float((ref.fx - other.fx).abs().max())
        print(f"{leg}: without {name} the frames are off by {miss:.3g}")
        assert miss >= 10 * TOL
    w, wu = PG.wide_reference(), PG.wide_reference(False)
    assert float((w.fx - wu.fx).abs().max()) >= 10 * TOL


def test_the_shapes_case_holds_its_shapes():
    cfg, sd, k, batch, noise, pins, com, pairs = PG.shapes_case()
    assert batch.pharm_ptr.diff().tolist() == [1, 2, 5, 3, 64]
    assert [len(r or []) for r in pairs] == [1, 1, 2, 0, 256]
    assert torch.equal(pins[1][1], pins[1][2]) and pins[0][1:3].tolist() == [1, 1]      # rho == 0 between two pinned centers
    assert pairs[2][0][0] == 4 and pairs[2][1][1] == 4 and (62, 63) == pairs[4][1][:2]   # the last centers are named
    forms = {(i is None, j is None) for i, j, _, _, _ in pairs[4]}
    assert forms == {(True, True), (False, False), (False, True), (True, False)}
    assert all(i != j or i is None for i, j, _, _, _ in pairs[4])
    ptr = batch.pharm_ptr.tolist()
    y = torch.randn(75, 3, generator=torch.Generator().manual_seed(0)).double() * 3
    g, E, st = PG.pair_terms(PG.make_pairs(pairs), batch.pharm_ptr, y, (pins[0] & 1) != 0, pins[1])
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(E).all())
    assert float(E[0]) == 0 and float(E[3]) == 0 and float(g[ptr[3]:ptr[4]].abs().max()) == 0
    assert float(E[1]) == 1.5 * 2.0 ** 2 and float(g[ptr[1]:ptr[2]].abs().max()) == 0     # E = w lo^2, no gradient


# ---- the energy and its gradient ------------------------------------------------------------------------------------------------
def _energy64(pairs, y, px, pin_x):
    """sum over restraints and covered pairs of w (max(0, lo - rho)^2 + max(0, rho - hi)^2): a plain loop, differentiable in y"""
    yy = torch.where(px[:, None], pin_x, y)
    n = y.shape[0]
    tot = torch.zeros((), dtype=torch.float64)
    for i, j, lo, hi, w in pairs:
        wild = lambda c: c is None or c == "*" or c < 0
        for a in range(n):
            for b in range(a + 1, n):
                if wild(i) and wild(j):
                    cov = True
                elif wild(i) or wild(j):
                    cov = (j if wild(i) else i) in (a, b)
                else:
                    cov = {i, j} == {a, b}
                if not cov:
                    continue
                rho = (yy[a] - yy[b]).norm()
                tot = tot + w * (torch.clamp(lo - rho, min=0) ** 2 + (torch.clamp(rho - hi, min=0) ** 2 if hi < INF else 0.0))
    return tot


def test_g_pair_is_autograd_of_the_fp64_energy_with_pinned_rows_zero():
    gen = torch.Generator().manual_seed(9)
    n = 7
    ptr = torch.tensor([0, n])
    y = (2.5 * torch.randn(n, 3, generator=gen)).double().requires_grad_(True)
    px = torch.tensor([True, False, False, True, False, False, False])
    pin_x = (2.0 * torch.randn(n, 3, generator=gen)).double()
    pairs = [(None, None, 4.0, INF, 1.0), (0, 5, 0.0, 2.0, 1.5), (1, 3, 5.0, 7.0, 2.0), (2, None, 3.0, 3.5, 0.5), (None, 6, 1.0, INF, 0.25),
             (4, 1, 0.5, 1.0, 3.0)]
    e = _energy64(pairs, y, px, pin_x)
    (want,) = torch.autograd.grad(e, y)
    g, E, st = PG.pair_terms(PG.make_pairs([pairs]), ptr, y.detach(), px, pin_x)
    assert st["lo_open"] > 0 and st["hi_open"] > 0 and st["covered"] == 21 + 1 + 1 + 6 + 6 + 1
    assert abs(float(E[0]) - float(e.detach())) <= 1e-12 * float(e.detach())
    assert float(want[px].abs().max()) == 0 and float(g[px].abs().max()) == 0            # a pinned center's point is a constant
    assert float((g - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # without the pin rule the pinned centers stand where the network puts them and take their gradient
    g2, E2, _ = PG.pair_terms(PG.make_pairs([pairs]), ptr, y.detach(), px, pin_x, pin_rule=False)
    e2 = _energy64(pairs, y, torch.zeros(n, dtype=torch.bool), pin_x)
    (want2,) = torch.autograd.grad(e2, y)
    assert float((g2 - want2).abs().max()) <= 1e-12 * float(want2.abs().max()) and float(g2[px].abs().max()) > 0
    # antisymmetry: a free pair's two halves cancel exactly
    g3, _, _ = PG.pair_terms(PG.make_pairs([[(1, 2, 9.0, INF, 1.0)]]), ptr, y.detach().float(), px, pin_x.float())
    assert torch.equal(g3[1], -g3[2]) and float(g3[1].abs().max()) > 0
    # fewer than two centers: exact zeros
    g1, E1, _ = PG.pair_terms(PG.make_pairs([[(None, None, 4.0, INF, 1.0)]]), torch.tensor([0, 1]), y.detach()[:1])
    assert float(g1.abs().max()) == 0 and float(E1[0]) == 0


def test_pair_restraint_energy_against_a_brute_force_loop():
    gen = torch.Generator().manual_seed(4)
    x = (2.0 * torch.randn(6, 3, generator=gen))
    pairs = [(None, None, 3.0, INF, 1.0), (0, 5, 0.0, 2.0, 1.5), ("*", 2, 1.0, 4.0, 0.5), (3, -1, 2.0, 2.0, 2.0)]
    e, v = pfa.analysis.pair_restraint_energy(x, pairs)
    none = torch.zeros(6, dtype=torch.bool)
    want = float(_energy64([(i if isinstance(i, int) else None, j if isinstance(j, int) else None, lo, hi, w) for i, j, lo, hi, w in pairs],
                           x.double(), none, x.double()))
    assert abs(e - want) <= 1e-12 * want and e > 0
    count = 0
    for i, j, lo, hi, w in pairs:
        i = None if i in (None, "*") or i < 0 else i
        j = None if j in (None, "*") or j < 0 else j
        for a in range(6):
            for b in range(a + 1, 6):
                cov = (i is None and j is None) or ((i is None) != (j is None) and (i if j is None else j) in (a, b)) or {i, j} == {a, b}
                rho = float((x[a].double() - x[b].double()).norm())
                count += int(cov and (rho < lo or rho > hi))
    assert v == count and v > 0
    assert pfa.analysis.pair_restraint_energy(x[:1], pairs[:1]) == (0.0, 0) and pfa.analysis.pair_restraint_energy(x, None) == (0.0, 0)
    with pytest.raises(ValueError, match="names center 6"):
        pfa.analysis.pair_restraint_energy(x, [(0, 6, 0.0, 1.0, 1.0)])
    # the reference's final energy is the same number
    cfg, sd, k, batch, noise, pins, com, restraints, prs = PG.case()
    ref = PG.reference()
    ptr = batch.pharm_ptr.tolist()
    fe = PG.final_pair_energy(prs, batch, ref.x0)
    for g in range(5):
        e, _ = pfa.analysis.pair_restraint_energy(ref.x0[ptr[g]:ptr[g + 1]], prs[g])
        assert abs(e - float(fe[g])) <= 1e-9 * max(1.0, e)


# ---- the parser ----------------------------------------------------------------------------------------------------------------
def test_parse_pair_restraints():
    from pharmacoforge_amd import pocket_io as P
    text = """# donor and aromatic center five to seven apart
pair 0 3 5 7 2.0
pair * * 3 inf 1   # no two centers closer than 3

pair 1 * 0 6.5 0.5
pair * 2 1e0 1 0
"""
    rows = P.parse_pair_restraints(text)
    assert rows == [(0, 3, 5.0, 7.0, 2.0), (None, None, 3.0, INF, 1.0), (1, None, 0.0, 6.5, 0.5), (None, 2, 1.0, 1.0, 0.0)]
    # a round trip through the text form
    again = "\n".join("pair %s %s %r %s %r" % ("*" if i is None else i, "*" if j is None else j, lo, "inf" if hi == INF else repr(hi), w)
                      for i, j, lo, hi, w in rows)
    assert P.parse_pair_restraints(again) == rows
    assert P.parse_pair_restraints("") == []
    for bad, line, what in (("attract 0 0 0 1 1", 1, "starts with 'pair'"), ("\npair 0 1 2 3", 2, "got 5 fields"),
                            ("pair 0 1 2 3 1 1", 1, "got 7 fields"), ("pair a 1 2 3 1", 1, "index or"), ("pair -1 1 2 3 1", 1, "must not be negative"),
                            ("pair 2 2 2 3 1", 1, "two different centers"), ("pair 0 1 x 3 1", 1, "must be numbers"),
                            ("pair 0 1 nan 3 1", 1, "LO must be finite"), ("pair 0 1 -1 3 1", 1, "LO must be finite"),
                            ("pair 0 1 inf inf 1", 1, "LO must be finite"), ("# c\n\npair 0 1 4 3 1", 3, "HI must not be below LO"),
                            ("pair 0 1 0 -inf 1", 1, "HI must not be below LO"), ("pair 0 1 0 nan 1", 1, "HI must not be below LO"),
                            ("pair 0 1 0 1 -1", 1, "WEIGHT"), ("pair 0 1 0 1 inf", 1, "WEIGHT")):
        with pytest.raises(ValueError, match=f"line {line}.*{what}"):
            P.parse_pair_restraints(bad, source="file.txt")
    with pytest.raises(ValueError, match="attract"):    # parse_restraints is what it was: it does not read pair lines
        P.parse_restraints("pair 0 1 2 3 1")


# ---- the argument rules (no device work is reached) -----------------------------------------------------------------------------
def _model_and_graph():
    from test_host_logic import make_model
    m = make_model(20)
    b = O.synthetic_batch([1], 20, 3, O.DynamicsConfig())
    g = pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, torch.zeros(3, 3), torch.zeros(3, 6))
    return m, g


def test_run_spec_rules():
    m, g = _model_and_graph()
    pr = [[(0, 2, 5.0, 7.0, 1.0)]]
    spec = m._run_spec(pins=False, guided=True, min_separation=3.0)
    assert spec.separation == (3.0, 1.0) and spec.guided
    assert m._run_spec(pins=False, guided=True, min_separation=3.0, separation_weight=0.5).separation == (3.0, 0.5)
    assert m._run_spec(pins=False, guided=False).separation is None
    # what a batch is armed with: its pair restraints, the minimum separation's row behind them on every graph
    assert spec.pairs_arg(None, 2) == [[(None, None, 3.0, INF, 1.0)]] * 2
    assert spec.pairs_arg([pr[0], None], 2) == [[(0, 2, 5.0, 7.0, 1.0), (None, None, 3.0, INF, 1.0)], [(None, None, 3.0, INF, 1.0)]]
    plain = m._run_spec(pins=False, guided=True)
    assert plain.pairs_arg(None, 2) is None and plain.pairs_arg([pr[0], None], 2) == [pr[0], None]
    # a minimum separation makes every batch guided, like a pocket field; pair restraints where there is one
    assert m._guided(None, None, None, None, 3.0) and m._guided(None, None, None, pr) and not m._guided(None, None, None, [None], None)
    # composes with pins, restraints, a pocket field, type guidance, seeds, first-order few-step sampling and both families
    for kw in (dict(pins=True, pinned=True), dict(pins=False, pocket_field=pfa.PocketField()), dict(pins=False, typed=True),
               dict(pins=False, sample_steps=4, sampler="ddim"), dict(pins=False, sample_steps=4),
               dict(pins=False, seeds=[1], seed_level=5), dict(pins=False, guide_family="wide")):
        assert m._run_spec(guided=True, min_separation=2.0, **kw).separation == (2.0, 1.0)
    for kw in (dict(pair_restraints=pr), dict(min_separation=3.0)):
        with pytest.raises(ValueError, match="resampling"):
            m.sample([g], [[4]], pin_resamples=2, **kw)
        with pytest.raises(ValueError, match="multistep"):
            m.sample([g], [[4]], sample_steps=4, sampler="multistep", **kw)
        with pytest.raises(ValueError, match="multistep"):
            m.sample_given_receptor(g, noise=torch.zeros(1, 3, 9), sample_steps=4, sampler="multistep", **kw)
    for bad, what in ((-1.0, "min_separation"), (INF, "min_separation"), (float("nan"), "min_separation")):
        with pytest.raises(ValueError, match=what):
            m.sample([g], [[4]], min_separation=bad)
    for bad in (-1.0, INF, float("nan")):
        with pytest.raises(ValueError, match="separation_weight"):
            m.sample([g], [[4]], min_separation=3.0, separation_weight=bad)
    with pytest.raises(ValueError, match="2 entries for 1 pockets"):
        m.sample([g], [[4]], pair_restraints=pr * 2)
    with pytest.raises(ValueError, match="names center 4 but sizes"):     # an index a requested size does not have
        m.sample([g], [[4, 5]], pair_restraints=[[(0, 4, 1.0, 2.0, 1.0)]])
    with pytest.raises(ValueError, match="names center 3 but sizes"):
        m.sample_given_receptor(g, pair_restraints=[[(3, None, 1.0, 2.0, 1.0)]])
    for row, what in (((1, 1, 1.0, 2.0, 1.0), "two different centers"), ((0, 1, 3.0, 2.0, 1.0), "lo <= hi"), ((0, 1, -1.0, 2.0, 1.0), "lo <= hi"),
                      ((0, 1, INF, INF, 1.0), "lo finite"), ((0, 1, 1.0, float("nan"), 1.0), "lo <= hi"), ((0, 1, 1.0, 2.0, -1.0), "weight"),
                      ((0, 1, 1.0, 2.0, INF), "weight"), ((0, 1, 1.0, 2.0), "is \\(i, j, lo, hi, weight\\)")):
        with pytest.raises(ValueError, match=what):
            m.sample([g], [[4]], pair_restraints=[[row]])
    with pytest.raises(ValueError, match="at most 256"):
        m.sample([g], [[4]], pair_restraints=[[(0, 1, 1.0, 2.0, 1.0)] * 256], min_separation=3.0)
    with pytest.raises(ValueError, match="at most 256"):
        m.sample([g], [[4]], pair_restraints=[[(0, 1, 1.0, 2.0, 1.0)] * 257])
    # wildcards in every spelling; an empty list is no restraint
    assert m._pair_restraints([[("*", -1, 1, 2, 1), (None, 2, 0, INF, 0)]], 1, "pockets") == [[(None, None, 1.0, 2.0, 1.0), (None, 2, 0.0, INF, 0.0)]]
    assert m._pair_restraints([[]], 1, "pockets") is None and m._pair_restraints(None, 1, "pockets") is None


def test_the_command_lines(tmp_path):
    f = tmp_path / "pairs.txt"
    f.write_text("pair 0 3 5 7 2\npair * * 3 inf 1\n")
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]
    a = cli.parse_arguments(base + ["--pair_restraints", str(f)])
    assert a.pair_restraint_list == [(0, 3, 5.0, 7.0, 2.0), (None, None, 3.0, INF, 1.0)]
    assert (a.min_separation, a.separation_weight, a.guide_family) == (None, 1.0, "wide")
    a = cli.parse_arguments(base + ["--min_separation", "3", "--separation_weight", "0.5", "--guide_family", "tuned", "--guide_scale", "2",
                                    "--sample_steps", "4", "--sampler", "ddim"])
    assert (a.min_separation, a.separation_weight, a.guide_family, a.guide_scale, a.pair_restraint_list) == (3.0, 0.5, "tuned", 2.0, None)
    assert cli.parse_arguments(base).pair_restraint_list is None and cli.parse_arguments(base).min_separation is None
    pin = tmp_path / "pin.xyz"
    pin.write_text("1\nC 0 0 0\n")
    for argv in (["--separation_weight", "2"], ["--min_separation", "-1"], ["--min_separation", "inf"],
                 ["--min_separation", "3", "--separation_weight", "nan"], ["--guide_scale", "2"],
                 ["--min_separation", "3", "--sample_steps", "4", "--sampler", "multistep"],
                 ["--pair_restraints", str(f), "--sample_steps", "4", "--sampler", "multistep"],
                 ["--min_separation", "3", "--pinned_centers", str(pin), "--pin_resamples", "2"],
                 ["--pair_restraints", str(f), "--pinned_centers", str(pin), "--pin_resamples", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(base + argv)
    with pytest.raises(ValueError, match="do not reach center 3"):
        cli.parse_arguments(base + ["--pair_restraints", str(f), "--samples_per_pocket", "2", "--pharm_sizes", "3", "5"])
    # scores.tsv gains the pair energy, behind the type energy
    from types import SimpleNamespace
    sc = SimpleNamespace(n_centers=3, total=1.0, per_center=0.5, pos=0.25, feat=0.25, position_error=0.1, type_accuracy=1.0)
    cli.write_scores(tmp_path / "scores.tsv", [0], [sc], None, None, [2.5])
    rows = [l.split("\t") for l in (tmp_path / "scores.tsv").read_text().splitlines()]
    assert rows[0][-1] == "pair_energy" and rows[1][-1] == "2.5" and len(rows[0]) == 9
    cli.write_scores(tmp_path / "scores.tsv", [0], [sc], [(2.0, 1)], [1.25], [2.5])
    assert (tmp_path / "scores.tsv").read_text().splitlines()[0].split("\t")[-4:] == ["clash_energy", "clashes", "type_energy", "pair_energy"]
    import test as tcli
    tb = ["--model_dir", "run"]
    a = tcli.parse_arguments(tb + ["--pair_restraints", str(f), "--min_separation", "2.5", "--guide_scale", "2"])
    assert len(a.pair_restraint_list) == 2 and (a.min_separation, a.separation_weight) == (2.5, 1.0) and a.pocket_field is None
    a = tcli.parse_arguments(tb)
    assert a.pair_restraint_list is None and a.min_separation is None
    for argv in (["--separation_weight", "2"], ["--min_separation", "-1"], ["--min_separation", "3", "--separation_weight", "inf"],
                 ["--min_separation", "3", "--sample_steps", "4", "--sampler", "multistep"],
                 ["--pair_restraints", str(f), "--pharm_sizes", "3", "--samples_per_pocket", "1"]):
        with pytest.raises(ValueError):
            tcli.parse_arguments(tb + argv)
