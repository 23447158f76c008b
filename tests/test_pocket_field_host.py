"""Host side of the pocket field (pf_guide_field_next): the conditions the GPU tests (test_gpu_pocket_field.py) put on their own
inputs, checked on the reference alone (tests/pocket_field_ref.py) -- without a field it is guidance_ref.guided_reference bit for
bit; in fp32 and in fp64 it agrees with itself within 5e-4 (DESIGN 4.15's demand); the field lowers the final clash and
complementarity energies on every graph; a reference that drops the field misses the guided frames by far more than the
tolerance --, the closed-form gradient against finite differences of the energy, the zero of a matched center, the tables, and the
argument rules of the model and the two command lines.  The argument validation of the C ABI is test_field_host.py's stand-alone
checker.  No GPU."""
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
import pocket_field_ref as F  # noqa: E402

TOL = G.TOL


# ---- the reference, and the conditions the GPU tests rest on ----------------------------------------------------------------
@pytest.mark.parametrize("ep", [False, True])
def test_without_a_field_the_reference_is_guided_reference(ep):
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    fd = F.case()[-1]
    want = G.reference(ep)
    for kw in (dict(field=None), dict(field=fd, use_field=False)):
        got = F.field_reference(sd, cfg, batch, G.T, G.PREC, noise, *pins, com, restraints, scale=G.GUIDE_SCALE, ep=ep, **kw)
        for name in ("x0", "h0", "fx", "fh", "E", "g0", "grad", "shift"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
        assert got.E3.shape[0] == 0
    un = F.field_reference(sd, cfg, batch, G.T, G.PREC, noise, *pins, com, None, None, scale=G.GUIDE_SCALE, ep=ep)
    assert torch.equal(un.fx, G.reference(ep, False, False).fx)


def test_the_case_holds_every_kind_of_graph_the_gpu_tests_rely_on():
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    assert batch.prot_ptr.diff().tolist() == [48, 300, 40, 64, 32] and batch.pharm_ptr.diff().tolist() == [3, 8, 5, 1, 6]
    assert [b - a for a, b in zip(fd.ph_ptr, fd.ph_ptr[1:])] == [0, 70, 5, 1, 3]
    assert [bool(r) for r in restraints] == [False, False, True, False, False]
    assert bool((fd.atom_r == 0).any()) and bool((fd.atom_r == 2.0).any())
    assert bool((pins[0][3:11] != 0).any())             # graph 1 has pinned centers
    match, dist = F.tables()
    u3 = fd.ph_type[fd.ph_ptr[3]:fd.ph_ptr[4]]
    assert sum(bool(match[t][u3].any()) for t in range(6)) < 6          # graph 3: some type has an empty set
    ref = F.reference()
    e3 = ref.E3
    assert bool((e3[:, 0, 2] == 0).all())               # no feature: exact zeros
    assert bool((e3[:, 2] > 0).any(dim=0).all())         # graph 2: all three terms act
    assert bool((e3[:, :, 1] > 0).any(dim=0).all())      # the clash term acts in every graph
    assert torch.equal((e3[..., 0] + e3[..., 1]) + e3[..., 2], ref.E)


@pytest.mark.parametrize("leg", ["noise", "ep", "wide"])
def test_fp32_against_fp64_composition(leg):
    """5e-4 on x_0, h_0 and all frames (4.15's demand); measured 2.9e-4 (noise), 9.7e-7 (endpoint)"""
    if leg == "wide":
        cfg, sd, k, batch, noise, pins, com, restraints, fd = F.wide_case()
        r32 = F.wide_reference()
        r64 = F.field_reference(sd, cfg, batch, G.WIDE_T, G.PREC, noise, *pins, com, restraints, fd, scale=G.GUIDE_SCALE, fnorm=2.0, double=True)
    else:
        r32, r64 = F.reference(leg == "ep"), F.reference(leg == "ep", True)
    d = {n: float((getattr(r32, n).double() - getattr(r64, n)).abs().max()) for n in ("x0", "h0", "fx", "fh")}
    dE = float(((r32.E.double() - r64.E).abs() / r64.E.abs().clamp(min=1.0)).max())
    print(f"{leg}: fp32 against fp64 composition {d}, energies {dE:.3g} relative")
    assert max(d.values()) <= 5e-4 and dE <= 5e-4


def test_the_field_lowers_its_energies():
    """final clash and complementarity energies of the guided run: no higher than the unguided run's on every graph"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    ref, un = F.reference(), F.reference(False, False, False)
    cl_g, co_g, n_g = F.final_energies(fd, batch, ref.x0, ref.h0)
    cl_u, co_u, n_u = F.final_energies(fd, batch, un.x0, un.h0)
    print("clash energies", cl_u.tolist(), "->", cl_g.tolist())
    print("clashing pairs", n_u.tolist(), "->", n_g.tolist())
    print("complementarity energies", co_u.tolist(), "->", co_g.tolist())
    assert bool((cl_g <= cl_u).all()) and bool((co_g <= co_u).all())
    assert bool((cl_g < cl_u).any()) and bool((co_g < co_u).any())
    assert int(n_g.sum()) < int(n_u.sum())


@pytest.mark.parametrize("ep", [False, True])
def test_a_reference_without_the_field_misses(ep):
    """the teeth of the GPU test: more than 10 x the 5e-3 tolerance on every graph (every graph has a term)"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    ref, un = F.reference(ep), F.reference(ep, False, False)
    ptr = batch.pharm_ptr.tolist()
    for g in range(5):
        miss = float((ref.fx[:, ptr[g]:ptr[g + 1]] - un.fx[:, ptr[g]:ptr[g + 1]]).abs().max())
        print(f"graph {g}: without the field the frames are off by {miss:.3g}")
        assert miss > 10 * TOL
    assert float((F.wide_reference().fx - F.wide_reference(False).fx).abs().max()) > 10 * TOL


# ---- the energies ------------------------------------------------------------------------------------------------------------
def _toy(seed=3, n_atoms=40, n_feat=30, nf=7):
    gen = torch.Generator().manual_seed(seed)
    cfg = O.DynamicsConfig()
    batch = O.batch64(O.synthetic_batch([seed], [n_atoms], [nf], cfg))
    c = O.segment_mean(batch.prot_x, batch.prot_ptr)[0]
    match, dist = F.tables()
    ph = ([0, n_feat], c[None].float() + 5.0 * torch.randn(n_feat, 3, generator=gen), torch.randint(0, 6, (n_feat,), generator=gen))
    fd = F.make_field(atom_r=torch.full((n_atoms,), 3.0), w_clash=1.5, ph=ph, match=match, dist=dist * 0.25, w_comp=0.75, kappa=4.0,
                      type_sharpness=2.0)
    x = c[None] + 2.5 * torch.randn(nf, 3, generator=gen).double()
    h = torch.randn(nf, 6, generator=gen).double()
    D = 0.3 * torch.randn(1, 3, generator=gen).double().expand(nf, 3)
    return fd, batch, x, D, h


def test_closed_form_gradient_is_the_finite_difference_of_the_energy():
    fd, batch, x, D, h = _toy()
    prot = batch.prot_x - D[:1]                          # the sampler's frame: y = x + D is then the caller's
    g_cl, g_co, E_cl, E_co = F.field_terms(fd, batch, prot, x, D, h)
    assert float(E_cl[0]) > 0 and float(E_co[0]) > 0 and float(g_cl.abs().max()) > 0 and float(g_co.abs().max()) > 0
    eps = 1e-6
    for which, g in (("clash", g_cl), ("comp", g_co)):
        fdiff = torch.zeros_like(x)
        for f in range(x.shape[0]):
            for c in range(3):
                xp, xm = x.clone(), x.clone()
                xp[f, c] += eps
                xm[f, c] -= eps
                ep_, em_ = F.field_terms(fd, batch, prot, xp, D, h), F.field_terms(fd, batch, prot, xm, D, h)
                i = 2 if which == "clash" else 3
                fdiff[f, c] = (ep_[i][0] - em_[i][0]) / (2 * eps)
        err = float((fdiff - g).abs().max()) / float(g.abs().max())
        print(f"{which}: finite differences against the closed form, {err:.3g} of the largest entry")
        assert err <= 1e-6
    # autograd agrees too, and no gradient reaches the features
    xx, hh = x.clone().requires_grad_(True), h.clone().requires_grad_(True)
    with torch.enable_grad():
        _, _, e1, e2 = F.field_terms(fd, batch, prot, xx, D, hh)
        (e1.sum() + e2.sum()).backward()
    assert float((xx.grad - (g_cl + g_co)).abs().max()) <= 1e-9 * float((g_cl + g_co).abs().max())
    assert hh.grad is None or bool((hh.grad == 0).all())


def test_a_matched_center_pays_nothing_and_degenerate_pairs_are_zero():
    match, dist = F.tables()
    cfg = O.DynamicsConfig()
    batch = O.batch64(O.synthetic_batch([4], [20], [3], cfg))
    far = batch.prot_x.mean(dim=0) + 100.0               # away from every atom
    q = torch.stack([far, far + torch.tensor([30.0, 0, 0])]).float()
    ph = ([0, 2], q, torch.tensor([2, 2]))               # two acceptors: they match donors (type 1) only
    fd = F.make_field(atom_r=torch.full((20,), 2.0), w_clash=1.0, ph=ph, match=match, dist=dist, w_comp=1.0, kappa=4.0, type_sharpness=50.0)
    x = torch.stack([q[0].double() + torch.tensor([float(dist[1]) - 0.01, 0, 0]).double(),      # within d of a partner
                     q[0].double() + torch.tensor([float(dist[1]) + 3.0, 0, 0]).double(),       # outside
                     q[0].double()])                                                            # on the feature: rho == 0
    h = torch.zeros(3, 6).double()
    h[:, 1] = 1.0                                       # donors, sharply
    D = torch.zeros(3, 3).double()
    g_cl, g_co, E_cl, E_co = F.field_terms(fd, batch, batch.prot_x, x, D, h)
    assert float(E_cl[0]) == 0.0 and bool((g_cl == 0).all())
    assert bool((g_co[0] == 0).all()) and bool((g_co[2] == 0).all()) and bool(torch.isfinite(g_co).all())
    assert float(g_co[1, 0]) > 0 and float(E_co[0]) > 0
    # the soft minimum never exceeds the nearest distance; the converse holds up to log|S| / kappa
    only1 = F.field_terms(fd, batch, batch.prot_x, x[1:2], D[:1], h[1:2])[3][0]
    assert abs(float(only1) - float(E_co[0])) <= 1e-12
    h[:, 1], h[:, 0] = 0.0, 1.0                          # aromatics: no acceptor matches them -- an empty set, no term
    assert float(F.field_terms(fd, batch, batch.prot_x, x, D, h)[3][0]) <= 1e-12
    # a center exactly on an atom: zero gradient from that pair, finite everywhere
    x2 = batch.prot_x[:3].clone()
    g_cl2, _, E_cl2, _ = F.field_terms(fd, batch, batch.prot_x, x2, D, h)
    assert bool(torch.isfinite(g_cl2).all()) and float(E_cl2[0]) >= 3 * 4.0


def test_tables_are_the_validity_metric():
    from pharmacoforge_amd import analysis as A
    match, dist = A.complementarity_tables()
    assert match.dtype == torch.int32 and dist.dtype == torch.float32 and match.shape == (6, 6)
    for t, name in enumerate(A.ph_idx_to_type):
        assert [A.ph_idx_to_type[u] for u in range(6) if match[t, u]] == sorted(A._MATCHING_TYPES[name], key=A.ph_idx_to_type.index)
        assert float(dist[t]) == A._MATCHING_DIST[name]
    e, n = A.clash_energy(torch.tensor([[0.0, 0, 0], [10.0, 0, 0]]), torch.tensor([[1.0, 0, 0], [0, 1.5, 0], [50.0, 0, 0]]), 2.0, 2.0)
    assert n == 2 and abs(e - 2.0 * (1.0 + 0.25)) <= 1e-12
    assert A.clash_energy(torch.zeros(0, 3), torch.zeros(4, 3)) == (0.0, 0)


# ---- the argument rules (no device work is reached) -----------------------------------------------------------------------------
def test_model_argument_rules():
    from test_host_logic import make_model
    m = make_model(20)
    b = O.synthetic_batch([1], 20, 3, O.DynamicsConfig())
    g = pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, torch.zeros(3, 3), torch.zeros(3, 6))
    pf = pfa.PocketField()
    assert (pf.clash_radius, pf.clash_weight, pf.comp_weight, pf.kappa, pf.type_sharpness) == (2.0, 1.0, 0.0, 4.0, 4.0)
    with pytest.raises(ValueError, match="resampling"):
        m.sample([g], [[4]], pocket_field=pf, pin_resamples=2)
    with pytest.raises(ValueError, match="multistep"):
        m.sample([g], [[4]], pocket_field=pf, sample_steps=4, sampler="multistep")
    with pytest.raises(ValueError, match="multistep"):
        m.sample_given_receptor(g, noise=torch.zeros(1, 3, 9), pocket_field=pf, sample_steps=4, sampler="multistep")
    with pytest.raises(ValueError, match="receptor features"):
        m.sample([g], [[4]], pocket_field=pfa.PocketField(comp_weight=0.5))
    with pytest.raises(ValueError, match="receptor features"):
        m.sample_given_receptor(g, noise=torch.zeros(21, 3, 9), pocket_field=pfa.PocketField(comp_weight=0.5))
    with pytest.raises(ValueError, match="20 atoms"):
        m.sample([g], [[4]], pocket_field=pfa.PocketField(clash_radius=torch.ones(7)))
    with pytest.raises(ValueError, match="2 entries for 1 pockets"):
        m.sample([g], [[4]], pocket_field=pfa.PocketField(clash_radius=[2.0, 2.0]))
    with pytest.raises(ValueError, match="PocketField"):
        m.sample([g], [[4]], pocket_field=dict(clash_radius=2.0))
    # what the engine receives: per-atom radii by graph, the sharpness on one-hot-scaled features, the features' argmax types
    import dataclasses
    g2 = dataclasses.replace(g, prot_ph_x=torch.ones(2, 3), prot_ph_h=torch.eye(6)[[4, 1]], prot_ph_ptr=torch.tensor([0, 2]))
    bg = pfa.batch(pfa.copy_graph(g2, 2, pharm_feats_per_copy=torch.tensor([3, 4])))
    kw = m._field_for_batch(bg, pfa.PocketField(clash_radius=1.5, comp_weight=0.25, type_sharpness=3.0), [1.5, torch.arange(20.0)])
    assert kw["atom_r"].tolist() == [1.5] * 20 + list(range(20)) and kw["w_comp"] == 0.25 and kw["w_clash"] == 1.0
    assert kw["type_sharpness"] == 3.0 * float(m.pharm_feat_norm_constant)
    assert kw["ph"][0].tolist() == [0, 2, 4] and kw["ph"][2].tolist() == [4, 1, 4, 1] and kw["ph"][1].shape == (4, 3)
    assert "ph" not in m._field_for_batch(bg, pfa.PocketField(), None) and m._field_for_batch(bg, None) is None


def test_the_command_lines(tmp_path):
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]
    a = cli.parse_arguments(base + ["--avoid_clashes"])
    assert a.avoid_clashes == 2.0 and a.clash_weight == 1.0 and a.guide_scale == 1.0 and a.guide_family == "wide"
    a = cli.parse_arguments(base + ["--avoid_clashes", "1.5", "--clash_weight", "3", "--guide_scale", "2.5", "--guide_clip", "1",
                                    "--guide_family", "tuned", "--sample_steps", "4", "--sampler", "ddim"])
    assert (a.avoid_clashes, a.clash_weight, a.guide_scale, a.guide_clip, a.guide_family) == (1.5, 3.0, 2.5, 1.0, "tuned")
    assert cli.parse_arguments(base).avoid_clashes is None
    f = tmp_path / "pin.xyz"
    f.write_text("1\nC 0 0 0\n")
    for argv in (["--clash_weight", "2"], ["--guide_scale", "2"], ["--guide_family", "tuned"], ["--avoid_clashes", "-1"],
                 ["--avoid_clashes", "--clash_weight", "-2"], ["--avoid_clashes", "nan"],
                 ["--avoid_clashes", "--sample_steps", "4", "--sampler", "multistep"],
                 ["--avoid_clashes", "--pinned_centers", str(f), "--pin_resamples", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(base + argv)
    import test as tcli
    tb = ["--model_dir", "run"]
    a = tcli.parse_arguments(tb + ["--avoid_clashes", "--guide_complementarity", "0.25", "--guide_scale", "2"])
    assert a.pocket_field == dict(clash_radius=2.0, clash_weight=1.0, comp_weight=0.25) and a.guide_scale == 2.0
    a = tcli.parse_arguments(tb + ["--guide_complementarity", "0.5", "--guide_family", "tuned"])
    assert a.pocket_field == dict(clash_radius=None, clash_weight=1.0, comp_weight=0.5) and a.guide_family == "tuned"
    assert tcli.parse_arguments(tb).pocket_field is None
    for argv in (["--guide_scale", "2"], ["--guide_clip", "1"], ["--guide_family", "wide"], ["--clash_weight", "1"],
                 ["--guide_complementarity", "-1"], ["--avoid_clashes", "-0.5"],
                 ["--avoid_clashes", "--sample_steps", "4", "--sampler", "multistep"]):
        with pytest.raises(ValueError):
            tcli.parse_arguments(tb + argv)
