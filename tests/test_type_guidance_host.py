"""Host side of type guidance (pf_guide_types_next): the conditions the GPU tests (test_gpu_type_guidance.py) put on their own
inputs, checked on the reference alone (tests/type_guidance_ref.py) -- without the arming it is pocket_field_ref.field_reference
bit for bit; in fp32 and in fp64 it agrees with itself within 5e-4 (DESIGN 4.15's demand); the final type energy falls on every
restrained graph and the restrained centers change their argmax types; a reference that drops J_h, and one that leaves g_eps_h
zero, miss the guided frames by more than ten times the tolerance --, the closed-form gradients against fp64 central differences,
and the argument rules of the model, the parser and the two command lines.  The argument validation of the C ABI is
test_types_host.py's stand-alone checker.  No GPU.

Recorded (fp32 composition, T = 24, feat_scale 4): fp32 against fp64 over all frames 5.1e-5 (x) / 2.7e-5 (h) in the noise
parameterisation; final type energy of graphs 1 / 2 / 3 without and with type guidance 92.8 / 43.2 / 33.9 -> 0.22 / 1.40 / 6e-5;
per graph 0..4 the frames (x / h) are missed by 0.013/0.057, 0.19/0.12, 2.6/2.6, 0.001/0.030, 0.068/0.18 without J_h and by
1e-6/1e-7, 0.033/0.022, 0.25/0.12, 3e-4/0.008, 3e-4/0.005 with a zero g_eps_h (its only way to the features is through the
coordinates of the windowed graph)."""
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
import type_guidance_ref as TG  # noqa: E402

TOL = G.TOL


# ---- the reference, and the conditions the GPU tests rest on ----------------------------------------------------------------
@pytest.mark.parametrize("ep", [False, True])
def test_without_type_guidance_the_reference_is_field_reference(ep):
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    want = F.reference(ep)
    for kw in (dict(types=None), dict(types=tg, use_types=False)):
        got = TG.types_reference(sd, cfg, batch, TG.T, TG.PREC, noise, *pins, com, restraints, fd, scale=TG.GUIDE_SCALE, ep=ep, **kw)
        for name in ("x0", "h0", "fx", "fh", "E", "g0", "grad", "shift", "E3"):
            assert torch.equal(getattr(got, name), getattr(want, name)), name
        assert got.E_type.shape[0] == 0 and got.g0_h.shape[0] == 0
    un = TG.types_reference(sd, cfg, batch, TG.T, TG.PREC, noise, *pins, com, None, None, None, scale=TG.GUIDE_SCALE, ep=ep)
    assert torch.equal(un.fx, G.reference(ep, False, False).fx)


def test_the_case_holds_every_kind_of_graph_the_gpu_tests_rely_on():
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    assert batch.pharm_ptr.diff().tolist() == [3, 8, 5, 1, 6]
    assert [b - a for a, b in zip(fd.ph_ptr, fd.ph_ptr[1:])] == F.N_FEATURES == [0, 70, 5, 1, 3]
    assert [len(r or []) for r in tg.raw] == [0, 1, 1, 1, 0]
    assert tg.raw[3][0][3] == 0.0 and tg.raw[3][0][1] == 0 and tg.raw[1][0][3] == 0.0      # no window: graphs 3 and 1
    assert tg.raw[2][0][3] > 0 and tg.comp and float(tg.unmatched) > 0                  # a window: graph 2
    ptr = batch.pharm_ptr.tolist()
    flags = pins[0]
    assert int(flags[ptr[1]]) & 2 and not bool((flags[ptr[1] + 2:ptr[2]] & 2).any())    # graph 1: a type-pinned center next to free ones
    ref = TG.reference()
    # the type-pinned center ignores its shift: its row of every frame is the run without the arming's, its shift is not zero
    assert float(ref.shift_h[:, ptr[1]].abs().max()) > 0
    assert torch.equal(ref.fh[:, ptr[1]], F.reference().fh[:, ptr[1]])
    # graph 0 has no feature: every type is unmatched there, the term is w_comp * centers * unmatched^2 and moves nothing
    assert torch.allclose(ref.E_type[:, 0], torch.tensor(float(fd.w_comp) * 3 * float(tg.unmatched) ** 2))
    # graph 4: no type restraint, yet a feature gradient from the complementarity term
    assert float(ref.g0_h[:, ptr[4]:ptr[5]].abs().max()) > 0
    # the window opens: the coordinate gradient of graph 2 differs from the field's
    assert float((ref.g0[0, ptr[2]:ptr[3]] - F.reference().g0[0, ptr[2]:ptr[3]]).abs().max()) > 0
    assert torch.equal(((ref.E3[..., 0] + ref.E3[..., 1]) + ref.E3[..., 2]) + ref.E_type, ref.E)


@pytest.mark.parametrize("leg", ["noise", "ep"])
def test_fp32_against_fp64_composition(leg):
    """5e-4 on x_0, h_0 and all frames (4.15's demand); measured 5.1e-5 (noise), 1.3e-6 (endpoint)"""
    r32, r64 = TG.reference(leg == "ep"), TG.reference(leg == "ep", True)
    d = {n: float((getattr(r32, n).double() - getattr(r64, n)).abs().max()) for n in ("x0", "h0", "fx", "fh")}
    dE = float(((r32.E.double() - r64.E).abs() / r64.E.abs().clamp(min=1.0)).max())
    dT = float(((r32.E_type.double() - r64.E_type).abs() / r64.E_type.abs().clamp(min=1.0)).max())
    print(f"{leg}: fp32 against fp64 composition {d}, energies {dE:.3g} / type energies {dT:.3g} relative")
    assert max(d.values()) <= 5e-4 and dE <= 5e-4 and dT <= 5e-4


def test_type_guidance_lowers_the_type_energy_and_changes_types():
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    ref, un = TG.reference(), F.reference()
    e_g, e_u = TG.final_type_energy(tg, batch, ref.x0, ref.h0), TG.final_type_energy(tg, batch, un.x0, un.h0)
    print("final type energies", e_u.tolist(), "->", e_g.tolist())
    print("per-step E_type, first and last", ref.E_type[0].tolist(), ref.E_type[-1].tolist())
    for g in (1, 2, 3):
        assert float(e_g[g]) < float(e_u[g]) and float(ref.E_type[-1, g]) < float(ref.E_type[0, g])
    assert float(e_g[0]) == 0 and float(e_g[4]) == 0
    ptr = batch.pharm_ptr.tolist()
    a_g, a_u = ref.h0.argmax(dim=1), un.h0.argmax(dim=1)
    print("argmax types", a_u.tolist(), "->", a_g.tolist())
    want1 = tg.raw[1][0][0]
    free1 = [f for f in range(ptr[1], ptr[2]) if not int(pins[0][f]) & 2]
    assert all(int(a_g[f]) == want1 for f in free1) and any(int(a_u[f]) != want1 for f in free1)
    assert int(a_g[ptr[3]]) == tg.raw[3][0][0] != int(a_u[ptr[3]])
    assert int(a_g[ptr[2]]) == tg.raw[2][0][0] != int(a_u[ptr[2]])
    assert int(a_g[ptr[1]]) == int(a_u[ptr[1]])         # the type-pinned center keeps its type
    # analysis.type_restraint_energy is the same number
    for g in (1, 2, 3):
        e = pfa.analysis.type_restraint_energy(ref.x0[ptr[g]:ptr[g + 1]], ref.h0[ptr[g]:ptr[g + 1]], tg.raw[g], float(tg.sharp))
        assert abs(e - float(e_g[g])) <= 1e-9 * max(1.0, float(e_g[g]))


def test_references_that_drop_a_term_miss():
    """the teeth of the GPU test: more than 10 x the 5e-3 tolerance over the guided frames; without J_h on every graph with a live
    feature gradient and free centers but the single-center one (0.03), with a zero g_eps_h on the windowed graph"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    ref = TG.reference()
    ptr = batch.pharm_ptr.tolist()
    miss = {}
    for name, other in (("the arming", TG.reference(False, False, False)), ("J_h", TG.reference(False, False, True, False)),
                        ("g_eps_h", TG.reference(False, False, True, True, True))):
        miss[name] = [max(float((ref.fx[:, ptr[g]:ptr[g + 1]] - other.fx[:, ptr[g]:ptr[g + 1]]).abs().max()),
                          float((ref.fh[:, ptr[g]:ptr[g + 1]] - other.fh[:, ptr[g]:ptr[g + 1]]).abs().max())) for g in range(5)]
        print(f"without {name} the frames of graphs 0..4 are off by", ["%.3g" % v for v in miss[name]])
        assert max(miss[name]) >= 10 * TOL
    assert all(miss["the arming"][g] >= 10 * TOL for g in range(5))
    assert all(miss["J_h"][g] >= 10 * TOL for g in (0, 1, 2, 4))
    assert miss["g_eps_h"][2] >= 10 * TOL
    w32, w_un = TG.wide_reference(), TG.wide_reference(False)
    assert float((w32.fh - w_un.fh).abs().max()) >= 10 * TOL


# ---- the energies ------------------------------------------------------------------------------------------------------------
def _toy(seed=5, n_atoms=30, n_feat=12, nf=6, types=(0, 2)):
    """one graph, fp64: centers around the pocket, features of two types only (the other sets are empty)"""
    gen = torch.Generator().manual_seed(seed)
    cfg = O.DynamicsConfig()
    batch = O.batch64(O.synthetic_batch([seed], [n_atoms], [nf], cfg))
    c = O.segment_mean(batch.prot_x, batch.prot_ptr)[0]
    match, dist = F.tables()
    ty = torch.tensor(types)[torch.randint(0, len(types), (n_feat,), generator=gen)]
    ph = ([0, n_feat], c[None].float() + 5.0 * torch.randn(n_feat, 3, generator=gen), ty)
    fd = F.make_field(ph=ph, match=match, dist=dist * 0.25, w_comp=0.75, kappa=4.0, type_sharpness=2.0)
    x = c[None] + 2.5 * torch.randn(nf, 3, generator=gen).double()
    h = torch.randn(nf, 6, generator=gen).double()
    D = 0.3 * torch.randn(1, 3, generator=gen).double().expand(nf, 3)
    tr = [[(3, None, (c + 0.5).tolist(), 6.0, 1.5), (1, 2, (0.0, 0.0, 0.0), 0.0, 2.0), (5, 4, c.tolist(), 0.5, 1.0)]]
    return fd, batch, x, D, h, tr


def _fdiff(fn, v, eps=1e-6):
    out = torch.zeros_like(v)
    for i in range(v.shape[0]):
        for c in range(v.shape[1]):
            vp, vm = v.clone(), v.clone()
            vp[i, c] += eps
            vm[i, c] -= eps
            out[i, c] = (fn(vp) - fn(vm)) / (2 * eps)
    return out


def test_closed_form_restraint_gradients_are_the_finite_differences_of_the_energy():
    """window and cross-entropy: dE/dy and dE/dh0_hat against fp64 central differences"""
    fd, batch, x, D, h, tr = _toy()
    tg = TG.make_types(tr, sharpness=2.0)
    y = x + D
    g0h, gy, E = TG.type_restraint_terms(tg, batch.pharm_ptr, y, h)
    assert float(E[0]) > 0 and float(gy.abs().max()) > 0 and float(g0h.abs().max()) > 0
    small = TG.make_types([tr[0][2:]], sharpness=2.0)   # center 4 is outside its small sphere: exact zeros from it, and no energy
    _, gy_s, E_s = TG.type_restraint_terms(small, batch.pharm_ptr, y, h)
    assert bool((gy_s == 0).all()) and float(E_s[0]) == 0
    assert bool((gy.abs().amax(dim=1) > 0).all())       # ... while the large window is open on every center
    fy = _fdiff(lambda v: TG.type_restraint_terms(tg, batch.pharm_ptr, v, h)[2][0], y)
    fh = _fdiff(lambda v: TG.type_restraint_terms(tg, batch.pharm_ptr, y, v)[2][0], h)
    ey, eh = float((fy - gy).abs().max()) / float(gy.abs().max()), float((fh - g0h).abs().max()) / float(g0h.abs().max())
    print(f"type restraints: finite differences against the closed form, dE/dy {ey:.3g}, dE/dh0_hat {eh:.3g} of the largest entry")
    assert ey <= 1e-6 and eh <= 1e-6
    # -log p_fc: the energy of a windowless restraint is the cross-entropy of the softmax
    one = TG.make_types([[(1, 2, (0.0, 0.0, 0.0), 0.0, 2.0)]], sharpness=2.0)
    e1 = TG.type_restraint_terms(one, batch.pharm_ptr, y, h)[2][0]
    assert abs(float(e1) + 2.0 * float(torch.log_softmax(2.0 * h[2], dim=0)[1])) <= 1e-12


@pytest.mark.parametrize("unmatched", [0.0, 1.5])
def test_closed_form_complementarity_type_gradient(unmatched):
    """dE/dh0_hat of E_comp + the unmatched term against fp64 central differences of that energy"""
    fd, batch, x, D, h, tr = _toy()
    tg = TG.make_types(None, sharpness=2.0, complementarity=True, unmatched=unmatched)
    prot = batch.prot_x - D[:1]

    def energy(hh):
        e_co = F.field_terms(fd, batch, prot, x, D, hh)[3][0]
        return e_co + TG.comp_type_terms(fd, tg, batch, x, D, hh)[1][0]
    g0h, E_un = TG.comp_type_terms(fd, tg, batch, x, D, h)
    assert (float(E_un[0]) > 0) == (unmatched > 0) and float(g0h.abs().max()) > 0
    fh = _fdiff(energy, h)
    err = float((fh - g0h).abs().max()) / float(g0h.abs().max())
    print(f"complementarity type term (unmatched {unmatched}): finite differences against the closed form, {err:.3g}")
    assert err <= 1e-6
    assert float(g0h.sum(dim=1).abs().max()) <= 1e-12 * float(g0h.abs().max()) + 1e-15     # a softmax's gradient sums to zero


# ---- the argument rules (no device work is reached) -----------------------------------------------------------------------------
def _model_and_graph():
    from test_host_logic import make_model
    m = make_model(20)
    b = O.synthetic_batch([1], 20, 3, O.DynamicsConfig())
    g = pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, torch.zeros(3, 3), torch.zeros(3, 6))
    return m, g


def test_run_spec_rules():
    m, g = _model_and_graph()
    tgd = pfa.TypeGuidance()
    assert (tgd.scale, tgd.clip, tgd.sharpness, tgd.complementarity, tgd.unmatched) == (1.0, 0.0, None, False, 0.0)
    tr = [[(m.ph_type_map[1], None, (0.0, 0.0, 0.0), 2.0, 1.0)]]
    spec = m._run_spec(pins=False, guided=True, typed=True)
    assert spec.types == (1.0, 0.0, 4.0 * float(m.pharm_feat_norm_constant), False, 0.0) and spec.guided
    assert m._run_spec(pins=False, guided=False).types is None
    # composes with pins, restraints, a pocket field, seeds, first-order few-step sampling and both families
    for kw in (dict(pins=True, pinned=True), dict(pins=False, pocket_field=pfa.PocketField()),
               dict(pins=False, sample_steps=4, sampler="ddim"), dict(pins=False, sample_steps=4),
               dict(pins=False, seeds=[1], seed_level=5), dict(pins=False, guide_family="wide")):
        assert m._run_spec(guided=True, typed=True, **kw).types is not None
    s = m._run_spec(pins=False, guided=True, pocket_field=pfa.PocketField(comp_weight=0.5, type_sharpness=3.0),
                    type_guidance=pfa.TypeGuidance(scale=2.0, clip=1.0, complementarity=True, unmatched=1.5))
    assert s.types == (2.0, 1.0, 3.0 * float(m.pharm_feat_norm_constant), True, 1.5)      # the sharpness is the field's
    assert s.types_kwargs([None]) == dict(restraints=[None], scale=2.0, clip=1.0, sharpness=s.types[2], complementarity=True, unmatched=1.5)
    with pytest.raises(ValueError, match="resampling"):
        m.sample([g], [[4]], type_restraints=tr, pin_resamples=2)
    with pytest.raises(ValueError, match="multistep"):
        m.sample([g], [[4]], type_restraints=tr, sample_steps=4, sampler="multistep")
    with pytest.raises(ValueError, match="multistep"):
        m.sample_given_receptor(g, noise=torch.zeros(1, 3, 9), type_restraints=tr, sample_steps=4, sampler="multistep")
    with pytest.raises(ValueError, match="comp_weight > 0"):
        m.sample([g], [[4]], type_restraints=tr, type_guidance=pfa.TypeGuidance(complementarity=True))
    with pytest.raises(ValueError, match="comp_weight > 0"):
        m.sample([g], [[4]], pocket_field=pfa.PocketField(), type_guidance=pfa.TypeGuidance(complementarity=True))
    with pytest.raises(ValueError, match="must agree"):
        m.sample([g], [[4]], type_restraints=tr, pocket_field=pfa.PocketField(type_sharpness=2.0), type_guidance=pfa.TypeGuidance(sharpness=4.0))
    with pytest.raises(ValueError, match="TypeGuidance"):
        m.sample([g], [[4]], type_restraints=tr, type_guidance=dict(scale=1.0))
    with pytest.raises(ValueError, match="scale must be >= 0"):
        m.sample([g], [[4]], type_restraints=tr, type_guidance=pfa.TypeGuidance(scale=-1.0))
    with pytest.raises(ValueError, match="2 entries for 1 pockets"):
        m.sample([g], [[4]], type_restraints=tr * 2)
    with pytest.raises(ValueError, match="names type 'Nonsense'"):
        m.sample([g], [[4]], type_restraints=[[("Nonsense", None, (0.0, 0.0, 0.0), 0.0, 1.0)]])
    with pytest.raises(ValueError, match="type index must be in 0..5"):
        m.sample([g], [[4]], type_restraints=[[(6, None, (0.0, 0.0, 0.0), 0.0, 1.0)]])
    with pytest.raises(ValueError, match="names center 4 but sizes"):
        m.sample([g], [[4]], type_restraints=[[(1, 4, (0.0, 0.0, 0.0), 0.0, 1.0)]])
    # names resolve to indices; an empty list is no restraint
    assert m._type_restraints(tr, 1, "pockets") == [[(1, None, (0.0, 0.0, 0.0), 2.0, 1.0)]]
    assert m._type_restraints([[]], 1, "pockets") is None and m._type_restraints(None, 1, "pockets") is None
    assert m._guided(None, None, [[(1, None, (0.0, 0.0, 0.0), 2.0, 1.0)]]) and not m._guided(None, None, None)


def test_parse_type_restraints():
    from pharmacoforge_amd import pocket_io as P
    text = """# a donor near the carbonyl
type HydrogenDonor 1.0 2.0 -3.5 4 2   # every center
type 3 0 0 0 0 1.5 2

type Aromatic 1e1 0 0 2.5 0 *
"""
    assert P.parse_type_restraints(text) == [("HydrogenDonor", None, (1.0, 2.0, -3.5), 4.0, 2.0), (3, 2, (0.0, 0.0, 0.0), 0.0, 1.5),
                                             ("Aromatic", None, (10.0, 0.0, 0.0), 2.5, 0.0)]
    assert P.parse_type_restraints("") == []
    for bad, line, what in (("attract 0 0 0 1 1", 1, "starts with 'type'"), ("\ntype 1 0 0 0 1", 2, "got 6 fields"),
                            ("type 1 0 0 0 1 1 2 3", 1, "got 9 fields"), ("type 1 0 0 x 1 1", 1, "must be numbers"),
                            ("type 1 0 0 nan 1 1", 1, "must be finite"), ("type 1 0 0 0 -1 1", 1, "must not be negative"),
                            ("type 1 0 0 0 1 -1", 1, "must not be negative"), ("type -1 0 0 0 1 1", 1, "type index"),
                            ("# c\n\ntype 1 0 0 0 1 1 first", 3, "index or"), ("type 1 0 0 0 1 1 -2", 1, "center index")):
        with pytest.raises(ValueError, match=f"line {line}.*{what}"):
            P.parse_type_restraints(bad, source="file.txt")
    # parse_restraints is what it was: it does not read type lines
    with pytest.raises(ValueError, match="attract"):
        P.parse_restraints("type 1 0 0 0 1 1")


def test_the_command_lines(tmp_path):
    f = tmp_path / "types.txt"
    f.write_text("type HydrogenDonor 1 2 3 4 2\ntype 0 0 0 0 0 1 3\n")
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]
    a = cli.parse_arguments(base + ["--type_restraints", str(f)])
    assert a.type_restraint_list == [("HydrogenDonor", None, (1.0, 2.0, 3.0), 4.0, 2.0), (0, 3, (0.0, 0.0, 0.0), 0.0, 1.0)]
    assert (a.guide_type_scale, a.guide_type_clip, a.type_sharpness, a.guide_family) == (1.0, 0.0, 4.0, "wide")
    a = cli.parse_arguments(base + ["--type_restraints", str(f), "--guide_type_scale", "2", "--guide_type_clip", "0.5", "--type_sharpness", "3",
                                    "--guide_family", "tuned", "--guide_scale", "2", "--sample_steps", "4", "--sampler", "ddim"])
    assert (a.guide_type_scale, a.guide_type_clip, a.type_sharpness, a.guide_family, a.guide_scale) == (2.0, 0.5, 3.0, "tuned", 2.0)
    assert cli.parse_arguments(base).type_restraint_list is None
    pin = tmp_path / "pin.xyz"
    pin.write_text("1\nC 0 0 0\n")
    for argv in (["--guide_type_scale", "2"], ["--guide_type_clip", "1"], ["--type_sharpness", "4"],
                 ["--type_restraints", str(f), "--guide_type_scale", "-1"], ["--type_restraints", str(f), "--type_sharpness", "nan"],
                 ["--type_restraints", str(f), "--sample_steps", "4", "--sampler", "multistep"],
                 ["--type_restraints", str(f), "--pinned_centers", str(pin), "--pin_resamples", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(base + argv)
    with pytest.raises(ValueError, match="do not reach center 3"):
        cli.parse_arguments(base + ["--type_restraints", str(f), "--samples_per_pocket", "2", "--pharm_sizes", "3", "5"])
    # scores.tsv gains the type energy
    from types import SimpleNamespace
    sc = SimpleNamespace(n_centers=3, total=1.0, per_center=0.5, pos=0.25, feat=0.25, position_error=0.1, type_accuracy=1.0)
    cli.write_scores(tmp_path / "scores.tsv", [0], [sc], None, [1.25])
    rows = [l.split("\t") for l in (tmp_path / "scores.tsv").read_text().splitlines()]
    assert rows[0][-1] == "type_energy" and rows[1][-1] == "1.25" and len(rows[0]) == 9
    cli.write_scores(tmp_path / "scores.tsv", [0], [sc], [(2.0, 1)], [1.25])
    assert (tmp_path / "scores.tsv").read_text().splitlines()[0].split("\t")[-3:] == ["clash_energy", "clashes", "type_energy"]
    import test as tcli
    tb = ["--model_dir", "run"]
    a = tcli.parse_arguments(tb + ["--type_restraints", str(f), "--guide_type_scale", "2"])
    assert a.type_guidance == dict(scale=2.0, clip=0.0, sharpness=4.0, complementarity=False, unmatched=0.0) and a.pocket_field is None
    assert len(a.type_restraint_list) == 2
    a = tcli.parse_arguments(tb + ["--guide_complementarity", "0.25", "--guide_complementarity_types", "--comp_unmatched", "1.5"])
    assert a.type_guidance == dict(scale=1.0, clip=0.0, sharpness=4.0, complementarity=True, unmatched=1.5)
    assert a.pocket_field == dict(clash_radius=None, clash_weight=1.0, comp_weight=0.25) and a.type_restraint_list is None
    assert tcli.parse_arguments(tb).type_guidance is None
    for argv in (["--guide_type_scale", "2"], ["--guide_complementarity_types"], ["--comp_unmatched", "1"],
                 ["--guide_complementarity", "0", "--guide_complementarity_types"], ["--type_restraints", str(f), "--guide_type_clip", "-1"],
                 ["--guide_complementarity", "0.5", "--guide_complementarity_types", "--comp_unmatched", "-1"],
                 ["--type_restraints", str(f), "--sample_steps", "4", "--sampler", "multistep"],
                 ["--type_restraints", str(f), "--pharm_sizes", "3", "--samples_per_pocket", "1"]):
        with pytest.raises(ValueError):
            tcli.parse_arguments(tb + argv)
