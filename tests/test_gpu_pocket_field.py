"""The pocket field of a guided run (pf_guide_field_next: clash and complementarity energies, k_guide_field behind k_guide_grad)
against the CPU composition of tests/pocket_field_ref.py: guidance_ref.guided_reference with the field's lines inserted.

Shape: guidance_ref.case() -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms, 3 / 8 / 5 / 1 / 6 centers, one graph with pins,
T = 24, live head, guide_scale 4 -- with radii of 2.0 (every seventh atom inert), 0 / 70 / 5 / 1 / 3 receptor features, graph 2
keeping its sphere restraints; w_clash 1, w_comp 0.25, kappa = type_sharpness = 4.  Whole runs at rtol = atol = 5e-3 in both
parameterisations on the tuned family and at (64, 32), T = 12 on the wide family; the same runs must MISS a reference that drops
the field.  One step read back against fp64 under helpers.within_budget; one tall step (600 atoms, 64 centers, 130 features) under
the same budget and bitwise equal on a second run.

Measured on the MI355X, worst |error| over x_0, h_0 and all frames: 3.1e-4 (noise; the reference's own fp32 noise is 2.9e-4;
energies 1.9e-4), 1.3e-6 (endpoint; energies 5.7e-6), 7.7e-4 at (64, 32) (energies 2.6e-2 on values of several hundred); clash only
3.0e-5, complementarity only 2.4e-6, no restraints 3.0e-4.  One step against the fp64 reference, ratio to max(e32, 2**-22) of
E / g0 / grad / shift / E3 restraints / clash / complementarity: 0.20 / 1.80 / 1.73 / 1.79 / 0.72 / 1.09 / 0.70 (noise),
0.10 / 0.80 / 0.52 / 0.51 / 0.07 / 0.63 / 0.48 (endpoint); the tall graph 0.70 / 0.59 / 0.81 / 0.79 / - / 0.62 / 0.63; of the allowed 8.

Conditions on the inputs are checked on the CPU by test_pocket_field_host.py (fp32 against fp64 composition <= 5e-4; a reference
without the field misses every graph by more than 10 x 5e-3)."""
import subprocess

import pytest
import torch

import pharmacoforge_amd as pfa
import guidance_ref as G
import pocket_field_ref as F
from helpers import within_budget
from oracle import pf_oracle as O
from test_gpu_guidance import ERR_ARG, ERR_STATE, arrays, check_run
from test_gpu_pinned import bound, engine_for

pytestmark = pytest.mark.gpu

T = F.T


def run_field(eng, n_t, noise, pins, com, restraints, fd, family="tuned", **kw):
    arr, parr, garr = arrays(eng, n_t)
    return eng.sample(arr, n_t, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr,
                      guide_scale=G.GUIDE_SCALE, guide_family=family, field=None if fd is None else F.field_kwargs(fd), **kw)


# 1. whole runs
@pytest.mark.parametrize("ep", [False, True])
def test_field_run_vs_composition(ep):
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_field(eng, T, noise, pins, com, restraints, fd, ep_coord=ep, ep_feat=ep, trajectory=True, energies=True)
    assert eng.train_family() == "tuned" and eng.train_input_grads() is False
    check_run(eng, cfg, got, F.reference(ep), pins, f"field, tuned {'ep' if ep else 'noise'} (k = {k})")
    # ... and it is no rounding error of the run without the field
    un = F.reference(ep, False, False)
    ptr = batch.pharm_ptr.tolist()
    tx = got[2].cpu()
    for g in range(5):
        miss = float((tx[:, ptr[g]:ptr[g + 1]] - un.fx[:, ptr[g]:ptr[g + 1]]).abs().max())
        print(f"graph {g}: the reference without the field is missed by {miss:.3g}")
        assert miss >= 10 * G.TOL
    with pytest.raises(AssertionError):
        torch.testing.assert_close(tx, un.fx, rtol=G.TOL, atol=G.TOL)


def test_field_run_width_generic_family():
    """(64, 32), T = 12, a pinned center, feat_norm_constant 2, the wide family"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_field(eng, G.WIDE_T, noise, pins, com, restraints, fd, family="wide", feat_norm_constant=2.0, trajectory=True, energies=True)
    assert eng.kernel_family(0) == 64
    check_run(eng, cfg, got, F.wide_reference(), pins, f"field (64, 32) (k = {k})")
    with pytest.raises(AssertionError):
        torch.testing.assert_close(got[2].cpu(), F.wide_reference(False).fx, rtol=G.TOL, atol=G.TOL)


# 2. one step read back
def one_step(eng, n_t, noise, pins, com, restraints, fd, ep=False):
    arr, parr, garr = arrays(eng, n_t)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned",
                     field=F.field_kwargs(fd))
    eng.guided_step(arr[0], parr[0], garr[0], noise[1], ep_coord=ep, ep_feat=ep)
    out = tuple(t.cpu() for t in eng.last_guidance()) + (eng.last_field_energies().cpu(),)
    eng.set_train_input_grads(False)
    return out


@pytest.mark.parametrize("ep", [False, True])
def test_one_step_within_the_fp64_budget(ep):
    leg = "field ep" if ep else "field noise"
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    kw = dict(scale=G.GUIDE_SCALE, ep=ep, n_steps=1)
    r32 = F.field_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, fd, **kw)
    r64 = F.field_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, fd, double=True, **kw)
    eng = bound(engine_for(cfg, sd), batch)
    g0, grad, shift, en, e3 = one_step(eng, T, noise, pins, com, restraints, fd, ep=ep)
    within_budget(en, r32.E[0], r64.E[0], f"{leg} E")
    within_budget(g0, r32.g0[0], r64.g0[0], f"{leg} g0")
    within_budget(grad, r32.grad[0], r64.grad[0], f"{leg} grad")
    within_budget(shift, r32.shift[0], r64.shift[0], f"{leg} shift")
    for c, name in enumerate(("restraints", "clash", "complementarity")):
        within_budget(e3[:, c], r32.E3[0][:, c], r64.E3[0][:, c], f"{leg} E3 {name}")
    assert torch.equal((e3[:, 0] + e3[:, 1]) + e3[:, 2], en)          # the total is the documented sum of the three
    # graph 0 has no feature and graph 3's single feature leaves most sets empty: exact zeros where the reference has them
    assert float(e3[0, 2]) == 0.0 and float(e3[0, 0]) == 0.0
    assert bool((e3[:, 2][r64.E3[0][:, 2] == 0] == 0).all())


def test_tall_graph_one_step_and_repeatable():
    """600 atoms (beyond the rows a lane keeps in registers), 64 centers (sixteen per wave), 130 features"""
    cfg, sd, k, batch, noise, pins, com, fd = F.tall_case()
    kw = dict(scale=G.GUIDE_SCALE, n_steps=1)
    r32 = F.field_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, None, fd, **kw)
    r64 = F.field_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, None, fd, double=True, **kw)
    assert float(r64.E3[0][0, 1]) > 0 and float(r64.E3[0][0, 2]) > 0
    eng = bound(engine_for(cfg, sd), batch)
    first = one_step(eng, T, noise, pins, com, None, fd)
    g0, grad, shift, en, e3 = first
    within_budget(en, r32.E[0], r64.E[0], "tall E")
    within_budget(g0, r32.g0[0], r64.g0[0], "tall g0")
    within_budget(grad, r32.grad[0], r64.grad[0], "tall grad")
    within_budget(shift, r32.shift[0], r64.shift[0], "tall shift")
    within_budget(e3[:, 1], r32.E3[0][:, 1], r64.E3[0][:, 1], "tall E3 clash")
    within_budget(e3[:, 2], r32.E3[0][:, 2], r64.E3[0][:, 2], "tall E3 complementarity")
    again = one_step(eng, T, noise, pins, com, None, fd)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


# 3. the terms alone
@pytest.mark.parametrize("leg", ["clash", "comp", "no_restraints"])
def test_single_terms(leg):
    clash, comp, restr = leg != "comp", leg != "clash", leg != "no_restraints"
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case(clash, comp)
    eng = bound(engine_for(cfg, sd), batch)
    got = run_field(eng, T, noise, pins, com, restraints if restr else None, fd, trajectory=True, energies=True)
    check_run(eng, cfg, got, F.reference(False, False, True, clash, comp, restr), pins, f"field, {leg}")
    arr, parr, garr = arrays(eng, T)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints if restr else None, guide_scale=G.GUIDE_SCALE,
                     guide_family="tuned", field=F.field_kwargs(fd))
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    e3 = eng.last_field_energies().cpu()
    eng.set_train_input_grads(False)
    assert bool((e3[:, 1] == 0).all()) != clash and bool((e3[:, 2] == 0).all()) != comp and bool((e3[:, 0] == 0).all()) != restr


# 4. bitwise: a field that weighs nothing, and what surrounds a field run
def test_zero_weights_are_the_run_without_a_field():
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    eng = bound(engine_for(cfg, sd), batch)
    want = run_field(eng, T, noise, pins, com, restraints, None, trajectory=True, energies=True)
    kw = dict(F.field_kwargs(fd), w_clash=0.0, w_comp=0.0)
    arr, parr, garr = arrays(eng, T)
    got = eng.sample(arr, T, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr,
                     guide_scale=G.GUIDE_SCALE, guide_family="tuned", field=kw, trajectory=True, energies=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_no_field_field_no_field_on_one_handle():
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.case()
    eng = bound(engine_for(cfg, sd), batch)
    first = run_field(eng, T, noise, pins, com, restraints, None, trajectory=True, energies=True)
    with pytest.raises(pfa.PfError, match=ERR_STATE):   # the run before had no field
        eng.last_field_energies()
    mid = run_field(eng, T, noise, pins, com, restraints, fd, trajectory=True, energies=True)
    assert not torch.equal(mid[0], first[0])
    again = run_field(eng, T, noise, pins, com, restraints, None, trajectory=True, energies=True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    mid2 = run_field(eng, T, noise, pins, com, restraints, fd, trajectory=True, energies=True)
    for a, b in zip(mid, mid2):
        assert torch.equal(a, b)
    # the step API equals the whole loop bitwise
    arr, parr, garr = arrays(eng, T)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned",
                     field=F.field_kwargs(fd))
    for i in range(T):
        eng.guided_step(arr[i], parr[i], garr[i], noise[1 + i])
    x1, h1 = eng.sample_end()
    eng.set_train_input_grads(False)
    assert torch.equal(x1, mid[0]) and torch.equal(h1, mid[1])
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


# 5. arming, state and argument errors
def test_arming_state_and_argument_errors():
    cfg, sd, k, batch, noise, pins, com, restraints, fd = F.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    eng.set_train_family("wide")
    arr, parr, garr = arrays(eng, G.WIDE_T)
    kw = F.field_kwargs(fd)
    # a plain run in progress stays usable through every refused arming and through an accepted one
    eng.sample_begin(noise[0], init_pharm_com=com)
    eng.denoise_step(arr[0], noise[1])
    before = [t.clone() for t in eng.sample_frame()]
    Np = int(batch.prot_ptr[-1])
    bad_r = torch.full((Np,), 2.0)
    bad_r[5] = -1.0
    nan_x = kw["ph"][1].clone()
    nan_x[2, 1] = float("nan")
    bad_t = kw["ph"][2].clone()
    bad_t[0] = cfg.pharm_nf
    for what, over in {"radius": dict(atom_r=bad_r), "w_clash": dict(w_clash=-1.0), "w_comp": dict(w_comp=float("inf")),
                       "kappa": dict(kappa=0.0), "sharpness": dict(type_sharpness=-0.5),
                       "position": dict(ph=(kw["ph"][0], nan_x, kw["ph"][2])), "type": dict(ph=(kw["ph"][0], kw["ph"][1], bad_t)),
                       "ptr": dict(ph=([0, 9, 5], kw["ph"][1], kw["ph"][2])),
                       "too many": dict(ph=([0, 0, 4097], torch.zeros(4097, 3), torch.zeros(4097, dtype=torch.long))),
                       "dist": dict(dist=[-1.0] * cfg.pharm_nf)}.items():
        with pytest.raises(pfa.PfError, match=ERR_ARG):
            eng.field_next(**dict(kw, **over))
    assert all(torch.equal(a, b) for a, b in zip(before, eng.sample_frame()))
    eng.denoise_step(arr[1], noise[2])                  # nothing was armed: the plain run goes on, and a plain begin is accepted
    eng.sample_begin(noise[0], init_pharm_com=com)
    # armed: the begin of another run kind is PF_ERR_STATE and drops the arming; the run in progress goes on
    eng.denoise_step(arr[0], noise[1])
    state = [t.clone() for t in eng.sample_frame()]
    eng.field_next(**kw)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pocket field"):
        eng.sample_begin(noise[0], init_pharm_com=com)
    assert all(torch.equal(a, b) for a, b in zip(state, eng.sample_frame()))
    eng.denoise_step(arr[1], noise[2])
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)      # dropped: the pinned begin is accepted
    eng.field_next(**kw)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pocket field"):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)
    eng.field_next(**kw)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pocket field"):
        eng.sample(arr, 2, noise, init_pharm_com=com)
    # a bind drops the arming: the guided run behind it has no field
    eng.field_next(**kw)
    bound(eng, batch)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_field_energies()
    plain_g0 = eng.last_guidance()[0].clone()
    # the field ends with its run: armed once, the second guided begin runs without it
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, field=kw)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    assert float(eng.last_field_energies()[:, 1:].abs().max()) > 0
    assert not torch.equal(eng.last_guidance()[0], plain_g0)
    # ... a refused arming inside it leaves it usable, an accepted one is for the NEXT run
    with pytest.raises(pfa.PfError, match=ERR_ARG):
        eng.field_next(**dict(kw, kappa=-1.0))
    eng.field_next(**dict(kw, w_clash=0.0, w_comp=0.0))
    eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    assert float(eng.last_field_energies()[:, 1:].abs().max()) > 0
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)     # consumes it
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    assert float(eng.last_field_energies()[:, 1:].abs().max()) == 0
    assert torch.equal(eng.last_guidance()[0], plain_g0)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_field_energies()
    # the Python layer
    with pytest.raises(ValueError, match="multistep"):
        eng.sample(None, 2, noise, ms_coef_arr=[None, None], field=kw)
    with pytest.raises(ValueError, match="one radius per atom"):
        eng.field_next(atom_r=torch.ones(3), w_clash=1.0)
    with pytest.raises(ValueError, match="match table"):
        eng.field_next(ph=kw["ph"], w_comp=1.0)
    assert eng.xchg_timeouts() == 0


# 6. model level and the command line
def test_model_level_pocket_field():
    """PharmacophoreDiff.sample(pocket_field=...) on two pockets with injected noise: every batch runs guided, with or without
    restraints, and is the engine-level run on the same batch bit for bit; composes with pinned=; refused like restraints."""
    from test_gpu_api import graph_from, make_model
    import dataclasses
    n_t = 12
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    feats = []
    for i, g in enumerate(pockets):                     # receptor features on the graphs: 5 and 3
        n = 5 if i == 0 else 3
        gen = torch.Generator().manual_seed(90 + i)
        x = g.prot_x.mean(dim=0)[None] + 4.0 * torch.randn(n, 3, generator=gen)
        h = torch.nn.functional.one_hot(torch.randint(0, 6, (n,), generator=gen), 6).float()
        feats.append((x.float(), h))
        pockets[i] = dataclasses.replace(g, prot_ph_x=x.float(), prot_ph_h=h, prot_ph_ptr=torch.tensor([0, n]))
    n_pharms = [[3, 5, 4], [4, 3, 6]]
    c0 = pockets[0].prot_x.mean(dim=0).float()
    restraints = [[("repel", None, c0.tolist(), 4.0, 1.0)], None]
    pinned = [(c0[None] + torch.tensor([[1.25, -0.5, 0.75]]), torch.tensor([2]), None), None]
    gen = torch.Generator().manual_seed(11)
    nz = [torch.randn(n_t + 1, 12, 9, generator=gen), torch.randn(n_t + 1, 13, 9, generator=gen)]
    kw = dict(max_batch_size=3, lanes=2, noise=nz)
    pf = pfa.PocketField(clash_radius=2.0, clash_weight=1.0, comp_weight=0.25, kappa=4.0, type_sharpness=4.0)
    out = m.sample(pockets, n_pharms, pocket_field=pf, restraints=restraints, pinned=pinned, guide_scale=2.0, guide_clip=1.5,
                   guide_family="tuned", **kw)
    plain = m.sample(pockets, n_pharms, restraints=restraints, pinned=pinned, guide_scale=2.0, guide_clip=1.5, guide_family="tuned", **kw)
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    for o, q in zip(out, plain):                        # both pockets moved: the one without restraints runs guided too
        assert any(not torch.equal(a.ph_coords, b.ph_coords) for a, b in zip(o, q))
    for p in out[0]:
        assert torch.equal(p.ph_coords[:1], pinned[0][0]) and bool(torch.isfinite(p.ph_coords).all())
    with pytest.raises(ValueError, match="resampling"):
        m.sample(pockets, n_pharms, pocket_field=pf, pinned=pinned, pin_resamples=2, **kw)
    with pytest.raises(ValueError, match="multistep"):
        m.sample(pockets, n_pharms, pocket_field=pf, sample_steps=4, sampler="multistep", **kw)
    bare = [dataclasses.replace(g, prot_ph_x=None, prot_ph_h=None, prot_ph_ptr=None) for g in pockets]
    with pytest.raises(ValueError, match="receptor features"):
        m.sample(bare, n_pharms, pocket_field=pf, **kw)
    # composes with few-step sampling: finite, and moved by the field ('ancestral': the shift scales with the posterior variance,
    # which 'ddim' at eta = 0 makes zero -- as for restraints)
    fs = dict(kw, noise=[t[:5] for t in nz], sample_steps=4, sampler="ancestral")
    a = m.sample(pockets, n_pharms, pocket_field=pf, guide_family="tuned", **fs)
    b = m.sample(pockets, n_pharms, **fs)
    assert all(bool(torch.isfinite(p.ph_coords).all()) for o in a for p in o)
    assert any(not torch.equal(p.ph_coords, q.ph_coords) for p, q in zip(a[1], b[1]))
    # the engine-level runs on the same batches, on the handle the model's lane 0 uses
    gamma = m.gamma.gamma
    order = list(reversed(range(n_t)))
    match, dist = pfa.analysis.complementarity_tables()
    for r in (0, 1):
        g0 = m._with_pins(pockets, n_pharms, pinned)[r]
        batch_g = pfa.batch(pfa.copy_graph(g0, n_copies=3, pharm_feats_per_copy=torch.tensor(n_pharms[r])))
        eng = m.dynamics.bind_graph(batch_g)
        arr = eng.coef_array(m.step_coefficients(), order)
        parr = eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order)
        garr = eng.guide_coef_array(pfa.schedule.guide_coefficients(gamma, n_t), order)
        com = pockets[r].prot_x.mean(dim=0).float().repeat(3, 1)
        n = feats[r][0].shape[0]
        field = dict(atom_r=2.0, w_clash=1.0, ph=([0, n, 2 * n, 3 * n], feats[r][0].repeat(3, 1), feats[r][1].argmax(dim=1).repeat(3)),
                     match=match, dist=dist, w_comp=0.25, kappa=4.0, type_sharpness=4.0 * float(m.pharm_feat_norm_constant))
        pins = None if batch_g.pharm_pin is None else (batch_g.pharm_pin, batch_g.pharm_pin_x, batch_g.pharm_pin_h)
        x0, h0 = eng.sample(arr, n_t, nz[r], init_pharm_com=com, ep_coord=m.endpoint_param_coord, ep_feat=m.endpoint_param_feat,
                            feat_norm_constant=float(m.pharm_feat_norm_constant), pins=pins, pin_coef_arr=parr,
                            restraints=[restraints[r]] * 3, guide_coef_arr=garr, guide_scale=2.0, guide_clip=1.5, guide_family="tuned",
                            field=field)
        eng.sample_status()
        x0, h0 = x0.cpu(), h0.cpu()
        ptr = batch_g.pharm_ptr.tolist()
        for i, p in enumerate(out[r]):
            assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.equal(p.g.pharm_h0, h0[ptr[i]:ptr[i + 1]])


def test_cli_with_avoid_clashes(tmp_path):
    """generate_pharmacophores.py --avoid_clashes writes the pharms.xyz the reference composition predicts (the pattern of
    test_gpu_guidance.test_cli_with_restraints: same files, same seed, same draws), and the clash columns of scores.tsv.  The
    seeded random weights of this fixture throw the centers hundreds of angstroms from the pocket, so the radius is chosen to reach
    them (450, with a weight of 0.001): the test is about the path from the flags to the kernel, not about chemistry."""
    import os
    import sys
    import yaml
    from test_gpu_api import _write_pocket_files
    from pharmacoforge_amd import pocket_io as P
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_pocket_files(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    n_t = 12
    cfg['diffusion']['n_timesteps'] = n_t
    cfg['dataset']['pocket_cutoff'] = 8
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True)
    yaml.dump(cfg, open(run / "config.yaml", "w"))
    m = pfa.model_from_config(cfg)
    sd = dict(O.make_state_dict(O.DynamicsConfig(), 0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m.save_checkpoint(run / "checkpoints" / "last.ckpt")
    emap, _ = P.get_prot_atom_ph_type_maps(cfg['dataset'])
    res = P.select_pocket_residues(P.read_pdb(tmp_path / "rec.pdb"), P.parse_ligand(tmp_path / "lig.sdf", True)[1], 8.0)
    pos = torch.tensor([a.coord.tolist() for r in res for a in r.atoms])
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
           str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "3", "--pharm_sizes", "3", "4", "5",
           "--max_batch_size", "3", "--output_dir", str(out), "--seed", "1", "--avoid_clashes", "450", "--clash_weight", "0.001",
           "--guide_scale", "2.0", "--guide_clip", "1.0", "--guide_family", "tuned", "--score_samples", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "clash energy per sample" in r.stdout
    xyz = (out / "rec" / "pharms.xyz").read_text().splitlines()
    e = O.radius_graph(pos, 3.5, torch.tensor([0, pos.shape[0]]), 100)
    pk = P.process_ligand_and_pocket(tmp_path / "rec.pdb", None, emap, cfg['graph']['graph_cutoffs'], 8.0, lig_file=tmp_path / "lig.sdf",
                                     pp_edges=(e[0], e[1]))
    pocket1 = O.PocketBatch(pk.prot_x, pk.prot_h, torch.tensor([0, pk.prot_x.shape[0]]), torch.tensor([0, 1]), pk.pp_src.long(), pk.pp_dst.long())
    torch.manual_seed(1)
    nz = torch.randn(n_t + 1, 12, 9, device="cuda").cpu()
    b = O.concat_pockets([O.copy_pocket(pocket1, n) for n in (3, 4, 5)])
    fd = F.make_field(atom_r=torch.full((int(b.prot_ptr[-1]),), 450.0), w_clash=0.001, kappa=4.0,
                      type_sharpness=4.0 * float(m.pharm_feat_norm_constant))
    free = (torch.zeros(12, dtype=torch.int32), torch.zeros(12, 3), torch.zeros(12, 6))
    com = O.segment_mean(b.prot_x, b.prot_ptr)
    prec = float(cfg['diffusion'].get('precision', 1e-5))
    ref = F.field_reference(sd, O.DynamicsConfig(), b, n_t, prec, nz, *free, com, None, fd, scale=2.0, clip=1.0)
    un = F.field_reference(sd, O.DynamicsConfig(), b, n_t, prec, nz, *free, com, None, None)
    assert float((ref.x0 - un.x0).abs().max()) > 0.1     # the field moved the samples
    rows = [l.split() for l in xyz if len(l.split()) == 4]
    assert len(rows) == 12
    scale = max(abs(float(v)) for r in rows for v in r[1:])
    for r, xw, kw in zip(rows, ref.x0.tolist(), ref.h0.argmax(1).tolist()):
        assert r[0] == "PSFNOC"[kw], (r, kw)
        assert all(abs(float(u) - v) <= 5e-3 * max(1.0, scale) for u, v in zip(r[1:], xw)), (r, xw)
    tsv = [l.split("\t") for l in (out / "rec" / "scores.tsv").read_text().splitlines()]
    assert tsv[0][-2:] == ["clash_energy", "clashes"] and len(tsv) == 4
    ptr = b.pharm_ptr.tolist()
    for i, row in enumerate(tsv[1:]):
        e_ref, n_ref = pfa.analysis.clash_energy(ref.x0[ptr[i]:ptr[i + 1]], pk.prot_x, 450.0, 0.001)
        assert int(row[-1]) == n_ref
        assert abs(float(row[-2]) - e_ref) <= 5e-2 * max(1.0, e_ref), (row, e_ref)
