"""Guided sampling on the tuned 128 / 16 kernels (guide_family="tuned": the tuned training forward, k_guide_grad, the tuned
inputs-only backward, the sampler update) against the CPU composition of tests/guidance_ref.py -- the reference, the shape and
the tolerances of tests/test_gpu_guidance.py: the five ragged pockets (48 / 300 / 40 / 64 / 32 atoms, 3 / 8 / 5 / 1 / 6 centers),
precision 0.25, T = 24, the scaled head (on it a run without J(g0) misses the frames by 0.16-1.3, test_guidance_host.py);
rtol = atol = guidance_ref.TOL (5e-3) for whole runs, helpers.within_budget (8 max(e32, 2**-22)) for one step's vectors.

Then what surrounds such a run: a batch without any restraint (shift exactly zero), the step API against the whole loop,
unguided -> guided -> unguided on one handle, the family and the switch restored after success and after an error, the changes
inside a run that a step refuses, a handle of other widths, the model level and the command line.

Measured on the MI355X, worst |error| over x_0, h_0 and all frames: 2.4e-6 (noise; energies 7.6e-6 on values up to 38), 8.9e-6
(endpoint; energies 4.3e-5).  One step against the fp64 reference, ratio to max(e32, 2**-22) of E / g0 / grad / shift: 0.26 / 0.47 /
1.36 / 1.42 (noise), 0.44 / 0.79 / 0.72 / 0.71 (endpoint), of the allowed 8.  Zero restraints against the pinned run on the same
handle: 1.9e-6."""
import pytest
import torch

import pharmacoforge_amd as pfa
import guidance_ref as G
from helpers import within_budget
from oracle import pf_oracle as O
from test_gpu_guidance import ERR_ARG, ERR_STATE, T, arrays, check_run
from test_gpu_pinned import bound, engine_for

pytestmark = pytest.mark.gpu


def run_tuned(eng, n_t, noise, pins, com, restraints, scale=G.GUIDE_SCALE, **kw):
    arr, parr, garr = arrays(eng, n_t)
    return eng.sample(arr, n_t, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr,
                      guide_scale=scale, guide_family="tuned", **kw)


def restored(eng):
    return eng.train_family() == "tuned" and eng.train_input_grads() is False


# 1. whole runs, both parameterisations
@pytest.mark.parametrize("ep", [False, True])
def test_guided_run_vs_composition(ep):
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_tuned(eng, T, noise, pins, com, restraints, ep_coord=ep, ep_feat=ep, trajectory=True, energies=True)
    assert restored(eng)                                # the family and the switch the engine was on are back
    ref = G.reference(ep)
    assert G.TOL == 5e-3
    check_run(eng, cfg, got, ref, pins, f"tuned {'ep' if ep else 'noise'} (k = {k})")
    ptr = batch.pharm_ptr.tolist()
    un = G.reference(ep, False, False)
    for g in range(1, 5):                               # the guidance is no rounding error of the unguided run
        assert float((got[0].cpu()[ptr[g]:ptr[g + 1]] - un.x0[ptr[g]:ptr[g + 1]]).abs().max()) >= 10 * G.TOL


# 2. one guided step, read back
def one_step(eng, n_t, noise, pins, com, restraints, ep=False):
    """sample_begin + the first guided step (s = T - 1) on the tuned family: (g0, grad, shift, E) on the host"""
    arr, parr, garr = arrays(eng, n_t)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned")
    assert eng.train_family() == "tuned" and eng.train_input_grads()
    eng.guided_step(arr[0], parr[0], garr[0], noise[1], ep_coord=ep, ep_feat=ep)
    return tuple(t.cpu() for t in eng.last_guidance())


@pytest.mark.parametrize("ep", [False, True])
def test_one_step_within_the_fp64_budget(ep):
    leg = "tuned ep" if ep else "tuned noise"
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    kw = dict(scale=G.GUIDE_SCALE, fnorm=1.0, ep=ep, n_steps=1)
    r32 = G.guided_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, **kw)
    r64 = G.guided_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, double=True, **kw)
    eng = bound(engine_for(cfg, sd), batch)
    g0, grad, shift, en = one_step(eng, T, noise, pins, com, restraints, ep=ep)
    assert eng.kernel_family(cfg.n_convs) == 0
    within_budget(en, r32.E[0], r64.E[0], f"{leg} E")
    within_budget(g0, r32.g0[0], r64.g0[0], f"{leg} g0")
    within_budget(grad, r32.grad[0], r64.grad[0], f"{leg} grad")
    within_budget(shift, r32.shift[0], r64.shift[0], f"{leg} shift")
    # a graph without restraints inside a guided batch: shift == 0 exactly
    n0 = int(batch.pharm_ptr[1])
    assert bool((shift[:n0] == 0).all()) and bool((g0[:n0] == 0).all()) and float(en[0]) == 0.0
    assert float(shift[n0:].abs().max()) > 0
    x, h = (t.cpu() for t in eng.sample_frame())
    fx_free, fh_free = (pins[0] & 1) == 0, (pins[0] & 2) == 0
    torch.testing.assert_close(x[fx_free], r32.fx[1][fx_free], rtol=G.TOL, atol=G.TOL)
    torch.testing.assert_close(h[fh_free], r32.fh[1][fh_free], rtol=G.TOL, atol=G.TOL)


# 3. no restraint anywhere: a zero upstream gradient in every graph
def test_zero_restraints_agree_with_the_pinned_run():
    cfg, sd, k, batch, noise, pins, com, _ = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, garr = arrays(eng)
    want = eng.sample(arr, T, noise, init_pharm_com=com, trajectory=True, pins=pins, pin_coef_arr=parr)
    got = run_tuned(eng, T, noise, pins, com, [None] * 5, trajectory=True, energies=True)
    assert bool((got[4] == 0).all())
    for t in got:
        assert bool(torch.isfinite(t).all())
    print("tuned, zero restraints against the pinned run, worst |difference|: %.3g"
          % max(float((a - b).abs().max()) for a, b in zip(got[:4], want)))
    for a, b in zip(got[:4], want):
        torch.testing.assert_close(a, b, rtol=G.TOL, atol=G.TOL)
    # one step of such a run, read back: the shift is exactly zero and nothing is non-finite
    g0, grad, shift, en = one_step(eng, T, noise, pins, com, [None] * 5)
    for t in (g0, grad, shift, en):
        assert bool((t == 0).all())
    assert all(bool(torch.isfinite(t).all()) for t in eng.sample_frame())


# 4. what surrounds a guided run
def test_unguided_guided_unguided_on_one_handle():
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, garr = arrays(eng)
    first = eng.sample(arr, T, noise, init_pharm_com=com)
    form = eng.kernel_family(cfg.n_convs)
    guided = run_tuned(eng, T, noise, pins, com, restraints)
    assert eng.kernel_family(cfg.n_convs) == 0 and restored(eng)
    again = eng.sample(arr, T, noise, init_pharm_com=com)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert eng.kernel_family(cfg.n_convs) == form       # the step-end form returns to the merged launch
    assert not torch.equal(guided[0], first[0])
    # the step API equals the whole loop bitwise
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned")
    for i in range(T):
        eng.guided_step(arr[i], parr[i], garr[i], noise[1 + i])
    x1, h1 = eng.sample_end()
    eng.set_train_input_grads(False)
    assert torch.equal(x1, guided[0]) and torch.equal(h1, guided[1])
    # the wide family's run of the same inputs is another summation order of the same mathematics
    wide = eng.sample(arr, T, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr,
                      guide_scale=G.GUIDE_SCALE)
    torch.testing.assert_close(wide[0], guided[0], rtol=G.TOL, atol=G.TOL)
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


def test_family_and_switch_are_restored_and_changes_inside_a_run_are_refused():
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, garr = arrays(eng)
    # after an argument error (a restraint that names a center the graph does not have)
    bad = [None, [("repel", 99, (0, 0, 0), 1.0, 1.0)], None, None, None]
    with pytest.raises(pfa.PfError, match=ERR_ARG):
        run_tuned(eng, T, noise, pins, com, bad)
    assert restored(eng)
    # from the wide family, with the switch already on: both come back as they were
    eng.set_train_family("wide")
    eng.set_train_input_grads(True)
    run_tuned(eng, 2, noise, pins, com, restraints)
    assert eng.train_family() == "wide" and eng.train_input_grads() is True
    eng.set_train_input_grads(False)
    eng.set_train_family("tuned")
    # the tuned family without the switch: refused as ever
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pf_train_set_family"):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints)
    # bf16 selected: PF_ERR_ARG, the message names the precision call
    eng.set_train_precision("bf16")
    with pytest.raises(pfa.PfError, match=r"\(-1\).*pf_train_set_precision"):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_family="tuned")
    eng.set_train_precision("f32")
    # inside a run: the switch off, then the other family -- the step is PF_ERR_STATE and the run goes on once they are back
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned")
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    state = [t.clone() for t in eng.sample_frame()]
    eng.set_train_input_grads(False)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pf_train_set_input_grads"):
        eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    eng.set_train_input_grads(True)
    eng.set_train_family("wide")
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pf_train_set_family"):
        eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    eng.set_train_family("tuned")
    assert all(torch.equal(a, b) for a, b in zip(state, eng.sample_frame()))
    eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    eng.set_train_input_grads(False)
    assert eng.xchg_timeouts() == 0


# 5. routing
def test_other_widths_refuse_the_tuned_family():
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    assert (cfg.n_hidden_scalars, cfg.vector_size) == (64, 32)
    eng = bound(engine_for(cfg, sd), batch)
    with pytest.raises(ValueError, match="128 / vector_size 16"):
        run_tuned(eng, G.WIDE_T, noise, pins, com, restraints)
    with pytest.raises(ValueError, match="128 / vector_size 16"):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_family="tuned")
    assert eng.train_family() == "tuned" and eng.train_input_grads() is False
    # the C ABI itself: the switch on such a handle does not make its tuned family guide
    eng.set_train_input_grads(True)
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints)


def test_model_level_sample_on_the_tuned_family():
    """PharmacophoreDiff.sample(restraints=..., guide_family="tuned"): the batch of the restrained pocket's copies is the
    engine-level tuned run on the same batch, bit for bit; the other pocket's batch runs the default path."""
    from test_gpu_api import graph_from, make_model
    n_t = 12
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[3, 5, 4], [4, 3, 6]]
    c0 = pockets[0].prot_x.mean(dim=0).float()
    restraints = [[("repel", None, c0.tolist(), 4.0, 1.0), ("attract", 2, (c0 + torch.tensor([3.0, 0.0, 1.0])).tolist(), 1.0, 2.0)], None]
    gen = torch.Generator().manual_seed(11)
    nz = [torch.randn(n_t + 1, 12, 9, generator=gen), torch.randn(n_t + 1, 13, 9, generator=gen)]
    kw = dict(max_batch_size=3, lanes=2, noise=nz)
    out = m.sample(pockets, n_pharms, restraints=restraints, guide_scale=2.0, guide_clip=1.5, guide_family="tuned", **kw)
    plain = m.sample(pockets, n_pharms, **kw)
    wide = m.sample(pockets, n_pharms, restraints=restraints, guide_scale=2.0, guide_clip=1.5, **kw)
    for p, q in zip(out[1], plain[1]):                  # the free pocket: the default path's samples
        assert torch.equal(p.ph_coords, q.ph_coords) and torch.equal(p.g.pharm_h0, q.g.pharm_h0)
    assert any(not torch.equal(p.ph_coords, q.ph_coords) for p, q in zip(out[0], plain[0]))
    for p, q in zip(out[0], wide[0]):                   # the two families: the same run in another summation order
        torch.testing.assert_close(p.ph_coords, q.ph_coords, rtol=G.TOL, atol=G.TOL)
    g0 = pockets[0]
    batch_g = pfa.batch(pfa.copy_graph(g0, n_copies=3, pharm_feats_per_copy=torch.tensor(n_pharms[0])))
    eng = m.dynamics.bind_graph(batch_g)
    assert restored(eng)
    gamma = m.gamma.gamma
    order = list(reversed(range(n_t)))
    arr = eng.coef_array(m.step_coefficients(), order)
    parr = eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order)
    garr = eng.guide_coef_array(pfa.schedule.guide_coefficients(gamma, n_t), order)
    com = pockets[0].prot_x.mean(dim=0).float().repeat(3, 1)
    x0, h0 = eng.sample(arr, n_t, nz[0], init_pharm_com=com, ep_coord=m.endpoint_param_coord, ep_feat=m.endpoint_param_feat,
                        feat_norm_constant=float(m.pharm_feat_norm_constant), pin_coef_arr=parr, restraints=[restraints[0]] * 3,
                        guide_coef_arr=garr, guide_scale=2.0, guide_clip=1.5, guide_family="tuned")
    eng.sample_status()
    x0, h0 = x0.cpu(), h0.cpu()
    ptr = batch_g.pharm_ptr.tolist()
    for i, p in enumerate(out[0]):
        assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.equal(p.g.pharm_h0, h0[ptr[i]:ptr[i + 1]])


def test_cli_with_guide_family_tuned(tmp_path):
    """generate_pharmacophores.py --restraints --guide_family tuned writes the pharms.xyz the reference composition predicts (the
    pattern of test_gpu_guidance.test_cli_with_restraints: same files, same seed, same draws)."""
    import os
    import subprocess
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
    c = pos.mean(dim=0)
    text = ("# keep the middle of the pocket free, pull center 1 to one side\n"
            f"repel {c[0]:.3f} {c[1]:.3f} {c[2]:.3f} 3.0 1.0\n"
            f"attract {c[0] + 4:.3f} {c[1]:.3f} {c[2] - 1:.3f} 1.0 2.0 1   # center 1\n")
    (tmp_path / "restraints.txt").write_text(text)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
           str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "3", "--pharm_sizes", "3", "4", "5",
           "--max_batch_size", "3", "--output_dir", str(out), "--seed", "1", "--restraints", str(tmp_path / "restraints.txt"),
           "--guide_scale", "2.0", "--guide_clip", "1.0", "--guide_family", "tuned"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    xyz = (out / "rec" / "pharms.xyz").read_text().splitlines()
    e = O.radius_graph(pos, 3.5, torch.tensor([0, pos.shape[0]]), 100)
    pk = P.process_ligand_and_pocket(tmp_path / "rec.pdb", None, emap, cfg['graph']['graph_cutoffs'], 8.0, lig_file=tmp_path / "lig.sdf",
                                     pp_edges=(e[0], e[1]))
    pocket1 = O.PocketBatch(pk.prot_x, pk.prot_h, torch.tensor([0, pk.prot_x.shape[0]]), torch.tensor([0, 1]), pk.pp_src.long(), pk.pp_dst.long())
    torch.manual_seed(1)
    nz = torch.randn(n_t + 1, 12, 9, device="cuda").cpu()
    b = O.concat_pockets([O.copy_pocket(pocket1, n) for n in (3, 4, 5)])
    restraints = [P.parse_restraints(text)] * 3
    free = (torch.zeros(12, dtype=torch.int32), torch.zeros(12, 3), torch.zeros(12, 6))
    com = O.segment_mean(b.prot_x, b.prot_ptr)
    prec = float(cfg['diffusion'].get('precision', 1e-5))
    ref = G.guided_reference(sd, O.DynamicsConfig(), b, n_t, prec, nz, *free, com, restraints, scale=2.0, clip=1.0)
    un = G.guided_reference(sd, O.DynamicsConfig(), b, n_t, prec, nz, *free, com, None)
    assert float((ref.x0 - un.x0).abs().max()) > 0.1     # the restraints moved the samples
    rows = [l.split() for l in xyz if len(l.split()) == 4]
    assert len(rows) == 12
    scale = max(abs(float(v)) for r in rows for v in r[1:])
    for r, xw, kw in zip(rows, ref.x0.tolist(), ref.h0.argmax(1).tolist()):
        assert r[0] == "PSFNOC"[kw], (r, kw)
        assert all(abs(float(u) - v) <= 5e-3 * max(1.0, scale) for u, v in zip(r[1:], xw)), (r, xw)
