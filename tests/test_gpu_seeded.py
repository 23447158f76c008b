"""Seeded sampling (pf_sample_seed_next): runs that start from a given pharmacophore noised to level a, against the CPU
composition of tests/seeded_ref.py -- resample_ref.resampled_reference's loop with the begin lines of include/pfdyn.h in front.

Shape: resample_ref.case() -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms (the 300-atom one exercises the strided
protein loops of the seed launch) with 3 / 8 / 5 / 1 / 6 centers (the one-center graph's COM is the center itself), T = 24,
precision 0.25, init_pharm_com = pocket mean + 0.5 (so the frame offset D is not zero).  The seed is a pins_for draw: positions =
pocket COM + 1.5 randn, rows = random one-hots.  Tolerances are the project's own: rtol = atol = 5e-3 for whole runs, atol = 2e-2 for
the width-generic family, the fp64 budget of helpers.within_budget where no network output is involved (the begin's own frame).

Conditions on the inputs, checked on the CPU by test_seeded_host.py: the composition in fp64 and in fp32 agrees with itself
within 3.3e-6 on x_0 and h_0 (the bound is 5e-4), and a seed that was not applied moves every center of every multi-center
graph by at least 0.31 A, so the 5e-3 tolerance discriminates.

Measured on the MI355X, worst |error| over x_0, h_0 and all frames: 1.9e-6 (plain runs, a = 1 / 9 / 24, all three legs), 6.0e-7
(pinned), 1.4e-6 (resampled), 4.3e-6 (guided, (64, 32)), 7.2e-7 at (64, 32).  Frame 0 against the fp64 reference: e 8.6e-8 of the
max for x (e32 1.2e-7), 3.1e-8 for h (e32 the same): ratio at most 0.36 of the allowed 8.

A graph of more than 256 centers cannot be bound (at most 64 per graph), so the seed kernel's path through memory is not tested."""
import ctypes

import pytest
import torch

import pharmacoforge_amd as pfa
import seeded_ref as R
from helpers import within_budget
from oracle import pf_oracle as O
from test_gpu_pinned import bound, engine_for, pins_for

pytestmark = pytest.mark.gpu

T, PREC = R.T, R.PREC
ERR_ARG = r"\(-1\)"
L = pfa._lib


def arrays(eng, a, n_t=T, prec=PREC):
    """(coef_arr, pin_coef_arr, guide_coef_arr, seed coefficients) of a seeded run from level a: the steps s = a-1 .. 0"""
    gamma = O.gamma_table(n_t, prec)
    order = list(reversed(range(a)))
    return (eng.coef_array(O.step_coefficients(gamma, n_t), order), eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order),
            eng.guide_coef_array(pfa.schedule.guide_coefficients(gamma, n_t), order), pfa.schedule.seed_coefficients(gamma, n_t, a))


def check(got, ref, what, rtol=5e-3, atol=5e-3):
    got = [t.cpu() for t in got]
    print("%s worst |error|: x0 %.3g h0 %.3g frames x %.3g h %.3g" % ((what,) + tuple(float((a - b).abs().max()) for a, b in zip(got, ref))))
    for a, b in zip(got, ref):
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=rtol, atol=atol)
    assert torch.equal(got[2][-1], got[0]) and torch.equal(got[3][-1], got[1])
    return got


# 1. whole runs
@pytest.mark.parametrize("leg", ["noise", "endpoint", "live"])
@pytest.mark.parametrize("a", [1, 9, 24])
def test_plain_run_vs_composition(a, leg):
    """x_0, h_0 and all a + 1 frames of pf_sample behind pf_sample_seed_next.  fp64 against fp32 composition: at most 3.3e-6."""
    ep, live = leg == "endpoint", leg == "live"
    cfg, sd, batch, noise, seed, pins, com = R.seeded_case()
    eng = bound(engine_for(cfg, R.live_sd()[0] if live else sd), batch)
    arr, _, _, sc = arrays(eng, a)
    got = eng.sample(arr, a, noise[:a + 1], init_pharm_com=com, ep_coord=ep, ep_feat=ep, trajectory=True, seed=seed + (sc,))
    assert eng.xchg_timeouts() == 0
    eng.sample_status()
    check(got, R.reference(a, ep=ep, live=live), f"a {a} {leg}")


def test_pinned_run():
    """a = 9 with resample_ref's flags: the pins act from the first step on, the begin does not look at them"""
    cfg, sd, batch, noise, seed, pins, com = R.seeded_case()
    a = 9
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, _, sc = arrays(eng, a)
    got = eng.sample(arr, a, noise[:a + 1], init_pharm_com=com, trajectory=True, pins=pins, pin_coef_arr=parr, seed=seed + (sc,))
    eng.sample_status()
    ref = R.reference(a, pinned=True)
    x0, h0, tx, th = check(got, ref, "pinned a 9")
    flags, pin_x, pin_h = pins
    mx, mh = (flags & 1) != 0, (flags & 2) != 0
    assert torch.equal(x0[mx], pin_x[mx]) and torch.equal(h0[mh], pin_h[mh])
    assert not torch.equal(tx[0][mx], pin_x[mx])        # the initial frame is the noised seed, pinned centers included
    assert eng.kernel_family(cfg.n_convs) == 0


def test_resampled_run():
    """plan_of(9, 5, 3): segments (9, 4) and (4, 0), three passes each -- 31 ops behind the seeded begin"""
    cfg, sd, batch, noise, seed, pins, com = R.seeded_case()
    a = 9
    plan = R.plan_of(a, 5, 3)
    assert len(plan) == 31 and plan == pfa.schedule.resample_plan(a, 5, 3)
    eng = bound(engine_for(cfg, sd), batch)
    gamma = O.gamma_table(T, PREC)
    pairs = [(op[1], op[2]) for op in plan if op[0] == "renoise"]
    arr, parr, op_arr, re_arr = eng.plan_arrays(plan, O.step_coefficients(gamma, T), pfa.schedule.pin_coefficients(gamma, T),
                                                pfa.schedule.renoise_coefficients(gamma, T, pairs))
    sc = pfa.schedule.seed_coefficients(gamma, T, a)
    got = eng.sample(arr, len(plan), noise[:len(plan) + 1], init_pharm_com=com, trajectory=True, pins=pins, pin_coef_arr=parr,
                     plan=(op_arr, re_arr), seed=seed + (sc,))
    eng.sample_status()
    check(got, R.reference(a, pinned=True, plan=tuple(plan)), "resampled a 9")


def wide_inputs():
    """guidance_ref.wide_case(): (64, 32), two pockets of 40 / 56 atoms with 3 / 5 centers, T = 12, the scaled head, one pinned
    center, feat_norm 2; its pin arrays are a pins_for draw for every center and serve as the seed"""
    import guidance_ref as G
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    return G, cfg, sd, batch, noise, (pins[1], pins[2]), pins, com, restraints


def test_guided_run():
    """a = 9 of T = 12 on the wide family, against guidance_ref's step with the seeded begin in front"""
    G, cfg, sd, batch, noise, seed, pins, com, restraints = wide_inputs()
    a, n_t, fnorm = 9, G.WIDE_T, 2.0
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, garr, sc = arrays(eng, a, n_t)
    got = eng.sample(arr, a, noise[:a + 1], init_pharm_com=com, feat_norm_constant=fnorm, trajectory=True, pins=pins, pin_coef_arr=parr,
                     restraints=restraints, guide_coef_arr=garr, guide_scale=G.GUIDE_SCALE, seed=seed + (sc,))
    eng.sample_status()
    kw = dict(fnorm=fnorm, restraints=restraints, scale=G.GUIDE_SCALE)
    ref = R.seeded_reference(sd, cfg, batch, n_t, PREC, a, R.steps_of(a), noise[:a + 1], seed, pins, com, **kw)
    check(got, ref, "guided a 9 (64, 32)")
    un = R.seeded_reference(sd, cfg, batch, n_t, PREC, a, R.steps_of(a), noise[:a + 1], None, pins, com, **kw)
    assert float((ref[0] - un[0]).abs().max()) > 0.1     # the seed is no rounding error of the unseeded guided run


def test_width_generic_family():
    """(64, 32): the move runs alone (k_step_update<MoveSeed>), the family launches its own encoders and edge build.  A plain and a
    pinned run at a = 7 of T = 12; the given rows are divided by a feat_norm_constant of 2."""
    G, cfg, sd, batch, noise, seed, pins, com, _ = wide_inputs()
    a, n_t, fnorm = 7, G.WIDE_T, 2.0
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, _, sc = arrays(eng, a, n_t)
    for pinned in (False, True):
        kw = dict(pins=pins, pin_coef_arr=parr) if pinned else {}
        got = eng.sample(arr, a, noise[:a + 1], init_pharm_com=com, feat_norm_constant=fnorm, trajectory=True, seed=seed + (sc,), **kw)
        assert eng.kernel_family(0) == 64
        ref = R.seeded_reference(sd, cfg, batch, n_t, PREC, a, R.steps_of(a), noise[:a + 1], seed, pins if pinned else None, com, fnorm=fnorm)
        check(got, ref, f"wide a 7 pinned {pinned}", rtol=0, atol=2e-2)


# 2. the begin's own output
@pytest.mark.parametrize("com_given", [True, False])
def test_frame_0_within_the_fp64_budget(com_given):
    """No network output is involved in the initial frame, so the fp64 budget applies (e <= 8 max(e32, 2**-22)): the noised seed
    in the caller's frame, on the tuned family (the move + the edge build) -- with init_pharm_com given (D = the offset) and
    without (the protein's own mean: D = 0 up to rounding).  The state's own rows are dead for the move: a run in front of it
    must not show."""
    cfg, sd, batch, noise, seed, pins, com = R.seeded_case()
    a = 9
    init = com if com_given else O.segment_mean(batch.prot_x, batch.prot_ptr)
    r32 = R.seeded_reference(sd, cfg, batch, T, PREC, a, [], noise[:1], seed, None, init)
    r64 = R.seeded_reference(sd, cfg, batch, T, PREC, a, [], noise[:1], seed, None, init, double=True)
    eng = bound(engine_for(cfg, sd), batch)
    arr, _, _, sc = arrays(eng, a)
    eng.sample(arr, a, noise[:a + 1], init_pharm_com=com)          # something else in the state
    eng.sample_begin(noise[0], init_pharm_com=com if com_given else None, seed=seed + (sc,))
    x, h = eng.sample_frame()
    print("frame 0 worst deviation: x %.3g h %.3g" % (float((x.cpu() - r32[2][0]).abs().max()), float((h.cpu() - r32[3][0]).abs().max())))
    within_budget(x, r32[2][0], r64[2][0], "frame 0 x")
    within_budget(h, r32[3][0], r64[3][0], "frame 0 h")
    # the edges the move's launch built are the oracle's on the composition's coordinates
    from helpers import edge_set
    bidx = batch.batch_idxs()
    c_init = O.segment_mean(batch.prot_x, batch.prot_ptr)
    prot0 = batch.prot_x - init[bidx["prot"]]
    prot_x, x_s, _ = R.seeded_begin(batch, bidx, c_init, prot0, *R.seed_coef(O.gamma_table(T, PREC), T, a), seed[0], seed[1], noise[0], 1.0)
    edges = O.build_dynamic_edges(cfg, batch, prot_x, x_s)
    for i, et in enumerate(("ff", "pf", "fp")):
        s, d = eng.get_edges(i)
        assert edge_set(s, d) == edge_set(*edges[et]), et
        assert s.numel() == edges[et][0].numel() > 0
    # ... and the first step reads them
    eng.denoise_step(arr[0], noise[1])
    x1, h1 = (t.cpu() for t in eng.sample_frame())
    ref1 = R.seeded_reference(sd, cfg, batch, T, PREC, a, R.steps_of(a)[:1], noise[:2], seed, None, init)
    torch.testing.assert_close(x1, ref1[2][1], rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(h1, ref1[3][1], rtol=5e-3, atol=5e-3)


# 3. bitwise and state checks
def n16_inputs():
    """test_gpu_n16.py:413's handle, whose plain runs take the merged launch: four pockets of 64 atoms, T = 100"""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 3)
    batch = O.synthetic_batch([700 + i for i in range(4)], 64, [4, 6, 5, 6], cfg)
    Nf = int(batch.pharm_ptr[-1])
    noise = torch.randn(5, Nf, 9, generator=torch.Generator().manual_seed(17))
    _, seed_x, seed_h = pins_for(batch, cfg, [0] * Nf)
    return cfg, sd, batch, noise, (seed_x, seed_h)


def test_seeded_plain_run_is_on_the_tuned_path():
    """After a seeded plain run kernel_family(n_convs) == 2: the merged last launch ran, as in an unseeded run.  And the center
    hoist is on from the first step: the snapshot its workgroups read is the one the seed move wrote."""
    cfg, sd, batch, noise, seed = n16_inputs()
    n_t, a = 100, 4
    eng = bound(engine_for(cfg, sd), batch)
    arr, _, _, sc = arrays(eng, a, n_t, 1e-5)
    eng.sample(arr, a, noise)
    assert eng.kernel_family(cfg.n_convs) == 2                      # the merged launch is what an unseeded run takes here
    eng.sample_begin(noise[0])
    eng.prepare_timesteps(arr)
    eng.denoise_step(arr[0], noise[1])
    hoist = eng.ahead()["center_hoist"]
    x0, h0 = eng.sample(arr, a, noise, seed=seed + (sc,))
    assert eng.kernel_family(cfg.n_convs) == 2
    eng.sample_begin(noise[0], seed=seed + (sc,))
    eng.prepare_timesteps(arr)
    eng.denoise_step(arr[0], noise[1])
    assert eng.kernel_family(cfg.n_convs) == 2
    assert eng.ahead()["center_hoist"] == hoist                     # what the unseeded first step hoists, the seeded one does
    for i in range(1, a):
        eng.denoise_step(arr[i], noise[1 + i])
    x1, h1 = eng.sample_end()
    assert torch.equal(x0, x1) and torch.equal(h0, h1)              # the whole-loop entry is arm + begin + steps + end, bitwise
    ref = R.seeded_reference(sd, cfg, batch, n_t, 1e-5, a, R.steps_of(a), noise, seed, None, O.segment_mean(batch.prot_x, batch.prot_ptr))
    torch.testing.assert_close(x0.cpu(), ref[0], rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(h0.cpu(), ref[1], rtol=5e-3, atol=5e-3)
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


def raw_seed_next(eng, coef, sx, sh, fnorm):
    with torch.cuda.device(eng.device):
        return eng.lib.pf_sample_seed_next(eng._h, None if coef is None else ctypes.byref(coef), None if sx is None else sx.data_ptr(),
                                           None if sh is None else sh.data_ptr(), float(fnorm), pfa.engine._stream_ptr())


def test_seed_is_consumed_and_argument_errors():
    cfg, sd, batch, noise, seed, pins, com = R.seeded_case()
    a = 9
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, _, sc = arrays(eng, a)
    nz = noise[:a + 1]
    plain = eng.sample(arr, a, nz, init_pharm_com=com)
    seeded = eng.sample(arr, a, nz, init_pharm_com=com, seed=seed + (sc,))
    assert not torch.equal(plain[0], seeded[0])
    # consumed: a second, unarmed run on the same handle is the unseeded run
    again = eng.sample(arr, a, nz, init_pharm_com=com)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    # arm -> a begin that is rejected -> an unarmed run: unseeded
    eng.seed_next(seed[0], seed[1], sc)
    with torch.cuda.device(eng.device):
        assert eng.lib.pf_sample_begin(eng._h, None, None, pfa.engine._stream_ptr()) == -1          # null noise
    again = eng.sample(arr, a, nz, init_pharm_com=com)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    # ... a rejected pinned begin consumes it too
    eng.seed_next(seed[0], seed[1], sc)
    with pytest.raises(pfa.PfError, match=ERR_ARG):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, feat_norm_constant=0.0)
    again = eng.sample(arr, a, nz, init_pharm_com=com)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    # arm -> bind -> begin: unseeded
    eng.seed_next(seed[0], seed[1], sc)
    bound(eng, batch)
    again = eng.sample(arr, a, nz, init_pharm_com=com)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    # every PF_ERR_ARG case leaves a run in progress usable, and arms nothing
    dev = eng.device
    sx, sh = seed[0].to(dev).contiguous(), seed[1].to(dev).contiguous()
    ok = L.PfSeedCoef(float(sc["alpha_a"]), float(sc["sigma_a"]))
    nan, inf = float("nan"), float("inf")
    bad = [(None, sx, sh, 1.0), (ok, None, sh, 1.0), (ok, sx, None, 1.0), (ok, sx, sh, 0.0), (ok, sx, sh, -1.0), (ok, sx, sh, nan),
           (L.PfSeedCoef(nan, 0.5), sx, sh, 1.0), (L.PfSeedCoef(0.5, nan), sx, sh, 1.0), (L.PfSeedCoef(inf, 0.5), sx, sh, 1.0),
           (L.PfSeedCoef(0.5, inf), sx, sh, 1.0), (L.PfSeedCoef(0.0, 0.5), sx, sh, 1.0), (L.PfSeedCoef(-0.5, 0.5), sx, sh, 1.0),
           (L.PfSeedCoef(0.5, -0.1), sx, sh, 1.0)]
    eng.sample_begin(noise[0], init_pharm_com=com)
    eng.prepare_timesteps(arr)
    for i in range(a):
        if i < len(bad):
            assert raw_seed_next(eng, *bad[i]) == -1, i
        eng.denoise_step(arr[i], noise[1 + i])
    for args in bad[a:]:
        assert raw_seed_next(eng, *args) == -1
    x, h = eng.sample_end()
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    again = eng.sample(arr, a, nz, init_pharm_com=com)
    assert torch.equal(again[0], plain[0])
    # sigma_a = 0 is allowed: the begin's frame is the seed itself in the caller's frame (up to the rounding of the frame change)
    eng.sample_begin(noise[0], init_pharm_com=com, seed=seed + ((1.0, 0.0),))
    x, h = eng.sample_frame()
    torch.testing.assert_close(x.cpu(), seed[0], rtol=0, atol=1e-4)
    assert torch.equal(h.cpu(), seed[1])
    # an armed seed outlives a run in progress on the handle: arming between two steps seeds the NEXT begin
    eng.sample_begin(noise[0], init_pharm_com=com)
    eng.denoise_step(arr[0], noise[1])
    eng.seed_next(seed[0], seed[1], sc)
    for i in range(1, a):
        eng.denoise_step(arr[i], noise[1 + i])
    x, h = eng.sample_end()
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    x, h = eng.sample(arr, a, nz, init_pharm_com=com)
    assert torch.equal(x, seeded[0]) and torch.equal(h, seeded[1])
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


# 4. model level and the command line
def test_model_level_seeded_sample():
    """PharmacophoreDiff.sample(seeds=..., seed_level=8) on two pockets with injected noise: every batch is the engine-level
    seeded run on the same batch and noise, bit for bit -- plain, and with seed_keep (a pinned run whose kept centers come back
    bit for bit)."""
    from test_gpu_api import graph_from, make_model
    n_t, a = 20, 8
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[4, 4, 4], [5, 5]]
    gen = torch.Generator().manual_seed(5)
    seeds = [(g.prot_x.mean(dim=0).float() + 1.5 * torch.randn(n, 3, generator=gen), torch.randint(0, 6, (n,), generator=gen))
             for g, n in zip(pockets, (4, 5))]
    nz = [torch.randn(a + 1, 12, 9, generator=gen), torch.randn(a + 1, 10, 9, generator=gen)]
    kw = dict(max_batch_size=3, lanes=2, noise=nz, seeds=seeds, seed_level=a)
    gamma = m.gamma.gamma
    order = list(reversed(range(a)))
    sc = pfa.schedule.seed_coefficients(gamma, n_t, a)
    unseeded = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2,
                        noise=[torch.cat([z, torch.randn(n_t - a, *z.shape[1:], generator=gen)]) for z in nz])
    for keep in (None, [[0, 2], []]):
        out = m.sample(pockets, n_pharms, seed_keep=keep, **kw)
        assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
        for r in range(2):
            g0 = m._with_seeds(pockets, n_pharms, seeds, keep)[r]
            n = len(n_pharms[r])
            batch_g = pfa.batch(pfa.copy_graph(g0, n_copies=n, pharm_feats_per_copy=torch.tensor(n_pharms[r])))
            eng = m.dynamics.bind_graph(batch_g)
            arr = eng.coef_array(m.step_coefficients(), order)
            pk = {}
            if keep is not None and keep[r]:
                pk = dict(pins=(batch_g.pharm_pin, batch_g.pharm_pin_x, batch_g.pharm_pin_h),
                          pin_coef_arr=eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order))
            com = pockets[r].prot_x.mean(dim=0).float().repeat(n, 1)
            x0, h0 = eng.sample(arr, a, nz[r], init_pharm_com=com, ep_coord=m.endpoint_param_coord, ep_feat=m.endpoint_param_feat,
                                feat_norm_constant=float(m.pharm_feat_norm_constant), seed=(batch_g.pharm_pin_x, batch_g.pharm_pin_h, sc), **pk)
            eng.sample_status()
            x0, h0 = x0.cpu(), h0.cpu()
            ptr = batch_g.pharm_ptr.tolist()
            for i, p in enumerate(out[r]):
                assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.equal(p.g.pharm_h0, h0[ptr[i]:ptr[i + 1]])
                assert torch.isfinite(p.ph_coords).all()
                if keep is not None and keep[r]:
                    assert torch.equal(p.ph_coords[keep[r]], seeds[r][0][keep[r]])
                    assert p.ph_feats_idxs[keep[r]].tolist() == seeds[r][1][keep[r]].tolist()
        assert all(not torch.equal(p.ph_coords, q.ph_coords) for o, u in zip(out, unseeded) for p, q in zip(o, u))


def test_cli_with_a_seed(tmp_path):
    """generate_pharmacophores.py --seed_pharmacophore writes the pharms.xyz the reference composition predicts (the pattern of
    test_gpu_guidance.test_cli_with_restraints: same files, same seed, same draws); with --seed_keep the kept center comes back
    as the file has it."""
    import os
    import subprocess
    import sys
    import yaml
    from test_gpu_api import _write_pocket_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_pocket_files(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    n_t, a = 12, 7
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
    from pharmacoforge_amd import pocket_io as P
    emap, _ = P.get_prot_atom_ph_type_maps(cfg['dataset'])
    res = P.select_pocket_residues(P.read_pdb(tmp_path / "rec.pdb"), P.parse_ligand(tmp_path / "lig.sdf", True)[1], 8.0)
    pos = torch.tensor([a_.coord.tolist() for r in res for a_ in r.atoms])
    c = pos.mean(dim=0)
    off = torch.tensor([[1.5, 0.0, -1.0], [-2.0, 1.0, 0.5], [0.25, -1.75, 2.0], [0.0, 2.5, 1.0]])
    elems = "PNCO"
    text = "4\n" + "".join(f"{e} {x:.3f} {y:.3f} {z:.3f}\n" for e, (x, y, z) in zip(elems, (c + off).tolist()))
    (tmp_path / "seed.xyz").write_text(text)
    from pharmacoforge_amd.analysis import read_pinned_centers
    seed_x, seed_t = read_pinned_centers(tmp_path / "seed.xyz")
    e = O.radius_graph(pos, 3.5, torch.tensor([0, pos.shape[0]]), 100)
    pk = P.process_ligand_and_pocket(tmp_path / "rec.pdb", None, emap, cfg['graph']['graph_cutoffs'], 8.0, lig_file=tmp_path / "lig.sdf",
                                     pp_edges=(e[0], e[1]))
    pocket1 = O.PocketBatch(pk.prot_x, pk.prot_h, torch.tensor([0, pk.prot_x.shape[0]]), torch.tensor([0, 1]), pk.pp_src.long(), pk.pp_dst.long())
    b = O.concat_pockets([O.copy_pocket(pocket1, 4) for _ in range(3)])
    com = O.segment_mean(b.prot_x, b.prot_ptr)
    prec = float(cfg['diffusion'].get('precision', 1e-5))
    seed = (seed_x.repeat(3, 1), torch.nn.functional.one_hot(seed_t, 6).float().repeat(3, 1))
    flags = torch.tensor([0, 3, 0, 0] * 3, dtype=torch.int32)
    for keep in ("1",):                                 # (one child process: the seeded pinned run covers the seed and the kept center)
        out = tmp_path / "out"
        cmd = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
               str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "3", "--max_batch_size", "3", "--output_dir", str(out),
               "--seed", "1", "--seed_pharmacophore", str(tmp_path / "seed.xyz"), "--seed_level", str(a)] + ([] if keep is None else ["--seed_keep", keep])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        xyz = (out / "rec" / "pharms.xyz").read_text().splitlines()
        torch.manual_seed(1)
        nz = torch.randn(a + 1, 12, 9, device="cuda").cpu()
        pins = None if keep is None else (flags,) + seed
        ref = R.seeded_reference(sd, O.DynamicsConfig(), b, n_t, prec, a, R.steps_of(a), nz, seed, pins, com)
        un = R.seeded_reference(sd, O.DynamicsConfig(), b, n_t, prec, a, R.steps_of(a), nz, None, pins, com)
        assert float((ref[0] - un[0]).abs().max()) > 0.1     # the seed moved the samples
        rows = [l.split() for l in xyz if len(l.split()) == 4]
        assert len(rows) == 12
        scale = max(abs(float(v)) for r_ in rows for v in r_[1:])
        for r_, xw, kw in zip(rows, ref[0].tolist(), ref[1].argmax(1).tolist()):
            assert r_[0] == "PSFNOC"[kw], (r_, kw)
            assert all(abs(float(u) - v) <= 5e-3 * max(1.0, scale) for u, v in zip(r_[1:], xw)), (r_, xw)
        if keep is not None:
            want = text.splitlines()[2].split()
            for i in (1, 5, 9):
                assert rows[i][0] == want[0] and [float(v) for v in rows[i][1:]] == [float(v) for v in want[1:]]
