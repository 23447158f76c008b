"""Few-step sampling on the device: strided first-order runs (ancestral, DDIM) through pf_sample, and the multistep move
(pf_denoise_step_ms / pf_sample_ms), against the CPU composition of tests/fewstep_ref.py.

Shapes, the project's smallest that still reach every loop: resample_ref.case() -- five ragged pockets of 48 / 300 / 40 / 64 / 32
atoms (the 300-atom one exercises the strided protein loop of the move) with 3 / 8 / 5 / 1 / 6 centers (the one-center graph's COM
is the center itself), T = 24, precision 0.25, init_pharm_com = pocket mean + 0.5 -- with the scaled head of resample_ref.live_sd,
so that eps_x is of order one and the previous output's term counts in the coordinates; guidance_ref.wide_case() ((64, 32),
T = 12); test_gpu_n16.py's merged-launch handle (four pockets of 64 atoms, T = 100).  At most 64 centers per graph can be bound,
so the move's loop for more than 256 centers of a graph is never taken.

Tolerance: the project's own for whole runs, rtol = atol = 5e-3 against the fp32 composition (test_gpu_seeded.check).  Every
comparison asserts first, on the CPU references, that the composition differs from its nearest wrong neighbour -- c1 forced to
0, unit-stride coefficients at the strided levels, eta = 1 in place of the run's -- by at least ten times that on some center.

Measured on the MI355X, worst |error| over x_0, h_0 and all frames: 1.4e-6 for every T = 24 run (ancestral in the three spacings,
DDIM eta 0 / 0.5, multistep N = 6 / 8 in the three parameterisations, hybrid, seeded) and at (64, 32); 1.5e-4 on values of several
hundred on the merged-launch handle (T = 100, precision 1e-5).  The smallest wrong-neighbour gap is 0.064 A (c1 = 0 in the hybrid
and the seeded run), 13 times the tolerance."""
import pytest
import torch

import pharmacoforge_amd as pfa
import fewstep_ref as F
import resample_ref as RR
from oracle import pf_oracle as O
from test_gpu_pinned import bound, engine_for
from test_gpu_seeded import check

pytestmark = pytest.mark.gpu

S = pfa.schedule
T, PREC, TOL = F.T, F.PREC, F.TOL
ERR_STATE = r"\(-3\)"
PARAMS = {"noise": (False, False), "endpoint_x": (True, False), "endpoint": (True, True)}


def gamma_of(n_t=T, prec=PREC):
    return O.gamma_table(n_t, prec)


def live_case():
    cfg, sd, batch, plan, noise, pins, com = RR.case()
    return cfg, RR.live_sd()[0], batch, noise, (pins[1], pins[2]), com


def first_arr(eng, lv, eta=1.0, n_t=T, prec=PREC):
    return eng.coef_array(S.strided_coefficients(gamma_of(n_t, prec), n_t, lv, eta), range(len(lv) - 1))


def ms_arr(eng, lv, ep=(False, False), n_t=T, prec=PREC):
    return eng.ms_coef_array(S.multistep_coefficients(gamma_of(n_t, prec), n_t, lv, *ep))


def discriminates(ref, wrong, what):
    gx, gh = F.worst_center_gap(ref, wrong)
    print(f"{what}: the wrong neighbour is off by {gx:.3g} (x_0) / {gh:.3g} (h_0)")
    assert max(gx, gh) >= 10 * TOL, (what, gx, gh)


# 1. strided ancestral runs
@pytest.mark.parametrize("spacing", ["uniform", "quadratic", "logsnr"])
def test_strided_ancestral_run(spacing):
    """N = 6 of 24: pf_sample with strided arrays, x_0, h_0 and all seven frames"""
    cfg, sd, batch, noise, seed, com = live_case()
    lv = S.level_plan(T, 6, spacing, gamma_table=gamma_of())
    ops = tuple(F.first_ops(lv))
    ref = F.reference(ops)
    discriminates(ref, F.reference(ops, wrong="unit_stride"), f"ancestral {spacing} {lv}")
    eng = bound(engine_for(cfg, sd), batch)
    got = eng.sample(first_arr(eng, lv), 6, noise[:7], init_pharm_com=com, trajectory=True)
    eng.sample_status()
    check(got, ref, f"ancestral {spacing}")


# 2. the merged-launch handle
def test_strided_run_stays_on_the_merged_launch():
    """N = 10 of 100 on test_gpu_n16.py's handle: kernel_family(n_convs) == 2 is the merged last launch (only
    merged_step_launch sets it), and the center hoist of the first step is what a unit-stride run's first step hoists -- the work
    done ahead is live at a stride, because the plan's timesteps are announced like any other -- and the next step consumes it
    (kernel_family(n_convs + 1) == 1: conv layer 0 started from the hoisted tables).
    Launch counts: profiling the step class switches the merged launch off, and the encode / build classes change how the forward
    is launched, so a count cannot name the merged launch itself.  What counts can show is asserted: with every OTHER class
    profiled the merged launch stays on, the step class -- the separate update + build launch -- is never entered, and the strided
    run launches per class exactly what a unit-stride run of as many steps launches."""
    from test_gpu_seeded import n16_inputs
    cfg, sd, batch, _, _ = n16_inputs()
    n_t, prec, N = 100, 1e-5, 10
    Nf = int(batch.pharm_ptr[-1])
    noise = torch.randn(N + 1, Nf, 9, generator=torch.Generator().manual_seed(17))
    com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    lv = F.uniform_plan(n_t, N)
    assert lv == S.level_plan(n_t, N)
    ref = F.fewstep_reference(sd, cfg, batch, n_t, prec, F.first_ops(lv), noise, com)
    discriminates(ref, F.fewstep_reference(sd, cfg, batch, n_t, prec, F.first_ops(lv), noise, com, wrong="unit_stride"), "merged-launch handle")
    eng = bound(engine_for(cfg, sd), batch)
    unit = eng.coef_array(O.step_coefficients(gamma_of(n_t, prec), n_t), reversed(range(n_t)))
    eng.sample_begin(noise[0])
    eng.prepare_timesteps(unit, 4)
    eng.denoise_step(unit[0], noise[1])
    assert eng.kernel_family(cfg.n_convs) == 2
    hoist = eng.ahead()["center_hoist"]
    arr = first_arr(eng, lv, n_t=n_t, prec=prec)
    got = eng.sample(arr, N, noise, trajectory=True)
    assert eng.kernel_family(cfg.n_convs) == 2
    eng.sample_begin(noise[0])
    eng.prepare_timesteps(arr)
    eng.denoise_step(arr[0], noise[1])
    assert eng.kernel_family(cfg.n_convs) == 2
    ahead = eng.ahead()
    print("ahead after the first strided step:", ahead)
    assert ahead["center_hoist"] == hoist and hoist > 0
    for i in range(1, N):
        eng.denoise_step(arr[i], noise[1 + i])
        assert eng.kernel_family(cfg.n_convs) == 2
    x1, h1 = eng.sample_end()
    assert torch.equal(got[0], x1) and torch.equal(got[1], h1)
    assert eng.xchg_timeouts() == 0
    eng.sample_status()
    check(got, ref, "merged-launch handle N 10 of 100")
    classes = eng.KERNEL_CLASSES
    mask = sum(1 << i for i, k in enumerate(classes) if k not in ("encode", "build_edges", "step_update"))

    def counted(coef, what):
        eng.profile_enable(mask)
        eng.sample_begin(noise[0])
        eng.prepare_timesteps(coef, N)
        consumed = []
        for i in range(N):
            eng.denoise_step(coef[i], noise[1 + i])
            assert eng.kernel_family(cfg.n_convs) == 2
            consumed.append((eng.kernel_family(cfg.n_convs + 1), eng.kernel_family(cfg.n_convs + 2)))
        counts = {k: int(n) for k, (_, n) in eng.profile_read().items()}
        res = eng.sample_end()
        eng.profile_enable(0)
        print(f"{what}: launches {counts}; (hoist consumed, rows ahead consumed) per step {consumed}")
        return counts, consumed, res
    c_unit, use_unit, _ = counted(unit, "unit stride")
    c_str, use_str, res = counted(arr, "strided")
    assert c_str == c_unit and c_str["noise_head"] == N and c_str["step_update"] == 0
    assert sum(c_str.values()) == 3 * N                                 # the merged three-launch step
    assert [u[0] for u in use_str] == [u[0] for u in use_unit] and use_str[1][0] == 1
    assert torch.equal(res[0], x1) and torch.equal(res[1], h1)          # counting the other classes changes no bit
    eng.sample_status()


# 3. DDIM runs
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_run(eta):
    cfg, sd, batch, noise, seed, com = live_case()
    lv = F.uniform_plan(T, 6)
    ops = tuple(F.first_ops(lv, eta))
    ref = F.reference(ops)
    discriminates(ref, F.reference(ops, wrong="eta1"), f"ddim eta {eta}")
    eng = bound(engine_for(cfg, sd), batch)
    got = eng.sample(first_arr(eng, lv, eta), 6, noise[:7], init_pharm_com=com, trajectory=True)
    eng.sample_status()
    check(got, ref, f"ddim eta {eta}")


# 4. multistep runs
def ms_loop(eng, arr, noise0, com, **begin):
    """begin + a loop of pf_denoise_step_ms + end, with the frames of a trajectory: (x_0, h_0, frames x, frames h)"""
    eng.sample_begin(noise0, init_pharm_com=com, **begin)
    eng.prepare_timesteps(arr)
    fr = [eng.sample_frame()]
    for c in arr:
        eng.ms_step(c)
        fr.append(eng.sample_frame())
    x0, h0 = eng.sample_end()
    return x0, h0, torch.stack([f[0] for f in fr[:-1]] + [x0]), torch.stack([f[1] for f in fr[:-1]] + [h0])


@pytest.mark.parametrize("param", list(PARAMS))
@pytest.mark.parametrize("N", [6, 8])
def test_multistep_run(N, param):
    """pf_sample_ms and a loop of pf_denoise_step_ms: the same bits, and the composition's frames and results"""
    ep = PARAMS[param]
    cfg, sd, batch, noise, seed, com = live_case()
    lv = F.uniform_plan(T, N)
    ops = tuple(F.ms_ops(lv))
    ref = F.reference(ops, ep=ep)
    discriminates(ref, F.reference(ops, ep=ep, wrong="c1_zero"), f"multistep N {N} {param}")
    eng = bound(engine_for(cfg, sd), batch)
    arr = ms_arr(eng, lv, ep)
    got = eng.sample(None, N, noise[:1], init_pharm_com=com, trajectory=True, ms_coef_arr=arr)
    assert eng.kernel_family(cfg.n_convs) == 0          # the separate launches, as in a pinned run
    eng.sample_status()
    got = check(got, ref, f"multistep N {N} {param}")
    loop = [t.cpu() for t in ms_loop(eng, arr, noise[0], com)]
    for a, b in zip(got, loop):
        assert torch.equal(a, b)


# 5. a hybrid run
def test_plain_then_multistep_steps():
    """two strided ancestral steps, then multistep steps over the rest of the plan (its first one first-order: no history)"""
    cfg, sd, batch, noise, seed, com = live_case()
    lv = F.uniform_plan(T, 6)
    ops = tuple(F.first_ops(lv[:3]) + F.ms_ops(lv[2:]))
    ref = F.reference(ops)
    discriminates(ref, F.reference(ops, wrong="c1_zero"), "hybrid")
    discriminates(ref, F.reference(ops, wrong="unit_stride"), "hybrid")
    eng = bound(engine_for(cfg, sd), batch)
    arr, marr = first_arr(eng, lv[:3]), ms_arr(eng, lv[2:])
    eng.sample_begin(noise[0], init_pharm_com=com)
    fr = [eng.sample_frame()]
    for i in range(2):
        eng.denoise_step(arr[i], noise[1 + i])
        fr.append(eng.sample_frame())
    for c in marr:
        eng.ms_step(c)
        fr.append(eng.sample_frame())
    x0, h0 = eng.sample_end()
    eng.sample_status()
    check((x0, h0, torch.stack([f[0] for f in fr[:-1]] + [x0]), torch.stack([f[1] for f in fr[:-1]] + [h0])), ref, "hybrid")


# 6. the history's rules
def test_history_rules():
    cfg, sd, batch, noise, seed, com = live_case()
    lv = F.uniform_plan(T, 6)
    eng = bound(engine_for(cfg, sd), batch)
    arr, marr = first_arr(eng, lv), ms_arr(eng, lv)
    second = marr[1]
    assert second.c1_x != 0.0 and marr[0].c1_x == 0.0 and marr[0].c1_h == 0.0
    clean = [t.clone() for t in eng.sample(None, 6, noise[:1], init_pharm_com=com, ms_coef_arr=marr)]
    # (a) right after a begin, (b) right after a plain step: refused, and the run goes on as if the call had not been made
    eng.sample_begin(noise[0], init_pharm_com=com)
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.ms_step(second)
    for c in marr:
        eng.ms_step(c)
    x, h = eng.sample_end()
    assert torch.equal(x, clean[0]) and torch.equal(h, clean[1])
    hyb = []
    for refuse in (False, True):
        eng.sample_begin(noise[0], init_pharm_com=com)
        eng.denoise_step(arr[0], noise[1])
        if refuse:
            with pytest.raises(pfa.PfError, match=ERR_STATE):
                eng.ms_step(second)
        for c in ms_arr(eng, lv[1:]):
            eng.ms_step(c)
        hyb.append(eng.sample_end())
    assert torch.equal(hyb[0][0], hyb[1][0]) and torch.equal(hyb[0][1], hyb[1][1])
    # a valid history does not survive a begin: the multistep run above left one
    eng.sample_begin(noise[0], init_pharm_com=com)
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.ms_step(second)
    # (c) the first step, c1 = 0, does not read the buffer: an earlier run with other outputs in it (another draw, the endpoint
    # coefficients) and a fresh handle whose buffer no run has written give the same bits
    eng.sample(None, 6, noise[7:8], init_pharm_com=com, ms_coef_arr=ms_arr(eng, lv, (True, True)))
    again = eng.sample(None, 6, noise[:1], init_pharm_com=com, ms_coef_arr=marr)
    fresh = bound(engine_for(cfg, sd), batch).sample(None, 6, noise[:1], init_pharm_com=com, ms_coef_arr=marr)
    for a, b, c in zip(clean, again, fresh):
        assert torch.equal(a, b) and torch.equal(a, c.to(a.device))
    # a null or non-finite coefficient is an argument error before anything runs
    eng.sample_begin(noise[0], init_pharm_com=com)
    bad = pfa._lib.PfMsCoef(1.0, float("nan"), 0.0, 0.0, 1.0, 0.0, 0.0)
    with pytest.raises(pfa.PfError, match=r"\(-1\)"):
        eng.ms_step(bad)
    for c in marr:
        eng.ms_step(c)
    x, h = eng.sample_end()
    assert torch.equal(x, clean[0]) and torch.equal(h, clean[1])
    eng.sample_status()


# 7. seeded multistep
def test_seeded_multistep_run():
    """a = 16 of 24, N = 4, the seed in the caller's frame: pf_sample_seed_next in front of pf_sample_ms"""
    cfg, sd, batch, noise, seed, com = live_case()
    a, N = 16, 4
    lv = F.uniform_plan(a, N)
    assert lv == S.level_plan(T, N, top=a)
    ops = tuple(F.ms_ops(lv))
    ref = F.reference(ops, seeded=True, level=a)
    discriminates(ref, F.reference(ops, seeded=True, level=a, wrong="c1_zero"), "seeded multistep")
    discriminates(ref, F.reference(ops), "seeded multistep against the unseeded run")
    eng = bound(engine_for(cfg, sd), batch)
    sc = S.seed_coefficients(gamma_of(), T, a)
    got = eng.sample(None, N, noise[:1], init_pharm_com=com, trajectory=True, ms_coef_arr=ms_arr(eng, lv), seed=seed + (sc,))
    eng.sample_status()
    got = check(got, ref, "seeded multistep a 16 N 4")
    loop = [t.cpu() for t in ms_loop(eng, ms_arr(eng, lv), noise[0], com, seed=seed + (sc,))]
    for p, q in zip(got, loop):
        assert torch.equal(p, q)


# 8. the width-generic family
def test_width_generic_family():
    """(64, 32), N = 4 of 12: the move runs alone (k_step_update<MoveMs>), the family builds its own edges; multistep and strided"""
    import guidance_ref as G
    cfg, sd, k, batch, noise, pins, com, _ = G.wide_case()
    n_t, N, fnorm = G.WIDE_T, 4, 2.0
    lv = F.uniform_plan(n_t, N)
    eng = bound(engine_for(cfg, sd), batch)
    kw = dict(fnorm=fnorm)
    ops = F.ms_ops(lv)
    ref = F.fewstep_reference(sd, cfg, batch, n_t, G.PREC, ops, noise, com, **kw)
    discriminates(ref, F.fewstep_reference(sd, cfg, batch, n_t, G.PREC, ops, noise, com, wrong="c1_zero", **kw), "wide multistep")
    got = eng.sample(None, N, noise[:1], init_pharm_com=com, feat_norm_constant=fnorm, trajectory=True,
                     ms_coef_arr=ms_arr(eng, lv, n_t=n_t, prec=G.PREC))
    assert eng.kernel_family(0) == 64
    check(got, ref, "wide multistep N 4 of 12")
    ops = F.first_ops(lv)
    ref = F.fewstep_reference(sd, cfg, batch, n_t, G.PREC, ops, noise, com, **kw)
    discriminates(ref, F.fewstep_reference(sd, cfg, batch, n_t, G.PREC, ops, noise, com, wrong="unit_stride", **kw), "wide strided")
    got = eng.sample(first_arr(eng, lv, n_t=n_t, prec=G.PREC), N, noise[:N + 1], init_pharm_com=com, feat_norm_constant=fnorm, trajectory=True)
    assert eng.kernel_family(0) == 64
    check(got, ref, "wide strided N 4 of 12")


# 9. repeatability
def test_multistep_runs_repeat_bitwise():
    cfg, sd, batch, noise, seed, com = live_case()
    lv = F.uniform_plan(T, 8)
    eng = bound(engine_for(cfg, sd), batch)
    arr = ms_arr(eng, lv, (True, False))
    a = [t.clone() for t in eng.sample(None, 8, noise[:1], init_pharm_com=com, trajectory=True, ms_coef_arr=arr)]
    b = eng.sample(None, 8, noise[:1], init_pharm_com=com, trajectory=True, ms_coef_arr=arr)
    for p, q in zip(a, b):
        assert torch.equal(p, q) and torch.isfinite(p).all()


# 10. model level and the command line
def test_model_level_few_step_sample():
    """PharmacophoreDiff.sample(sample_steps=..., sampler=...): the requested sizes, N + 1 trajectory frames, and every batch is
    the engine-level run on the same batch and noise, bit for bit; the refusals come before any bind"""
    from test_gpu_api import graph_from, make_model
    n_t, N = 20, 5
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[4, 4, 4], [5, 5]]
    gen = torch.Generator().manual_seed(5)
    gamma = m.gamma.gamma
    binds = []
    real_bind = m.dynamics.bind_graph
    m.dynamics.bind_graph = lambda g: (binds.append(1), real_bind(g))[1]
    for kw, msg in ((dict(sample_steps=N, sampler="multistep", pinned=[(torch.zeros(1, 3), torch.tensor([0]), None), None]), "composes with seeds only"),
                    (dict(sample_steps=N, pin_resamples=2), "pin_resamples > 1"),
                    (dict(sample_steps=n_t + 1), "1 <= sample_steps"),
                    (dict(sampler="ddim"), "pass sample_steps")):
        with pytest.raises(ValueError, match=msg):
            m.sample(pockets, n_pharms, **kw)
    assert not binds
    m.dynamics.bind_graph = real_bind
    for sampler, spacing, rows in (("multistep", "quadratic", 1), ("ddim", "uniform", N + 1), ("ancestral", "logsnr", N + 1)):
        nz = [torch.randn(rows, 12, 9, generator=gen), torch.randn(rows, 10, 9, generator=gen)]
        out = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, noise=nz, visualize_trajectory=True, sample_steps=N, sampler=sampler,
                       spacing=spacing)
        assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
        lv = S.level_plan(n_t, N, spacing, gamma_table=gamma)
        for r in range(2):
            n = len(n_pharms[r])
            batch_g = pfa.batch(pfa.copy_graph(pockets[r], n_copies=n, pharm_feats_per_copy=torch.tensor(n_pharms[r])))
            eng = m.dynamics.bind_graph(batch_g)
            com = pockets[r].prot_x.mean(dim=0).float().repeat(n, 1)
            ekw = dict(init_pharm_com=com, feat_norm_constant=float(m.pharm_feat_norm_constant), trajectory=True)
            if sampler == "multistep":
                ms = S.multistep_coefficients(gamma, n_t, lv, bool(m.endpoint_param_coord), bool(m.endpoint_param_feat))
                x0, h0, tx, th = eng.sample(None, N, nz[r], ms_coef_arr=eng.ms_coef_array(ms), **ekw)
            else:
                arr = eng.coef_array(S.strided_coefficients(gamma, n_t, lv, 0.0 if sampler == "ddim" else 1.0), range(N))
                x0, h0, tx, th = eng.sample(arr, N, nz[r], ep_coord=m.endpoint_param_coord, ep_feat=m.endpoint_param_feat, **ekw)
            eng.sample_status()
            x0, tx = x0.cpu(), tx.cpu()
            ptr = batch_g.pharm_ptr.tolist()
            for i, p in enumerate(out[r]):
                assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.isfinite(p.ph_coords).all()
                fx, fh = p.pos_frames, p.feat_frames
                assert fx.shape[0] == N + 1 and fh.shape[0] == N + 1 and torch.equal(fx, tx[:, ptr[i]:ptr[i + 1]])


def test_model_level_seeded_multistep():
    """sample(seeds=, seed_level=8, sample_steps=4, sampler='multistep') and sample_given_receptor with the same keywords: the
    seed rides on the graph's pin fields with all flags zero, and the run is pf_sample_seed_next + pf_sample_ms -- every batch is
    the engine-level seeded multistep run on the same batch and noise, bit for bit, and differs from the unseeded one"""
    from test_gpu_api import graph_from, make_model
    n_t, a, N = 20, 8, 4
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[4, 4, 4], [5, 5]]
    gen = torch.Generator().manual_seed(5)
    seeds = [(g.prot_x.mean(dim=0).float() + 1.5 * torch.randn(n, 3, generator=gen), torch.randint(0, 6, (n,), generator=gen))
             for g, n in zip(pockets, (4, 5))]
    nz = [torch.randn(1, 12, 9, generator=gen), torch.randn(1, 10, 9, generator=gen)]
    gamma = m.gamma.gamma
    kw = dict(sample_steps=N, sampler="multistep")
    out = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, noise=nz, seeds=seeds, seed_level=a, **kw)
    unseeded = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, noise=nz, **kw)
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    assert all(not torch.equal(p.ph_coords, q.ph_coords) for o, u in zip(out, unseeded) for p, q in zip(o, u))
    lv = S.level_plan(n_t, N, top=a)
    assert lv == F.uniform_plan(a, N)
    sc = S.seed_coefficients(gamma, n_t, a)
    ms = S.multistep_coefficients(gamma, n_t, lv, bool(m.endpoint_param_coord), bool(m.endpoint_param_feat))
    for r in range(2):
        g0 = m._with_seeds(pockets, n_pharms, seeds, None)[r]
        n = len(n_pharms[r])
        batch_g = pfa.batch(pfa.copy_graph(g0, n_copies=n, pharm_feats_per_copy=torch.tensor(n_pharms[r])))
        assert not bool((batch_g.pharm_pin != 0).any())
        eng = m.dynamics.bind_graph(batch_g)
        com = pockets[r].prot_x.mean(dim=0).float().repeat(n, 1)
        x0, h0 = eng.sample(None, N, nz[r], init_pharm_com=com, feat_norm_constant=float(m.pharm_feat_norm_constant),
                            ms_coef_arr=eng.ms_coef_array(ms), seed=(batch_g.pharm_pin_x, batch_g.pharm_pin_h, sc))
        eng.sample_status()
        x0, h0 = x0.cpu(), h0.cpu()
        ptr = batch_g.pharm_ptr.tolist()
        for i, p in enumerate(out[r]):
            assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.equal(p.g.pharm_h0, h0[ptr[i]:ptr[i + 1]])
            assert torch.isfinite(p.ph_coords).all()
        if r == 0:                                      # sample_given_receptor: the same keywords on a batch of plain graphs
            plain = pfa.batch(pfa.copy_graph(pockets[r], n_copies=n, pharm_feats_per_copy=torch.tensor(n_pharms[r])))
            got = m.sample_given_receptor(plain, init_pharm_com=com, noise=nz[r], seeds=[seeds[r]] * n, seed_level=a, **kw)
            for i, p in enumerate(got):
                assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]])


def test_cli_multistep(tmp_path):
    """generate_pharmacophores.py --sample_steps 6 --sampler multistep writes the pharms.xyz the composition predicts (the pattern
    of test_gpu_seeded.test_cli_with_a_seed: same files, same seed, same draw -- one row: the initial one)"""
    import os
    import subprocess
    import sys
    import yaml
    from test_gpu_api import _write_pocket_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_pocket_files(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    n_t, N = 12, 6
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
    e = O.radius_graph(pos, 3.5, torch.tensor([0, pos.shape[0]]), 100)
    pk = P.process_ligand_and_pocket(tmp_path / "rec.pdb", None, emap, cfg['graph']['graph_cutoffs'], 8.0, lig_file=tmp_path / "lig.sdf",
                                     pp_edges=(e[0], e[1]))
    pocket1 = O.PocketBatch(pk.prot_x, pk.prot_h, torch.tensor([0, pk.prot_x.shape[0]]), torch.tensor([0, 1]), pk.pp_src.long(), pk.pp_dst.long())
    b = O.concat_pockets([O.copy_pocket(pocket1, 4) for _ in range(3)])
    com = O.segment_mean(b.prot_x, b.prot_ptr)
    prec = float(cfg['diffusion'].get('precision', 1e-5))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
           str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "3", "--max_batch_size", "3", "--output_dir", str(out),
           "--seed", "1", "--pharm_sizes", "4", "4", "4", "--sample_steps", str(N), "--sampler", "multistep"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    xyz = (out / "rec" / "pharms.xyz").read_text().splitlines()
    torch.manual_seed(1)
    nz = torch.randn(1, 12, 9, device="cuda").cpu()
    lv = F.uniform_plan(n_t, N)
    ref = F.fewstep_reference(sd, O.DynamicsConfig(), b, n_t, prec, F.ms_ops(lv), nz, com)
    rows = [l.split() for l in xyz if len(l.split()) == 4]
    assert len(rows) == 12
    scale = max(abs(float(v)) for r_ in rows for v in r_[1:])
    # the nearest wrong neighbour of a command line: the flags were not applied -- the default run of the same seed (T + 1 rows
    # from the same generator state, every level).  With these unscaled random weights eps_x is ~1e-5 and the plans of a
    # deterministic solver all end alike, so the previous output's term is checked at the engine level (above), not here
    torch.manual_seed(1)
    nz_all = torch.randn(n_t + 1, 12, 9, device="cuda").cpu()
    default = F.fewstep_reference(sd, O.DynamicsConfig(), b, n_t, prec, F.first_ops(list(range(n_t, -1, -1))), nz_all, com)
    gx, gh = F.worst_center_gap(ref, default)
    print(f"cli: the default run of the same seed is off by {gx:.3g} (x_0); coordinates up to {scale:.3g}")
    assert gx >= 10 * 5e-3 * max(1.0, scale)
    for r_, xw, kw in zip(rows, ref[0].tolist(), ref[1].argmax(1).tolist()):
        assert r_[0] == "PSFNOC"[kw], (r_, kw)
        assert all(abs(float(u) - v) <= 5e-3 * max(1.0, scale) for u, v in zip(r_[1:], xw)), (r_, xw)
