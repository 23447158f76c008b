"""Pinned runs with resampling jumps (pf_sample_pinned_resampled / pf_renoise_step) against the CPU composition of
tests/resample_ref.py: test_gpu_pinned.py's `pinned_reference` loop opened up to a plan, with one more branch for R(b -> a).

Shape: test_gpu_pinned.py's own -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms (the 300-atom one exercises the strided
protein loop of the re-noise launch) with 3 / 8 / 5 / 1 / 6 centers (the one-center graph's COM is the center itself) and the
same flags (graph 2 is pinned throughout), precision 0.25.  T = 24, jump 5, resamples 3: segments of 5, 5, 5, 5 and 4 levels,
82 ops, 83 frames.  Tolerances are the project's own: rtol = atol = 5e-3 for trajectories, atol = 2e-2 for the width-generic
family, the fp64 budget of helpers.within_budget where no network output is involved.

Conditions on the inputs, checked on the CPU by test_resample_host.py (noise seed 42): the composition evaluated in fp64 and in
fp32 agrees with itself on every frame within 4.1e-6 (x) / 6.8e-6 (h) in the noise parameterisation, 8.5e-7 / 6.1e-7 in the
endpoint one and 9.2e-6 / 3.7e-6 with the live head (k = 13) -- the bound is 5e-4, a tenth of the tolerance; and behind the two
R ops of the op-alone test the fp32 and fp64 coordinates give identical edge sets."""
import ctypes

import pytest
import torch

import pharmacoforge_amd as pfa
import resample_ref as R
from helpers import edge_set, within_budget
from oracle import pf_oracle as O
from test_gpu_pinned import bound, engine_for, pins_for

pytestmark = pytest.mark.gpu

T, PREC = R.T, R.PREC
ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"


def plan_arrays(eng, plan, n_t=T, prec=PREC):
    """(coef_arr, pin_coef_arr, op_arr, renoise_arr) of a plan, one entry per op"""
    gamma = O.gamma_table(n_t, prec)
    pairs = [(op[1], op[2]) for op in plan if op[0] == "renoise"]
    return eng.plan_arrays(plan, O.step_coefficients(gamma, n_t), pfa.schedule.pin_coefficients(gamma, n_t),
                           pfa.schedule.renoise_coefficients(gamma, n_t, pairs))


def step_arrays(eng, n_t=T, prec=PREC):
    gamma = O.gamma_table(n_t, prec)
    order = list(reversed(range(n_t)))
    return (eng.coef_array(O.step_coefficients(gamma, n_t), order),
            eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order))


def run_resampled(eng, plan, noise, pins, com, **kw):
    arr, parr, op_arr, re_arr = plan_arrays(eng, plan)
    return eng.sample(arr, len(plan), noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, plan=(op_arr, re_arr), **kw)


def check_run(eng, cfg, got, ref, pins, what):
    flags, pin_x, pin_h = pins
    x0, h0, tx, th = (t.cpu() for t in got)
    rx, rh, rfx, rfh = ref
    assert eng.kernel_family(cfg.n_convs) == 0          # no tail, fused-tail or merged launch in a pinned run
    assert eng.xchg_timeouts() == 0
    eng.sample_status()
    assert tx.shape == rfx.shape and th.shape == rfh.shape
    print("%s worst |error|: x0 %.3g h0 %.3g frames x %.3g h %.3g" % ((what,) + tuple(float((a - b).abs().max()) for a, b in
                                                                                     ((x0, rx), (h0, rh), (tx, rfx), (th, rfh)))))
    for a, b in ((x0, rx), (h0, rh), (tx, rfx), (th, rfh)):
        torch.testing.assert_close(a, b, rtol=5e-3, atol=5e-3)
    mx, mh = (flags & 1) != 0, (flags & 2) != 0
    assert torch.equal(x0[mx], pin_x[mx]) and torch.equal(h0[mh], pin_h[mh])
    assert torch.equal(tx[-1][mx], pin_x[mx]) and torch.equal(th[-1][mh], pin_h[mh])
    assert torch.equal(tx[-1], x0) and torch.equal(th[-1], h0)
    assert not torch.equal(tx[len(tx) // 2][mx], pin_x[mx])        # earlier frames show the noised state


@pytest.mark.parametrize("ep", [False, True])
def test_resampled_run_vs_composition(ep):
    """82 ops, 83 frames, both parameterisations.  fp64 against fp32 composition: 4.1e-6 / 6.8e-6 (noise), 8.5e-7 / 6.1e-7
    (endpoint).  Measured on the MI355X, worst |error| over x0, h0 and all frames: 6.7e-6 (noise), 7.2e-7 (endpoint)."""
    cfg, sd, batch, plan, noise, pins, com = R.case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_resampled(eng, plan, noise, pins, com, ep_coord=ep, ep_feat=ep, trajectory=True)
    check_run(eng, cfg, got, R.reference(ep), pins, "ep" if ep else "noise")


def test_live_head():
    """The noise-parameterised case with the scaled head: eps_x counts in the D ops behind an R op, so a dynamics call that saw
    stale edges or unshifted protein rows after a re-noise moves the result by far more than the tolerance.  fp64 against fp32
    composition: 9.2e-6 / 3.7e-6 (k = 13).  Measured on the MI355X, worst |error|: 7.6e-6."""
    cfg, sd, batch, plan, noise, pins, com = R.case()
    sd_live, k = R.live_sd()
    plain = R.reference(False)
    ref = R.reference(False, True)
    assert float((ref[2] - plain[2]).abs().max()) > 0.1              # the head is live: the trajectory is another one
    eng = bound(engine_for(cfg, sd_live), batch)
    got = run_resampled(eng, plan, noise, pins, com, trajectory=True)
    check_run(eng, cfg, got, ref, pins, f"live head (k = {k})")


def check_edges(eng, cfg, batch, state, what):
    edges = O.build_dynamic_edges(cfg, batch, state[0], state[1])
    for i, et in enumerate(("ff", "pf", "fp")):
        assert O.ETYPES[i] == et
        s, d = eng.get_edges(i)
        assert edge_set(s, d) == edge_set(*edges[et]), (what, et)
        assert s.numel() == edges[et][0].numel()


def test_the_op_alone():
    """sample_begin, R(4 -> 9) of T = 24 twice, then one denoising step.  No network output is involved in the frames behind the R
    ops, so the fp64 budget applies (e <= 8 max(e32, 2**-22)).  The edge sets the step's dynamics call reads are those the second R
    launch built -- with the encoders on the fly a pinned step ends by building the NEXT call's edges into the same tables, so
    get_edges shows the dynamics call's own edges in front of the step and the next call's behind it: both must be the oracle's on
    the composition's coordinates (the second set depends on the first through the step's dynamics call).
    Measured on the MI355X: e 8.9e-8 / 1.2e-7 of the max for x behind the two ops (e32 1.3e-7 / 7.9e-8), 6.5e-8 / 5.8e-8 for h (e32 the
    same): ratio at most 0.48 of the allowed 8."""
    cfg, sd, batch, plan, noise, pins, com = R.case()
    ref32, ref64 = R.op_alone_reference(False), R.op_alone_reference(True)
    a_ab, s_ab = R.renoise_coef(O.gamma_table(T, PREC), T, 4, 9)
    coef = pfa._lib.PfRenoiseCoef(float(a_ab), float(s_ab))
    eng = bound(engine_for(cfg, sd), batch)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)
    for i in (1, 2):                                    # the second op moves protein rows the first one shifted
        eng.renoise_step(coef, noise[i])
        x, h = eng.sample_frame()
        within_budget(x, ref32[0][i], ref64[0][i], f"frame x behind R op {i}")
        within_budget(h, ref32[1][i], ref64[1][i], f"frame h behind R op {i}")
    check_edges(eng, cfg, batch, ref32[2], "the edges the step's dynamics call reads")
    arr, parr = step_arrays(eng)
    eng.denoise_step(arr[T - 9], noise[3], pin_coef=parr[T - 9])            # D(8): t = 9 / 24
    check_edges(eng, cfg, batch, ref32[3], "behind the step")
    x, h = (t.cpu() for t in eng.sample_frame())
    rx, rh = ref32[3][1] + (O.segment_mean(batch.prot_x, batch.prot_ptr)
                            - O.segment_mean(ref32[3][0], batch.prot_ptr))[batch.batch_idxs()["pharm"]], ref32[3][2]
    torch.testing.assert_close(x, rx, rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(h, rh, rtol=5e-3, atol=5e-3)
    assert eng.kernel_family(cfg.n_convs) == 0 and eng.xchg_timeouts() == 0


def test_no_resampling_through_the_new_entry_is_pf_sample_pinned():
    cfg, sd, batch, _, noise, pins, com = R.case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr = step_arrays(eng)
    want = eng.sample(arr, T, noise[:T + 1], init_pharm_com=com, trajectory=True, pins=pins, pin_coef_arr=parr)
    plan = pfa.schedule.resample_plan(T, R.JUMP, 1)
    assert len(plan) == T
    got = run_resampled(eng, plan, noise[:T + 1], pins, com, trajectory=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_step_api_and_state():
    cfg, sd, batch, plan, noise, pins, com = R.case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, op_arr, re_arr = plan_arrays(eng, plan)
    with pytest.raises(pfa.PfError, match=ERR_STATE):   # after a bind
        eng.renoise_step(re_arr[5], noise[1])
    s_arr, _ = step_arrays(eng)
    first = eng.sample(s_arr, T, noise[:T + 1], init_pharm_com=com)
    form = eng.kernel_family(cfg.n_convs)
    x0, h0 = eng.sample(arr, len(plan), noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, plan=(op_arr, re_arr))
    assert eng.kernel_family(cfg.n_convs) == 0
    # the step API driven by the plan equals the whole loop bitwise
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)
    for i, op in enumerate(plan):
        if op[0] == "renoise":
            eng.renoise_step(re_arr[i], noise[1 + i])
            assert eng.kernel_family(cfg.n_convs) == 0
        else:
            eng.denoise_step(arr[i], noise[1 + i], pin_coef=parr[i])
    x1, h1 = eng.sample_end()
    assert torch.equal(x0, x1) and torch.equal(h0, h1)
    # outside a pinned run
    eng.sample_begin(noise[0], init_pharm_com=com)
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.renoise_step(re_arr[5], noise[1])
    eng.denoise_step(s_arr[0], noise[1])                # ... which the plain step continues
    # an unknown op kind is refused before anything is enqueued
    bad = (ctypes.c_int32 * len(plan))(*op_arr)
    bad[len(plan) - 1] = 2
    with pytest.raises(pfa.PfError, match=ERR_ARG):
        eng.sample(arr, len(plan), noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, plan=(bad, re_arr))
    with pytest.raises(pfa.PfError, match=ERR_STATE):   # (nothing began: the handle is still in the plain run)
        eng.renoise_step(re_arr[5], noise[1])
    # unpinned -> resampled -> unpinned on one handle: the first run's bits and the step-end form come back
    again = eng.sample(s_arr, T, noise[:T + 1], init_pharm_com=com)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert eng.kernel_family(cfg.n_convs) == form
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


def test_width_generic_family():
    """(64, 32): the move runs alone (k_step_update<MoveRenoise>), the family launches its own encoders and edge build.  T = 12, jump 4,
    resamples 2: 27 ops.  The given rows are divided by a feat_norm_constant of 2.  Measured on the MI355X, worst |error|: 1.4e-6."""
    n_t, fnorm = 12, 2.0
    cfg = O.DynamicsConfig(n_hidden_scalars=64, vector_size=32)
    sd = O.make_state_dict(cfg, 0)
    batch = O.synthetic_batch([0, 1], [40, 56], [3, 5], cfg)
    plan = pfa.schedule.resample_plan(n_t, 4, 2)
    assert len(plan) == 27 and plan == R.plan_of(n_t, 4, 2)
    noise = torch.randn(len(plan) + 1, 8, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(42))
    pins = pins_for(batch, cfg, [3, 0, 0] + [0, 0, 3, 0, 0])
    flags, pin_x, pin_h = pins
    com = O.segment_mean(batch.prot_x, batch.prot_ptr) + 0.5
    ref = R.resampled_reference(sd, cfg, batch, n_t, PREC, plan, noise, *pins, com, fnorm=fnorm)
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, op_arr, re_arr = plan_arrays(eng, plan, n_t)
    got = [t.cpu() for t in eng.sample(arr, len(plan), noise, init_pharm_com=com, feat_norm_constant=fnorm, trajectory=True,
                                       pins=pins, pin_coef_arr=parr, plan=(op_arr, re_arr))]
    assert eng.kernel_family(0) == 64 and eng.kernel_family(cfg.n_convs) == 0
    print("wide worst |error|: x0 %.3g h0 %.3g frames x %.3g h %.3g" % tuple(float((a - b).abs().max()) for a, b in zip(got, ref)))
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=2e-2)
    mx, mh = (flags & 1) != 0, (flags & 2) != 0
    assert torch.equal(got[0][mx], pin_x[mx]) and torch.equal(got[1][mh], pin_h[mh])
    assert torch.equal(got[2][-1][mx], pin_x[mx]) and torch.equal(got[3][-1][mh], pin_h[mh])


def test_model_level_sample_with_resampling():
    """PharmacophoreDiff.sample(pinned=..., pin_resamples=2, pin_jump=4) on two pockets with injected noise: the batch of the
    pinned pocket's copies is the engine-level resampled run on the same batch, bit for bit; the batch of the other pocket runs
    the default path with T + 1 noise rows and returns the samples of a call without `pinned`."""
    from test_gpu_api import graph_from, make_model
    n_t = 20
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[3, 5, 4], [4, 3, 6]]
    pin_x = (pockets[0].prot_x.mean(dim=0) + torch.tensor([[1.25, -0.5, 0.75], [-1.0, 1.5, 0.125]])).float()
    types = torch.tensor([2, 5])
    pinned = [(pin_x, types, None), None]
    plan = pfa.schedule.resample_plan(n_t, 4, 2)
    assert len(plan) == 45
    gen = torch.Generator().manual_seed(11)
    nz = [torch.randn(len(plan) + 1, 12, 9, generator=gen), torch.randn(n_t + 1, 13, 9, generator=gen)]
    out = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, noise=nz, pinned=pinned, pin_resamples=2, pin_jump=4)
    plain = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, noise=[nz[0][:n_t + 1], nz[1]])
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    for p, q in zip(out[1], plain[1]):                  # the free pocket: the default path's samples
        assert not p.pinned.any()
        assert torch.equal(p.ph_coords, q.ph_coords) and torch.equal(p.g.pharm_h0, q.g.pharm_h0)
    for p in out[0]:
        assert p.pinned.tolist() == [3, 3] + [0] * (p.n_ph_centers - 2)
        assert torch.equal(p.ph_coords[:2], pin_x) and p.ph_feats_idxs[:2].tolist() == types.tolist()
        assert torch.isfinite(p.ph_coords).all()
    with pytest.raises(ValueError, match="46 noise rows, got 21"):
        m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, noise=[nz[0][:n_t + 1], nz[1]], pinned=pinned, pin_resamples=2, pin_jump=4)
    # the engine-level run on the same batch, on the handle the model's lane 0 uses
    g0 = m._with_pins(pockets, n_pharms, pinned)[0]
    batch_g = pfa.batch(pfa.copy_graph(g0, n_copies=3, pharm_feats_per_copy=torch.tensor(n_pharms[0])))
    eng = m.dynamics.bind_graph(batch_g)
    gamma = m.gamma.gamma
    pairs = [(op[1], op[2]) for op in plan if op[0] == "renoise"]
    arr, parr, op_arr, re_arr = eng.plan_arrays(plan, m.step_coefficients(), pfa.schedule.pin_coefficients(gamma, n_t),
                                                pfa.schedule.renoise_coefficients(gamma, n_t, pairs))
    com = pockets[0].prot_x.mean(dim=0).float().repeat(3, 1)
    x0, h0 = eng.sample(arr, len(plan), nz[0], init_pharm_com=com, ep_coord=m.endpoint_param_coord, ep_feat=m.endpoint_param_feat,
                        feat_norm_constant=float(m.pharm_feat_norm_constant), pins=(batch_g.pharm_pin, batch_g.pharm_pin_x, batch_g.pharm_pin_h),
                        pin_coef_arr=parr, plan=(op_arr, re_arr))
    eng.sample_status()
    x0, h0 = x0.cpu(), h0.cpu()
    ptr = batch_g.pharm_ptr.tolist()
    for i, p in enumerate(out[0]):
        assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.equal(p.g.pharm_h0, h0[ptr[i]:ptr[i + 1]])
    # resampling changed the completion: the free centers are not those of the pinned run without it
    once = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, noise=[nz[0][:n_t + 1], nz[1]], pinned=pinned)
    assert any(not torch.equal(p.ph_coords[2:], q.ph_coords[2:]) for p, q in zip(out[0], once[0]))
