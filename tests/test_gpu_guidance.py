"""Guided sampling (pf_sample_guided / pf_sample_begin_guided / pf_denoise_step_guided / pf_dynamics_input_vjp) against the CPU
composition of tests/guidance_ref.py: the pinned reference's loop with the restraint energies, their gradient through the
dynamics (the oracle's autograd on the edge set decided in fp32), the shift and the clip inserted.

Shape: the five ragged pockets of test_gpu_resample.py (48 / 300 / 40 / 64 / 32 atoms, 3 / 8 / 5 / 1 / 6 centers), precision 0.25,
T = 24, the scaled head (helpers.sampler_live_head: with the recorded head J(g0) is ~1e-5 of g0 and a kernel that dropped the VJP
would pass); a smaller leg at (64, 32) with T = 12; one endpoint-parameterised leg.  Tolerances are the project's own: rtol = atol =
5e-3 for whole runs, helpers.within_budget (8 max(e32, 2**-22)) for one step's vectors.

Conditions on the inputs, checked on the CPU by test_guidance_host.py: the composition in fp64 and in fp32 agrees with itself
within 5e-4 on x_0, h_0 and all frames (measured 3.3e-6 noise / 3.6e-5 endpoint); the guided x_0 differs from the unguided by at
least 0.05 on every restrained graph (measured >= 1.8); a reference without J(g0) misses the frames by at least 0.05 (>= 0.16).

Measured on the MI355X, worst |error| over x_0, h_0 and all frames: 2.7e-6 (noise; energies 1.6e-5 on values up to 38), 3.2e-5
(endpoint; energies 1.5e-4), 1.5e-4 at (64, 32) (energies 9.5e-4).  One step against the fp64 reference, ratio to max(e32, 2**-22)
of E / g0 / grad / shift: 0.31 / 0.48 / 1.03 / 1.03 (noise), 0.21 / 0.97 / 1.91 / 1.91 (endpoint), 1.27 / 0.82 / 0.28 / 0.29 at (64, 32),
of the allowed 8.  Zero restraints against the pinned run on the same handle: 2.4e-6."""
import ctypes

import pytest
import torch

import pharmacoforge_amd as pfa
import guidance_ref as G
from helpers import within_budget
from oracle import pf_oracle as O
from test_gpu_pinned import bound, engine_for

pytestmark = pytest.mark.gpu

T, PREC = G.T, G.PREC
ERR_ARG, ERR_STATE = r"\(-1\)", r"\(-3\)"


def arrays(eng, n_t=T, prec=PREC):
    gamma = O.gamma_table(n_t, prec)
    order = list(reversed(range(n_t)))
    return (eng.coef_array(O.step_coefficients(gamma, n_t), order),
            eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order),
            eng.guide_coef_array(pfa.schedule.guide_coefficients(gamma, n_t), order))


def run_guided(eng, n_t, noise, pins, com, restraints, scale=G.GUIDE_SCALE, **kw):
    arr, parr, garr = arrays(eng, n_t)
    return eng.sample(arr, n_t, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr,
                      guide_scale=scale, **kw)


def check_run(eng, cfg, got, ref, pins, what):
    flags, pin_x, pin_h = pins
    x0, h0, tx, th, en = (t.cpu() for t in got)
    assert eng.kernel_family(cfg.n_convs) == 0          # no tail, fused-tail or merged launch in a guided run
    assert eng.xchg_timeouts() == 0
    eng.sample_status()
    pairs = ((x0, ref.x0), (h0, ref.h0), (tx, ref.fx), (th, ref.fh), (en, ref.E))
    print("%s worst |error|: x0 %.3g h0 %.3g frames x %.3g h %.3g E %.3g" % ((what,) + tuple(float((a - b).abs().max()) for a, b in pairs)))
    for a, b in pairs:
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=5e-3, atol=5e-3)
    mx, mh = (flags & 1) != 0, (flags & 2) != 0
    assert torch.equal(x0[mx], pin_x[mx]) and torch.equal(h0[mh], pin_h[mh])
    assert torch.equal(tx[-1], x0) and torch.equal(th[-1], h0)


# 1. whole runs, three legs
@pytest.mark.parametrize("ep", [False, True])
def test_guided_run_vs_composition(ep):
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_guided(eng, T, noise, pins, com, restraints, ep_coord=ep, ep_feat=ep, trajectory=True, energies=True)
    assert eng.train_family() == "tuned"                # the family the engine was on is back
    ref = G.reference(ep)
    check_run(eng, cfg, got, ref, pins, f"{'ep' if ep else 'noise'} (k = {k})")
    ptr = batch.pharm_ptr.tolist()
    un = G.reference(ep, False, False)
    for g in range(1, 5):                               # the guidance is no rounding error of the unguided run
        assert float((got[0].cpu()[ptr[g]:ptr[g + 1]] - un.x0[ptr[g]:ptr[g + 1]]).abs().max()) >= 10 * G.TOL


def test_guided_run_width_generic_family():
    """(64, 32), T = 12, a pinned center, the given rows divided by a feat_norm_constant of 2"""
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_guided(eng, G.WIDE_T, noise, pins, com, restraints, feat_norm_constant=2.0, trajectory=True, energies=True)
    assert eng.kernel_family(0) == 64
    check_run(eng, cfg, got, G.wide_reference(), pins, f"(64, 32) (k = {k})")


# 2. one guided step, read back
def one_step(eng, n_t, noise, pins, com, restraints, ep=False, fnorm=1.0, scale=G.GUIDE_SCALE, clip=0.0):
    """sample_begin + the first guided step (s = T - 1) on the wide family: (g0, grad, shift, E) on the host"""
    arr, parr, garr = arrays(eng, n_t)
    eng.set_train_family("wide")
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, feat_norm_constant=fnorm, restraints=restraints, guide_scale=scale,
                     guide_clip=clip)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1], ep_coord=ep, ep_feat=ep)
    return tuple(t.cpu() for t in eng.last_guidance())


@pytest.mark.parametrize("leg", ["noise", "ep", "wide"])
def test_one_step_within_the_fp64_budget(leg):
    wide, ep = leg == "wide", leg == "ep"
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case() if wide else G.case()
    n_t, fnorm = (G.WIDE_T, 2.0) if wide else (T, 1.0)
    kw = dict(scale=G.GUIDE_SCALE, fnorm=fnorm, ep=ep, n_steps=1)
    r32 = G.guided_reference(sd, cfg, batch, n_t, PREC, noise, *pins, com, restraints, **kw)
    r64 = G.guided_reference(sd, cfg, batch, n_t, PREC, noise, *pins, com, restraints, double=True, **kw)
    eng = bound(engine_for(cfg, sd), batch)
    g0, grad, shift, en = one_step(eng, n_t, noise, pins, com, restraints, ep=ep, fnorm=fnorm)
    assert eng.kernel_family(cfg.n_convs) == 0
    within_budget(en, r32.E[0], r64.E[0], f"{leg} E")
    within_budget(g0, r32.g0[0], r64.g0[0], f"{leg} g0")
    within_budget(grad, r32.grad[0], r64.grad[0], f"{leg} grad")
    within_budget(shift, r32.shift[0], r64.shift[0], f"{leg} shift")
    if not wide:                                        # a graph without restraints inside a guided batch: shift == 0 exactly
        n0 = int(batch.pharm_ptr[1])
        assert bool((shift[:n0] == 0).all()) and bool((g0[:n0] == 0).all()) and float(en[0]) == 0.0
        assert float(shift[n0:].abs().max()) > 0
    # the state behind the step (the one-step reference's last frame carries the given values: free rows only)
    x, h = (t.cpu() for t in eng.sample_frame(fnorm))
    fx_free, fh_free = (pins[0] & 1) == 0, (pins[0] & 2) == 0
    torch.testing.assert_close(x[fx_free], r32.fx[1][fx_free], rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(h[fh_free], r32.fh[1][fh_free], rtol=5e-3, atol=5e-3)


def test_clip():
    """every row with |shift| > clip comes out at norm clip, the others are untouched bitwise"""
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    _, grad_u, shift_u, _ = one_step(eng, T, noise, pins, com, restraints)
    n_u = shift_u.double().norm(dim=1)
    clip = float(n_u[n_u > 0].median())
    over = n_u > clip * (1 + 1e-5)
    under = n_u < clip * (1 - 1e-5)
    assert bool(over.any()) and bool((under & (n_u > 0)).any())
    _, grad_c, shift_c, _ = one_step(eng, T, noise, pins, com, restraints, clip=clip)
    assert torch.equal(grad_c, grad_u)
    assert torch.equal(shift_c[under], shift_u[under])
    n_c = shift_c.double().norm(dim=1)
    assert float(((n_c[over] - clip).abs() / clip).max()) <= 1e-6
    cos = (shift_c[over].double() * shift_u[over].double()).sum(dim=1) / (n_c[over] * n_u[over])
    assert float((1 - cos).abs().max()) <= 1e-6          # the direction is kept


# 3. the inputs-only backward
@pytest.mark.parametrize("name", ["train_grads 128/16", "train_grads 64/32"])
def test_input_vjp_is_bitwise_the_full_pass(name):
    from test_gpu_input_grads import forward_on
    c, eng, _, _, _ = forward_on(name)
    plain = eng.train_backward(c.w_h, c.w_x)
    grad, g_x, g_h = eng.train_backward(c.w_h, c.w_x, input_grads=True)
    v_x, v_h = eng.input_vjp(c.w_h, c.w_x)
    assert float(g_x.abs().max()) > 0 and float(g_h.abs().max()) > 0
    assert torch.equal(v_x, g_x) and torch.equal(v_h, g_h)
    w_x, w_h = eng.input_vjp(c.w_h, c.w_x)              # the same bits on a second call
    assert torch.equal(w_x, g_x) and torch.equal(w_h, g_h)
    x_only, none_h = eng.input_vjp(c.w_h, c.w_x, want=(True, False))
    none_x, h_only = eng.input_vjp(c.w_h, c.w_x, want=(False, True))
    assert none_h is None and none_x is None and torch.equal(x_only, g_x) and torch.equal(h_only, g_h)
    # the full pass afterwards: the parameter gradient is what it is without the VJP calls in between
    assert torch.equal(eng.train_backward(c.w_h, c.w_x), plain) and torch.equal(grad, plain)
    with pytest.raises(pfa.PfError, match=ERR_ARG):     # at least one output
        eng.input_vjp(c.w_h, c.w_x, want=(False, False))
    again = eng.input_vjp(c.w_h, c.w_x)                 # ... and the kept forward stays good
    assert torch.equal(again[0], g_x)
    if name.endswith("128/16"):
        eng.set_train_family("tuned")
        eng.train_forward(c.x_t, c.h_t, c.t, prot_x=c.prot_x)
        with pytest.raises(pfa.PfError, match=ERR_ARG):  # the tuned family has no input gradients
            eng.input_vjp(c.w_h, c.w_x)
        eng.train_backward(c.w_h, c.w_x)                 # the kept forward stays good for pf_train_backward


def test_input_vjp_needs_a_forward():
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    eng.set_train_family("wide")
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.input_vjp(torch.zeros(8, cfg.pharm_nf), torch.zeros(8, 3))


# 4. zero restraints, and what surrounds a guided run
def test_zero_restraints_agree_with_the_pinned_run():
    """A guided run without a restraint against the pinned run on the same handle, at the tolerance test_gpu_pinned.py uses
    between forms (rtol = atol = 5e-3).  Not bitwise: the guided step's dynamics call is the width-generic training forward
    (fp32 MFMA Linears in another summation order than the tuned kernels), the pinned step's the tuned inference path."""
    cfg, sd, k, batch, noise, pins, com, _ = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, garr = arrays(eng)
    want = eng.sample(arr, T, noise, init_pharm_com=com, trajectory=True, pins=pins, pin_coef_arr=parr)
    got = run_guided(eng, T, noise, pins, com, [None] * 5, trajectory=True, energies=True)
    assert bool((got[4] == 0).all())
    print("zero restraints against the pinned run, worst |difference|: %.3g" % max(float((a - b).abs().max()) for a, b in zip(got[:4], want)))
    for a, b in zip(got[:4], want):
        torch.testing.assert_close(a, b, rtol=5e-3, atol=5e-3)
    ref = G.reference(False, False, False)
    for a, b in zip(got[:4], (ref.x0, ref.h0, ref.fx, ref.fh)):
        torch.testing.assert_close(a.cpu(), b, rtol=5e-3, atol=5e-3)


def test_unguided_guided_unguided_on_one_handle():
    cfg, sd, k, batch, noise, pins, com, restraints = G.case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, garr = arrays(eng)
    first = eng.sample(arr, T, noise, init_pharm_com=com)
    form = eng.kernel_family(cfg.n_convs)
    guided = run_guided(eng, T, noise, pins, com, restraints)
    assert eng.kernel_family(cfg.n_convs) == 0 and eng.train_family() == "tuned"
    again = eng.sample(arr, T, noise, init_pharm_com=com)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert eng.kernel_family(cfg.n_convs) == form       # the step-end form returns to the merged launch
    assert not torch.equal(guided[0], first[0])
    # the step API equals the whole loop bitwise
    eng.set_train_family("wide")
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)
    for i in range(T):
        eng.guided_step(arr[i], parr[i], garr[i], noise[1 + i])
    x1, h1 = eng.sample_end()
    eng.set_train_family("tuned")
    assert torch.equal(x1, guided[0]) and torch.equal(h1, guided[1])
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


def _begin_raw(eng, noise0, pins, rp, rk, rc, rx, rr, rw, scale=1.0, clip=0.0):
    import numpy as np
    keep = [noise0.cuda().contiguous()] + [t.cuda().contiguous() for t in pins]
    a = [np.ascontiguousarray(v, dtype=d) for v, d in ((rp, np.int32), (rk, np.int32), (rc, np.int32), (rx, np.float32),
                                                      (rr, np.float32), (rw, np.float32))]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc_ = eng.lib.pf_sample_begin_guided(eng._h, None, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), 1.0,
                                         *[v.ctypes.data for v in a], float(scale), float(clip),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc_


def test_state_and_argument_errors():
    cfg, sd, k, batch, noise, pins, com, restraints = G.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr, garr = arrays(eng, G.WIDE_T)
    with pytest.raises(pfa.PfError, match=ERR_STATE):   # after a bind
        eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_guidance()
    # the tuned family: refused, and the message names the switch
    with pytest.raises(pfa.PfError, match=r"\(-3\).*pf_train_set_family"):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints)
    eng.set_train_family("wide")
    # a plain run in progress stays usable through every refused begin
    eng.sample_begin(noise[0], init_pharm_com=com)
    eng.denoise_step(arr[0], noise[1])
    before = [t.clone() for t in eng.sample_frame()]
    ok = ([0, 1, 2], [1, 0], [-1, 1], [[0, 0, 0], [1, 1, 1]], [3.0, 1.0], [1.0, 1.0])
    bad = {
        "kind": ([0, 1, 2], [1, 2], ok[2], ok[3], ok[4], ok[5]),
        "center too large": ([0, 1, 2], ok[1], [-1, 5], ok[3], ok[4], ok[5]),
        "center below -1": ([0, 1, 2], ok[1], [-2, 1], ok[3], ok[4], ok[5]),
        "non-finite p": ([0, 1, 2], ok[1], ok[2], [[0, float("nan"), 0], [1, 1, 1]], ok[4], ok[5]),
        "negative r": ([0, 1, 2], ok[1], ok[2], ok[3], [-1.0, 1.0], ok[5]),
        "negative w": ([0, 1, 2], ok[1], ok[2], ok[3], ok[4], [1.0, -0.5]),
        "ptr": ([0, 2, 1], ok[1], ok[2], ok[3], ok[4], ok[5]),
    }
    for what, a in bad.items():
        assert _begin_raw(eng, noise[0], pins, *a) == -1, what
    assert _begin_raw(eng, noise[0], pins, *ok, scale=-1.0) == -1
    assert _begin_raw(eng, noise[0], pins, *ok, clip=-1.0) == -1
    many = ([0, 257, 257], [0] * 257, [-1] * 257, [[0, 0, 0]] * 257, [1.0] * 257, [1.0] * 257)
    assert _begin_raw(eng, noise[0], pins, *many) == -1
    assert "256" in eng.lib.pf_last_error(eng._h).decode()
    with pytest.raises(pfa.PfError, match=ERR_STATE):   # nothing began: the handle is still in the plain run
        eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    after = eng.sample_frame()
    assert all(torch.equal(a, b) for a, b in zip(before, after))       # nothing was enqueued
    eng.denoise_step(arr[1], noise[2])                  # ... which the plain step continues
    # inside a guided run the other steps are refused; the guided step continues
    assert _begin_raw(eng, noise[0], pins, *ok) == 0
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    state = [t.clone() for t in eng.sample_frame()]
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.denoise_step(arr[1], noise[2])
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.denoise_step(arr[1], noise[2], pin_coef=parr[1])
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.renoise_step(pfa._lib.PfRenoiseCoef(0.9, 0.4), noise[2])
    assert all(torch.equal(a, b) for a, b in zip(state, eng.sample_frame()))
    eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    assert eng.kernel_family(cfg.n_convs) == 0
    # a guided run ends at the next begin of any kind, and at the next bind
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    eng.denoise_step(arr[0], noise[1], pin_coef=parr[0])
    assert _begin_raw(eng, noise[0], pins, *ok) == 0
    bound(eng, batch)
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    # the Python layer: a plan together with restraints, and missing arrays
    with pytest.raises(ValueError):
        eng.sample(arr, G.WIDE_T, noise, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr, plan=((), ()))
    with pytest.raises(ValueError):
        eng.sample(arr, G.WIDE_T, noise, pins=pins, pin_coef_arr=parr, restraints=restraints)
    # on error the family the engine was on comes back
    eng.set_train_family("tuned")
    with pytest.raises(pfa.PfError, match=ERR_ARG):
        run_guided(eng, G.WIDE_T, noise, pins, com, [[("repel", 9, (0, 0, 0), 1.0, 1.0)], None])
    assert eng.train_family() == "tuned"
    assert eng.xchg_timeouts() == 0


# 5. model level
def test_model_level_sample_with_restraints():
    """PharmacophoreDiff.sample(restraints=...) on two pockets with injected noise: the batch of the restrained pocket's copies is
    the engine-level guided run on the same batch, bit for bit; the batch of the other pocket runs the default path and returns
    the samples of a call without `restraints`.  Composes with `pinned`; with pin_resamples > 1 it is a ValueError."""
    from test_gpu_api import graph_from, make_model
    n_t = 20
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[3, 5, 4], [4, 3, 6]]
    c0 = pockets[0].prot_x.mean(dim=0).float()
    restraints = [[("repel", None, c0.tolist(), 4.0, 1.0), ("attract", 2, (c0 + torch.tensor([3.0, 0.0, 1.0])).tolist(), 1.0, 2.0)], None]
    pin_x = (c0 + torch.tensor([[1.25, -0.5, 0.75]])).float()
    pinned = [(pin_x, torch.tensor([2]), None), None]
    gen = torch.Generator().manual_seed(11)
    nz = [torch.randn(n_t + 1, 12, 9, generator=gen), torch.randn(n_t + 1, 13, 9, generator=gen)]
    kw = dict(max_batch_size=3, lanes=2, noise=nz)
    out = m.sample(pockets, n_pharms, restraints=restraints, guide_scale=2.0, guide_clip=1.5, pinned=pinned, **kw)
    plain = m.sample(pockets, n_pharms, pinned=pinned, **kw)
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    for p, q in zip(out[1], plain[1]):                  # the free pocket: the default path's samples
        assert torch.equal(p.ph_coords, q.ph_coords) and torch.equal(p.g.pharm_h0, q.g.pharm_h0)
    assert any(not torch.equal(p.ph_coords, q.ph_coords) for p, q in zip(out[0], plain[0]))
    for p in out[0]:
        assert torch.equal(p.ph_coords[:1], pin_x) and torch.isfinite(p.ph_coords).all()
    with pytest.raises(ValueError, match="resampling"):
        m.sample(pockets, n_pharms, restraints=restraints, pinned=pinned, pin_resamples=2, **kw)
    with pytest.raises(ValueError, match="center 2"):
        m.sample(pockets, [[2, 5, 4], [4, 3, 6]], restraints=restraints, **kw)
    # the engine-level run on the same batch, on the handle the model's lane 0 uses
    g0 = m._with_pins(pockets, n_pharms, pinned)[0]
    batch_g = pfa.batch(pfa.copy_graph(g0, n_copies=3, pharm_feats_per_copy=torch.tensor(n_pharms[0])))
    eng = m.dynamics.bind_graph(batch_g)
    gamma = m.gamma.gamma
    order = list(reversed(range(n_t)))
    arr = eng.coef_array(m.step_coefficients(), order)
    parr = eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order)
    garr = eng.guide_coef_array(pfa.schedule.guide_coefficients(gamma, n_t), order)
    com = pockets[0].prot_x.mean(dim=0).float().repeat(3, 1)
    x0, h0 = eng.sample(arr, n_t, nz[0], init_pharm_com=com, ep_coord=m.endpoint_param_coord, ep_feat=m.endpoint_param_feat,
                        feat_norm_constant=float(m.pharm_feat_norm_constant), pins=(batch_g.pharm_pin, batch_g.pharm_pin_x, batch_g.pharm_pin_h),
                        pin_coef_arr=parr, restraints=[restraints[0]] * 3, guide_coef_arr=garr, guide_scale=2.0, guide_clip=1.5)
    eng.sample_status()
    x0, h0 = x0.cpu(), h0.cpu()
    ptr = batch_g.pharm_ptr.tolist()
    for i, p in enumerate(out[0]):
        assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.equal(p.g.pharm_h0, h0[ptr[i]:ptr[i + 1]])
    # a call whose restraints are all empty is the call without them
    empty = m.sample(pockets, n_pharms, restraints=[[], None], pinned=pinned, **kw)
    for a, b in zip(empty[0] + empty[1], plain[0] + plain[1]):
        assert torch.equal(a.ph_coords, b.ph_coords)


def test_cli_with_restraints(tmp_path):
    """generate_pharmacophores.py --restraints writes the pharms.xyz the reference composition predicts (the pattern of
    test_gpu_api.test_generate_pharmacophores_cli_end_to_end: same files, same seed, same draws)."""
    import os
    import subprocess
    import sys
    import yaml
    from test_gpu_api import _write_pocket_files
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_pocket_files(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    T = 12
    cfg['diffusion']['n_timesteps'] = T
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
           "--guide_scale", "2.0", "--guide_clip", "1.0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    xyz = (out / "rec" / "pharms.xyz").read_text().splitlines()
    e = O.radius_graph(pos, 3.5, torch.tensor([0, pos.shape[0]]), 100)
    pk = P.process_ligand_and_pocket(tmp_path / "rec.pdb", None, emap, cfg['graph']['graph_cutoffs'], 8.0, lig_file=tmp_path / "lig.sdf",
                                     pp_edges=(e[0], e[1]))
    pocket1 = O.PocketBatch(pk.prot_x, pk.prot_h, torch.tensor([0, pk.prot_x.shape[0]]), torch.tensor([0, 1]), pk.pp_src.long(), pk.pp_dst.long())
    torch.manual_seed(1)
    nz = torch.randn(T + 1, 12, 9, device="cuda").cpu()
    b = O.concat_pockets([O.copy_pocket(pocket1, n) for n in (3, 4, 5)])
    restraints = [P.parse_restraints(text)] * 3
    free = (torch.zeros(12, dtype=torch.int32), torch.zeros(12, 3), torch.zeros(12, 6))
    com = O.segment_mean(b.prot_x, b.prot_ptr)
    prec = float(cfg['diffusion'].get('precision', 1e-5))
    ref = G.guided_reference(sd, O.DynamicsConfig(), b, T, prec, nz, *free, com, restraints, scale=2.0, clip=1.0)
    un = G.guided_reference(sd, O.DynamicsConfig(), b, T, prec, nz, *free, com, None)
    assert float((ref.x0 - un.x0).abs().max()) > 0.1     # the restraints moved the samples
    rows = [l.split() for l in xyz if len(l.split()) == 4]
    assert len(rows) == 12
    scale = max(abs(float(v)) for r in rows for v in r[1:])
    for r, xw, kw in zip(rows, ref.x0.tolist(), ref.h0.argmax(1).tolist()):
        assert r[0] == "PSFNOC"[kw], (r, kw)
        assert all(abs(float(u) - v) <= 5e-3 * max(1.0, scale) for u, v in zip(r[1:], xw)), (r, xw)
