"""GPU tests of the guarded optimiser step (pf_adam_step_guarded, csrc/pf_optim.hip): the three launches on vectors of every
length at which they take another path (pf_debug_optim_step), then FlatAdam's new arguments on the model.

Adam is nearly scale-invariant in the gradient (at step 1 the update is about lr * sign(g) whatever coef is), so every
comparison includes exp_avg and exp_avg_sq, and the "would a wrong kernel pass" assertions are made on the moments."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O
from helpers import BUDGET_FACTOR, BUDGET_FLOOR, batch_from, load, within_budget
import optim_ref as R
from test_gpu_api import _write_pocket_files, graph_from, make_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
CHUNK = pfa._lib.load().pf_debug_optim_chunk()
SIZES = [1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17]
N_BIG = 3 * CHUNK + 17
MODES = {"none": R.CLIP_NONE, "norm": R.CLIP_NORM, "value": R.CLIP_VALUE}


@pytest.fixture(scope="module")
def eng():
    e = pfa.PfEngine(device="cuda:0")
    e.load_state_dict(O.make_state_dict(O.DynamicsConfig(), 0))
    e.param_layout()
    return e


def _dev(arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).clone().cuda() for a in arrs]


def _clip_kw(mode, clip):
    return {R.CLIP_NONE: {}, R.CLIP_NORM: dict(clip_norm=clip), R.CLIP_VALUE: dict(clip_value=clip)}[mode]


def _step(eng, arrs, state, mode=R.CLIP_NONE, clip=0.0, grad_scale=1.0, ema_decay=0.0):
    """pf_debug_optim_step on device copies of (p, g, m, v, ema); returns them (ema None stays None)"""
    t = _dev(arrs)
    eng.debug_optim_step(t[0], t[1], t[2], t[3], state, grad_scale=grad_scale, ema=t[4], ema_decay=ema_decay, **_clip_kw(mode, clip), **OPTS)
    return t


def _raw(state):
    return state.cpu().numpy().tobytes()


def _budget(ref32, ref64):
    m = float(np.abs(ref64).max())
    return BUDGET_FACTOR * max(float(np.abs(ref32.astype(np.float64) - ref64).max()) / m, BUDGET_FLOOR) * m


# ---- the norm ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_norm_against_fp64_and_bit_reproducible(eng, n):
    """norm = (float)sqrt(fp64 sum): fp64 accumulation leaves ~1e-13, the fp32 rounding of the result (half an ulp, 2**-24
    relative) dominates; 2**-22 is the bound.  Two calls on the same input: the same bits, in the norm and in every vector."""
    arrs = R.six_decades(n, 100 + n)
    want = R.grad_norm64(arrs[1])
    outs = []
    for _ in range(2):
        st = eng.optim_state()
        t = _step(eng, arrs, st, ema_decay=0.9)
        outs.append((_raw(st), [x.cpu() for x in t]))
    got = struct.unpack_from("<f", outs[0][0], 16)[0]
    rel = abs(got - want) / want
    print(f"norm n={n}: rel err {rel:.3e}")
    assert rel <= 2.0 ** -22
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)
    s = pfa.PfEngine.read_optim_state(st)
    assert s["applied"] == 1 and s["skipped"] == 0 and s["finite"] and s["coef"] == 1.0


# ---- the step against the fp64 reference --------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", SIZES)
def test_step_within_the_fp64_budget(eng, n, mode):
    mode = MODES[mode]
    arrs = R.six_decades(n, 200 + n)
    p, g, m, v, ema = arrs
    scale = 0.5
    norm = R.grad_norm64(g) * scale
    clip = {R.CLIP_NONE: 0.0, R.CLIP_NORM: 0.25 * norm, R.CLIP_VALUE: 0.25 * float(np.abs(g).max()) * scale}[mode]
    kw = dict(step=4, grad_scale=scale, clip_mode=mode, clip=clip, ema_decay=0.9, **OPTS)
    r64 = R.guarded_step(p, g, m, v, ema, **kw)
    r32 = R.guarded_step(p, g, m, v, ema, dtype=np.float32, **kw)
    if mode != R.CLIP_NONE:
        # on the reference alone: a kernel that dropped the clipping would miss the budget of m by far
        un = R.guarded_step(p, g, m, v, ema, **dict(kw, clip_mode=R.CLIP_NONE))
        assert np.abs(un.m - r64.m).max() >= 10 * _budget(r32.m, r64.m)
        assert np.abs(un.v - r64.v).max() >= 10 * _budget(r32.v, r64.v)
    st = eng.optim_state(3)                                      # three applied steps behind it: this one is step 4
    t = _step(eng, arrs, st, mode, clip, scale, 0.9)
    for name, got in zip(("p", "g", "m", "v", "ema"), t):
        if name == "g":
            assert torch.equal(got.cpu(), torch.from_numpy(g))
            continue
        within_budget(got, getattr(r32, name), getattr(r64, name), f"n={n} mode={mode} {name}")
    s = pfa.PfEngine.read_optim_state(st)
    assert s["applied"] == 4 and s["skipped"] == 0 and s["finite"]
    assert abs(s["norm"] - norm) <= 2.0 ** -21 * norm            # two fp32 roundings: the norm, then the scale
    assert abs(s["coef"] - r64.coef) <= 1e-6 and (mode != R.CLIP_NORM or abs(s["coef"] - 0.25) < 1e-5)


def test_unaligned_vectors_take_the_scalar_path_to_the_same_bits(eng):
    """vectors that start 4 bytes into an allocation (not 16-byte aligned): 4-byte accesses, the same elements per thread"""
    n = CHUNK + 5
    arrs = R.six_decades(n, 7)
    st = eng.optim_state()
    want = _step(eng, arrs, st, R.CLIP_NORM, 1.0, 1.0, 0.9)
    raw_a = _raw(st)
    pads = [torch.zeros(n + 1, device="cuda") for _ in range(5)]
    t = [q[1:] for q in pads]
    for dst, a in zip(t, arrs):
        dst.copy_(torch.from_numpy(a))
    assert all(x.data_ptr() % 16 == 4 for x in t)
    st = eng.optim_state()
    eng.debug_optim_step(t[0], t[1], t[2], t[3], st, ema=t[4], ema_decay=0.9, clip_norm=1.0, **OPTS)
    assert _raw(st) == raw_a
    for a, b in zip(want, t):
        assert torch.equal(a, b)
    assert all(float(q[0]) == 0.0 for q in pads)


# ---- exactness against pf_adam_step -----------------------------------------------------------------------------
def test_moments_are_bitwise_those_of_pf_adam_step(eng):
    """coef = 1 (max_norm = 4 * norm), scale 1, no EMA: exp_avg and exp_avg_sq carry k_adam's bits; the parameters are held to
    the budget (the bias corrections come from the device's own beta^t, not from std::pow)."""
    n = eng.n_params
    p, g, m, v, _ = R.six_decades(n, 11)
    a = _dev((p, g, m, v))
    eng.adam_step(a[0], a[1], a[2], a[3], 1, OPTS["lr"], OPTS["betas"], OPTS["eps"], OPTS["weight_decay"])
    clip = 4.0 * R.grad_norm64(g)
    st = eng.optim_state()
    b = _step(eng, (p, g, m, v, None), st, R.CLIP_NORM, clip)
    assert pfa.PfEngine.read_optim_state(st)["coef"] == 1.0
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert not torch.equal(b[2].cpu(), torch.from_numpy(m))
    kw = dict(step=1, clip_mode=R.CLIP_NORM, clip=clip, **OPTS)
    within_budget(b[0], R.guarded_step(p, g, m, v, dtype=np.float32, **kw).p, R.guarded_step(p, g, m, v, **kw).p, "exactness p")
    within_budget(a[0], R.guarded_step(p, g, m, v, dtype=np.float32, **kw).p, R.guarded_step(p, g, m, v, **kw).p, "pf_adam_step p")


# ---- the non-finite skip ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "chunk"])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=["inf", "-inf", "nan"])
def test_non_finite_gradient_skips_the_step(eng, bad, where):
    n = N_BIG
    arrs = R.six_decades(n, 31)
    p, g, m, v, ema = arrs
    gb = g.copy()
    gb[{"first": 0, "last": n - 1, "chunk": CHUNK}[where]] = bad
    st = eng.optim_state()
    t = _step(eng, (p, gb, m, v, ema), st, R.CLIP_NORM, 1.0, 1.0, 0.9)
    for got, want in zip(t, (p, gb, m, v, ema)):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    s = pfa.PfEngine.read_optim_state(st)
    assert s["skipped"] == 1 and s["applied"] == 0 and not s["finite"] and not np.isfinite(s["norm"])
    # the next, finite, step is APPLIED step 1 (bias corrections 1 - beta), not 2
    kw = dict(grad_scale=1.0, clip_mode=R.CLIP_NORM, clip=1.0, ema_decay=0.9, **OPTS)
    r64, r32 = R.guarded_step(*arrs, step=1, **kw), R.guarded_step(*arrs, step=1, dtype=np.float32, **kw)
    assert np.abs(R.guarded_step(*arrs, step=2, **kw).p - r64.p).max() >= 10 * _budget(r32.p, r64.p)
    t[1].copy_(torch.from_numpy(g))
    eng.debug_optim_step(t[0], t[1], t[2], t[3], st, ema=t[4], ema_decay=0.9, clip_norm=1.0, **OPTS)
    for name, got in zip(("p", "g", "m", "v", "ema"), t):
        if name != "g":
            within_budget(got, getattr(r32, name), getattr(r64, name), f"after skip {name}")
    s = pfa.PfEngine.read_optim_state(st)
    assert s["skipped"] == 1 and s["applied"] == 1 and s["finite"]


# ---- accumulation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_doubled_gradient_at_half_scale_is_the_same_step(eng, mode):
    """g + g is exact in fp32 and so is the product with 0.5: bitwise the step on g at scale 1"""
    mode = MODES[mode]
    arrs = R.six_decades(N_BIG, 41)
    p, g, m, v, ema = arrs
    clip = 0.25 * R.grad_norm64(g) if mode == R.CLIP_NORM else 0.25 * float(np.abs(g).max())
    sa, sb = eng.optim_state(), eng.optim_state()
    a = _step(eng, arrs, sa, mode, clip, 1.0, 0.9)
    b = _step(eng, (p, g + g, m, v, ema), sb, mode, clip, 0.5, 0.9)
    for name, x, y in zip(("p", "g", "m", "v", "ema"), a, b):
        if name != "g":
            assert torch.equal(x, y), name
    assert _raw(sa) == _raw(sb)
    assert not torch.equal(a[2].cpu(), torch.from_numpy(m))


# ---- argument errors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(lr=float("nan")), dict(eps=float("inf")), dict(weight_decay=float("nan")), dict(betas=(1.0, 0.999)),
                                 dict(betas=(0.9, float("nan"))), dict(clip_norm=-1.0), dict(clip_value=-0.5),
                                 dict(clip_norm=float("inf")), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(grad_scale=0.0),
                                 dict(grad_scale=-1.0), dict(grad_scale=float("nan"))], ids=lambda d: "-".join(d))
def test_bad_options_are_refused_before_anything_runs(eng, bad):
    arrs = R.six_decades(300, 51)
    st = eng.optim_state(5)
    before = _raw(st)
    t = _dev(arrs)
    kw = dict(OPTS, grad_scale=1.0, ema_decay=0.9)
    kw.update(bad)
    with pytest.raises(pfa.PfError, match=r"\(-1\)"):             # PF_ERR_ARG
        eng.debug_optim_step(t[0], t[1], t[2], t[3], st, ema=t[4], **kw)
    torch.cuda.synchronize()
    for got, want in zip(t, arrs):
        assert got.cpu().numpy().tobytes() == want.tobytes()
    assert _raw(st) == before


def test_bad_clip_mode_and_null_vectors_are_refused(eng):
    L = pfa._lib
    st = eng.optim_state()
    t = _dev(R.six_decades(16, 1)[:4])
    ptr = lambda x: None if x is None else L.ctypes.c_void_p(x.data_ptr())
    opts = L.PfOptimOpts(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 3, 0.0, 0.0)
    assert eng.lib.pf_debug_optim_step(eng._h, 16, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), None, ptr(st), L.ctypes.byref(opts), None) == -1
    opts.clip_mode = 0
    assert eng.lib.pf_debug_optim_step(eng._h, 0, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), None, ptr(st), L.ctypes.byref(opts), None) == -1
    assert eng.lib.pf_debug_optim_step(eng._h, 16, ptr(t[0]), None, ptr(t[2]), ptr(t[3]), None, ptr(st), L.ctypes.byref(opts), None) == -1
    assert eng.lib.pf_adam_step_guarded(eng._h, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), None, None, L.ctypes.byref(opts), None) == -1
    assert eng.lib.pf_optim_state_init(eng._h, ptr(st), -1, None) == -1
    assert pfa.PfEngine.read_optim_state(st)["applied"] == 0 and eng.optim_chunk() == CHUNK


# =================================================================================================================
# the model: FlatAdam's new arguments on the train_grads.npz case of test_flat_adam_matches_torch_adam
# =================================================================================================================
@pytest.fixture(scope="module")
def case():
    z = load("train_grads.npz")
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    T = int(z["T"])
    inj2 = dict(t_int=(z["t_int"].long() + 7) % T, eps={'h': -z["eps_h"], 'x': z["eps_x"].flip(0)})
    m = _train_model(T)
    g = graph_from(batch_from(z), z["x0"], z["h0"]).to("cuda")
    m.zero_grad(set_to_none=True)
    m.training_step(g, 0, **inj).backward()
    g0 = m.dynamics._last_flat_grad.detach().double()
    return dict(z=z, b=batch_from(z), inj=inj, inj2=inj2, T=T, norm0=float(g0.norm()), max0=float(g0.abs().max()))


def _train_model(T):
    m = make_model(T)
    m.train()
    m.dynamics.dropout_rate = 0.0
    return m


def _graph(case):
    return graph_from(case["b"], case["z"]["x0"], case["z"]["h0"]).to("cuda")


@pytest.mark.parametrize("how", ["norm", "value"])
def test_flat_adam_with_clipping_matches_torch_clipping_then_adam(case, how):
    """Three steps; torch side: clip_grad_norm_ / clip_grad_value_ then torch.optim.Adam on the 244 tensors.  Parameters at the
    tolerance of test_flat_adam_matches_torch_adam (rtol 2e-4, atol 2e-6).  The moments per parameter: the same rtol -- the
    parameters differ only through them -- with the absolute part scaled to the tensor (2e-4 of its largest entry: the moments
    of this model are of order 1e-4 and 1e-8, the parameters' 2e-6 would hide them).  A step without the clipping is off by
    a factor 4 in exp_avg and 16 in exp_avg_sq."""
    clip = 0.25 * (case["norm0"] if how == "norm" else case["max0"])
    res = []
    for use_flat in (False, True):
        m = _train_model(case["T"])
        g = _graph(case)
        params = list(m.dynamics.parameters())
        opt = (pfa.FlatAdam(m.dynamics, lr=1e-3, weight_decay=1e-2, **{"clip_" + how: clip}) if use_flat
               else torch.optim.Adam(params, lr=1e-3, weight_decay=1e-2))
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            m.training_step(g, 0, **case["inj"]).backward()
            if not use_flat:
                with_grad = [p for p in params if p.grad is not None]
                if how == "norm":
                    total = torch.nn.utils.clip_grad_norm_(with_grad, clip)
                    assert float(total) > clip
                else:
                    assert any(bool((p.grad.abs() > clip).any()) for p in with_grad)
                    torch.nn.utils.clip_grad_value_(with_grad, clip)
            opt.step()
            if use_flat:
                assert opt.last_clip_coef() < 1.0 if how == "norm" else opt.last_clip_coef() == 1.0
                assert opt.last_grad_norm() > 0
        named = dict(m.dynamics.named_parameters())
        out = {}
        for name, off, n in m.dynamics.engine().param_layout():
            if n == 0:
                continue
            p = named[name[len("dynamics."):]]
            if use_flat:
                mom = (opt.exp_avg[off:off + n], opt.exp_avg_sq[off:off + n])
            else:
                mom = (opt.state[p]["exp_avg"].reshape(-1), opt.state[p]["exp_avg_sq"].reshape(-1))
            out[name] = tuple(x.detach().cpu().clone() for x in (p.reshape(-1),) + mom)
        if use_flat:
            assert opt.applied_steps() == 3 and opt.skipped_steps() == 0
        res.append(out)
    ref, got = res
    assert len(ref) > 200
    for name in ref:
        torch.testing.assert_close(got[name][0], ref[name][0], rtol=2e-4, atol=2e-6, msg=lambda s: f"{name}: {s}")
        for k, what in ((1, "exp_avg"), (2, "exp_avg_sq")):
            torch.testing.assert_close(got[name][k], ref[name][k], rtol=2e-4, atol=2e-4 * float(ref[name][k].abs().max()),
                                       msg=lambda s: f"{name} {what}: {s}")


def test_flat_adam_without_new_arguments_is_the_legacy_step(case):
    """Bitwise the parameters that pf_adam_step gives when it is called the way FlatAdam.step called it before the guarded
    entry existed."""
    ma, mb = _train_model(case["T"]), _train_model(case["T"])
    g = _graph(case)
    opt = pfa.FlatAdam(ma.dynamics, lr=1e-3, weight_decay=1e-2)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        ma.training_step(g, 0, **case["inj"]).backward()
        opt.step()
    assert not opt.guarded and opt._state is None and opt.t == 3 and opt.applied_steps() == 3 and opt.ema is None
    dyn = mb.dynamics
    ea = es = None
    for t in range(1, 4):
        mb.zero_grad(set_to_none=True)
        mb.training_step(g, 0, **case["inj"]).backward()
        if ea is None:
            ea, es = torch.zeros_like(dyn._flat), torch.zeros_like(dyn._flat)
        dyn._engine.adam_step(dyn._flat, dyn._last_flat_grad, ea, es, t, 1e-3, (0.9, 0.999), 1e-8, 1e-2)
    assert torch.equal(ma.dynamics._flat, dyn._flat) and torch.equal(opt.exp_avg, ea) and torch.equal(opt.exp_avg_sq, es)


def _forward(m, g, B):
    with torch.no_grad():
        eh, ex = m.dynamics(g, torch.full((B,), 0.37, device="cuda"))
    return eh.clone(), ex.clone()


def test_ema_weights_context_swaps_and_restores(case, tmp_path):
    m = _train_model(case["T"])
    g = _graph(case)
    g.x_t, g.h_t = case["z"]["x0"].cuda(), case["z"]["h0"].cuda()
    B = case["b"].batch_size
    opt = pfa.FlatAdam(m.dynamics, lr=1e-2, ema_decay=0.5)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        m.training_step(g, 0, **case["inj"]).backward()
        opt.step()
    m.eval()
    flat_before = m.dynamics._flat.clone()
    assert not torch.equal(opt.ema, flat_before)
    out_before = _forward(m, g, B)
    m.save_checkpoint(tmp_path / "ema.ckpt", ema_state_dict=opt.ema_state_dict())
    other = make_model(case["T"])
    other.load_ema_weights(tmp_path / "ema.ckpt")
    want = _forward(other, g, B)
    assert torch.equal(other.dynamics._flat, opt.ema)
    with opt.ema_weights():
        assert torch.equal(m.dynamics._flat, opt.ema)
        inside = _forward(m, g, B)
    assert torch.equal(inside[0], want[0]) and torch.equal(inside[1], want[1])
    assert not torch.equal(inside[0], out_before[0])
    after = _forward(m, g, B)
    assert torch.equal(m.dynamics._flat, flat_before) and torch.equal(after[0], out_before[0]) and torch.equal(after[1], out_before[1])
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    after = _forward(m, g, B)
    assert torch.equal(m.dynamics._flat, flat_before) and torch.equal(after[0], out_before[0]) and torch.equal(after[1], out_before[1])
    with pytest.raises(RuntimeError, match="ema_decay"):
        with pfa.FlatAdam(m.dynamics).ema_weights():
            pass


def test_two_micro_batches_accumulate_into_one_scaled_step(case):
    m = _train_model(case["T"])
    g = _graph(case)
    dyn = m.dynamics
    clip = 0.25 * case["norm0"]
    opt = pfa.FlatAdam(dyn, clip_norm=clip, ema_decay=0.9, **OPTS)
    opt.zero_grad(set_to_none=True)
    m.training_step(g, 0, **case["inj"]).backward()
    opt.step()                                                   # (a first step: the gradient views are bound, lazy clears apply)
    single = []
    for inj in (case["inj"], case["inj2"]):
        opt.zero_grad()
        m.training_step(g, 0, **inj).backward()
        single.append(dyn._last_flat_grad.clone())
    assert not torch.equal(single[0], single[1])
    opt.zero_grad(lazy=True)                                     # on the first micro-batch only
    m.training_step(g, 0, **case["inj"]).backward()
    m.training_step(g, 1, **case["inj2"]).backward()
    gsum = dyn._last_flat_grad.clone()
    assert torch.equal(gsum, single[0] + single[1])
    before = [x.detach().cpu().numpy().copy() for x in (dyn._flat, gsum, opt.exp_avg, opt.exp_avg_sq, opt.ema)]
    opt.step(grad_scale=0.5)
    kw = dict(step=2, grad_scale=0.5, clip_mode=R.CLIP_NORM, clip=clip, ema_decay=0.9, **OPTS)
    r64, r32 = R.guarded_step(*before, **kw), R.guarded_step(*before, dtype=np.float32, **kw)
    for name, got in (("p", dyn._flat), ("m", opt.exp_avg), ("v", opt.exp_avg_sq), ("ema", opt.ema)):
        within_budget(got, getattr(r32, name), getattr(r64, name), "accumulated " + name)
    assert opt.applied_steps() == 2 and abs(opt.last_grad_norm() - r64.norm) <= 2.0 ** -21 * r64.norm
    assert abs(opt.last_clip_coef() - r64.coef) <= 1e-6 and r64.coef < 1.0


def test_state_dict_carries_the_applied_count_and_a_resumed_run_continues_bitwise(case):
    m = _train_model(case["T"])
    g = _graph(case)
    dyn = m.dynamics
    opt = pfa.FlatAdam(dyn, lr=1e-3, weight_decay=1e-2, clip_norm=0.25 * case["norm0"], ema_decay=0.9, ema_warmup=True)
    for k in range(2):
        opt.zero_grad(set_to_none=True)
        m.training_step(g, 0, **case["inj"]).backward()
        if k == 1:                                               # a poisoned gradient: this step is skipped on the device
            keep = [x.clone() for x in (dyn._flat, opt.exp_avg, opt.exp_avg_sq, opt.ema)]
            dyn._last_flat_grad[12345] = float("nan")
        opt.step()
    for a, b in zip(keep, (dyn._flat, opt.exp_avg, opt.exp_avg_sq, opt.ema)):
        assert torch.equal(a, b)
    assert opt.skipped_steps() == 1 and opt.applied_steps() == 1 and not np.isfinite(opt.last_grad_norm())
    sd = opt.state_dict()
    assert sd["state"]["step"] == 1 and sd["guard"]["skipped"] == 1 and sd["guard"]["calls"] == 2
    m2 = make_model(case["T"])
    m2.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, strict=True)
    m2.train()
    m2.dynamics.dropout_rate = 0.0
    opt2 = pfa.FlatAdam(m2.dynamics)
    m2.dynamics.engine()
    opt2.load_state_dict(sd)
    assert opt2.guarded and opt2.clip_norm == opt.clip_norm and opt2.ema_decay == 0.9 and opt2.ema_warmup
    assert torch.equal(m2.dynamics._flat, dyn._flat) and torch.equal(opt2.ema, opt.ema)
    for mm, oo in ((m, opt), (m2, opt2)):
        oo.zero_grad(set_to_none=True)
        mm.training_step(g, 0, **case["inj"]).backward()
        oo.step()
    assert opt.applied_steps() == 2 and opt2.applied_steps() == 2
    assert not torch.equal(keep[0], dyn._flat)
    for a, b in ((dyn._flat, m2.dynamics._flat), (opt.exp_avg, opt2.exp_avg), (opt.exp_avg_sq, opt2.exp_avg_sq), (opt.ema, opt2.ema)):
        assert torch.equal(a, b)


def test_train_driver_with_accumulation_clipping_and_ema(tmp_path):
    """train.py with accumulate_grad_batches 2, gradient_clip_val and ema_decay: exits 0, logs grad_norm, names the trainer
    argument it ignores, and writes a checkpoint from which generate_pharmacophores.py --use_ema samples."""
    rng = np.random.default_rng(0)
    proc = tmp_path / "processed"
    for split in range(3):
        d = proc / f"split_{split}"
        d.mkdir(parents=True)
        n_g = 6
        np_, nf_ = np.full(n_g, 40), rng.integers(3, 8, n_g)
        pos = np.concatenate([O.synthetic_pocket(100 * split + i, 40)[0].numpy() for i in range(n_g)]).astype(np.float32)

        def idx(c):
            e = np.cumsum(c)
            return np.stack([e - c, e], 1)
        np.savez(d / 'prot_pharm_tensors.npz', prot_pos=pos, prot_feat=rng.integers(0, 4, np_.sum()), prot_idx=idx(np_),
                 pharm_pos=(rng.normal(size=(nf_.sum(), 3)) * 3).astype(np.float32), pharm_feat=rng.integers(0, 6, nf_.sum()),
                 pharm_idx=idx(nf_), prot_ph_pos=np.zeros((0, 3), np.float32), prot_ph_feat=np.zeros((0,), np.int64),
                 prot_ph_idx=np.zeros((n_g, 2), np.int64))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "dev_config_subset.yml")))
    cfg['diffusion']['n_timesteps'] = 12
    cfg['dataset'].update(processed_data_dir=str(proc), raw_data_dir=str(tmp_path), pocket_cutoff=8)
    cfg['training'].update(output_dir=str(tmp_path / "runs"), batch_size=2, num_workers=0, validation_splits=[2], ema_decay=0.9)
    cfg['training']['trainer_args'] = dict(max_epochs=1, accumulate_grad_batches=2, gradient_clip_val=0.5, log_every_n_steps=10)
    cfg.setdefault('wandb', {})['name'] = 'guarded'
    yaml.dump(cfg, open(tmp_path / "cfg.yml", "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--config", str(tmp_path / "cfg.yml"), "--seed", "0",
                        "--bind_prefetch"],                  # (the EMA swap joins the look-ahead bind; a deepcopy of the model would fail here)
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "grad_norm" in r.stdout and "val total loss" in r.stdout
    assert "trainer_args not acted on by this driver: log_every_n_steps" in r.stdout
    assert "accumulate_grad_batches 2" in r.stdout and "clip_norm 0.5" in r.stdout
    ck = list((tmp_path / "runs").glob("*/checkpoints/last.ckpt"))
    assert len(ck) == 1
    saved = torch.load(str(ck[0]), map_location="cpu", weights_only=False)
    assert saved["optimizer_states"][0]["state"]["step"] + saved["optimizer_states"][0]["guard"]["skipped"] == saved["global_step"] >= 2
    ema = saved["ema_state_dict"]
    assert any(not torch.equal(ema[k], saved["state_dict"][k]) for k in ema) and all(torch.isfinite(v).all() for v in ema.values())
    _write_pocket_files(tmp_path)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
                        str(tmp_path / "lig.sdf"), "--model_dir", str(ck[0].parent.parent), "--samples_per_pocket", "2", "--pharm_sizes",
                        "3", "4", "--output_dir", str(out), "--seed", "1", "--use_ema"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "EMA weights" in r.stdout and (out / "rec" / "pharms.xyz").exists()
