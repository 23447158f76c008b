"""Run kinds do not leak into each other: a handle that has finished a run of kind A gives, for a run of kind B, the bits a fresh
handle gives -- for every ordered pair of plain, pinned, resampled (jump 3, 2 resamples) and guided.  What a run leaves on the
handle (the run state, the pin and restraint arrays, the snapshot, the center hoist, the rows computed ahead, the tail flags, the
edges' records, the training family) must not reach the next one.

Shape: two graphs of 12 and 20 atoms with 2 and 3 centers, n_convs 2, T = 8 (the resampled run has 19 ops, 3 of them jumps).
The assertion is torch.equal: the sampler is bitwise repeatable."""
import functools

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O
from test_gpu_pinned import bound, engine_for, pins_for

pytestmark = pytest.mark.gpu

T, PREC, JUMP, RESAMPLES = 8, 0.25, 3, 2
KINDS = ("plain", "pinned", "resampled", "guided")


@functools.lru_cache(maxsize=None)
def case():
    cfg = O.DynamicsConfig()
    assert cfg.n_convs == 2
    sd = O.make_state_dict(cfg, 0)
    batch = O.synthetic_batch([21, 22], [12, 20], [2, 3], cfg)
    plan = pfa.schedule.resample_plan(T, JUMP, RESAMPLES)
    noise = torch.randn(len(plan) + 1, 5, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(11))
    pins = pins_for(batch, cfg, [3, 0] + [1, 2, 0])
    com = O.segment_mean(batch.prot_x, batch.prot_ptr) + 0.5
    restraints = [[("attract", 1, (com[0] + 1.0).tolist(), 1.0, 1.0)], [("repel", None, (com[1] - 1.0).tolist(), 3.0, 0.5)]]
    return cfg, sd, batch, plan, noise, pins, com, restraints


def run(eng, kind):
    """one whole run of ``kind`` with the case's noise: (x_0, h_0, frames x, frames h) on the host"""
    cfg, sd, batch, plan, noise, pins, com, restraints = case()
    gamma = O.gamma_table(T, PREC)
    coef, pin = O.step_coefficients(gamma, T), pfa.schedule.pin_coefficients(gamma, T)
    order = list(reversed(range(T)))
    kw = dict(init_pharm_com=com, trajectory=True)
    if kind == "resampled":
        pairs = [(op[1], op[2]) for op in plan if op[0] == "renoise"]
        arr, parr, op_arr, re_arr = eng.plan_arrays(plan, coef, pin, pfa.schedule.renoise_coefficients(gamma, T, pairs))
        out = eng.sample(arr, len(plan), noise, pins=pins, pin_coef_arr=parr, plan=(op_arr, re_arr), **kw)
    elif kind == "plain":
        out = eng.sample(eng.coef_array(coef, order), T, noise[:T + 1], **kw)
    else:
        if kind == "guided":
            kw.update(restraints=restraints, guide_coef_arr=eng.guide_coef_array(pfa.schedule.guide_coefficients(gamma, T), order), guide_scale=2.0)
        out = eng.sample(eng.coef_array(coef, order), T, noise[:T + 1], pins=pins, pin_coef_arr=eng.pin_coef_array(pin, order), **kw)
    out = tuple(t.cpu() for t in out)
    eng.sample_status()
    return out


def fresh_engine():
    cfg, sd, batch = case()[:3]
    return bound(engine_for(cfg, sd), batch)


@functools.lru_cache(maxsize=None)
def fresh(kind):
    return run(fresh_engine(), kind)


def test_the_kinds_differ():
    """the four runs are four different runs (a test of leaks between equal runs would prove nothing)"""
    for a in KINDS:
        for b in KINDS:
            if a < b and fresh(a)[0].shape == fresh(b)[0].shape:
                assert not torch.equal(fresh(a)[0], fresh(b)[0]), (a, b)


@pytest.mark.parametrize("second", KINDS)
@pytest.mark.parametrize("first", KINDS)
def test_second_run_equals_the_fresh_handle(first, second):
    eng = fresh_engine()
    got_first = run(eng, first)
    for a, b in zip(got_first, fresh(first)):
        assert torch.equal(a, b)
    got = run(eng, second)
    want = fresh(second)
    assert len(got) == len(want) == 4
    for name, a, b in zip(("x0", "h0", "frames x", "frames h"), got, want):
        assert a.shape == b.shape and torch.equal(a, b), f"{first} then {second}: {name} differs by {float((a - b).abs().max()):.3g}"
    assert eng.train_family() == "tuned"
    if second != "plain":                               # the given values come back bit for bit
        flags, pin_x, pin_h = case()[5]
        mx, mh = (flags & 1) != 0, (flags & 2) != 0
        assert torch.equal(got[0][mx], pin_x[mx]) and torch.equal(got[1][mh], pin_h[mh])
        assert torch.equal(got[2][-1][mx], pin_x[mx]) and torch.equal(got[3][-1][mh], pin_h[mh])
