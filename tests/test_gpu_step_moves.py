"""The sampler's move kernels (csrc/pf_stepmove.h: one skeleton, one struct per run kind) at the shapes the other suites do not
reach -- tests/step_move_cases.py: four graphs of 300 / 70 / 33 / 48 atoms with 64 / 1 / 17 / 2 centers, so every lane of the wave
that owns a graph's centers, the stride-64 loop of the frame offset, the stride-256 loop of the COM removal and a graph whose single
center is its own COM.  pharm_nf 6, rec_nf 11, T = 24 at precision 0.25, the live head.

pinned_renoise / seeded / multistep run as test_gpu_feature_counts.test_other_step_kinds runs them, against the CPU compositions of
resample_ref / seeded_ref / fewstep_ref at rtol = atol = 5e-3, twice: the default (the move + the edge build in one launch) and
PFDYN_NO_ENC_FLY=1 (the move alone).  The two are NOT compared bit for bit: with the encoders in launches of their own the dynamics
call reads them through h[N][128] and its outputs differ in the last bits (test_gpu_parity.test_fused_update_and_edge_build_variants_agree
asserts 1e-5 between those two environments, not equality), so each form is held to the reference.  The guided run (the move alone
in every environment) is driven through the step API: the first step's E / g0 / grad / shift inside helpers.within_budget as
test_gpu_guidance.test_one_step_within_the_fp64_budget, the four steps' frames and energies at 5e-3 as its check_run.  Given
positions and rows come back bit for bit.

Conditions on the inputs, on the CPU (test_step_moves_host.py): fp32 against fp64 composition 4.4e-7 (pinned + re-noise), 8.6e-7
(seeded), 8.8e-7 (multistep), 2.0e-6 (guided; E 8.7e-6 on values up to 65, shift 2.9e-6 with the clip active)."""
import pytest
import torch

import guidance_ref as G
import step_move_cases as M
import test_gpu_feature_counts as FC
from helpers import within_budget
from oracle import pf_oracle as O
from test_gpu_wide import engine_for, set_batch

pytestmark = pytest.mark.gpu

FORMS = {"build": {}, "alone": {"PFDYN_NO_ENC_FLY": "1"}}


def engine(c, sd, env, monkeypatch):
    monkeypatch.setenv("PFDYN_NO_CENTER_HOIST", "1")       # as test_other_step_kinds
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_for(c.cfg, sd)
    for k in env:
        monkeypatch.delenv(k)
    set_batch(eng, c.batch)
    return eng


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["pinned_renoise", "seeded", "multistep"])
def test_move_kinds_at_the_edge_shapes(kind, form, monkeypatch):
    from test_gpu_seeded import check
    assert (FC.RUN_T, FC.RUN_PREC, FC.PINNED_PLAN, FC.SEED_LEVEL, FC.MS_LEVELS) == (M.RUN_T, M.RUN_PREC, M.PINNED_PLAN, M.SEED_LEVEL, M.MS_LEVELS)
    c, sd, noise, pins, com, _ = M.case()
    eng = engine(c, sd, FORMS[form], monkeypatch)
    got = FC.run_kind(kind, eng, c, noise, pins, com)
    eng.sample_status()
    assert eng.xchg_timeouts() == 0
    x0, h0, tx, th = check(got, M.reference(kind), f"step moves, edge shapes: {kind}, {form}")
    if kind == "pinned_renoise":
        flags, pin_x, pin_h = pins
        mx, mh = (flags & 1) != 0, (flags & 2) != 0
        assert int(mx.sum()) == 7 and int(mh.sum()) == 6
        assert eng.kernel_family(c.cfg.n_convs) == 0      # no tail, fused-tail or merged launch in a pinned run
        assert torch.equal(x0[mx], pin_x[mx]) and torch.equal(h0[mh], pin_h[mh])
        assert torch.equal(tx[-1][mx], pin_x[mx]) and torch.equal(th[-1][mh], pin_h[mh])
        assert not torch.equal(tx[2][mx], pin_x[mx])      # earlier frames show the noised state


def test_guided_move_at_the_edge_shapes():
    """Four guided steps with pins, scale guidance_ref.GUIDE_SCALE, clip 0.5: an attract on center 63 of graph 0 plus a repel sphere
    on all its centers, an attract on the single (given) center of graph 1, none on graph 2, a repel on the two given centers of graph 3."""
    from test_gpu_guidance import arrays
    c, sd, noise, pins, com, restraints = M.case()
    flags, pin_x, pin_h = pins
    r32, r64 = M.reference("guided"), M.reference("guided", True)
    eng = engine_for(c.cfg, sd)
    set_batch(eng, c.batch)
    arr, parr, garr = arrays(eng, M.RUN_T, M.RUN_PREC)
    eng.set_train_family("wide")
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_clip=M.GUIDE_CLIP)
    fx, fh = ([t.cpu()] for t in eng.sample_frame())
    en = []
    for i in range(M.GUIDED_STEPS):
        eng.guided_step(arr[i], parr[i], garr[i], noise[i + 1])
        g0, grad, shift, e = (t.cpu() for t in eng.last_guidance())
        en.append(e)
        if i == 0:                                          # one step from the reference's own state: the fp64 budget
            within_budget(e, r32.E[0], r64.E[0], "step moves guided E")
            within_budget(g0, r32.g0[0], r64.g0[0], "step moves guided g0")
            within_budget(grad, r32.grad[0], r64.grad[0], "step moves guided grad")
            within_budget(shift, r32.shift[0], r64.shift[0], "step moves guided shift")
        n = shift.double().norm(dim=1)
        assert float(n.max()) <= M.GUIDE_CLIP * (1 + 1e-6) and bool((n >= M.GUIDE_CLIP * (1 - 1e-6)).any())      # the clip is active
        torch.testing.assert_close(shift, r32.shift[i], rtol=5e-3, atol=5e-3)
        if i < M.GUIDED_STEPS - 1:
            x, h = eng.sample_frame()
            fx.append(x.cpu()); fh.append(h.cpu())
    x0, h0 = (t.cpu() for t in eng.sample_end())
    assert eng.kernel_family(c.cfg.n_convs) == 0 and eng.xchg_timeouts() == 0
    eng.sample_status()
    tx, th, en = torch.stack(fx + [x0]), torch.stack(fh + [h0]), torch.stack(en)
    pairs = ((x0, r32.x0), (h0, r32.h0), (tx, r32.fx), (th, r32.fh), (en, r32.E))
    print("step moves, edge shapes: guided worst |error|: x0 %.3g h0 %.3g frames x %.3g h %.3g E %.3g" % tuple(float((a - b).abs().max()) for a, b in pairs))
    for a, b in pairs:
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=5e-3, atol=5e-3)
    mx, mh = (flags & 1) != 0, (flags & 2) != 0
    assert torch.equal(x0[mx], pin_x[mx]) and torch.equal(h0[mh], pin_h[mh])
