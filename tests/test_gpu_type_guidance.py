"""Type guidance of a guided run (pf_guide_types_next: typed restraints and the complementarity energy's type gradient steer the
centers' feature rows; k_guide_types and the TYPES form of k_guide_field behind k_guide_grad, the feature-shift form of the step
end) against the CPU composition of tests/type_guidance_ref.py: pocket_field_ref.field_reference with the lines of DESIGN 4.24.

Shape: pocket_field_ref.case() -- five ragged pockets of 48 / 300 / 40 / 64 / 32 atoms, 3 / 8 / 5 / 1 / 6 centers, graph 1 with a
type-pinned center, T = 24, live head, the field with 0 / 70 / 5 / 1 / 3 receptor features -- with type restraints on graphs 1 (no
window, every center), 2 (a window of 6 A on every center) and 3 (no window, the single center), complementarity with a type
gradient and unmatched = 1.5 everywhere, feat_scale 4.  Whole runs at rtol = atol = 5e-3 in both parameterisations on the tuned
family and at (64, 32), T = 12 on the wide family; the same runs must MISS the references that ignore the arming, drop J_h, or leave
g_eps_h zero.  One step read back against fp64 under helpers.within_budget, also at pharm_nf = 7; one tall step (64 centers)
bitwise equal on a second run.

Measured on the MI355X, worst |error| over x_0, h_0 and all frames: 1.0e-4 (noise; energies 7.3e-4, the last E_type 4.7e-6),
1.3e-6 (endpoint; energies 7.6e-6), 8.4e-4 at (64, 32) (energies 3.3e-2 on values of several hundred); the noise run misses the
references without the arming / without J_h / with a zero g_eps_h by 6.29 / 2.56 / 0.254.  One step against the fp64 reference,
ratio to max(e32, 2**-22) of E / g0 / grad / shift / g0_h / grad_h / shift_h / E_type: 0.14 / 1.62 / 1.22 / 1.21 / 0.90 / 0.96 /
1.03 / 0.08 (noise), 0.26 / 0.85 / 0.75 / 0.75 / 0.46 / 0.48 / 0.49 / 0.15 (endpoint), 0.06 / 0.27 / 0.28 / 0.26 / 0.57 / 0.60 /
0.58 / 0.06 (pharm_nf = 7), 0.36 / 0.61 / 0.79 / 0.75 / 0.45 / 0.46 / 0.53 / 0.26 (the tall graph); of the allowed 8.

Conditions on the inputs are checked on the CPU by test_type_guidance_host.py."""

import pytest
import torch

import pharmacoforge_amd as pfa
import guidance_ref as G
import pocket_field_ref as F
import type_guidance_ref as TG
from helpers import within_budget
from oracle import pf_oracle as O
from test_gpu_guidance import ERR_ARG, ERR_STATE, arrays, check_run
from test_gpu_pinned import bound, engine_for

pytestmark = pytest.mark.gpu

T = TG.T


def run_types(eng, n_t, noise, pins, com, restraints, fd, tg, family="tuned", **kw):
    arr, parr, garr = arrays(eng, n_t)
    return eng.sample(arr, n_t, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr,
                      guide_scale=G.GUIDE_SCALE, guide_family=family, field=None if fd is None else F.field_kwargs(fd),
                      types=None if tg is None else (tg if isinstance(tg, dict) else TG.types_kwargs(tg)), **kw)


# 1. whole runs
@pytest.mark.parametrize("ep", [False, True])
def test_types_run_vs_composition(ep):
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_types(eng, T, noise, pins, com, restraints, fd, tg, ep_coord=ep, ep_feat=ep, trajectory=True, energies=True)
    assert eng.train_family() == "tuned" and eng.train_input_grads() is False
    ref = TG.reference(ep)
    check_run(eng, cfg, got, ref, pins, f"types, tuned {'ep' if ep else 'noise'} (k = {k})")
    e_type = eng.last_type_guidance()[3].cpu()
    print("E_type of the last step, worst |error|: %.3g" % float((e_type - ref.E_type[-1]).abs().max()))
    torch.testing.assert_close(e_type, ref.E_type[-1], rtol=G.TOL, atol=G.TOL)
    if ep:
        return
    # ... and it is no rounding error of a run that ignored the arming, dropped J_h or kept the zero g_eps_h
    tx, th = got[2].cpu(), got[3].cpu()
    for name, un in (("without the arming", TG.reference(ep, False, False)), ("without J_h", TG.reference(ep, False, True, False)),
                     ("with a zero g_eps_h", TG.reference(ep, False, True, True, True))):
        miss = max(float((tx - un.fx).abs().max()), float((th - un.fh).abs().max()))
        print(f"the reference {name} is missed by {miss:.3g}")
        assert miss >= 10 * G.TOL
        with pytest.raises(AssertionError):
            torch.testing.assert_close(torch.cat([tx, th], dim=2), torch.cat([un.fx, un.fh], dim=2), rtol=G.TOL, atol=G.TOL)


def test_types_run_width_generic_family():
    """(64, 32), T = 12, a type-pinned center, feat_norm_constant 2, the wide family"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    got = run_types(eng, G.WIDE_T, noise, pins, com, restraints, fd, tg, family="wide", feat_norm_constant=2.0, trajectory=True,
                    energies=True)
    assert eng.kernel_family(0) == 64
    ref = TG.wide_reference()
    check_run(eng, cfg, got, ref, pins, f"types (64, 32) (k = {k})")
    torch.testing.assert_close(eng.last_type_guidance()[3].cpu(), ref.E_type[-1], rtol=G.TOL, atol=G.TOL)
    with pytest.raises(AssertionError):
        torch.testing.assert_close(got[3].cpu(), TG.wide_reference(False).fh, rtol=G.TOL, atol=G.TOL)


# 2. one step read back
def one_step(eng, n_t, noise, pins, com, restraints, fd, tg, ep=False, family="tuned"):
    arr, parr, garr = arrays(eng, n_t)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family=family,
                     field=None if fd is None else F.field_kwargs(fd), types=tg if isinstance(tg, dict) else TG.types_kwargs(tg))
    eng.guided_step(arr[0], parr[0], garr[0], noise[1], ep_coord=ep, ep_feat=ep)
    out = tuple(t.cpu() for t in eng.last_guidance()) + tuple(t.cpu() for t in eng.last_type_guidance())
    if family == "tuned":
        eng.set_train_input_grads(False)
    return out


def budget(got, r32, r64, leg):
    g0, grad, shift, en, g0_h, grad_h, shift_h, e_type = got
    within_budget(en, r32.E[0], r64.E[0], f"{leg} E")
    within_budget(g0, r32.g0[0], r64.g0[0], f"{leg} g0")
    within_budget(grad, r32.grad[0], r64.grad[0], f"{leg} grad")
    within_budget(shift, r32.shift[0], r64.shift[0], f"{leg} shift")
    within_budget(g0_h, r32.g0_h[0], r64.g0_h[0], f"{leg} g0_h")
    within_budget(grad_h, r32.grad_h[0], r64.grad_h[0], f"{leg} grad_h")
    within_budget(shift_h, r32.shift_h[0], r64.shift_h[0], f"{leg} shift_h")
    within_budget(e_type, r32.E_type[0], r64.E_type[0], f"{leg} E_type")


@pytest.mark.parametrize("ep", [False, True])
def test_one_step_within_the_fp64_budget(ep):
    leg = "types ep" if ep else "types noise"
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    kw = dict(scale=G.GUIDE_SCALE, ep=ep, n_steps=1)
    r32 = TG.types_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, fd, tg, **kw)
    r64 = TG.types_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, restraints, fd, tg, double=True, **kw)
    eng = bound(engine_for(cfg, sd), batch)
    got = one_step(eng, T, noise, pins, com, restraints, fd, tg, ep=ep)
    budget(got, r32, r64, leg)
    # the pocket field's three components keep their meaning, and the total is the documented sum
    e3 = eng.last_field_energies().cpu()
    for c, name in enumerate(("restraints", "clash", "complementarity")):
        within_budget(e3[:, c], r32.E3[0][:, c], r64.E3[0][:, c], f"{leg} E3 {name}")
    assert torch.equal(((e3[:, 0] + e3[:, 1]) + e3[:, 2]) + got[7], got[3])


def test_one_step_at_seven_feature_types():
    """pharm_nf = 7 (nf_cases.nf_case(7, 5): three pockets with 5 / 1 / 6 centers): the lanes-as-types mapping at a count other
    than 6, on the tuned family -- windowless and windowed restraints, one on the highest type; no field (the complementarity
    tables are those of the six types)"""
    from helpers import sampler_live_head
    from nf_cases import nf_case
    c = nf_case(7, 5)
    cfg, batch = c.cfg, c.batch
    Nf = int(batch.pharm_ptr[-1])
    n_t = 8
    noise = torch.randn(2, Nf, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(5))
    sd, k = sampler_live_head(c.sd, cfg, batch, n_t, G.PREC, noise)
    pins = (torch.zeros(Nf, dtype=torch.int32), torch.zeros(Nf, 3), torch.zeros(Nf, cfg.pharm_nf))
    pcom = O.segment_mean(batch.prot_x, batch.prot_ptr)
    com = pcom + 0.5
    tr = [[(6, None, (0.0, 0.0, 0.0), 0.0, 1.0), (2, 3, pcom[0].tolist(), 40.0, 2.0)], [(0, 0, (0.0, 0.0, 0.0), 0.0, 1.0)],
          [(5, None, pcom[2].tolist(), 50.0, 1.0), (6, 1, (0.0, 0.0, 0.0), 0.0, 0.5)]]
    tg = TG.make_types(tr, scale=TG.FEAT_SCALE, sharpness=TG.SHARP)
    kw = dict(scale=G.GUIDE_SCALE, n_steps=1)
    r32 = TG.types_reference(sd, cfg, batch, n_t, G.PREC, noise, *pins, com, None, None, tg, **kw)
    r64 = TG.types_reference(sd, cfg, batch, n_t, G.PREC, noise, *pins, com, None, None, tg, double=True, **kw)
    assert float(r64.g0[0].abs().max()) > 0 and bool((r64.g0_h[0].abs().amax(dim=1) > 0).all())
    eng = bound(engine_for(cfg, sd), batch)
    budget(one_step(eng, n_t, noise, pins, com, None, None, tg), r32, r64, "types nf = 7")


def tall_types(cfg, batch):
    pcom = O.segment_mean(batch.prot_x, batch.prot_ptr)
    return TG.make_types([[(3, None, pcom[0].tolist(), 12.0, 1.0), (1, 40, (0.0, 0.0, 0.0), 0.0, 2.0)]], scale=TG.FEAT_SCALE,
                         sharpness=TG.SHARP, complementarity=True, unmatched=TG.UNMATCHED)


def test_tall_graph_one_step_and_repeatable():
    """64 centers (sixteen per wave) in one graph of 600 atoms and 130 features"""
    cfg, sd, k, batch, noise, pins, com, fd = F.tall_case()
    tg = tall_types(cfg, batch)
    kw = dict(scale=G.GUIDE_SCALE, n_steps=1)
    r32 = TG.types_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, None, fd, tg, **kw)
    r64 = TG.types_reference(sd, cfg, batch, T, G.PREC, noise, *pins, com, None, fd, tg, double=True, **kw)
    assert float(r64.E_type[0][0]) > 0
    eng = bound(engine_for(cfg, sd), batch)
    first = one_step(eng, T, noise, pins, com, None, fd, tg)
    budget(first, r32, r64, "types tall")
    again = one_step(eng, T, noise, pins, com, None, fd, tg)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_feature_clip():
    """rows under the clip keep their shift bit for bit, the others end at norm feat_clip"""
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    eng = bound(engine_for(cfg, sd), batch)
    free = one_step(eng, T, noise, pins, com, restraints, fd, tg)
    norms = free[6].double().norm(dim=1)
    clip = float(norms.median())
    over = norms > clip
    assert 0 < int(over.sum()) < norms.numel()
    got = one_step(eng, T, noise, pins, com, restraints, fd, dict(TG.types_kwargs(tg), clip=clip))
    clip32 = float(torch.tensor(clip, dtype=torch.float32))
    assert torch.equal(got[6][~over], free[6][~over])
    assert float((got[6][over].double().norm(dim=1) - clip32).abs().max()) <= 1e-6 * max(1.0, clip32)
    assert torch.equal(got[5], free[5]) and torch.equal(got[4], free[4])      # the gradients are what they were


# 3. unchanged behaviour, bitwise
def test_inert_armings_are_the_run_without():
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    eng = bound(engine_for(cfg, sd), batch)
    want = run_types(eng, T, noise, pins, com, restraints, fd, None, trajectory=True, energies=True)
    # no type restraint, comp_types off, feat_scale 0: nothing launched that was not, a zero shift
    got = run_types(eng, T, noise, pins, com, restraints, fd, dict(restraints=None, scale=0.0, sharpness=TG.SHARP), trajectory=True,
                    energies=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert float(eng.last_type_guidance()[0].abs().max()) == 0 and float(eng.last_type_guidance()[2].abs().max()) == 0
    # all weights zero (the launches alone): the restraints weigh nothing, the complementarity has no type gradient to scale
    zero_w = [None if r is None else [(t, c, p, rr, 0.0) for t, c, p, rr, w in r] for r in tg.raw]
    got = run_types(eng, T, noise, pins, com, restraints, fd, dict(restraints=zero_w, scale=0.0, sharpness=TG.SHARP), trajectory=True,
                    energies=True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    g0_h, grad_h, shift_h, e_type = eng.last_type_guidance()
    assert float(g0_h.abs().max()) == 0 and float(shift_h.abs().max()) == 0 and float(e_type.abs().max()) == 0
    assert float(grad_h.abs().max()) > 0                # J_h of the coordinate energies: what feat_scale would have applied


def test_types_then_plain_on_one_handle():
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.case()
    eng = bound(engine_for(cfg, sd), batch)
    first = run_types(eng, T, noise, pins, com, restraints, fd, None, trajectory=True, energies=True)
    fam = [eng.kernel_family(i) for i in range(cfg.n_convs + 1)]
    with pytest.raises(pfa.PfError, match=ERR_STATE):   # the run before had no type guidance
        eng.last_type_guidance()
    mid = run_types(eng, T, noise, pins, com, restraints, fd, tg, trajectory=True, energies=True)
    assert not torch.equal(mid[1], first[1])
    again = run_types(eng, T, noise, pins, com, restraints, fd, None, trajectory=True, energies=True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert [eng.kernel_family(i) for i in range(cfg.n_convs + 1)] == fam
    # an unguided run behind it is the one in front of everything
    arr = arrays(eng, T)[0]
    p1 = eng.sample(arr, T, noise, init_pharm_com=com)
    run_types(eng, T, noise, pins, com, restraints, fd, tg)
    p2 = eng.sample(arr, T, noise, init_pharm_com=com)
    assert torch.equal(p1[0], p2[0]) and torch.equal(p1[1], p2[1])
    # the step API equals the whole loop bitwise
    arr, parr, garr = arrays(eng, T)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, guide_family="tuned",
                     field=F.field_kwargs(fd), types=TG.types_kwargs(tg))
    for i in range(T):
        eng.guided_step(arr[i], parr[i], garr[i], noise[1 + i])
    x1, h1 = eng.sample_end()
    eng.set_train_input_grads(False)
    assert torch.equal(x1, mid[0]) and torch.equal(h1, mid[1])
    assert eng.xchg_timeouts() == 0
    eng.sample_status()


# 4. arming, state and argument errors
def test_arming_state_and_argument_errors():
    cfg, sd, k, batch, noise, pins, com, restraints, fd, tg = TG.wide_case()
    eng = bound(engine_for(cfg, sd), batch)
    eng.set_train_family("wide")
    arr, parr, garr = arrays(eng, G.WIDE_T)
    kw = TG.types_kwargs(tg)
    fkw = F.field_kwargs(fd)
    # a plain run in progress stays usable through every refused arming and through an accepted one
    eng.sample_begin(noise[0], init_pharm_com=com)
    eng.denoise_step(arr[0], noise[1])
    before = [t.clone() for t in eng.sample_frame()]
    one = lambda **o: [[tuple(o.get(n, v) for n, v in zip(("t", "c", "p", "r", "w"), (2, 1, (0.0, 0.0, 0.0), 1.0, 1.0)))], None]
    for what, over in {"type": dict(restraints=one(t=cfg.pharm_nf)), "negative type": dict(restraints=one(t=-1)),
                       "center": dict(restraints=one(c=3)), "point": dict(restraints=one(p=(0.0, float("nan"), 0.0))),
                       "radius": dict(restraints=one(r=-1.0)), "weight": dict(restraints=one(w=float("inf"))),
                       "too many": dict(restraints=[[(0, None, (0.0, 0.0, 0.0), 0.0, 1.0)] * 257, None]),
                       "scale": dict(scale=-1.0), "clip": dict(clip=float("nan")), "sharpness": dict(sharpness=-0.5),
                       "unmatched": dict(unmatched=-1.0)}.items():
        with pytest.raises(pfa.PfError, match=ERR_ARG):
            eng.types_next(**dict(kw, **over))
    assert all(torch.equal(a, b) for a, b in zip(before, eng.sample_frame()))
    eng.denoise_step(arr[1], noise[2])                  # nothing was armed: the plain run goes on, and a plain begin is accepted
    eng.sample_begin(noise[0], init_pharm_com=com)
    # armed: the begin of another run kind is PF_ERR_STATE and drops the arming; the run in progress goes on
    eng.denoise_step(arr[0], noise[1])
    state = [t.clone() for t in eng.sample_frame()]
    eng.types_next(**kw)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*type guidance"):
        eng.sample_begin(noise[0], init_pharm_com=com)
    assert all(torch.equal(a, b) for a, b in zip(state, eng.sample_frame()))
    eng.denoise_step(arr[1], noise[2])
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)      # dropped: the pinned begin is accepted
    eng.types_next(**kw)
    with pytest.raises(pfa.PfError, match=r"\(-3\).*type guidance"):
        eng.sample(arr, 2, noise, init_pharm_com=com)
    # a bind drops the arming: the guided run behind it has no type guidance
    eng.types_next(**kw)
    bound(eng, batch)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_type_guidance()
    plain_g0 = eng.last_guidance()[0].clone()
    # a field armed with another sharpness: the begin is PF_ERR_ARG, consumes both, and the next begin runs without either
    eng.field_next(**dict(fkw, type_sharpness=2.0))
    eng.types_next(**kw)
    with pytest.raises(pfa.PfError, match=r"\(-1\).*must agree"):
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)
    eng.guided_step(arr[1], parr[1], garr[1], noise[2])            # the run in progress goes on
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    assert torch.equal(eng.last_guidance()[0], plain_g0)
    # it ends with its run; a refused arming inside the run leaves it usable, an accepted one is for the NEXT run
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE, types=kw)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    assert float(eng.last_type_guidance()[0].abs().max()) > 0
    with pytest.raises(pfa.PfError, match=ERR_ARG):
        eng.types_next(**dict(kw, scale=-2.0))
    eng.types_next(restraints=None, scale=0.0)
    eng.guided_step(arr[1], parr[1], garr[1], noise[2])
    assert float(eng.last_type_guidance()[0].abs().max()) > 0
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)     # consumes it
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    assert float(eng.last_type_guidance()[0].abs().max()) == 0
    assert torch.equal(eng.last_guidance()[0], plain_g0)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE)
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    with pytest.raises(pfa.PfError, match=ERR_STATE):
        eng.last_type_guidance()
    # comp_types without a field is accepted and inert
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=G.GUIDE_SCALE,
                     types=dict(restraints=None, scale=0.0, complementarity=True, unmatched=1.0))
    eng.guided_step(arr[0], parr[0], garr[0], noise[1])
    assert float(eng.last_type_guidance()[3].abs().max()) == 0 and torch.equal(eng.last_guidance()[0], plain_g0)
    # the Python layer
    with pytest.raises(ValueError, match="multistep"):
        eng.sample(None, 2, noise, ms_coef_arr=[None, None], types=kw)
    with pytest.raises(ValueError, match="one entry per graph"):
        eng.types_next(restraints=[None])
    assert eng.xchg_timeouts() == 0


# 5. model level
def test_model_level_type_restraints():
    """PharmacophoreDiff.sample(type_restraints=..., type_guidance=...) on two pockets with injected noise: a batch with a type
    restraint runs guided, the other runs the default path, and each is the engine-level run on the same batch bit for bit"""
    from test_gpu_api import graph_from, make_model
    n_t = 12
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[3, 5, 4], [4, 3, 6]]
    c0 = pockets[0].prot_x.mean(dim=0).float()
    name = m.ph_type_map[2]
    tr = [[(name, None, c0.tolist(), 500.0, 1.0), (4, 1, (0.0, 0.0, 0.0), 0.0, 2.0)], None]
    gen = torch.Generator().manual_seed(11)
    nz = [torch.randn(n_t + 1, 12, 9, generator=gen), torch.randn(n_t + 1, 13, 9, generator=gen)]
    kw = dict(max_batch_size=3, lanes=2, noise=nz)
    tgd = pfa.TypeGuidance(scale=2.0, clip=1.5, sharpness=4.0)
    out = m.sample(pockets, n_pharms, type_restraints=tr, type_guidance=tgd, guide_family="tuned", **kw)
    plain = m.sample(pockets, n_pharms, **kw)
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    assert any(not torch.equal(a.g.pharm_h0, b.g.pharm_h0) for a, b in zip(out[0], plain[0]))
    for a, b in zip(out[1], plain[1]):                  # the pocket without a type restraint: the default path's bits
        assert torch.equal(a.ph_coords, b.ph_coords) and torch.equal(a.g.pharm_h0, b.g.pharm_h0)
    with pytest.raises(ValueError, match="resampling"):
        m.sample(pockets, n_pharms, type_restraints=tr, pinned=[(c0[None], torch.tensor([2]), None), None], pin_resamples=2, **kw)
    with pytest.raises(ValueError, match="multistep"):
        m.sample(pockets, n_pharms, type_restraints=tr, sample_steps=4, sampler="multistep", **kw)
    with pytest.raises(ValueError, match="comp_weight > 0"):
        m.sample(pockets, n_pharms, type_restraints=tr, type_guidance=pfa.TypeGuidance(complementarity=True), **kw)
    # the engine-level run on pocket 0's batch, on the handle the model's lane 0 uses
    gamma = m.gamma.gamma
    order = list(reversed(range(n_t)))
    batch_g = pfa.batch(pfa.copy_graph(pockets[0], n_copies=3, pharm_feats_per_copy=torch.tensor(n_pharms[0])))
    eng = m.dynamics.bind_graph(batch_g)
    arr = eng.coef_array(m.step_coefficients(), order)
    parr = eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order)
    garr = eng.guide_coef_array(pfa.schedule.guide_coefficients(gamma, n_t), order)
    com = pockets[0].prot_x.mean(dim=0).float().repeat(3, 1)
    rows = [(2, None, c0.tolist(), 500.0, 1.0), (4, 1, (0.0, 0.0, 0.0), 0.0, 2.0)]
    x0, h0 = eng.sample(arr, n_t, nz[0], init_pharm_com=com, ep_coord=m.endpoint_param_coord, ep_feat=m.endpoint_param_feat,
                        feat_norm_constant=float(m.pharm_feat_norm_constant), pin_coef_arr=parr, guide_coef_arr=garr,
                        guide_family="tuned",
                        types=dict(restraints=[rows] * 3, scale=2.0, clip=1.5, sharpness=4.0 * float(m.pharm_feat_norm_constant)))
    eng.sample_status()
    x0, h0 = x0.cpu(), h0.cpu()
    ptr = batch_g.pharm_ptr.tolist()
    for i, p in enumerate(out[0]):
        assert torch.equal(p.ph_coords, x0[ptr[i]:ptr[i + 1]]) and torch.equal(p.g.pharm_h0, h0[ptr[i]:ptr[i + 1]])


# 6. the command line
def test_cli_with_type_restraints(tmp_path):
    """generate_pharmacophores.py --type_restraints writes the pharms.xyz the reference composition predicts (the pattern of
    test_gpu_pocket_field.test_cli_with_avoid_clashes: same files, same seed, same draws), and the type_energy column of
    scores.tsv.  The seeded random weights of this fixture throw the centers hundreds of angstroms from the pocket, so the window
    is chosen to reach them (a radius of 500): the test is about the path from the flags to the kernels, not about chemistry."""
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
    e = O.radius_graph(pos, 3.5, torch.tensor([0, pos.shape[0]]), 100)
    pk = P.process_ligand_and_pocket(tmp_path / "rec.pdb", None, emap, cfg['graph']['graph_cutoffs'], 8.0, lig_file=tmp_path / "lig.sdf",
                                     pp_edges=(e[0], e[1]))
    c = pk.prot_x.mean(dim=0).tolist()
    name = m.ph_type_map[2]
    (tmp_path / "types.txt").write_text(f"# a window that reaches the centers, and one center's type outright\n"
                                        f"type {name} {c[0]:.4f} {c[1]:.4f} {c[2]:.4f} 500 1.0\ntype 4 0 0 0 0 2.0 1\n")
    rows = [(2, None, tuple(float(f"{v:.4f}") for v in c), 500.0, 1.0), (4, 1, (0.0, 0.0, 0.0), 0.0, 2.0)]
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
           str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "3", "--pharm_sizes", "3", "4", "5",
           "--max_batch_size", "3", "--output_dir", str(out), "--seed", "1", "--type_restraints", str(tmp_path / "types.txt"),
           "--guide_type_scale", "2.0", "--guide_type_clip", "1.5", "--guide_family", "tuned", "--score_samples", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "type energy per sample" in r.stdout
    xyz = (out / "rec" / "pharms.xyz").read_text().splitlines()
    pocket1 = O.PocketBatch(pk.prot_x, pk.prot_h, torch.tensor([0, pk.prot_x.shape[0]]), torch.tensor([0, 1]), pk.pp_src.long(), pk.pp_dst.long())
    torch.manual_seed(1)
    nz = torch.randn(n_t + 1, 12, 9, device="cuda").cpu()
    b = O.concat_pockets([O.copy_pocket(pocket1, n) for n in (3, 4, 5)])
    fnorm = float(m.pharm_feat_norm_constant)
    tg = TG.make_types([rows] * 3, scale=2.0, clip=1.5, sharpness=4.0 * fnorm)
    free = (torch.zeros(12, dtype=torch.int32), torch.zeros(12, 3), torch.zeros(12, 6))
    com = O.segment_mean(b.prot_x, b.prot_ptr)
    prec = float(cfg['diffusion'].get('precision', 1e-5))
    ref = TG.types_reference(sd, O.DynamicsConfig(), b, n_t, prec, nz, *free, com, None, None, tg, fnorm=fnorm)
    un = TG.types_reference(sd, O.DynamicsConfig(), b, n_t, prec, nz, *free, com, None, None, None, fnorm=fnorm)
    assert float((ref.h0 - un.h0).abs().max()) > 0.1     # the type guidance moved the feature rows
    lines = [l.split() for l in xyz if len(l.split()) == 4]
    assert len(lines) == 12
    scale = max(abs(float(v)) for l in lines for v in l[1:])
    for l, xw, kw in zip(lines, ref.x0.tolist(), ref.h0.argmax(1).tolist()):
        assert l[0] == "PSFNOC"[kw], (l, kw)
        assert all(abs(float(u) - v) <= 5e-3 * max(1.0, scale) for u, v in zip(l[1:], xw)), (l, xw)
    tsv = [l.split("\t") for l in (out / "rec" / "scores.tsv").read_text().splitlines()]
    assert tsv[0][-1] == "type_energy" and len(tsv) == 4
    ptr = b.pharm_ptr.tolist()
    for i, row in enumerate(tsv[1:]):
        e_ref = pfa.analysis.type_restraint_energy(ref.x0[ptr[i]:ptr[i + 1]], ref.h0[ptr[i]:ptr[i + 1]], rows, 4.0)
        assert abs(float(row[-1]) - e_ref) <= 5e-2 * max(1.0, e_ref), (row, e_ref)
