"""Feature counts other than pharm_nf = 6 / rec_nf = 11 in every kernel family.

pf_create accepts pharm_nf in 1..16 and any rec_nf >= 1; the rest of the suite runs 6 / 11 with element types 0..3 only.  The
inputs here (tests/nf_cases.py) put a type on every column, and tests/test_oracle_feature_counts.py proves on the CPU oracle
that a kernel which ignores any one encoder column, or reads the wrong type-table row, misses the bounds used here by a factor
of ten or more.  (pharm_nf, rec_nf) and why:

    (1, 1)      the minimum counts
    (7, 5)      nf + 1 = 8 fills the batch of eight of n16_encode_pharm; rec_nf odd (nke = (rec_nf + 2) / 2)
    (8, 16)     the limits of training and of pf_score; a second batch of eight with one live entry; K = 17 fills the LDS row of
                the wide training encoder; the last rec_nf on the per-(graph, element) sums of the encoder's backward
    (15, 17)    the last pharm_nf with the n16 tail packing
    (16, 40)    SB_MAXNF; no n16 tail packing; the exchange row holds 19 of 20 words
    (6, 127) / (6, 130)   the static hoist's gate rec_nf < 128 on and off (pf_k = 16)
    (7, 33)     radius pf edges (pf_k = 0): an atom is the source of many pf edges, the type tables serve them without the fused launch
    (9, 11)     the first pharm_nf beyond the eight features a move keeps in registers (pf_stepmove.h; the pinned move: six)

Tolerances are the suite's own: a dynamics call 2e-4 + 2e-4 |ref| plus the fp64 budget of helpers.check_live, edge sets exact,
sampler states 2e-4 (i + 1) after step i, whole runs 5e-3, gradients per 16 x 16 block inside grad_budget's fp64 budget, the
bf16 leg test_gpu_train.py's contract, the fused loss test_gpu_endpoint_loss.py's."""
import functools

import pytest
import torch

import fewstep_ref as F
import grad_budget as G
import resample_ref as RR
import score_ref as SC
import seeded_ref as SR
from oracle import pf_oracle as O
from helpers import check_live, edge_set, sampler_live_head, within_budget
from nf_cases import nf_case, score_case, score_reference
from test_gpu_norm_floor import FORWARD_LEGS, STEP_FORMS, _expect, _fam
from test_gpu_parity import ATOL, RTOL, close
from test_gpu_train import _cos_rel, flat_to_dict
from test_gpu_wide import engine_for, set_batch
from test_gpu_wide_train import masks_from_engine

pytestmark = pytest.mark.gpu

COUNTS = [(1, 1), (7, 5), (8, 16), (15, 17), (16, 40), (6, 127), (6, 130), (7, 33)]
EVERY_LEG = [(7, 5), (16, 40)]
SOME_LEGS = ["default", "no_l0_hoist", "one_wave_per_tile", "row_groups_4", "n16_mask7_compact", "wide"]


# ---- a. one dynamics call -------------------------------------------------------------------------------------------------------
def hoist_possible(c):
    """the static hoist of conv layer 0 needs one-hot protein rows and rec_nf < 128 (pf_host.cpp: l0_hoist_ok)"""
    return c.features == "onehot" and c.cfg.rec_nf < 128


def _n16_without_tables(eng, cfg):
    """PFDYN_N16=7 where conv layer 0 has no type tables: it stays on the row-group kernels, nothing is fused, the last layer
    runs the n16 kernels"""
    fam = _fam(eng, cfg)
    assert fam == [4, 16] and eng.l0_hoist() == 0, (fam, eng.l0_hoist())


# what the legs name where the hoist's gate is off (one-hot rows at rec_nf >= 128, dense rows): no tables, so neither the hoisted
# items nor conv layer 0 on the n16 kernels nor the fused launch
WITHOUT_TABLES = {
    "default": _expect(families={4, 8, 16, 17}, hoist=False),
    "no_l0_hoist": _expect(families={4, 8, 16, 17}, hoist=False),
    "one_wave_per_tile": FORWARD_LEGS["one_wave_per_tile"][1],
    "row_groups_4": _expect(families={4}, hoist=False),
    "n16_mask7_compact": _n16_without_tables,
    "wide": FORWARD_LEGS["wide"][1],
}


def dynamics_leg(c, env, expect, what, monkeypatch):
    """test_gpu_norm_floor._dynamics_leg with the three dynamic edge sets asserted in every case"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_for(c.cfg, c.live.sd)
    set_batch(eng, c.batch)
    eps_h, eps_x = eng.dynamics(c.x_t, c.h_t, c.t)
    print(f"feature counts {what}: kernel families {_fam(eng, c.cfg)}, l0 hoist {eng.l0_hoist()}")
    expect(eng, c.cfg)
    edges = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)
    for i, et in enumerate(("ff", "pf", "fp")):
        s, d = eng.get_edges(i)
        assert edge_set(s, d) == edge_set(*edges[et]) and s.numel() == edges[et][0].numel(), et
    assert eps_h.shape == (c.x_t.shape[0], c.cfg.pharm_nf)
    assert bool(torch.isfinite(eps_h).all()) and bool(torch.isfinite(eps_x).all())
    check_live(eps_h, eps_x, c.live, f"feature counts {what}", RTOL, ATOL)
    return eng


DYNAMICS = [(nf, rf, "onehot", leg) for nf, rf in COUNTS for leg in (list(FORWARD_LEGS) if (nf, rf) in EVERY_LEG else SOME_LEGS)]
DYNAMICS.append((8, 16, "dense", "default"))


@pytest.mark.parametrize("pharm_nf,rec_nf,features,leg", DYNAMICS, ids=[f"{a}-{b}-{f}-{leg}" for a, b, f, leg in DYNAMICS])
def test_dynamics_call(pharm_nf, rec_nf, features, leg, monkeypatch):
    """One dynamics call (live head) under the default policy and under the forward families the suite forces -- every leg of
    test_gpu_norm_floor.FORWARD_LEGS at (7, 5) and (16, 40), six of them elsewhere, dense protein rows at (8, 16) --: the family
    the leg names, the three dynamic edge sets exactly, against the fp32 oracle and inside the fp64 budget."""
    c = nf_case(pharm_nf, rec_nf, features=features)
    env, expect = FORWARD_LEGS[leg]
    if not hoist_possible(c):
        expect = WITHOUT_TABLES[leg]
    eng = dynamics_leg(c, env, expect, f"({pharm_nf}, {rec_nf}) {features} {leg}", monkeypatch)
    if leg == "default":
        # the gate of the static hoist: on up to rec_nf = 127, off from 128 (and for rows that are no one-hots)
        assert (eng.l0_hoist() > 0) == hoist_possible(c), eng.l0_hoist()


@pytest.mark.parametrize("pharm_nf,rec_nf", [(1, 1), (16, 40)])
def test_dynamics_call_wide_model_64_32(pharm_nf, rec_nf, monkeypatch):
    """A 64 / 32 model: the width-generic family at its own widths"""
    c = nf_case(pharm_nf, rec_nf, n_hidden_scalars=64, vector_size=32)
    dynamics_leg(c, {}, _expect(families={64}), f"({pharm_nf}, {rec_nf}) wide 64/32", monkeypatch)


# ---- b. sampler steps -----------------------------------------------------------------------------------------------------------
T_STEPS, N_STEPS = 50, 4


@functools.lru_cache(maxsize=None)
def step_case(pharm_nf, rec_nf, n_prot=None, n_pharm=None, n_steps=N_STEPS):
    """nf_case's batch and weights with a live head for a sampling run (k from the run's first dynamics call), the noise
    [n_steps + 1, Nf, 3 + pharm_nf] and the oracle's frames"""
    c = nf_case(pharm_nf, rec_nf, n_prot, n_pharm)
    Nf = int(c.batch.pharm_ptr[-1])
    noise = torch.randn(n_steps + 1, Nf, 3 + pharm_nf, generator=torch.Generator().manual_seed(17))
    sd, _ = sampler_live_head(c.sd, c.cfg, c.batch, T_STEPS, 1e-5, noise)
    x0, h0, frames = O.sample_given_receptor(sd, c.cfg, c.batch, T_STEPS, 1e-5, noise, return_traj=True, n_steps=n_steps)
    return c, sd, noise, (x0, h0), frames


def step_form_families(form, pharm_nf):
    """(kernel_family(n_convs), kernel_family(n_convs - 1)) a step form ends on.  The n16 form of the tail launch carries
    to_scalar_output in gate rows 1 .. pharm_nf of a 16-row block and is packed for pharm_nf <= 15 only (pf_pack.cpp); at 16 the
    host finds no such stream and the tail launch takes its row-group form, whose head stores pharm_nf <= 16 columns
    (node_launch: tail_form == 16 && pk.n16_tail != 0 ? 16 : 4)."""
    fam_end, fam_last = STEP_FORMS[form][3:]
    if pharm_nf == 16 and form == "tail_n16":
        fam_end = 4
    return fam_end, fam_last


@pytest.mark.parametrize("form", list(STEP_FORMS))
@pytest.mark.parametrize("pharm_nf,rec_nf", [(7, 5), (15, 17), (16, 40)])
def test_sampler_steps_every_step_form(pharm_nf, rec_nf, form, monkeypatch):
    """Four denoising steps at T = 50 through every form of a step's end, the state after every step against
    O.sample_given_receptor's frames at 2e-4 (i + 1)."""
    c, sd, noise, _, frames = step_case(pharm_nf, rec_nf)
    mask, tform, hsb = STEP_FORMS[form][:3]
    fam_end, fam_last = step_form_families(form, pharm_nf)
    monkeypatch.setenv("PFDYN_N16", mask)
    monkeypatch.setenv("PFDYN_TAIL_FORM", tform)
    monkeypatch.setenv("PFDYN_HS_BUILD", hsb)
    eng = engine_for(c.cfg, sd)
    set_batch(eng, c.batch)
    coef = O.step_coefficients(O.gamma_table(T_STEPS, 1e-5), T_STEPS)
    arr = eng.coef_array(coef, reversed(range(T_STEPS)))
    eng.sample_begin(noise[0])
    for i in range(N_STEPS):
        eng.denoise_step(arr[i], noise[i + 1])
        fams = _fam(eng, c.cfg) + [eng.kernel_family(c.cfg.n_convs)]
        print(f"feature counts sampler ({pharm_nf}, {rec_nf}) {form} step {i}: kernel families {fams}")
        assert fams[-1] == fam_end and (fam_last is None or fams[-2] == fam_last), fams
        x, h = eng.sample_frame()
        assert h.shape[1] == pharm_nf
        tol = 2e-4 * (i + 1)
        close(x, frames[i + 1][0], tol, tol); close(h, frames[i + 1][1], tol, tol)
    assert eng.xchg_timeouts() == 0


@pytest.mark.parametrize("hoist", [True, False])
@pytest.mark.parametrize("pharm_nf,rec_nf", [(7, 5), (16, 40)])
def test_sampler_run_center_hoist(pharm_nf, rec_nf, hoist, monkeypatch):
    """The same four steps as one pf_sample run, which announces its timesteps: the merged launch leaves the center-hoist tables
    (pf_cenhoist.h: 16 encoder columns in registers, read at clamped indices beyond pharm_nf) and the next call's ff / fp items
    start from them; PFDYN_NO_CENTER_HOIST=1: they encode on the fly.  As test_sampler_run_center_hoist_on_floor_weights."""
    c, sd, noise, _, frames = step_case(pharm_nf, rec_nf)
    if not hoist:
        monkeypatch.setenv("PFDYN_NO_CENTER_HOIST", "1")
    eng = engine_for(c.cfg, sd)
    set_batch(eng, c.batch)
    coef = O.step_coefficients(O.gamma_table(T_STEPS, 1e-5), T_STEPS)
    x0, h0, tx, th = eng.sample(eng.coef_array(coef, reversed(range(T_STEPS))), N_STEPS, noise, trajectory=True)
    torch.cuda.synchronize()
    eng.sample_status()
    print(f"feature counts sampler run ({pharm_nf}, {rec_nf}): kernel families {_fam(eng, c.cfg)}, step end "
          f"{eng.kernel_family(c.cfg.n_convs)}, center hoist {eng.kernel_family(c.cfg.n_convs + 1)}")
    assert eng.kernel_family(0) == 16 and eng.kernel_family(c.cfg.n_convs + 1) == (1 if hoist else 0)
    assert eng.xchg_timeouts() == 0
    for i in range(N_STEPS + 1):
        tol = 2e-4 * max(i, 1)
        close(tx[i], frames[i][0], tol, tol); close(th[i], frames[i][1], tol, tol)


def test_merged_launch_with_640_feature_words(monkeypatch):
    """(16, 40) with a graph of 40 centers: 640 feature words for the 192 feature lanes of the merged launch's update, so every
    lane reloads words on demand (pf_stepbuild.h: j != fj).  Five steps through pf_sample on the merged launch and with the
    generic update + build bodies (PFDYN_NO_FAST_BUILD=1, separate launches): bit for bit, and against the oracle as
    test_fused_update_and_edge_build_variants_agree."""
    monkeypatch.setenv("PFDYN_NO_CENTER_HOIST", "1")       # (only the merged launch leaves the center-hoist tables: its own test compares them)
    c, sd, noise, (ox, oh), _ = step_case(16, 40, (150, 64), (40, 5), 5)
    assert int(c.batch.pharm_ptr[1]) * c.cfg.pharm_nf == 640
    mask, tform, hsb = STEP_FORMS["merged"][:3]
    for k, v in (("PFDYN_N16", mask), ("PFDYN_TAIL_FORM", tform), ("PFDYN_HS_BUILD", hsb)):
        monkeypatch.setenv(k, v)
    res = []
    for generic in (False, True):
        if generic:
            monkeypatch.setenv("PFDYN_NO_FAST_BUILD", "1")
        eng = engine_for(c.cfg, sd)
        monkeypatch.delenv("PFDYN_NO_FAST_BUILD", raising=False)
        set_batch(eng, c.batch)
        coef = O.step_coefficients(O.gamma_table(T_STEPS, 1e-5), T_STEPS)
        x0, h0 = eng.sample(eng.coef_array(coef, reversed(range(T_STEPS))), 5, noise)
        eng.sample_status()
        print(f"feature counts merged launch, generic bodies {generic}: step end {eng.kernel_family(c.cfg.n_convs)}")
        assert eng.kernel_family(c.cfg.n_convs) == (0 if generic else 2) and eng.xchg_timeouts() == 0
        res.append((x0.cpu(), h0.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    close(res[0][0], ox, 5e-3, 5e-3); close(res[0][1], oh, 5e-3, 5e-3)


# ---- c. pinned with a renoise jump, seeded, multistep ---------------------------------------------------------------------------
KIND_COUNTS = [(9, 11), (16, 40)]
RUN_T, RUN_PREC = RR.T, RR.PREC
PINNED_PLAN = [("denoise", 23), ("denoise", 22), ("renoise", 22, 24), ("denoise", 23)]
SEED_LEVEL = 4
MS_LEVELS = F.uniform_plan(RUN_T, 4)


@functools.lru_cache(maxsize=None)
def kind_case(pharm_nf, rec_nf):
    """nf_case's batch for the other run kinds, drawn as resample_ref.case draws: noise rows [5, Nf, 3 + pharm_nf], pins
    (test_gpu_pinned.pins_for: the first center of every graph given in full, the second its position, the third its row),
    init_pharm_com = pocket mean + 0.5, the live head of the run's first dynamics call"""
    from test_gpu_pinned import pins_for
    c = nf_case(pharm_nf, rec_nf)
    Nf = int(c.batch.pharm_ptr[-1])
    noise = torch.randn(5, Nf, 3 + pharm_nf, generator=torch.Generator().manual_seed(RR.NOISE_SEED))
    flags = []
    for n in (c.batch.pharm_ptr[1:] - c.batch.pharm_ptr[:-1]).tolist():
        flags += ([3, 1, 2] + [0] * n)[:n]
    pins = pins_for(c.batch, c.cfg, flags)
    com = O.segment_mean(c.batch.prot_x, c.batch.prot_ptr) + 0.5
    sd, _ = sampler_live_head(c.sd, c.cfg, c.batch, RUN_T, RUN_PREC, noise)
    return c, sd, noise, pins, com


def run_kind(kind, eng, c, noise, pins, com):
    import pharmacoforge_amd as pfa
    S = pfa.schedule
    gamma = O.gamma_table(RUN_T, RUN_PREC)
    if kind == "pinned_renoise":
        pairs = [(op[1], op[2]) for op in PINNED_PLAN if op[0] == "renoise"]
        arr, parr, op_arr, re_arr = eng.plan_arrays(PINNED_PLAN, O.step_coefficients(gamma, RUN_T), S.pin_coefficients(gamma, RUN_T),
                                                    S.renoise_coefficients(gamma, RUN_T, pairs))
        return eng.sample(arr, len(PINNED_PLAN), noise, init_pharm_com=com, trajectory=True, pins=pins, pin_coef_arr=parr,
                          plan=(op_arr, re_arr))
    if kind == "seeded":
        a = SEED_LEVEL
        arr = eng.coef_array(O.step_coefficients(gamma, RUN_T), list(reversed(range(a))))
        return eng.sample(arr, a, noise[:a + 1], init_pharm_com=com, trajectory=True,
                          seed=(pins[1], pins[2], S.seed_coefficients(gamma, RUN_T, a)))
    arr = eng.ms_coef_array(S.multistep_coefficients(gamma, RUN_T, MS_LEVELS, False, False))
    return eng.sample(None, len(MS_LEVELS) - 1, noise[:1], init_pharm_com=com, trajectory=True, ms_coef_arr=arr)


@functools.lru_cache(maxsize=None)
def kind_reference(kind, pharm_nf, rec_nf):
    c, sd, noise, pins, com = kind_case(pharm_nf, rec_nf)
    if kind == "pinned_renoise":
        return RR.resampled_reference(sd, c.cfg, c.batch, RUN_T, RUN_PREC, PINNED_PLAN, noise, *pins, com)
    if kind == "seeded":
        a = SEED_LEVEL
        return SR.seeded_reference(sd, c.cfg, c.batch, RUN_T, RUN_PREC, a, SR.steps_of(a), noise[:a + 1], (pins[1], pins[2]), None, com)
    return F.fewstep_reference(sd, c.cfg, c.batch, RUN_T, RUN_PREC, F.ms_ops(MS_LEVELS), noise, com)


@pytest.mark.parametrize("kind", ["pinned_renoise", "seeded", "multistep"])
@pytest.mark.parametrize("pharm_nf,rec_nf", KIND_COUNTS)
def test_other_step_kinds(pharm_nf, rec_nf, kind, monkeypatch):
    """A pinned run with one resampling jump (D(23) D(22) R(22 -> 24) D(23)), a seeded run from level 4 and a second-order
    multistep run over 24, 18, 12, 6, 0 at T = 24, precision 0.25: x_0, h_0 and every frame against the CPU compositions of
    resample_ref / seeded_ref / fewstep_ref at rtol = atol = 5e-3 (test_gpu_resample.check_run, test_gpu_seeded.check); and the
    same run on the generic update + build bodies (PFDYN_NO_FAST_BUILD=1) bit for bit.  pharm_nf 9 and 16: the moves
    keep eight features (pinned: six) in registers and loop over the rest."""
    from test_gpu_seeded import check
    # (the plain steps of a seeded run end on the merged launch, which leaves the center-hoist tables; they equal the on-the-fly
    # encoding up to summation order, not bit for bit: test_sampler_run_center_hoist compares them)
    monkeypatch.setenv("PFDYN_NO_CENTER_HOIST", "1")
    c, sd, noise, pins, com = kind_case(pharm_nf, rec_nf)
    ref = kind_reference(kind, pharm_nf, rec_nf)
    res = []
    for generic in (False, True):
        if generic:
            monkeypatch.setenv("PFDYN_NO_FAST_BUILD", "1")
        eng = engine_for(c.cfg, sd)
        monkeypatch.delenv("PFDYN_NO_FAST_BUILD", raising=False)
        set_batch(eng, c.batch)
        got = run_kind(kind, eng, c, noise, pins, com)
        eng.sample_status()
        assert eng.xchg_timeouts() == 0
        res.append(check(got, ref, f"feature counts ({pharm_nf}, {rec_nf}) {kind}, generic bodies {generic}"))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    if kind == "pinned_renoise":
        flags, pin_x, pin_h = pins
        mx, mh = (flags & 1) != 0, (flags & 2) != 0
        assert int(mx.sum()) >= 2 and int(mh.sum()) >= 2
        assert torch.equal(res[0][0][mx], pin_x[mx]) and torch.equal(res[0][1][mh], pin_h[mh])


# ---- d. score -------------------------------------------------------------------------------------------------------------------
W_POS, W_FEAT = [0.5, 0.25, 2.0], [1.0, 0.125, 0.75]


@pytest.mark.parametrize("pharm_nf,rec_nf", [(8, 16), (1, 1)])
def test_score_terms_match_the_composition(pharm_nf, rec_nf):
    """pf_score at its limit of eight feature columns and at one (a softmax over one class), all four parameterisations, as
    test_gpu_score.test_terms_and_score_match_the_composition: pos, feat, err and the weighted score inside the fp64 budget,
    hits exactly.  With one class the cross-entropy is log(exp(0)) = 0 for every center in any arithmetic: asserted as zero."""
    s = score_case(pharm_nf, rec_nf)
    eng = engine_for(s.cfg, s.sd)
    set_batch(eng, s.batch)
    _, al, sg = SC.tables()
    ref32, ref64 = score_reference(pharm_nf, rec_nf, False), score_reference(pharm_nf, rec_nf, True)
    for ep_coord, ep_feat in SC.PARAMS:
        score, terms = eng.score(s.x0, s.h0, SC.LEVELS, s.noise, W_POS, W_FEAT, al, sg, SC.T, ep_coord=ep_coord, ep_feat=ep_feat)
        t32, t64 = ref32[(ep_coord, ep_feat)][0], ref64[(ep_coord, ep_feat)][0]
        s32, s64 = SC.score_of(t32, W_POS, W_FEAT), SC.score_of(t64, W_POS, W_FEAT)
        what = f"feature counts score ({pharm_nf}, {rec_nf}) ep=({int(ep_coord)},{int(ep_feat)})"
        for q, name in enumerate(("pos", "feat", "err")):
            if float(t64[:, :, q].abs().max()) == 0.0:
                assert pharm_nf == 1 and ep_feat and name == "feat"
                assert float(terms[:, :, q].abs().max()) == 0.0 and float(score[:, 1].abs().max()) == 0.0
                continue
            within_budget(terms[:, :, q], t32[:, :, q], t64[:, :, q], f"{what} {name}")
        assert torch.equal(terms[:, :, 3].cpu().double(), t64[:, :, 3]), (what, terms[:, :, 3].cpu(), t64[:, :, 3])
        for q, name in enumerate(("score pos", "score feat")):
            if float(s64[:, q].abs().max()) > 0.0:
                within_budget(score[:, q], s32[:, q], s64[:, q], f"{what} {name}")


def test_score_is_refused_above_eight_columns():
    import pharmacoforge_amd as pfa
    c = nf_case(9, 11)
    eng = engine_for(c.cfg, c.sd)
    set_batch(eng, c.batch)
    _, al, sg = SC.tables()
    Nf = int(c.batch.pharm_ptr[-1])
    with pytest.raises(pfa.PfError, match="at most 8 feature columns"):
        eng.score(torch.zeros(Nf, 3), torch.zeros(Nf, 9), SC.LEVELS, torch.zeros(3, Nf, 12), W_POS, W_FEAT, al, sg, SC.T)


# ---- e. training ----------------------------------------------------------------------------------------------------------------
P_DROP, DROP_SEED = 0.1, 1234
GRAD_LEGS = {      # name -> (pharm_nf, rec_nf, features, training family, (S, V))
    "tuned_8_16_onehot": (8, 16, "onehot", "tuned", (128, 16)),
    "tuned_8_16_dense": (8, 16, "dense", "tuned", (128, 16)),
    "tuned_7_5": (7, 5, "onehot", "tuned", (128, 16)),
    "tuned_1_1": (1, 1, "onehot", "tuned", (128, 16)),
    "wide_8_16_128_16": (8, 16, "onehot", "wide", (128, 16)),
    "wide_8_16_64_32": (8, 16, "onehot", "wide", (64, 32)),
}
_GRAD_REFS = {}


@functools.lru_cache(maxsize=None)
def grad_case(pharm_nf, rec_nf, features, S, V):
    """nf_case's inputs as a grad_budget case: live head (k from the eval-mode forward), random upstream weights"""
    c = nf_case(pharm_nf, rec_nf, features=features, n_hidden_scalars=S, vector_size=V)
    return G.make_case(c.cfg, c.batch, c.prot_x, c.x_t, c.h_t, c.t, c.sd, 21, live=True)


def train_engine(c, family):
    eng = engine_for(c.cfg, c.sd)
    if family == "wide":
        eng.set_train_family("wide")
    set_batch(eng, c.batch)
    return eng


@pytest.mark.parametrize("leg", list(GRAD_LEGS))
def test_gradients_within_the_fp64_budget(leg):
    """One training forward (dropout 0.1) and two backwards as test_gpu_grad_budget.py: eps_h and eps_x under the engine's masks
    inside helpers.within_budget, every 16 x 16 block of every parameter gradient inside grad_budget.gradients_within_budget
    (the encoders' first Linears are [S, rec_nf + 1] and [S, pharm_nf + 1]: their last, ragged column blocks are blocks of their
    own), the second backward bit for bit.  (8, 16) with one-hot rows: all 16 types in every graph, the per-(graph, element)
    sums of the encoder's backward; with dense rows: every atom on its own."""
    pharm_nf, rec_nf, features, family, (S, V) = GRAD_LEGS[leg]
    c = grad_case(pharm_nf, rec_nf, features, S, V)
    what = f"feature counts gradients {leg}"
    eng = train_engine(c, family)
    Np, Nf = int(c.batch.prot_ptr[-1]), int(c.batch.pharm_ptr[-1])
    eps_h, eps_x = eng.train_forward(c.x_t, c.h_t, c.t, prot_x=c.prot_x, dropout=P_DROP, seed=DROP_SEED)
    print(f"{what}: training family {eng.train_family()}, kernel families {_fam(eng, c.cfg)}")
    assert eng.train_family() == family
    drop = masks_from_engine(eng, c.cfg, P_DROP, DROP_SEED, Np, Nf)
    key = (pharm_nf, rec_nf, features, S)
    if key not in _GRAD_REFS:
        _GRAD_REFS[key] = (drop,) + G.reference_draws(c, drop)
    for a, b in zip(_GRAD_REFS[key][0], drop):
        for nt in a:
            assert all(torch.equal(p, q) for p, q in zip(a[nt], b[nt])), "the legs of a case must draw the same dropout masks"
    draws, g64, (oh, ox), (h64, x64) = _GRAD_REFS[key][1:]
    assert float(ox.abs().max()) >= 0.25                         # the live head: eps_x counts
    for k in ("dynamics.prot_encoder.0.weight", "dynamics.pharm_encoder.0.weight"):
        assert bool((g64[k].abs().amax(dim=0) > 0).all()), k     # every encoder column has a gradient to get right
    got = flat_to_dict(eng, eng.train_backward(c.w_h, c.w_x))
    again = flat_to_dict(eng, eng.train_backward(c.w_h, c.w_x))
    res = G.gradients_within_budget(got, draws, g64, what, check=False)
    within_budget(eps_h.cpu(), oh, h64, what + " eps_h")
    within_budget(eps_x.cpu(), ox, x64, what + " eps_x")
    assert not res.bad, (f"{what}: {len(res.bad)} blocks outside 8 units of the fp64 gradient (ratio, err, unit, block)", res.bad[:8])
    for k in got:
        assert torch.equal(again[k], got[k]), k


def test_bf16_leg_gradients_against_the_fp32_path_at_8_16():
    """test_gpu_train.test_bf16_leg_gradients_against_the_fp32_path's contract at (8, 16): every tensor's gradient cosine >=
    0.999 and relative L2 error <= 2e-2 against the fp32 path, the whole vector cosine >= 0.9999, outputs within 5e-3, fp32
    again bit for bit"""
    c = grad_case(8, 16, "onehot", 128, 16)
    eng = train_engine(c, "tuned")
    res = {}
    for mode in ("f32", "bf16", "f32 again"):
        eng.set_train_precision(mode.split()[0])
        assert eng.train_precision() == mode.split()[0]
        eh, ex = eng.train_forward(c.x_t, c.h_t, c.t, prot_x=c.prot_x, dropout=0.1, seed=77)
        res[mode] = (eh.cpu(), ex.cpu(), eng.train_backward(c.w_h, c.w_x).cpu())
    assert torch.equal(res["f32"][2], res["f32 again"][2])
    assert not torch.equal(res["f32"][2], res["bf16"][2])            # the bf16 kernels really ran
    for q in (0, 1):
        assert float((res["bf16"][q] - res["f32"][q]).norm() / res["f32"][q].norm()) <= 5e-3
    g32, g16 = res["f32"][2], res["bf16"][2]
    live = 0
    for k, off, n in eng.param_layout():
        r = g32[off:off + n]
        if n == 0 or float(r.abs().max()) == 0.0:
            continue
        cs, e = _cos_rel(g16[off:off + n], r)
        live += 1
        assert cs >= 0.999 and e <= 2e-2, (k, cs, e)
    assert live >= 150
    assert _cos_rel(g16, g32)[0] >= 0.9999


def model_at(pharm_nf, rec_nf, T):
    import pharmacoforge_amd as pfa
    from test_gpu_api import DEV_DYN, DEV_GRAPH
    m = pfa.PharmacophoreDiff(pharm_nf, rec_nf, [f"type{i}" for i in range(pharm_nf)], None, n_timesteps=T, graph_config=DEV_GRAPH,
                              dynamics_config=DEV_DYN, precision=1e-5)
    sd = dict(O.make_state_dict(O.DynamicsConfig(pharm_nf=pharm_nf, rec_nf=rec_nf), 0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    return m.to("cuda").eval()


@pytest.mark.parametrize("ep_coord,ep_feat", [(False, False), (True, True)])
@pytest.mark.parametrize("pharm_nf,rec_nf", [(8, 16), (1, 1)])
def test_fused_loss_equals_the_restatement(pharm_nf, rec_nf, ep_coord, ep_feat):
    """The fused loss call (k_loss_prepare / k_loss_eval) against the framework-op restatement in forward(), losses, metrics and
    the flat gradient, as test_gpu_endpoint_loss.test_fused_call_equals_the_restatement -- eight classes and one (the
    cross-entropy of a softmax over one class is zero and so is its gradient)"""
    import pharmacoforge_amd as pfa
    from test_gpu_endpoint_loss import assert_same, fused_and_restated, random_inputs, set_flags
    T = 100
    c = nf_case(pharm_nf, rec_nf)
    m = model_at(pharm_nf, rec_nf, T)
    set_flags(m, ep_coord, ep_feat, True, False)
    x0, h0, inj = random_inputs(c.batch, T, 9, nf=pharm_nf)
    b = c.batch
    g = pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, x0, h0).to("cuda")
    assert_same(fused_and_restated(m, g, inj))


@pytest.mark.parametrize("pharm_nf,rec_nf,limit", [(9, 11, "pharm_nf <= 8"), (6, 17, "rec_nf <= 16")])
def test_training_is_refused_beyond_its_counts_before_anything_runs(pharm_nf, rec_nf, limit):
    import pharmacoforge_amd as pfa
    c = nf_case(pharm_nf, rec_nf)
    eng = engine_for(c.cfg, c.sd)
    set_batch(eng, c.batch)
    eng.dynamics(c.x_t, c.h_t, c.t)
    before = eng.counts()
    assert before["centers"] == int(c.batch.pharm_ptr[-1]) and before["pf"] > 0
    with pytest.raises(pfa.PfError, match=limit):
        eng.train_forward(c.x_t, c.h_t, c.t, prot_x=c.prot_x)
    assert eng.counts() == before
    eh, ex = eng.dynamics(c.x_t, c.h_t, c.t)                     # the handle goes on serving inference
    assert bool(torch.isfinite(eh).all()) and bool(torch.isfinite(ex).all())
