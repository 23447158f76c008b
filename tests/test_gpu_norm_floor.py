"""The 1e-8 floor of norm_no_nan (gvp.py:12-19) in every kernel family, forward and backward.

The reference clamps a squared norm at 1e-8 before the square root in three places: sh = |Vh| inside every GVP, the vector
statistic of every GVPLayerNorm, and the edge geometry d = sqrt(max(|x_src - x_dst|^2, 1e-8)) + 1e-8.  The HIP code restates
it by hand in about thirty places ("the norm floor"), the gradient kernels with the matching indicator.
With seeded weights the floor acts on ~1 % of the entries and a kernel without it passes the rest of the suite; the inputs here
(helpers.floor_weights, helpers.twin_inputs) put it to work on ~45 % of them and on the edge geometry, and
tests/test_oracle_norm_floor.py proves on the CPU oracle that a kernel without the floor, or a gradient kernel that
differentiates through the clamp, misses the tolerances used here by a factor of ten or more.

Tolerances are the suite's own: a chain 5e-5 (UNIT_TOL), a dynamics call 2e-4 + 2e-4 |ref| plus the fp64 budget of
helpers.check_live, sampler states 2e-4 (i + 1) after step i (test_tail_launch_steps_equal_separate_launches), gradients 2e-3
of a tensor's max and outputs 2e-4 (test_gradients_vs_oracle).  Every leg prints the kernel family it ran."""
import functools
import os

import pytest
import torch

from oracle import pf_oracle as O
from helpers import (BUDGET_FLOOR, check_live, edge_set, floor_weights, live_head, norm_census, sampler_live_head, within_budget)
from test_gpu_parity import ATOL, RTOL, UNIT_TOL, close
from test_gpu_train import compare, flat_to_dict
from test_gpu_wide import engine_for, set_batch
from test_gpu_wide_train import masks_from_engine
from test_oracle_norm_floor import FLOOR_SEEDS, floor_case, oracle_gradients, twin_case

pytestmark = pytest.mark.gpu

ET_NAMES = ["pharm_ff_pharm", "prot_pf_pharm", "pharm_fp_prot", "prot_pp_prot"]
HEAD = "dynamics.noise_predictor.noise_predictor."


def sd64(sd):
    return O.state_dict64(sd)


# ---- a. chain units -------------------------------------------------------------------------------------------------------------
def _chain_check(got, ref32, ref64, what):
    for g, r32, r64, part in zip(got, ref32, ref64, ("scalars", "vectors")):
        close(g, r32, UNIT_TOL, UNIT_TOL)
        within_budget(g, r32, r64, f"{what} {part}")


@pytest.mark.parametrize("form", ["rg", "n16"])
def test_chain_units_on_floor_weights(form):
    """Every message chain (layer x edge type), update chain (layer x node type) and -- row-group form -- the head through
    pf_debug_chain on floor weights and randn rows: half of every sh sits on the floor.  Kinds 0 / 1 / 3 (row-group chain code) and
    16 / 17 (n16 chain code); the ragged row counts of test_chain_units_every_chain_vs_oracle; against the oracle at UNIT_TOL and
    inside the fp64 budget of the same rows."""
    cfg = O.DynamicsConfig()
    sd = floor_weights(O.make_state_dict(cfg, 7))
    s64 = sd64(sd)
    eng = engine_for(cfg, sd)
    gen = torch.Generator().manual_seed(3)
    k_msg, k_upd = (0, 1) if form == "rg" else (16, 17)
    for layer in range(cfg.n_convs):
        p = f"dynamics.noise_predictor.conv_layers.{layer}."
        for et in range(4):
            n = 5 + 4 * layer + et
            s, v = torch.randn(n, 144, generator=gen), torch.randn(n, 17, 3, generator=gen)
            s[:, 128:] = s[:, 128:].abs().clamp(max=1.0)
            key = p + f"edge_message_fns.{ET_NAMES[et]}."
            with norm_census(lambda: O.gvp_chain(sd, key, cfg.n_message_gvps, s, v)) as census:
                pass
            assert 0.4 <= census.clamped_share() <= 0.6, census.clamped_share()
            got = eng.debug_chain(k_msg, layer, et, s, v)
            _chain_check(got, census.result, O.gvp_chain(s64, key, cfg.n_message_gvps, s.double(), v.double()),
                         f"chain {form} msg layer {layer} {ET_NAMES[et]}")
        for nt, name in enumerate(("prot", "pharm")):
            n = 6 + nt
            s, v = torch.randn(n, 128, generator=gen), torch.randn(n, 16, 3, generator=gen)
            key = p + f"node_update_fns.{name}."
            got = eng.debug_chain(k_upd, layer, nt, s, v)
            _chain_check(got, O.gvp_chain(sd, key, cfg.n_update_gvps, s, v),
                         O.gvp_chain(s64, key, cfg.n_update_gvps, s.double(), v.double()), f"chain {form} upd layer {layer} {name}")
    if form == "n16":
        return
    s, v = torch.randn(9, 128, generator=gen), torch.randn(9, 16, 3, generator=gen)
    sd_live, _ = live_head(sd, cfg, O.noise_head(sd, HEAD, cfg, s, v)[1])
    got = engine_for(cfg, sd_live).debug_chain(3, 0, 0, s, v)
    ref = O.noise_head(sd_live, HEAD, cfg, s, v)
    assert float(ref[1].abs().max()) >= 0.5
    _chain_check(got, ref, O.noise_head(sd64(sd_live), HEAD, cfg, s.double(), v.double()), "chain rg head (live)")


# ---- b. GVPLayerNorm sweep ------------------------------------------------------------------------------------------------------
def test_layernorm_sweep_over_vector_magnitudes():
    """pf_debug_chain kind 2 on plain weights: row j's vectors are randn * 2**-j, j = 0..24 -- the per-channel squared norms cross
    the floor around j = 13 --, one all-zero row, one row with half of its channels scaled by 2**-20.  Per ROW inside the fp64
    budget: a tiny row's output is tiny, and a tensor-wide maximum would not look at it."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 7)
    s64 = sd64(sd)
    eng = engine_for(cfg, sd)
    gen = torch.Generator().manual_seed(4)
    n = 27
    for layer in range(cfg.n_convs):
        for nt, name in enumerate(("prot", "pharm")):
            for which, ln in enumerate(("message_layer_norms", "update_layer_norms")):
                s, v = torch.randn(n, 128, generator=gen), torch.randn(n, 16, 3, generator=gen)
                v[:25] *= (2.0 ** -torch.arange(25.0))[:, None, None]
                v[25] = 0.0
                v[26, ::2] *= 2.0 ** -20
                key = f"dynamics.noise_predictor.conv_layers.{layer}.{ln}.{name}."
                with norm_census(lambda: O.gvp_layernorm(sd, key, s, v)) as census:
                    pass
                share = [float((ss.reshape(n, -1) < 1e-8).float().mean(dim=1)[j]) for ss in census.sites[key + "vn"] for j in (0, 26, 24)]
                assert share == [0.0, 0.5, 1.0], share
                ro, rv = census.result
                r64o, r64v = O.gvp_layernorm(s64, key, s.double(), v.double())
                so, vo = eng.debug_chain(2, layer, 2 * nt + which, s, v)
                what = f"layernorm layer {layer} {ln}.{name}"
                close(so, ro, UNIT_TOL, UNIT_TOL); close(vo, rv, UNIT_TOL, UNIT_TOL)
                within_budget(so, ro, r64o, what + " scalars")
                assert bool(torch.all(vo[25] == 0)) and bool(torch.isfinite(vo).all())
                for j in list(range(25)) + [26]:
                    within_budget(vo[j], rv[j], r64v[j], f"{what} row {j}")


# ---- c. whole dynamics call -----------------------------------------------------------------------------------------------------
def _fam(eng, cfg):
    return [eng.kernel_family(layer) for layer in range(cfg.n_convs)]


def _expect(families=None, hoist=None, n16=None):
    def check(eng, cfg):
        fam = _fam(eng, cfg)
        if families is not None:
            assert all(f in families for f in fam), (fam, families)
        if hoist is not None:
            assert (eng.l0_hoist() > 0) == hoist, eng.l0_hoist()
        if n16 is not None:
            mask, variant = n16
            fusable = cfg.n_convs == 2 and cfg.pf_k > 0 and variant == "compact"
            if mask & 1:
                assert fam[-1] == (17 if (mask & 4) and fusable else 16), fam
            if mask & 2:
                assert fam[0] == 16 and eng.l0_hoist() == 16, (fam, eng.l0_hoist())
    return check


BIG = "100000000"
ONE_WAVE = {"PFDYN_RG_ROWS_MAX": "0", "PFDYN_COOP_EDGE_MAX": "0", "PFDYN_COOP2_EDGE_MAX": "0", "PFDYN_COOP_NODE_MAX": "0",
            "PFDYN_NO_PRUNE": "1"}
FORWARD_LEGS = {                       # name -> (environment, the family the leg names)
    "default": ({}, _expect(families={4, 8, 16, 17})),
    "one_wave_per_tile": (ONE_WAVE, _expect(families={32}, hoist=False)),
    "four_waves_per_tile": ({"PFDYN_RG_ROWS_MAX": "0"}, _expect(families={128}, hoist=False)),
    "four_waves_per_tile_dense": ({"PFDYN_RG_ROWS_MAX": "0", "PFDYN_NO_PRUNE": "1"}, _expect(families={128}, hoist=False)),
    "two_workgroups_per_cu": ({"PFDYN_RG_ROWS_MAX": "0", "PFDYN_COOP_EDGE_MAX": "0", "PFDYN_COOP2_EDGE_MAX": "1000000"},
                              _expect(families={128}, hoist=False)),
    "two_workgroups_per_cu_dense": ({"PFDYN_RG_ROWS_MAX": "0", "PFDYN_COOP_EDGE_MAX": "0", "PFDYN_COOP2_EDGE_MAX": "1000000",
                                     "PFDYN_NO_PRUNE": "1"}, _expect(families={128}, hoist=False)),
    "no_l0_hoist": ({"PFDYN_NO_L0_HOIST": "1"}, _expect(families={4, 8, 16, 17}, hoist=False)),
    # (the center hoist's tables are left by a denoising step's merged launch: the sampler legs below run it; a lone dynamics
    # call under the switch takes the on-the-fly encoding either way)
    "no_center_hoist": ({"PFDYN_NO_CENTER_HOIST": "1"}, _expect(families={4, 8, 16, 17})),
    "wide": ({"PFDYN_WIDE": "1"}, _expect(families={64})),
}
for _rows in (4, 8, "4 on two waves"):
    for _dense in (False, True):
        _env = {"PFDYN_RG_ROWS_MAX": BIG, "PFDYN_RG2_ROWS_MIN": "0" if _rows == 8 else BIG,
                "PFDYN_RG_SPLIT_MAX": BIG if _rows == "4 on two waves" else "0"}
        if _dense:
            _env.update({"PFDYN_NO_PRUNE": "1", "PFDYN_NO_FUSE_HEAD": "1"})
        FORWARD_LEGS[f"row_groups_{str(_rows).replace(' ', '_')}" + ("_dense" if _dense else "")] = (
            _env, _expect(families={8 if _rows == 8 else 4}, hoist=True))
for _mask in (1, 2, 3, 5, 7):
    for _variant in ("compact", "dense"):
        _env = {"PFDYN_N16": str(_mask), "PFDYN_N16_ROWS_MAX": BIG}
        if _variant == "dense":
            _env["PFDYN_NO_PRUNE"] = "1"
        FORWARD_LEGS[f"n16_mask{_mask}_{_variant}"] = (_env, _expect(n16=(_mask, _variant)))

FORWARD_CASES = {"floor": lambda: floor_case(), "twin_dev": lambda: twin_case("dev"),
                 "twin_knnff_radiuspf_gnorm": lambda: twin_case("knnff_radiuspf_gnorm")}


def _dynamics_leg(c, env, expect, what, monkeypatch, twin):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_for(c.cfg, c.live.sd)
    set_batch(eng, c.batch)
    eps_h, eps_x = eng.dynamics(c.x_t, c.h_t, c.t)
    print(f"norm floor leg {what}: kernel families {_fam(eng, c.cfg)}, l0 hoist {eng.l0_hoist()}")
    expect(eng, c.cfg)
    if twin:
        edges = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)
        for i, et in enumerate(("ff", "pf", "fp")):
            s, d = eng.get_edges(i)
            assert edge_set(s, d) == edge_set(*edges[et]) and s.numel() == edges[et][0].numel(), et
    assert bool(torch.isfinite(eps_h).all()) and bool(torch.isfinite(eps_x).all())
    check_live(eps_h, eps_x, c.live, f"norm floor {what}", RTOL, ATOL)


@pytest.mark.parametrize("leg", list(FORWARD_LEGS))
@pytest.mark.parametrize("case", list(FORWARD_CASES))
def test_dynamics_call_every_forward_family(case, leg, monkeypatch):
    """One dynamics call on the floor weights (live head) and on the twin inputs (plain weights, live head; the dev config and
    the kNN-ff / radius-pf / per-graph-norm config) under the default policy and under every forward family the suite forces,
    against the fp32 oracle at the family's tolerance and inside the fp64 budget; twin inputs: the dynamic edge sets exactly."""
    env, expect = FORWARD_LEGS[leg]
    _dynamics_leg(FORWARD_CASES[case](), env, expect, f"{leg} {case}", monkeypatch, case.startswith("twin"))


def test_dynamics_call_wide_model_64_32():
    """A 64 / 32 model (the width-generic family's own widths) on floor weights."""
    _dynamics_leg(floor_case(64, 32), {}, _expect(families={64}), "wide 64/32 floor", None, False)


# ---- d. sampler steps -----------------------------------------------------------------------------------------------------------
STEP_FORMS = {      # form -> (PFDYN_N16, PFDYN_TAIL_FORM, PFDYN_HS_BUILD, kernel_family(n_convs), kernel_family(n_convs - 1))
    "separate": ("3", "rg", "0", 0, 16),
    "fused": ("7", "rg", "0", 0, 17),
    "tail_rg": ("15", "rg", "0", 4, None),
    "tail_n16": ("15", "n16", "0", 16, None),
    "merged": ("7", "rg", "1", 2, 17),
}
T_STEPS, N_STEPS = 50, 4


@functools.lru_cache(maxsize=None)
def sampler_case(start):
    """floor weights from a random x_T, or plain weights from the twin inputs as x_T (in the pocket's frame: init_pharm_com = 0
    keeps the planted offsets exact); a live head either way; the oracle's four steps, every frame"""
    c = floor_case() if start == "floor" else twin_case("dev")
    Nf, B = int(c.batch.pharm_ptr[-1]), c.batch.batch_size
    noise = torch.randn(N_STEPS + 1, Nf, 9, generator=torch.Generator().manual_seed(17))
    com = None
    if start == "twin":
        noise[0, :, :3] = c.x_t
        com = torch.zeros(B, 3)
    sd, _ = sampler_live_head(c.sd, c.cfg, c.batch, T_STEPS, 1e-5, noise)
    x0, h0, frames = O.sample_given_receptor(sd, c.cfg, c.batch, T_STEPS, 1e-5, noise, init_pharm_com=com, return_traj=True,
                                             n_steps=N_STEPS)
    return c, sd, noise, com, frames


@pytest.mark.parametrize("form", list(STEP_FORMS))
@pytest.mark.parametrize("start", ["floor", "twin"])
def test_sampler_steps_every_step_form(start, form, monkeypatch):
    """Four denoising steps at T = 50 through every form of a step's end, the state after every step against
    O.sample_given_receptor's frames at 2e-4 (i + 1)."""
    c, sd, noise, com, frames = sampler_case(start)
    mask, tform, hsb, fam_end, fam_last = STEP_FORMS[form]
    monkeypatch.setenv("PFDYN_N16", mask)
    monkeypatch.setenv("PFDYN_TAIL_FORM", tform)
    monkeypatch.setenv("PFDYN_HS_BUILD", hsb)
    eng = engine_for(c.cfg, sd)
    set_batch(eng, c.batch)
    coef = O.step_coefficients(O.gamma_table(T_STEPS, 1e-5), T_STEPS)
    arr = eng.coef_array(coef, reversed(range(T_STEPS)))
    eng.sample_begin(noise[0], init_pharm_com=com)
    for i in range(N_STEPS):
        eng.denoise_step(arr[i], noise[i + 1])
        fams = _fam(eng, c.cfg) + [eng.kernel_family(c.cfg.n_convs)]
        print(f"norm floor sampler {start} {form} step {i}: kernel families {fams}")
        assert fams[-1] == fam_end and (fam_last is None or fams[-2] == fam_last), fams
        x, h = eng.sample_frame()
        tol = 2e-4 * (i + 1)
        close(x, frames[i + 1][0], tol, tol); close(h, frames[i + 1][1], tol, tol)
    assert eng.xchg_timeouts() == 0


@pytest.mark.parametrize("hoist", [True, False])
def test_sampler_run_center_hoist_on_floor_weights(hoist, monkeypatch):
    """The same four steps as one pf_sample run, which announces its timesteps: the merged launch then leaves the center-hoist
    tables and the next call's ff / fp items start from them (PFDYN_NO_CENTER_HOIST=1: they encode on the fly)."""
    c, sd, noise, com, frames = sampler_case("floor")
    if not hoist:
        monkeypatch.setenv("PFDYN_NO_CENTER_HOIST", "1")
    eng = engine_for(c.cfg, sd)
    set_batch(eng, c.batch)
    coef = O.step_coefficients(O.gamma_table(T_STEPS, 1e-5), T_STEPS)
    x0, h0, tx, th = eng.sample(eng.coef_array(coef, reversed(range(T_STEPS))), N_STEPS, noise, trajectory=True)
    torch.cuda.synchronize()
    eng.sample_status()
    print(f"norm floor sampler run: kernel families {_fam(eng, c.cfg)}, center hoist {eng.kernel_family(c.cfg.n_convs + 1)}")
    assert eng.kernel_family(0) == 16 and eng.kernel_family(c.cfg.n_convs + 1) == (1 if hoist else 0)
    assert eng.xchg_timeouts() == 0
    for i in range(N_STEPS + 1):
        tol = 2e-4 * max(i, 1)
        close(tx[i], frames[i][0], tol, tol); close(th[i], frames[i][1], tol, tol)


# ---- e. gradients ---------------------------------------------------------------------------------------------------------------
P_DROP, DROP_SEED = 0.1, 1234
TRAIN_LEGS = {                         # name -> (environment, training family, kernel_family(0) of the training forward)
    "default": ({}, "tuned", 4),
    "no_fixed_shapes": ({"PFDYN_NO_FIXED_SHAPES": "1"}, "tuned", 4),
    "tile_head": ({"PFDYN_TRAIN_TILE_HEAD": "1"}, "tuned", 4),
    "node_recompute": ({"PFDYN_TRAIN_NODE_RECOMPUTE": "1"}, "tuned", 4),
    "tile_edge": ({"PFDYN_TRAIN_TILE_EDGE": "1"}, "tuned", 32),
    "tile_node": ({"PFDYN_TRAIN_TILE_NODE": "1"}, "tuned", 32),
    "dense": ({"PFDYN_NO_PRUNE": "1", "PFDYN_NO_PRE": "1"}, "tuned", 4),
    "wide_128_16": ({}, "wide", None),
    "wide_64_32": ({}, "wide", None),
}
BUDGET_ROWS = []


def grad_case(inputs, leg):
    S, V = (64, 32) if leg == "wide_64_32" else (128, 16)
    if inputs == "floor":
        return floor_case(S, V)
    if (S, V) == (128, 16):
        return twin_case(inputs[len("twin_"):])
    return _wide_twin()


@functools.lru_cache(maxsize=None)
def _wide_twin():
    from helpers import twin_inputs
    from test_oracle_norm_floor import _inputs
    wseed, iseed = FLOOR_SEEDS[(64, 32)]
    c = _inputs(O.DynamicsConfig(n_hidden_scalars=64, vector_size=32), iseed)
    c.batch, c.x_t, c.planted = twin_inputs(c.batch, c.x_t, c.cfg)
    c.prot_x = c.batch.prot_x
    c.sd = O.make_state_dict(c.cfg, wseed)
    return c


_GRAD_REFS = {}


def grad_reference(key, c, drop):
    """the fp32 and fp64 oracle gradients of a case under the engine's masks: every leg of a case draws the same masks (one hash
    of seed, layer, site, node, column), so they are computed once and left unchanged"""
    if key not in _GRAD_REFS:
        with norm_census() as c32:
            g32, oh, ox = oracle_gradients(c, c.sd, drop)
        with norm_census() as c64:
            g64, _, _ = oracle_gradients(c, sd64(c.sd), drop)
        print(f"norm floor gradients {key}: {c32.clamped_share():.3f} of the norm entries clamped in the training forward, "
              f"nearest to the threshold {c32.nearest_to_threshold():.2e}")
        assert torch.equal(c32.sides(), c64.sides())
        _GRAD_REFS[key] = (drop, g32, g64, oh, ox)
    ref = _GRAD_REFS[key]
    for a, b in zip(ref[0], drop):
        for nt in a:
            assert all(torch.equal(p, q) for p, q in zip(a[nt], b[nt])), "the legs of a case must draw the same dropout masks"
    return ref[1:]


def record_budget(what, got, g32, g64):
    """every tensor's error against the fp64 oracle's gradient as a ratio to max(e32, 2**-22); recorded, not asserted here --
    tests/test_gpu_grad_budget.py asserts it, per 16 x 16 block and with a unit from several reference draws
    (grad_budget.gradients_within_budget)"""
    rows = []
    for k, r64 in g64.items():
        m = float(r64.abs().max()) if r64.numel() else 0.0
        if m == 0.0:
            continue
        e = float((got[k].reshape(r64.shape).double() - r64).abs().max()) / m
        e32 = float((g32[k].double() - r64).abs().max()) / m
        rows.append((e / max(e32, BUDGET_FLOOR), e, e32, k))
    rows.sort(reverse=True)
    for ratio, e, e32, k in rows:
        print(f"gradient budget {what}: {k} e {e:.3e} e32 {e32:.3e} ratio {ratio:.2f}")
    ratios = torch.tensor([r[0] for r in rows])
    lines = [f"{what}: {len(rows)} tensors, worst ratio {rows[0][0]:.2f}, median {float(ratios.median()):.2f}"]
    lines += [f"    {ratio:8.2f}  e {e:.3e}  e32 {e32:.3e}  {k.replace('dynamics.noise_predictor.', '')}" for ratio, e, e32, k in rows[:6]]
    BUDGET_ROWS.extend(lines)
    out = os.environ.get("PF_GRADIENT_BUDGET_FILE")
    if out:
        with open(out, "w") as f:
            f.write("Gradient error against the fp64 oracle's autograd, per leg of tests/test_gpu_norm_floor.py::test_gradients_every_training_family:\n"
                    "per tensor e = max|got - g64| / max|g64|, e32 the same for the fp32 oracle's gradient, ratio = e / max(e32, 2**-22).\n"
                    "Per leg: the number of tensors with a non-zero gradient, the worst and the median ratio, and the six worst tensors\n"
                    "(the test prints every tensor).  Recorded, not asserted.\n\n" + "\n".join(BUDGET_ROWS) + "\n")


@pytest.mark.parametrize("leg", list(TRAIN_LEGS))
@pytest.mark.parametrize("inputs", ["floor", "twin_dev"])
def test_gradients_every_training_family(inputs, leg, monkeypatch):
    """pf_train_forward / pf_train_backward on floor weights (plain head) and on the twin inputs (plain weights), dropout 0.1,
    random upstream weights, under the tuned family's default and each of its switches and on the wide training family (forced at
    128 / 16; a 64 / 32 model): parameter gradients against the oracle's autograd under the engine's own masks at 2e-3 of a
    tensor's max, outputs at 2e-4, a second backward bit for bit; the error against the fp64 oracle's gradient is recorded."""
    env, family, fam0 = TRAIN_LEGS[leg]
    c = grad_case(inputs, leg)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_for(c.cfg, c.sd)
    if family == "wide":
        eng.set_train_family("wide")
    set_batch(eng, c.batch)
    Np, Nf = int(c.batch.prot_ptr[-1]), int(c.batch.pharm_ptr[-1])
    eps_h, eps_x = eng.train_forward(c.x_t, c.h_t, c.t, prot_x=c.prot_x, dropout=P_DROP, seed=DROP_SEED)
    print(f"norm floor gradients {inputs} {leg}: training family {eng.train_family()}, kernel families {_fam(eng, c.cfg)}")
    assert eng.train_family() == family
    if fam0 is not None:
        assert eng.kernel_family(0) == fam0, _fam(eng, c.cfg)
    drop = masks_from_engine(eng, c.cfg, P_DROP, DROP_SEED, Np, Nf)
    g32, g64, oh, ox = grad_reference((inputs, c.cfg.n_hidden_scalars), c, drop)
    dh, dx = float((eps_h.cpu() - oh).abs().max()), float((eps_x.cpu() - ox).abs().max())
    print(f"norm floor gradients {inputs} {leg}: max |eps_h - oracle| {dh:.3e}, max |eps_x - oracle| {dx:.3e}")
    assert dh < 2e-4 and dx < 2e-4
    got = flat_to_dict(eng, eng.train_backward(c.w_h, c.w_x))
    again = flat_to_dict(eng, eng.train_backward(c.w_h, c.w_x))
    record_budget(f"{inputs} {leg}", got, g32, g64)
    assert sum(r.numel() > 0 and float(r.abs().max()) > 0 for r in g32.values()) >= 100
    compare(got, g32, 2e-3, f"{inputs} {leg}")
    for k in got:
        assert torch.equal(again[k], got[k]), k


def test_gradients_twin_inputs_knnff_radiuspf_gnorm():
    """The twin inputs on the kNN-ff / radius-pf / per-graph-norm config, the tuned family's default."""
    c = twin_case("knnff_radiuspf_gnorm")
    eng = engine_for(c.cfg, c.sd)
    set_batch(eng, c.batch)
    Np, Nf = int(c.batch.prot_ptr[-1]), int(c.batch.pharm_ptr[-1])
    eps_h, eps_x = eng.train_forward(c.x_t, c.h_t, c.t, prot_x=c.prot_x, dropout=P_DROP, seed=DROP_SEED)
    print(f"norm floor gradients twin_knnff_radiuspf_gnorm: training family {eng.train_family()}, kernel families {_fam(eng, c.cfg)}")
    drop = masks_from_engine(eng, c.cfg, P_DROP, DROP_SEED, Np, Nf)
    g32, g64, oh, ox = grad_reference(("twin_knnff_radiuspf_gnorm", 128), c, drop)
    assert float((eps_h.cpu() - oh).abs().max()) < 2e-4 and float((eps_x.cpu() - ox).abs().max()) < 2e-4
    got = flat_to_dict(eng, eng.train_backward(c.w_h, c.w_x))
    again = flat_to_dict(eng, eng.train_backward(c.w_h, c.w_x))
    record_budget("twin_knnff_radiuspf_gnorm default", got, g32, g64)
    compare(got, g32, 2e-3, "twin_knnff_radiuspf_gnorm")
    for k in got:
        assert torch.equal(again[k], got[k]), k
