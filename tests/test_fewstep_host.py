"""Few-step sampling, host side: schedule.level_plan / strided_coefficients / multistep_coefficients, the model's keyword rules
and the CLIs' flags -- no GPU.  The solver-exactness tests use a synthetic consistent "network": with x0 and e fixed and
z_t = alpha_t x0 + sigma_t e, a network that returns e (noise block) or x0 (endpoint block) makes every deterministic solver
exact, so any plan must end at alpha_0 x0 + sigma_0 e."""
import os
import sys

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import generate_pharmacophores as cli  # noqa: E402
import fewstep_ref as F  # noqa: E402
from test_host_logic import make_model  # noqa: E402
from test_seeded_host import pocket  # noqa: E402

S = pfa.schedule
SPACINGS = ("uniform", "quadratic", "logsnr")
FIELDS = ("alpha_t_given_s", "var_terms", "sigma", "ep_zt", "ep_pred")


def n_list(top):
    return sorted({1, 2, 3, 6, 10, top // 2, top - 1, top} & set(range(1, top + 1)))


# ---- level_plan ----
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("T", [24, 100, 1000])
def test_level_plan_shape(T, spacing):
    gamma = O.gamma_table(T, 1e-5)
    for top in (T, max(T // 3, 1)):
        for N in n_list(top):
            lv = S.level_plan(T, N, spacing, top=top, gamma_table=gamma)
            assert len(lv) == N + 1 and all(isinstance(l, int) for l in lv), (T, top, N)
            assert lv[0] == top and lv[-1] == 0 and all(a > b for a, b in zip(lv[:-1], lv[1:])), (T, top, N, lv)
            assert lv == S.level_plan(T, N, spacing, top=top, gamma_table=gamma)          # deterministic
        assert S.level_plan(T, top, spacing, top=top, gamma_table=gamma) == list(range(top, -1, -1))
    assert S.level_plan(T, 6, spacing, gamma_table=gamma) == S.level_plan(T, 6, spacing, top=T, gamma_table=gamma)


def test_level_plan_spacings_and_refusals():
    assert S.level_plan(24, 6) == [24, 20, 16, 12, 8, 4, 0] == F.uniform_plan(24, 6)
    assert S.level_plan(100, 10) == F.uniform_plan(100, 10) and S.level_plan(24, 8) == F.uniform_plan(24, 8)
    q = S.level_plan(1000, 10, "quadratic")
    gaps = [a - b for a, b in zip(q[:-1], q[1:])]
    assert gaps == sorted(gaps, reverse=True) and gaps[0] > 10 * gaps[-1]              # denser near 0
    gamma = O.gamma_table(1000, 1e-5)
    lv = S.level_plan(1000, 10, "logsnr", gamma_table=gamma)
    lam = -0.5 * gamma.double()[torch.tensor(lv)]
    steps = lam[1:] - lam[:-1]
    assert float(steps.max() / steps.min()) < 1.2                                       # uniform in lambda up to the level grid
    for bad in (0, -1, 25):
        with pytest.raises(ValueError, match="1 <= n_steps <= 24"):
            S.level_plan(24, bad)
    with pytest.raises(ValueError, match="1 <= n_steps <= 9"):
        S.level_plan(24, 10, top=9)
    with pytest.raises(ValueError, match="1 <= top <= 24"):
        S.level_plan(24, 3, top=25)
    with pytest.raises(ValueError, match="spacing must be"):
        S.level_plan(24, 3, "cosine")
    with pytest.raises(ValueError, match="needs gamma_table"):
        S.level_plan(24, 3, "logsnr")


# ---- strided_coefficients ----
@pytest.mark.parametrize("T,prec", [(24, 0.25), (100, 1e-5), (500, 1e-5)])
def test_unit_stride_is_step_coefficients_bitwise(T, prec):
    gamma = O.gamma_table(T, prec)
    full = S.step_coefficients(gamma, T)
    got = S.strided_coefficients(gamma, T, list(range(T, -1, -1)))
    assert set(got) == set(full)
    for k in full:
        assert got[k].dtype == torch.float32 and torch.equal(got[k], full[k].flip(0)), k
    a = 7                                                                                # a seeded run's plan: the last a entries
    part = S.strided_coefficients(gamma, T, S.level_plan(T, a, top=a))
    for k in full:
        assert torch.equal(part[k], full[k][:a].flip(0)), k
    order = list(range(T))
    assert bytes(pfa.PfEngine.coef_array(got, order)) == bytes(pfa.PfEngine.coef_array(full, reversed(order)))


@pytest.mark.parametrize("spacing", SPACINGS)
def test_eta_1_is_the_oracle_posterior_at_a_stride(spacing):
    T, prec = 100, 1e-5
    gamma = O.gamma_table(T, prec)
    lv = S.level_plan(T, 10, spacing, gamma_table=gamma)
    got = S.strided_coefficients(gamma, T, lv)
    sp = torch.nn.functional.softplus(gamma)
    for i, (t, s) in enumerate(zip(lv[:-1], lv[1:])):
        ref = F.first_coef(gamma, T, s, t, 1.0)
        # the two evaluate the same fp32 expressions, one pair alone and one pair inside a T-long tensor; torch's softplus may round
        # by an ulp differently in the two, and sigma2_{t|s} = -expm1(softplus(g_s) - softplus(g_t)) amplifies that by
        # max(softplus) / |difference|; 1e-6 for the other roundings
        tol = 1e-6 + 4 * 2.0 ** -23 * float(max(sp[s], sp[t]) / (sp[t] - sp[s]).abs())
        for k, r in zip(FIELDS, ref):
            assert abs(float(got[k][i]) - float(r)) <= tol * abs(float(r)), (i, k, float(got[k][i]), float(r), tol)
        assert float(got["t"][i]) == float(torch.tensor(t).float() / T) and float(got["s"][i]) == float(torch.tensor(s).float() / T)
    # the pin and guide tables selected at the plan's levels
    pin, pin_all = S.pin_coefficients(gamma, T, lv), S.pin_coefficients(gamma, T)
    gd, gd_all = S.guide_coefficients(gamma, T, lv), S.guide_coefficients(gamma, T)
    for i, (t, s) in enumerate(zip(lv[:-1], lv[1:])):
        assert float(pin["alpha_s"][i]) == float(pin_all["alpha_s"][s]) and float(pin["sigma_s"][i]) == float(pin_all["sigma_s"][s])
        assert float(gd["alpha_t"][i]) == float(gd_all["alpha_t"][t - 1]) and float(gd["sigma_t"][i]) == float(gd_all["sigma_t"][t - 1])


def test_ddim_branch():
    """eta = 0 injects exactly nothing; the DDIM branch against fewstep_ref's own formulas; eta -> 1 meets the posterior branch to
    fp32 rounding: 1e-5 relative to each field's largest entry (the posterior branch is evaluated in fp32 with ~10 roundings of
    6e-8 each, amplified where sigma2_{t|s} is a difference of nearly equal numbers)."""
    T, prec = 100, 1e-5
    gamma = O.gamma_table(T, prec)
    lv = S.level_plan(T, 10)
    c0 = S.strided_coefficients(gamma, T, lv, 0.0)
    assert torch.equal(c0["sigma"], torch.zeros(10)) and c0["sigma"].dtype == torch.float32
    for eta in (0.0, 0.5):
        got = S.strided_coefficients(gamma, T, lv, eta)
        for i, (t, s) in enumerate(zip(lv[:-1], lv[1:])):
            for k, r in zip(FIELDS, F.first_coef(gamma, T, s, t, eta)):
                assert abs(float(got[k][i]) - float(r)) <= 1e-6 * max(abs(float(r)), 1e-3), (eta, i, k)
    post = S.strided_coefficients(gamma, T, lv, 1.0)
    near = S.strided_coefficients(gamma, T, lv, 1.0 - 1e-12)
    for k in FIELDS:
        assert float((post[k] - near[k]).abs().max()) <= 1e-5 * float(post[k].abs().max()), k
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta must lie"):
            S.strided_coefficients(gamma, T, lv, bad)
    with pytest.raises(ValueError, match="descend strictly"):
        S.strided_coefficients(gamma, T, [10, 10, 0])


# ---- solver exactness ----
U = 2.0 ** -24 * 1.01            # the relative error of one fp32 rounding (round to nearest), with room for second-order terms


def consistent_end(gamma, T, lv, step):
    """runs ``step(i, z, x0, e) -> (the multiplier of z, the move's terms)`` over the plan in fp64 from z = alpha_top x0 +
    sigma_top e and sums the terms; returns (z_end, expected, the largest magnitude a term took, the forward error bound of
    fp32 coefficient rounding: bound' = |multiplier| bound + U * sum of the terms' magnitudes)"""
    gen = torch.Generator().manual_seed(5)
    x0, e = torch.randn(7, 3, generator=gen, dtype=torch.float64), torch.randn(7, 3, generator=gen, dtype=torch.float64)
    g = gamma.double()
    al, sg = torch.sqrt(torch.sigmoid(-g)), torch.sqrt(torch.sigmoid(g))
    z = al[lv[0]] * x0 + sg[lv[0]] * e
    want = al[0] * x0 + sg[0] * e
    scale, bound = float(want.abs().max()), 0.0
    for i in range(len(lv) - 1):
        mult, terms = step(i, z, x0, e)
        scale = max([scale] + [float(t.abs().max()) for t in terms])
        bound = abs(float(mult)) * bound + U * sum(float(t.abs().max()) for t in terms)
        z = sum(terms)
    return z, want, scale, bound


@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("T,N", [(24, 6), (100, 10), (1000, 20), (1000, 50), (100, 1), (24, 24)])
def test_solvers_are_exact_for_a_consistent_network(T, N, spacing):
    """fp64 evaluation with the fp32 coefficients.  Two bounds, both asserted.
    (1) The issue's 1e-5 relative -- fp32 coefficient rounding over at most 50 steps.  Relative to what: a coefficient c rounded
    to fp32 is off by 2^-24 |c|, which moves the state by 2^-24 |c z| -- the size of the TERM, not of the sum.  A noise block that
    starts at alpha_T ~ 0.003 (precision 1e-5) has cz = alpha_s / alpha_t up to ~300 and a c0 e that cancels it: no fp32 triple can
    hold the end point to 1e-5 of ITS size there (one step T -> 0 at T = 100: 1.96e-5 abs on values of ~1, i.e. 2e-8 of the
    316 |z| term).  So the 1e-5 is measured against the largest term of the run; for an endpoint block, whose terms are no larger
    than the state, that is the size of the result.
    (2) The forward error bound of that rounding, worked out for the plan at hand: every step adds 2^-24 of each of its terms
    and multiplies what the steps before it left by its |cz|.  It is the worst case of the only error source there is (the
    evaluation is fp64, the coefficients are float64 values cast once), so nothing correct can exceed it, and it is one to two
    orders below (1) for the noise blocks: 1.4e-5 seen against 1.1e-4 allowed at T = 24, N = 6, where (1) allows 1.6e-3."""
    gamma = O.gamma_table(T, 1e-5)
    lv = S.level_plan(T, N, spacing, gamma_table=gamma)
    dd = {k: v.double() for k, v in S.strided_coefficients(gamma, T, lv, 0.0).items()}
    for ep in (False, True):
        def ddim(i, z, x0, e):
            if ep:
                return dd["ep_zt"][i], (dd["ep_zt"][i] * z, dd["ep_pred"][i] * x0)
            return 1.0 / dd["alpha_t_given_s"][i], (z / dd["alpha_t_given_s"][i], -dd["var_terms"][i] * e)
        ms = {k: v.double() for k, v in S.multistep_coefficients(gamma, T, lv, ep, ep).items()}

        def multistep(i, z, x0, e):
            o = x0 if ep else e
            return ms["cz_x"][i], (ms["cz_x"][i] * z, ms["c0_x"][i] * o, ms["c1_x"][i] * o)      # (a consistent network: o_prev = o)
        for name, step in (("ddim", ddim), ("multistep", multistep)):
            z, want, scale, bound = consistent_end(gamma, T, lv, step)
            err = float((z - want).abs().max())
            print(f"T {T} N {N} {spacing} ep {ep}: {name} error {err:.3g}, rounding bound {bound:.3g}, largest term {scale:.3g}")
            assert err <= 1e-5 * scale, (name, ep)
            assert err <= bound, (name, ep, err, bound)
            if ep and name == "ddim":                      # (an endpoint block's first-order terms are no larger than the state)
                assert scale <= 1.5 * float(want.abs().max())


# ---- multistep coefficients ----
@pytest.mark.parametrize("ep_coord,ep_feat", [(False, False), (True, False), (True, True)])
def test_multistep_coefficients(ep_coord, ep_feat):
    T = 100
    gamma = O.gamma_table(T, 1e-5)
    for N in (1, 2, 3, 10):
        lv = S.level_plan(T, N, "quadratic")
        ms = S.multistep_coefficients(gamma, T, lv, ep_coord, ep_feat)
        assert set(ms) == {"t", "cz_x", "c0_x", "c1_x", "cz_h", "c0_h", "c1_h"} and all(v.dtype == torch.float32 and v.shape == (N,) for v in ms.values())
        for blk in ("x", "h"):
            c1 = ms[f"c1_{blk}"]
            assert float(c1[0]) == 0.0 and float(c1[-1]) == 0.0 and not bool(torch.signbit(c1[0])) and not bool(torch.signbit(c1[-1]))
            assert bool((c1[1:-1] != 0).all())
        assert torch.equal(ms["t"], torch.tensor(lv[:-1]).float() / T)
        for i in range(N):                                  # against fewstep_ref's own formulas
            for blk, ep in (("x", ep_coord), ("h", ep_feat)):
                ref = F.ms_coef(gamma, T, lv[i - 1] if i else None, lv[i], lv[i + 1], ep)
                for name, r in zip(("cz", "c0", "c1"), ref):
                    assert abs(float(ms[f"{name}_{blk}"][i]) - float(r)) <= 1e-6 * max(abs(float(r)), 1e-3), (N, i, blk, name)
        arr = pfa.PfEngine.ms_coef_array(ms)
        assert len(arr) == N and arr[0].t == float(ms["t"][0]) and arr[N - 1].c0_h == float(ms["c0_h"][N - 1])
    # the first step is the eta = 0 DDIM step, to fp32 rounding (two fp32 coefficient sets applied in fp64 to random z, o)
    lv = S.level_plan(T, 10)
    ms = {k: v.double() for k, v in S.multistep_coefficients(gamma, T, lv, ep_coord, ep_feat).items()}
    dd = {k: v.double() for k, v in S.strided_coefficients(gamma, T, lv, 0.0).items()}
    gen = torch.Generator().manual_seed(3)
    z, o = torch.randn(50, generator=gen, dtype=torch.float64), torch.randn(50, generator=gen, dtype=torch.float64)
    for blk, ep in (("x", ep_coord), ("h", ep_feat)):
        a = ms[f"cz_{blk}"][0] * z + ms[f"c0_{blk}"][0] * o
        b = dd["ep_zt"][0] * z + dd["ep_pred"][0] * o if ep else z / dd["alpha_t_given_s"][0] - dd["var_terms"][0] * o
        scale = float(max(ms[f"cz_{blk}"][0].abs(), ms[f"c0_{blk}"][0].abs()))
        assert float((a - b).abs().max()) <= 1e-6 * scale * float(max(z.abs().max(), o.abs().max())), blk


# ---- the model's keywords ----
def test_model_value_errors_and_arrays():
    T = 12
    m = make_model(T)
    g = pocket(3, 1)
    sd3 = (torch.zeros(3, 3), torch.tensor([0, 1, 2]))
    pin = [(torch.zeros(1, 3), torch.tensor([0]), None)]
    restr = [[("repel", None, [0.0, 0.0, 0.0], 3.0, 1.0)]]
    cases = [(dict(sample_steps=4, sampler="multistep", pinned=pin), "composes with seeds only"),
             (dict(sample_steps=4, sampler="multistep", restraints=restr), "composes with seeds only"),
             (dict(sample_steps=4, sampler="multistep", seeds=[sd3], seed_level=6, seed_keep=[[0]]), "composes with seeds only"),
             (dict(sample_steps=4, sampler="multistep", eta=0.0), "takes no eta"),
             (dict(sample_steps=4, pinned=pin, pin_resamples=2), "pin_resamples > 1"),
             (dict(sample_steps=4, sampler="euler"), "sampler must be"),
             (dict(sample_steps=4, spacing="cosine"), "spacing must be"),
             (dict(sample_steps=4, sampler="ddim", eta=1.5), "eta must lie"),
             (dict(sample_steps=4, sampler="ancestral", eta=0.5), "is eta = 1"),
             (dict(sample_steps=0), "1 <= sample_steps <= 12"),
             (dict(sample_steps=13), "1 <= sample_steps <= 12"),
             (dict(sample_steps=7, seeds=[sd3], seed_level=6), "1 <= sample_steps <= 6"),
             (dict(sampler="ddim"), "pass sample_steps"),
             (dict(eta=0.0), "pass sample_steps"),
             (dict(spacing="uniform"), "pass sample_steps")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            m.sample([g], [[3]], **kw)
        if "pinned" not in kw:
            kw = dict(kw)
            if "restraints" in kw:
                kw["restraints"] = restr
            with pytest.raises(ValueError, match=msg):
                m.sample_given_receptor(g, **kw)
    with pytest.raises(ValueError, match=r"ddim run of 4 steps needs 5 noise row\(s\), got 13"):
        m.sample_given_receptor(g, noise=torch.zeros(13, 3, 9), sample_steps=4, sampler="ddim")
    with pytest.raises(ValueError, match=r"multistep run of 4 steps needs 1 noise row\(s\), got 5"):
        m.sample_given_receptor(g, noise=torch.zeros(5, 3, 9), sample_steps=4, sampler="multistep")
    # the arrays are keyed by the plan
    few = m._fewstep(4, "ddim", 0.5, "quadratic")
    assert few == (4, "ddim", 0.5, "quadratic") and m._fewstep(4, None, None, None) == (4, "ancestral", 1.0, "uniform")
    assert m._fewstep(None, None, None, None) is None and m._fewstep(4, "ddim", None, None)[2] == 0.0
    lv = m._fewstep_arrays("levels", few)
    assert lv == S.level_plan(T, 4, "quadratic")
    arr = m._fewstep_arrays("coef", few)
    assert arr is m._fewstep_arrays("coef", few) and arr is not m._fewstep_arrays("coef", (4, "ddim", 0.0, "quadratic"))
    assert bytes(arr) == bytes(pfa.PfEngine.coef_array(S.strided_coefficients(m.gamma.gamma, T, lv, 0.5), range(4)))
    assert bytes(m._fewstep_arrays("pin", few)) == bytes(pfa.PfEngine.pin_coef_array(S.pin_coefficients(m.gamma.gamma, T, lv), range(4)))
    assert bytes(m._fewstep_arrays("guide", few)) == bytes(pfa.PfEngine.guide_coef_array(S.guide_coefficients(m.gamma.gamma, T, lv), range(4)))
    ms = m._fewstep_arrays("ms", (4, "multistep", 0.0, "uniform"), top=6)
    assert len(ms) == 4 and ms[0].t == 6 / T and ms[0].c1_x == 0.0 and ms[1].c1_x != 0.0 and ms[3].c1_h == 0.0
    full = (T, "ancestral", 1.0, "uniform")                 # every level: the default run's arrays
    assert bytes(m._fewstep_arrays("coef", full)) == bytes(m._step_arrays("coef"))


def test_cli_flags(capsys):
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]
    a = cli.parse_arguments(base)
    assert a.sample_steps is None and a.sampler is None and a.eta is None and a.spacing is None
    a = cli.parse_arguments(base + ["--sample_steps", "6", "--sampler", "multistep", "--spacing", "logsnr"])
    assert (a.sample_steps, a.sampler, a.eta, a.spacing) == (6, "multistep", None, "logsnr")
    a = cli.parse_arguments(base + ["--sample_steps", "6", "--sampler", "ddim", "--eta", "0.5"])
    assert a.eta == 0.5
    for extra, msg in ((["--sampler", "ddim"], "--sampler needs --sample_steps"),
                       (["--eta", "0.5"], "--eta needs --sample_steps"),
                       (["--spacing", "uniform"], "--spacing needs --sample_steps"),
                       (["--sample_steps", "0"], "--sample_steps must be at least 1"),
                       (["--sample_steps", "4", "--eta", "0.5"], "--eta needs --sampler ddim"),
                       (["--sample_steps", "4", "--sampler", "ddim", "--eta", "2"], "--eta must lie in 0..1"),
                       (["--sample_steps", "4", "--sampler", "multistep", "--restraints", "r.txt"], "composes with --seed_pharmacophore only")):
        with pytest.raises(SystemExit) as e:
            cli.parse_arguments(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    import importlib.util
    spec = importlib.util.spec_from_file_location("pf_test_cli", os.path.join(ROOT, "test.py"))     # (`test` is also a stdlib package)
    test_cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(test_cli)
    t = test_cli.parse_arguments(["--model_dir", "run", "--sample_steps", "20", "--sampler", "ddim", "--eta", "0.2", "--spacing", "quadratic"])
    assert (t.sample_steps, t.sampler, t.eta, t.spacing) == (20, "ddim", 0.2, "quadratic")
    with pytest.raises(ValueError, match="need --sample_steps"):
        test_cli.parse_arguments(["--model_dir", "run", "--sampler", "ddim"])
