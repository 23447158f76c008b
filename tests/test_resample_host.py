"""Host side of pinned runs with resampling jumps: the plan, the coefficient arrays, the re-noise coefficients against an fp64
evaluation, the argument rules of the model and the command line -- and the conditions the GPU tests (test_gpu_resample.py) put
on their own inputs, checked here on the CPU: the composition of tests/resample_ref.py reproduces `pinned_reference` without
resampling, and evaluated in fp64 and in fp32 it agrees with itself to a tenth of the trajectory tolerance.  No GPU."""
import dataclasses
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
import resample_ref as R  # noqa: E402
from test_host_logic import make_model  # noqa: E402

S = pfa.schedule


def D(*ss):
    return [("denoise", s) for s in ss]


def test_plan_is_the_one_written_out():
    assert S.resample_plan(7, 3, 2) == (D(6, 5, 4) + [("renoise", 4, 7)] + D(6, 5, 4)
                                        + D(3, 2, 1) + [("renoise", 1, 4)] + D(3, 2, 1)
                                        + D(0) + [("renoise", 0, 1)] + D(0))
    assert len(S.resample_plan(7, 3, 2)) == 17
    for T in (50, 500):
        for j in (1, 10, 600):
            assert S.resample_plan(T, j, 1) == D(*reversed(range(T))), (T, j)
    # the case of the GPU tests: segments of 5, 5, 5, 5, 4 levels, three passes each
    plan = S.resample_plan(R.T, R.JUMP, R.RESAMPLES)
    assert len(plan) == 82 and plan == R.plan_of(R.T, R.JUMP, R.RESAMPLES)
    assert [op[1:] for op in plan if op[0] == "renoise"] == [(19, 24)] * 2 + [(14, 19)] * 2 + [(9, 14)] * 2 + [(4, 9)] * 2 + [(0, 4)] * 2
    for T, j, r in ((7, 3, 2), (24, 5, 3), (50, 10, 4), (9, 20, 2)):
        assert S.resample_plan(T, j, r) == R.plan_of(T, j, r)


@pytest.mark.parametrize("T", [50, 500])
def test_without_resampling_the_model_builds_todays_arrays(T):
    m = make_model(T)
    order = list(reversed(range(T)))
    coef_arr = pfa.PfEngine.coef_array(m.step_coefficients(), order)
    pin_arr = pfa.PfEngine.pin_coef_array(S.pin_coefficients(m.gamma.gamma, T), order)
    for j in (1, 10, 600):
        n_ops, arr, parr, op_arr, re_arr = m._plan_arrays(j, 1)
        assert n_ops == T and len(arr) == T and len(parr) == T
        assert bytes(arr) == bytes(coef_arr) and bytes(parr) == bytes(pin_arr)
        assert list(op_arr) == [0] * T
    again = m._plan_arrays(600, 1)
    assert again is m._plan_arrays(600, 1)              # cached per (T, jump, resamples)
    n_ops, arr, parr, op_arr, re_arr = m._plan_arrays(10, 2)
    plan = S.resample_plan(T, 10, 2)
    assert n_ops == len(plan) == 2 * T + T // 10 and list(op_arr) == [int(op[0] == "renoise") for op in plan]
    i = plan.index(("renoise", T - 10, T))
    rc = S.renoise_coefficients(m.gamma.gamma, T, [(T - 10, T)])
    assert re_arr[i].alpha_t_given_s == float(rc["alpha_t_given_s"][0]) and re_arr[i].sigma_t_given_s == float(rc["sigma_t_given_s"][0])
    assert arr[i + 1].t == coef_arr[0].t and parr[i + 1].alpha_s == pin_arr[0].alpha_s      # D(T-1) follows the jump back to T


def segments(T, j):
    out, a = [], T
    while a > 0:
        out.append((max(a - j, 0), a))
        a = max(a - j, 0)
    return out


@pytest.mark.parametrize("prec", [1e-5, 0.25])
@pytest.mark.parametrize("T", [50, 500])
def test_renoise_coefficients_against_fp64(T, prec):
    """alpha_{a|b} alpha_b = alpha_a and alpha_{a|b}^2 sigma_b^2 + sigma_{a|b}^2 = sigma_a^2 with the levels' alpha / sigma
    evaluated in fp64 on the fp32 gamma table, each within 1e-5 relative: a handful of fp32 roundings."""
    gamma = O.gamma_table(T, prec)
    g64 = gamma.double()
    al64, sg64 = torch.sqrt(torch.sigmoid(-g64)), torch.sqrt(torch.sigmoid(g64))
    worst = [0.0, 0.0]
    for j in (1, 10):
        pairs = segments(T, j)
        assert pairs[0][1] == T and pairs[-1][0] == 0 and all(p[1] == q[0] for p, q in zip(pairs[1:], pairs[:-1]))
        rc = S.renoise_coefficients(gamma, T, pairs)
        assert rc["alpha_t_given_s"].dtype == torch.float32 and rc["alpha_t_given_s"].shape == (len(pairs),)
        for i, (b, a) in enumerate(pairs):
            a_ab, s_ab = rc["alpha_t_given_s"][i].double(), rc["sigma_t_given_s"][i].double()
            e_a = float((a_ab * al64[b] - al64[a]).abs() / al64[a])
            e_s = float((a_ab ** 2 * sg64[b] ** 2 + s_ab ** 2 - sg64[a] ** 2).abs() / sg64[a] ** 2)
            worst = [max(worst[0], e_a), max(worst[1], e_s)]
            assert e_a <= 1e-5 and e_s <= 1e-5, (T, prec, j, b, a, e_a, e_s)
            # the reference composition's own coefficients (the oracle's functions, one pair at a time) are these within the same
            # budget: torch's vectorised and scalar softplus / expm1 need not round alike, and a small sigma_{a|b}^2 is the
            # difference of two softplus values of order one
            ra, rs = R.renoise_coef(gamma, T, b, a)
            assert float((ra.double() - a_ab).abs() / a_ab) <= 1e-5
            assert float((rs.double() ** 2 - s_ab ** 2).abs() / sg64[a] ** 2) <= 1e-5
    print(f"T {T} precision {prec}: worst relative error alpha {worst[0]:.2e} sigma^2 {worst[1]:.2e}")
    arr = pfa.PfEngine.renoise_coef_array(rc)
    assert len(arr) == len(pairs) and arr[0].alpha_t_given_s == float(rc["alpha_t_given_s"][0])
    with pytest.raises(ValueError):
        S.renoise_coefficients(gamma, T, [(3, 3)])
    with pytest.raises(ValueError):
        S.renoise_coefficients(gamma, T, [(0, T + 1)])


def pinned_pocket():
    b = O.synthetic_batch([1], 20, 3, O.DynamicsConfig())
    g = pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, torch.zeros(3, 3), torch.zeros(3, 6))
    return dataclasses.replace(g, pharm_pin=torch.tensor([3, 0, 0], dtype=torch.int32), pharm_pin_x=torch.zeros(3, 3),
                               pharm_pin_h=torch.eye(6)[:3])


def test_value_errors():
    for bad in ((0, 2), (-1, 2), (3, 0), (3, -2)):
        with pytest.raises(ValueError):
            S.resample_plan(10, *bad)
    m = make_model(12)
    g = pinned_pocket()
    n_ops = len(S.resample_plan(12, 4, 2))
    assert n_ops == 27
    with pytest.raises(ValueError, match=r"27 ops.*28 noise rows, got 13"):       # T + 1 rows for a resampled batch
        m.sample_given_receptor(g, noise=torch.zeros(13, 3, 9), pin_resamples=2, pin_jump=4)
    for kw in ({"pin_resamples": 0}, {"pin_jump": 0}):
        with pytest.raises(ValueError, match="at least 1"):
            m.sample_given_receptor(g, noise=torch.zeros(13, 3, 9), **kw)
        with pytest.raises(ValueError, match="at least 1"):
            m.sample([g], [[3]], **kw)
    with pytest.raises(ValueError, match="needs pins"):
        pfa.PfEngine.sample(None, None, 3, torch.zeros(4, 3, 9), plan=(None, None))
    with pytest.raises(ValueError, match="expected"):
        pfa.PfEngine.plan_arrays([("noise", 1)], None, None, None)


def test_cli_resample_rules(tmp_path, capsys):
    f = tmp_path / "pins.xyz"
    f.write_text("2\nP 0.000 1.000 2.000\nC 1.000 1.000 1.000\n")
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]
    a = cli.parse_arguments(base)
    assert a.pin_resamples == 1 and a.pin_jump == 10
    a = cli.parse_arguments(base + ["--pinned_centers", str(f)])
    assert a.pin_resamples == 1 and a.pin_jump == 10
    a = cli.parse_arguments(base + ["--pinned_centers", str(f), "--pin_resamples", "4", "--pin_jump", "20"])
    assert a.pin_resamples == 4 and a.pin_jump == 20
    for extra, msg in ((["--pin_resamples", "2"], "--pin_resamples needs --pinned_centers"),
                       (["--pin_jump", "5"], "--pin_jump needs --pinned_centers"),
                       (["--pinned_centers", str(f), "--pin_resamples", "0"], "--pin_resamples must be at least 1"),
                       (["--pinned_centers", str(f), "--pin_jump", "-3"], "--pin_jump must be at least 1")):
        with pytest.raises(SystemExit) as e:            # an argparse error: usage + message on stderr, exit status 2
            cli.parse_arguments(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err


def test_composition_without_resampling_is_pinned_reference():
    """resamples = 1 through resample_ref's loop gives `pinned_reference`'s outputs exactly (both parameterisations)"""
    from test_gpu_pinned import pinned_reference
    cfg, sd, batch, _, noise, pins, com = R.case()
    n_t = 6
    plan = S.resample_plan(n_t, 4, 1)
    for ep in (False, True):
        want = pinned_reference(sd, cfg, batch, n_t, R.PREC, noise, *pins, com, fnorm=2.0, ep=ep)
        got = R.resampled_reference(sd, cfg, batch, n_t, R.PREC, plan, noise, *pins, com, fnorm=2.0, ep=ep)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


# measured (fp32 against fp64 composition, worst |difference| over all frames, x / h): noise parameterisation 4.1e-6 / 6.8e-6,
# endpoint 8.5e-7 / 6.1e-7, live head (k = 13) 9.2e-6 / 3.7e-6 -- test_gpu_resample.py's docstrings quote these
PRECONDITION = 5e-4


@pytest.mark.parametrize("ep,live", [(False, False), (True, False), (False, True)], ids=["noise", "endpoint", "live"])
def test_reference_agrees_with_itself_in_fp64(ep, live):
    """Condition on the GPU tests' inputs: the 82-op composition in fp64 and in fp32 agree within 5e-4 on every frame -- a tenth of
    the trajectory tolerance, so no edge decision flips inside the reference itself."""
    r32, r64 = R.reference(ep, live, False), R.reference(ep, live, True)
    ex = float((r32[2].double() - r64[2]).abs().max())
    eh = float((r32[3].double() - r64[3]).abs().max())
    print(f"fp32 against fp64 composition (ep {ep}, live {live}): frames x {ex:.3e} h {eh:.3e}")
    assert r64[2].shape == (83, 23, 3) and r64[3].shape == (83, 23, 6)
    assert ex <= PRECONDITION and eh <= PRECONDITION
    assert float((r32[0].double() - r64[0]).abs().max()) <= PRECONDITION and float((r32[1].double() - r64[1]).abs().max()) <= PRECONDITION


def test_op_alone_edge_sets_agree_in_fp64():
    """Condition of the op-alone GPU test: behind the two R(4 -> 9) ops on the initial draw, and behind the D(8) that follows, the
    fp32 and the fp64 composition's coordinates give identical ff / pf / fp edge sets (the edges are decided in fp32 on the
    rounded coordinates)."""
    from helpers import edge_set
    cfg, batch = R.case()[0], R.case()[2]
    r32, r64 = R.op_alone_reference(False), R.op_alone_reference(True)
    for k in (2, 3):
        e32 = O.build_dynamic_edges(cfg, batch, r32[k][0], r32[k][1])
        e64 = O.build_dynamic_edges(cfg, batch, r64[k][0].float(), r64[k][1].float())
        for et in ("ff", "pf", "fp"):
            assert edge_set(*e32[et]) == edge_set(*e64[et]), (k, et)
            assert e32[et][0].numel() > 0
    moved = O.build_dynamic_edges(cfg, batch, r32[3][0], r32[3][1])
    first = O.build_dynamic_edges(cfg, batch, r32[2][0], r32[2][1])
    assert edge_set(*moved["pf"]) != edge_set(*first["pf"])          # the two points of the GPU test check different sets
