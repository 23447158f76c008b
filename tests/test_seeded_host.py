"""Host side of seeded sampling (pf_sample_seed_next): the seed coefficients against an fp64 evaluation, the argument rules of
the model and the command line -- and the conditions the GPU tests (test_gpu_seeded.py) put on their own inputs, checked here on
the CPU: the composition of tests/seeded_ref.py evaluated in fp64 and in fp32 agrees with itself to a tenth of the trajectory
tolerance, and a seed that was not applied moves every center of every multi-center graph by far more than that tolerance.
No GPU."""
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
import seeded_ref as R  # noqa: E402
from test_host_logic import make_model  # noqa: E402

S = pfa.schedule
LEVELS = (4, 9, 16, 24)


@pytest.mark.parametrize("T,prec", [(24, 0.25), (500, 1e-5)])
def test_seed_coefficients_against_fp64(T, prec):
    """alpha_a / sigma_a are the fp32 alpha / sigma of gamma(a / T): against alpha^2 = sigmoid(-gamma), sigma^2 = sigmoid(gamma)
    in fp64 on the fp32 table, and equal to the reference composition's own pair.  The bound, 1e-6 relative, is a few fp32 ulps
    of sqrt(sigmoid(.)) (each of the two roundings is half an ulp of 6e-8 relative, plus the hardware-independent libm error)."""
    gamma = O.gamma_table(T, prec)
    g64 = gamma.double()
    for a in sorted({1, 2, T // 2, T - 1, T}):
        c = S.seed_coefficients(gamma, T, a)
        assert c["alpha_a"].dtype == torch.float32 and c["alpha_a"].shape == () and c["sigma_a"].shape == ()
        al64, sg64 = torch.sqrt(torch.sigmoid(-g64[a])), torch.sqrt(torch.sigmoid(g64[a]))
        assert float((c["alpha_a"].double() - al64).abs() / al64) <= 1e-6, (T, a)
        assert float((c["sigma_a"].double() - sg64).abs() / sg64) <= 1e-6, (T, a)
        ra, rs = R.seed_coef(gamma, T, a)
        assert float(ra) == float(c["alpha_a"]) and float(rs) == float(c["sigma_a"])
        st = pfa.PfEngine.seed_coef_struct(c)
        assert st.alpha_a == float(c["alpha_a"]) and st.sigma_a == float(c["sigma_a"])
    # level a is the level t of step s = a - 1: the guided step's coefficients of that step
    gc = S.guide_coefficients(gamma, T)
    c = S.seed_coefficients(gamma, T, 3)
    assert float(c["alpha_a"]) == float(gc["alpha_t"][2]) and float(c["sigma_a"]) == float(gc["sigma_t"][2])
    for bad in (0, -1, T + 1):
        with pytest.raises(ValueError, match="seed level"):
            S.seed_coefficients(gamma, T, bad)


def pocket(n=3, seed=1):
    b = O.synthetic_batch([seed], 20, n, O.DynamicsConfig())
    return pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, torch.zeros(n, 3), torch.zeros(n, 6))


def test_value_errors():
    m = make_model(12)
    g, g2 = pocket(3, 1), pocket(4, 2)
    sd3 = (torch.zeros(3, 3), torch.tensor([0, 1, 2]))
    sd4 = (torch.zeros(4, 3), torch.tensor([0, 1, 2, 3]))
    with pytest.raises(ValueError, match="pocket 1 has no seed"):
        m.sample([g, g2], [[3], [4]], seeds=[sd3, None], seed_level=4)
    with pytest.raises(ValueError, match="pocket 0 has no seed"):
        m.sample([g, g2], [[3], [4]], seeds=[None, None], seed_level=4)
    with pytest.raises(ValueError, match=r"pocket 1: the seed has 4 centers but sizes \[5\]"):
        m.sample([g, g2], [[3, 3], [4, 5]], seeds=[sd3, sd4], seed_level=4)
    with pytest.raises(ValueError, match="go together"):
        m.sample([g], [[3]], seeds=[sd3])
    with pytest.raises(ValueError, match="go together"):
        m.sample([g], [[3]], seed_level=4)
    with pytest.raises(ValueError, match="seed_keep without seeds"):
        m.sample([g], [[3]], seed_keep=[[0]])
    with pytest.raises(ValueError, match="use seed_keep"):
        m.sample([g], [[3]], seeds=[sd3], seed_level=4, pinned=[(torch.zeros(1, 3), torch.tensor([0]), None)])
    for bad in (0, 13):
        with pytest.raises(ValueError, match="1 <= seed_level <= 12"):
            m.sample([g], [[3]], seeds=[sd3], seed_level=bad)
    with pytest.raises(ValueError, match="seed_keep names center 3"):
        m.sample([g], [[3]], seeds=[sd3], seed_level=4, seed_keep=[[0, 3]])
    with pytest.raises(ValueError, match="seed types"):
        m.sample([g], [[3]], seeds=[(torch.zeros(3, 3), torch.tensor([0, 1, 6]))], seed_level=4)
    with pytest.raises(ValueError, match="seeds lists 1 entries for 2 pockets"):
        m.sample([g, g2], [[3], [4]], seeds=[sd3], seed_level=4)
    # sample_given_receptor has the same keywords and rules
    with pytest.raises(ValueError, match="go together"):
        m.sample_given_receptor(g, seeds=[sd3])
    with pytest.raises(ValueError, match="go together"):
        m.sample_given_receptor(g, seed_level=4)
    with pytest.raises(ValueError, match="pocket 0 has no seed"):
        m.sample_given_receptor(g, seeds=[None], seed_level=4)
    with pytest.raises(ValueError, match="the seed has 4 centers but a pharmacophore of 3"):
        m.sample_given_receptor(g, seeds=[sd4], seed_level=4)
    # the noise of a seeded batch has n_ops + 1 rows: a + 1 without resampling, the plan of (a, jump, resamples) + 1 with it
    with pytest.raises(ValueError, match=r"seeded run of 4 ops \(seed level 4\) needs 5 noise rows, got 13"):
        m.sample_given_receptor(g, noise=torch.zeros(13, 3, 9), seeds=[sd3], seed_level=4)
    n_ops = len(S.resample_plan(9, 4, 2))
    assert n_ops == 21
    with pytest.raises(ValueError, match=r"21 ops.*22 noise rows, got 10"):
        m.sample_given_receptor(g, noise=torch.zeros(10, 3, 9), seeds=[sd3], seed_level=9, seed_keep=[[1]], pin_resamples=2, pin_jump=4)


def test_model_arrays():
    """Without seeds the model builds today's arrays; a seeded run's arrays are the last a entries of them, and its plan is
    resample_plan(a, jump, resamples) -- cached by its top level."""
    T = 50
    m = make_model(T)
    order = list(reversed(range(T)))
    full = {"coef": pfa.PfEngine.coef_array(m.step_coefficients(), order),
            "pin": pfa.PfEngine.pin_coef_array(S.pin_coefficients(m.gamma.gamma, T), order),
            "guide": pfa.PfEngine.guide_coef_array(S.guide_coefficients(m.gamma.gamma, T), order)}
    for name, arr in full.items():
        assert bytes(m._step_arrays(name)) == bytes(arr) and m._step_arrays(name) is m._step_arrays(name, T)
        for a in (1, 7, 49):
            got = m._step_arrays(name, a)
            assert len(got) == a and bytes(got) == bytes(arr)[len(bytes(arr)) // T * (T - a):]
            assert got is m._step_arrays(name, a)
    n_ops, arr, parr, op_arr, re_arr = m._plan_arrays(10, 1)
    assert n_ops == T and bytes(arr) == bytes(full["coef"]) and bytes(parr) == bytes(full["pin"])
    assert m._plan_arrays(10, 1) is m._plan_arrays(10, 1, T)
    n_ops, arr, parr, op_arr, re_arr = m._plan_arrays(4, 2, 9)
    plan = S.resample_plan(9, 4, 2)
    assert n_ops == len(plan) == 21 and list(op_arr) == [int(op[0] == "renoise") for op in plan]
    assert arr[0].t == full["coef"][T - 9].t and plan[0] == ("denoise", 8)
    assert m._plan_arrays(4, 2, 9) is not m._plan_arrays(4, 2)
    # the seed rides on the pin fields: values for all centers, seed_keep as the flags
    g = pocket(3, 1)
    x = torch.arange(9.0).reshape(3, 3)
    out = m._with_seeds([g], [[3, 3]], [(x, torch.tensor([5, 0, 2]))], [[2]])
    assert out[0].pharm_pin.tolist() == [0, 0, 3] and torch.equal(out[0].pharm_pin_x, x)
    assert out[0].pharm_pin_h.argmax(dim=1).tolist() == [5, 0, 2] and out[0].pharm_pin_h.sum().item() == 3
    assert m._with_seeds([g], [[3]], [(x, torch.tensor([5, 0, 2]))], None)[0].pharm_pin.tolist() == [0, 0, 0]


def test_cli_seed_rules(tmp_path, capsys):
    f = tmp_path / "seed.xyz"
    f.write_text("3\nP 0.000 1.000 2.000\nC 1.000 1.000 1.000\nN 2.000 0.500 1.000\n")
    pins = tmp_path / "pins.xyz"
    pins.write_text("1\nP 0.000 1.000 2.000\n")
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]
    a = cli.parse_arguments(base)
    assert a.seed_centers is None and a.seed == 42 and a.seed_level is None and a.seed_keep_list is None
    a = cli.parse_arguments(base + ["--seed_pharmacophore", str(f), "--seed_level", "7"])
    assert a.seed_level == 7 and a.seed_keep_list is None and a.seed_centers[0].shape == (3, 3) and len(a.seed_centers[1]) == 3
    a = cli.parse_arguments(base + ["--seed_pharmacophore", str(f), "--seed_level", "7", "--seed_keep", "0,2", "--samples_per_pocket", "2",
                                    "--pharm_sizes", "3", "3", "--pin_resamples", "2"])
    assert a.seed_keep_list == [0, 2] and a.pharm_sizes == [3, 3] and a.pin_resamples == 2
    for extra, msg in ((["--seed_level", "4"], "--seed_level needs --seed_pharmacophore"),
                       (["--seed_keep", "0"], "--seed_keep needs --seed_pharmacophore"),
                       (["--seed_pharmacophore", str(f)], "--seed_pharmacophore needs --seed_level"),
                       (["--seed_pharmacophore", str(f), "--seed_level", "0"], "--seed_level must be at least 1"),
                       (["--seed_pharmacophore", str(f), "--seed_level", "4", "--pinned_centers", str(pins)], "use --seed_keep"),
                       (["--seed_pharmacophore", str(f), "--seed_level", "4", "--pharm_sizes", "4"], "differ from the 3 centers"),
                       (["--seed_pharmacophore", str(f), "--seed_level", "4", "--seed_keep", "0,3"], "outside the 3 centers"),
                       (["--seed_pharmacophore", str(f), "--seed_level", "4", "--seed_keep", "a"], "comma-separated"),
                       (["--seed_pharmacophore", str(f), "--seed_level", "4", "--pin_resamples", "2"], "--pin_resamples needs --pinned_centers")):
        with pytest.raises(SystemExit) as e:            # an argparse error: usage + message on stderr, exit status 2
            cli.parse_arguments(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra


def test_unseeded_composition_is_the_resampled_reference():
    """seeded_ref's loop without a seed, on the full plan, gives resample_ref.resampled_reference's outputs exactly: the begin
    lines are the only difference between the two references."""
    from resample_ref import case, resampled_reference
    cfg, sd, batch, plan, noise, pins, com = case()
    n_t = 6
    ops = R.plan_of(n_t, 4, 2)
    want = resampled_reference(sd, cfg, batch, n_t, R.PREC, ops, noise, *pins, com, fnorm=2.0)
    got = R.seeded_reference(sd, cfg, batch, n_t, R.PREC, n_t, ops, noise, None, pins, com, fnorm=2.0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# measured here (fp32 against fp64 composition, worst |difference| over x_0 and h_0, recorded and live head, a = 4 / 9 / 16 / 24):
# at most 3.3e-6 -- test_gpu_seeded.py's docstrings quote it
PRECONDITION = 5e-4


@pytest.mark.parametrize("live", [False, True], ids=["recorded", "live"])
@pytest.mark.parametrize("a", LEVELS)
def test_reference_conditions(a, live):
    """Conditions on the GPU tests' inputs.  (1) The composition in fp64 and in fp32 agree within 5e-4 -- the bound
    test_guidance_host.py demands, a tenth of the trajectory tolerance.  (2) The seeded and the unseeded run of the same steps
    differ by more than 0.1 A on every center of every multi-center graph (a single-center graph's center is its COM, which the
    sampler removes: it sits where the frame puts it, seeded or not), so the GPU tolerance of 5e-3 discriminates a seed that was
    not applied.  The distances to the seed are printed, not asserted."""
    cfg, sd, batch, noise, seed, pins, com = R.seeded_case()
    r32, r64 = R.reference(a, live=live), R.reference(a, live=live, double=True)
    d = max(float((p.double() - q).abs().max()) for p, q in zip(r32, r64))
    un = R.reference(a, live=live, seeded=False)
    sizes = (batch.pharm_ptr[1:] - batch.pharm_ptr[:-1])
    multi = (sizes > 1)[batch.batch_idxs()["pharm"]]
    moved = (r32[0] - un[0]).norm(dim=1)[multi]
    to_seed = (r32[0] - seed[0]).norm(dim=1)
    print(f"a {a} live {live}: fp32 against fp64 {d:.3e}; seeded against unseeded x_0: min {float(moved.min()):.3f} mean {float(moved.mean()):.3f} A; "
          f"distance to the seed: mean {float(to_seed.mean()):.3f} max {float(to_seed.max()):.3f} A")
    assert r64[2].shape == (a + 1, 23, 3) and r64[3].shape == (a + 1, 23, 6)
    assert d <= PRECONDITION
    assert int(multi.sum()) == 22 and float(moved.min()) > 0.1
