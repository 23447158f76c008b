"""The tuned family's input gradients without a GPU: the two 128 / 16 cases the GPU test adds to input_grad_ref.CASES calibrated and
proved on the CPU oracle alone, the library's new switch, and guide_family's validation in Python and in the CLI parser.

The cases live here, next to input_grad_ref.CASES (tests/test_gpu_input_grads_tuned.py reads them through ``case``):
  deep 128/16                         four conv layers, 9 centers, 96 atoms
  single_layer_single_center 128/16   one conv layer, 4 centers in graphs of one or two
Calibration as in tests/test_input_grad_host.py: a held-out fp32 draw of the reference within grad_budget.CALIBRATION_RATIO (4)
units of the fp64 input gradients in every center row; two wrong input gradients (the rbf path lost, the direction path lost)
outside helpers.BUDGET_FACTOR (8) in at least one row.  Nothing here comes from a kernel."""
import ctypes
import functools

import pytest
import torch

from oracle import pf_oracle as O
import grad_budget as G
import input_grad_ref as R
from helpers import BUDGET_FACTOR
from test_input_grad_host import P_DROP, DROP_SEED, _no_direction_path, _no_rbf_path

# name -> (builder, live head), as input_grad_ref.CASES
TUNED_CASES = {
    "deep 128/16": (lambda: G.build_case("deep", 128, 16), True),
    "single_layer_single_center 128/16": (lambda: G.build_case("single_layer_single_center", 128, 16), True),
}
assert not set(TUNED_CASES) & set(R.CASES)
_ORACLE = (O.rbf, O.gvp_chain)
_REFS = {}


@functools.lru_cache(maxsize=None)
def case(name):
    """a case of input_grad_ref.CASES or of TUNED_CASES"""
    return R.case(name) if name in R.CASES else TUNED_CASES[name][0]()


def live_head(name):
    return (R.CASES[name] if name in R.CASES else TUNED_CASES[name])[1]


def refs(name):
    """(case, masks, draws32, (g_x64, g_h64), eps_x32): computed once and left unchanged"""
    if name not in _REFS:
        c = case(name)
        drop = O.dropout_masks(c.cfg, int(c.batch.pharm_ptr[-1]), int(c.batch.prot_ptr[-1]), P_DROP, DROP_SEED)
        draws, g64, (_, ox) = R.reference_draws(c, drop)
        _REFS[name] = (c, drop, draws, g64, ox)
    return _REFS[name]


def test_the_cases_are_what_they_say():
    deep, single = case("deep 128/16"), case("single_layer_single_center 128/16")
    for c in (deep, single):
        assert (c.cfg.n_hidden_scalars, c.cfg.vector_size) == (128, 16)
    assert deep.cfg.n_convs == 4 and int(deep.batch.pharm_ptr[-1]) == 9 and int(deep.batch.prot_ptr[-1]) == 96
    assert single.cfg.n_convs == 1 and int(single.batch.pharm_ptr[-1]) == 4


@pytest.mark.parametrize("name", list(TUNED_CASES))
def test_held_out_reference_draw_is_within_half_the_budget(name):
    c, drop, draws, g64, ox = refs(name)
    assert len(draws) == G.K_DRAWS
    assert float(ox.abs().max()) >= 0.25                          # the live head: eps_x counts
    hx, hh = R.draw(c, drop, G.HELD_OUT)
    wx, wh = R.rows_within_budget(hx, hh, draws, g64, f"held-out draw {name}", factor=G.CALIBRATION_RATIO)
    assert wx <= G.CALIBRATION_RATIO and wh <= G.CALIBRATION_RATIO


@pytest.mark.parametrize("mutant", [_no_rbf_path, _no_direction_path])
@pytest.mark.parametrize("name", list(TUNED_CASES))
def test_mutants_fall_outside_the_budget(name, mutant):
    c, drop, draws, g64, _ = refs(name)
    with mutant():
        mx, mh, _, _ = R.oracle_input_gradients(c, drop)
    wx, wh = R.rows_within_budget(mx, mh, draws, g64, f"{mutant.__name__} {name}", check=False)
    assert max(wx, wh) > BUDGET_FACTOR, (name, mutant.__name__, wx, wh)
    with pytest.raises(AssertionError, match="outside|exactly zero"):
        R.rows_within_budget(mx, mh, draws, g64, f"{mutant.__name__} {name}")
    assert O.rbf is _ORACLE[0] and O.gvp_chain is _ORACLE[1]     # the oracle is restored


def test_library_exports_the_switch():
    import pharmacoforge_amd as pfa
    assert "pf_train_set_input_grads" in pfa._lib.SYMBOLS and "pf_train_get_input_grads" in pfa._lib.SYMBOLS
    lib = pfa._lib.load()
    out = ctypes.c_int32(7)
    assert lib.pf_train_set_input_grads(None, 1) == -1            # PF_ERR_ARG: a NULL handle
    assert lib.pf_train_set_input_grads(None, 0) == -1
    assert lib.pf_train_get_input_grads(None, ctypes.byref(out)) == -1 and out.value == 7


class _Cfg:
    def __init__(self, S, V):
        self.n_hidden_scalars, self.vector_size = S, V


def test_engine_validates_guide_family_before_any_call():
    """PfEngine._check_guide_family needs the configuration only: an engine object that was never created on a device"""
    import pharmacoforge_amd as pfa
    eng = object.__new__(pfa.PfEngine)
    eng.cfg = _Cfg(128, 16)
    assert eng._check_guide_family("wide") == "wide" and eng._check_guide_family("tuned") == "tuned"
    for bad in ("fast", None, "", "Tuned"):
        with pytest.raises(ValueError, match="guide_family must be 'wide' or 'tuned'"):
            eng._check_guide_family(bad)
    eng.cfg = _Cfg(64, 32)
    assert eng._check_guide_family("wide") == "wide"
    with pytest.raises(ValueError, match="128 / vector_size 16"):
        eng._check_guide_family("tuned")
    # sample() and sample_begin() check it first: no library handle exists on this object
    with pytest.raises(ValueError, match="128 / vector_size 16"):
        eng.sample(None, 1, None, restraints=[None], pin_coef_arr=[], guide_coef_arr=[], guide_family="tuned")
    with pytest.raises(ValueError, match="guide_family must be"):
        eng.sample(None, 1, None, guide_family="quick")
    with pytest.raises(ValueError, match="128 / vector_size 16"):
        eng.sample_begin(None, restraints=[None], guide_family="tuned")
    eng.cfg = _Cfg(128, 16)
    with pytest.raises(ValueError, match="guided runs"):
        eng.sample_begin(None, guide_family="tuned")
    eng._h = None                                                 # (what __del__ looks at)


def _model(S, V):
    import pharmacoforge_amd as pfa
    from test_host_logic import DEV_DYN, DEV_GRAPH
    return pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=8, graph_config=DEV_GRAPH,
                                 dynamics_config={**DEV_DYN, "n_hidden_scalars": S, "vector_size": V}, precision=1e-5)


def test_model_validates_guide_family_before_any_device_work():
    m128, m64 = _model(128, 16), _model(64, 32)
    assert m128._check_guide_family("tuned") == "tuned" and m64._check_guide_family("wide") == "wide"
    with pytest.raises(ValueError, match="guide_family must be"):
        m128._check_guide_family("both")
    with pytest.raises(ValueError, match="128 / vector_size 16"):
        m64._check_guide_family("tuned")
    with pytest.raises(ValueError, match="128 / vector_size 16"):
        m64.sample([], [], guide_family="tuned")
    with pytest.raises(ValueError, match="guide_family must be"):
        m128.sample([], [], guide_family="quick")
    assert m128.sample([], [], guide_family="tuned") == []        # valid, and nothing to do


def _cli(argv):
    import generate_pharmacophores as cli
    return cli.parse_arguments(argv)


def test_cli_parser_knows_guide_family(tmp_path, capsys):
    restr = tmp_path / "r.txt"
    restr.write_text("attract 0 0 0 2.0 1.0 *\n")
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]
    assert _cli(base + ["--restraints", str(restr)]).guide_family == "wide"
    assert _cli(base + ["--restraints", str(restr), "--guide_family", "tuned"]).guide_family == "tuned"
    assert _cli(base).guide_family == "wide"
    for bad in (["--guide_family", "tuned"], ["--restraints", str(restr), "--guide_family", "fast"]):
        with pytest.raises(SystemExit):
            _cli(base + bad)
        assert "guide_family" in capsys.readouterr().err
