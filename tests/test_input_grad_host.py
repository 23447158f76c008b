"""input_grad_ref.rows_within_budget calibrated and proved on the CPU oracle alone, and the library's new entry without a GPU.

Calibration: a held-out fp32 draw of the reference (permutation seed 4, in no unit) must sit within HALF the budget factor of
the fp64 input gradients in every center row of every case the GPU test runs.  With PF_INPUT_GRAD_CALIBRATION_FILE naming a file
the ratios are written there (profiles/input_grads/reference_calibration.txt).

Teeth: two wrong input gradients, restated on the oracle -- the rbf path of the edge geometry lost, the direction path lost --
must each put at least one row of every case outside the budget."""
import ctypes
import os

import pytest
import torch

from oracle import pf_oracle as O
import grad_budget as G
import input_grad_ref as R
from helpers import BUDGET_FACTOR

P_DROP, DROP_SEED = 0.1, 5
CALIBRATION_ROWS = {}
_REFS = {}
_ORACLE = (O.rbf, O.gvp_chain)


def refs(name):
    """(case, masks, draws32, (g_x64, g_h64)): computed once and left unchanged"""
    if name not in _REFS:
        c = R.case(name)
        drop = O.dropout_masks(c.cfg, int(c.batch.pharm_ptr[-1]), int(c.batch.prot_ptr[-1]), P_DROP, DROP_SEED)
        draws, g64, _ = R.reference_draws(c, drop)
        _REFS[name] = (c, drop, draws, g64)
    return _REFS[name]


def _write_calibration():
    out = os.environ.get("PF_INPUT_GRAD_CALIBRATION_FILE")
    if not out:
        return
    head = (f"Calibration of tests/input_grad_ref.py::rows_within_budget on the reference alone (tests/test_input_grad_host.py::\n"
            f"test_held_out_reference_draw_is_within_half_the_budget): per center row of g_x [Nf, 3] and of g_h [Nf, pharm_nf],\n"
            f"unit = max(max over K = {G.K_DRAWS} fp32 oracle draws of max|draw - g64|, 2**-22 max|g64[row]|), factor {BUDGET_FACTOR:g}.  A held-out\n"
            f"fp32 draw (permutation seed {G.HELD_OUT}) against the fp64 gradient, dropout {P_DROP}: every row ratio must be <= "
            f"{G.CALIBRATION_RATIO:g}.\nNothing here was measured on a GPU.\n\n")
    with open(out, "w") as f:
        f.write(head + "\n".join(CALIBRATION_ROWS[k] for k in sorted(CALIBRATION_ROWS)) + "\n")


@pytest.mark.parametrize("name", list(R.CASES))
def test_held_out_reference_draw_is_within_half_the_budget(name):
    c, drop, draws, g64 = refs(name)
    assert len(draws) == G.K_DRAWS
    hx, hh = R.draw(c, drop, G.HELD_OUT)
    wx, wh = R.rows_within_budget(hx, hh, draws, g64, f"held-out draw {name}", factor=G.CALIBRATION_RATIO)
    assert wx <= G.CALIBRATION_RATIO and wh <= G.CALIBRATION_RATIO
    # the mapping back is the right one: in fp64 the permuted case gives the same rows
    pc, pd = G.permuted_case(c, G.HELD_OUT, drop)
    px, ph, _, _ = R.oracle_input_gradients(pc, pd, fp64=True)
    perm = R.center_permutation(c, G.HELD_OUT)
    assert float((px - g64[0][perm]).abs().max()) <= 1e-10 * float(g64[0].abs().max())
    assert float((ph - g64[1][perm]).abs().max()) <= 1e-10 * float(g64[1].abs().max())
    rows = g64[0].abs().amax(dim=1)
    CALIBRATION_ROWS[name] = (f"{name}: {rows.numel()} centers, worst ratio g_x {wx:.2f} / g_h {wh:.2f}; row maxima of g_x "
                              f"{float(rows.min()):.1e} .. {float(rows.max()):.1e}")
    _write_calibration()


class _no_rbf_path:
    """O.rbf detaches its distance argument: dL/d(rbf) never reaches the coordinates"""
    def __enter__(self):
        self.orig = O.rbf
        O.rbf = lambda D, *a, **k: self.orig(D.detach(), *a, **k)

    def __exit__(self, *exc):
        O.rbf = self.orig


class _no_direction_path:
    """the normalised difference is detached where conv_layer hands it to the message chain (vector channel 0)"""
    def __enter__(self):
        self.orig = O.gvp_chain

        def chain(sd, prefix, n, s, v, *a, **k):
            if ".edge_message_fns." in prefix:
                v = torch.cat([v[:, :1].detach(), v[:, 1:]], dim=1)
            return self.orig(sd, prefix, n, s, v, *a, **k)
        O.gvp_chain = chain

    def __exit__(self, *exc):
        O.gvp_chain = self.orig


@pytest.mark.parametrize("mutant", [_no_rbf_path, _no_direction_path])
@pytest.mark.parametrize("name", list(R.CASES))
def test_mutants_fall_outside_the_budget(name, mutant):
    c, drop, draws, g64 = refs(name)
    with mutant():
        mx, mh, _, _ = R.oracle_input_gradients(c, drop)
    wx, wh = R.rows_within_budget(mx, mh, draws, g64, f"{mutant.__name__} {name}", check=False)
    assert max(wx, wh) > BUDGET_FACTOR, (name, mutant.__name__, wx, wh)
    with pytest.raises(AssertionError, match="outside|exactly zero"):
        R.rows_within_budget(mx, mh, draws, g64, f"{mutant.__name__} {name}")
    assert O.rbf is _ORACLE[0] and O.gvp_chain is _ORACLE[1]     # the oracle is restored


def test_library_exports_the_input_gradient_entry():
    import pharmacoforge_amd as pfa
    assert "pf_train_backward_inputs" in pfa._lib.SYMBOLS
    lib = pfa._lib.load()
    fn = lib.pf_train_backward_inputs
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert fn(None, p, p, p, p, p, None) == -1                   # PF_ERR_ARG: a NULL handle, output pointers given
    assert fn(None, p, p, p, None, None, None) == -1             # ... and as pf_train_backward
