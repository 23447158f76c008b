"""Conditions test_gpu_step_moves.py puts on its own inputs (tests/step_move_cases.py), checked here on the CPU: evaluated in fp64
and in fp32, each kind's composition agrees with itself on x_0, h_0 and every frame to a tenth of the GPU test's tolerance (5e-4 of
5e-3, as test_resample_host.py asks of its case), so no edge decision flips inside the reference itself; the guided case's energies
and shifts do too, its clip is active and its restraints move the centers.  No GPU."""
import pytest
import torch

import step_move_cases as M

PRECONDITION = 5e-4


def worst(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("kind", ["pinned_renoise", "seeded", "multistep"])
def test_reference_agrees_with_itself_in_fp64(kind):
    r32, r64 = M.reference(kind), M.reference(kind, True)
    Nf = sum(M.N_PHARM)
    assert r64[2].shape == (5, Nf, 3) and r64[3].shape == (5, Nf, 6)
    errs = [worst(a, b) for a, b in zip(r32, r64)]
    print(f"fp32 against fp64 composition ({kind}): x0 {errs[0]:.3e} h0 {errs[1]:.3e} frames x {errs[2]:.3e} h {errs[3]:.3e}")
    assert max(errs) <= PRECONDITION


def test_guided_reference_agrees_with_itself_in_fp64():
    c, sd, noise, pins, com, restraints = M.case()
    r32, r64 = M.reference("guided"), M.reference("guided", True)
    pairs = {"x0": (r32.x0, r64.x0), "h0": (r32.h0, r64.h0), "frames x": (r32.fx, r64.fx), "frames h": (r32.fh, r64.fh),
             "E": (r32.E, r64.E), "shift": (r32.shift, r64.shift)}
    errs = {k: worst(a, b) for k, (a, b) in pairs.items()}
    print("fp32 against fp64 composition (guided): " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"; E up to {float(r64.E.max()):.3g}")
    assert r64.fx.shape == (M.GUIDED_STEPS + 1, sum(M.N_PHARM), 3) and r64.E.shape == (M.GUIDED_STEPS, len(M.N_PHARM))
    assert max(errs.values()) <= PRECONDITION
    # the clip is active on some rows and idle on others; graph 2 has no restraints: exact zeros
    n = r64.shift.norm(dim=2)
    assert bool((n >= M.GUIDE_CLIP * (1 - 1e-6)).any()) and bool(((n > 0) & (n < 0.9 * M.GUIDE_CLIP)).any())
    assert float(n.max()) <= M.GUIDE_CLIP * (1 + 1e-6)
    ptr = c.batch.pharm_ptr.tolist()
    assert float(r32.shift[:, ptr[2]:ptr[3]].abs().max()) == 0.0 and float(r32.E[:, 2].abs().max()) == 0.0
    assert float(r32.shift[:, ptr[0] + 63].abs().max()) > 0      # the center of lane 63
    # the guidance is no rounding error of the pinned run
    import guidance_ref as G
    un = G.guided_reference(sd, c.cfg, c.batch, M.RUN_T, M.RUN_PREC, noise, *pins, com, None, n_steps=M.GUIDED_STEPS)
    free = (pins[0] & 1) == 0
    free[ptr[1]:] = False                                        # graph 0 (both centers of graph 3 are given: they ignore their shifts)
    assert worst(r32.x0[free], un.x0[free]) >= 10 * G.TOL
    assert float(r32.shift[:, ptr[3]:].abs().max()) > 0 and torch.equal(r32.x0[ptr[3]:], un.x0[ptr[3]:])
