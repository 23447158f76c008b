"""The oracle's fp64 mode and the live noise head (CPU): what the GPU suite's `live` legs and error budgets rest on.

oracle.pf_oracle evaluates in the dtype it is given; dynamics_forward64 casts weights and inputs to double and keeps the
edge set decided in fp32.  helpers.live_head scales the last head GVP's Wu by 2**k, which scales eps_x by 2**k exactly."""
import importlib.util
import os

import pytest
import torch

from oracle import pf_oracle as O
from helpers import DYN_CASES, GOLDEN, GRAD_CASES, batch_from, dropout_from, edge_set, live_head, load, within_budget

ATOL = 2e-4                    # the single-call absolute tolerance of the GPU parity tests
FP64_VS_RECORDED = 2.5e-6      # ~3x the worst fp32-vs-fp64 deviation of the reference's recorded outputs (7.4e-7 of the max)


@pytest.fixture(scope="module", params=list(DYN_CASES))
def case(request):
    name = request.param
    z, cfg = load(name), DYN_CASES[name]
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    return name, z, cfg, batch, sd


def test_fp64_evaluation_of_the_goldens(case):
    name, z, cfg, batch, sd = case
    h64, x64, edges = O.dynamics_forward64(sd, cfg, batch, z["prot_x"], z["x_t"], z["h_t"], z["t"], return_edges=True)
    assert h64.dtype == torch.float64 and x64.dtype == torch.float64
    for et in ("ff", "pf", "fp"):
        assert edge_set(*edges[et]) == edge_set(z[f"e_{et}_src"].long(), z[f"e_{et}_dst"].long()), et
        assert edges[et][0].numel() == z[f"e_{et}_src"].numel()
    for got, ref in ((h64, z["eps_h"]), (x64, z["eps_x"])):
        m = float(got.abs().max())
        assert float((got - ref.double()).abs().max()) <= FP64_VS_RECORDED * m, name
    # edges= : the same evaluation on a supplied edge set
    h2, x2 = O.dynamics_forward(O.state_dict64(sd), cfg, O.batch64(batch), z["prot_x"].double(), z["x_t"].double(),
                                z["h_t"].double(), z["t"].double(), edges=edges)
    assert torch.equal(h2, h64) and torch.equal(x2, x64)


def test_live_head_scales_eps_x_exactly(case):
    name, z, cfg, batch, sd = case
    sd_live, k = live_head(sd, cfg, z["eps_x"])
    assert set(sd_live) == set(sd) and sum(not torch.equal(sd_live[n], sd[n]) for n in sd) == 1
    oh, ox = O.dynamics_forward(sd_live, cfg, batch, z["prot_x"], z["x_t"], z["h_t"], z["t"])
    assert torch.equal(ox, z["eps_x"] * 2.0 ** k) and torch.equal(oh, z["eps_h"]), (name, k)
    assert 0.5 <= float(ox.abs().max()) < 1.0
    assert float(ox.abs().min()) > ATOL
    # the budget helper on the reference alone: an fp32 evaluation is within its own noise
    h64, x64 = O.dynamics_forward64(sd_live, cfg, batch, z["prot_x"], z["x_t"], z["h_t"], z["t"])
    within_budget(oh, oh, h64, name + " eps_h")
    e, e32 = within_budget(ox, ox, x64, name + " eps_x")
    assert e == e32 < 1e-6
    with pytest.raises(AssertionError):
        within_budget(torch.zeros_like(ox), ox, x64, name + " zeros")
    with pytest.raises(AssertionError):
        within_budget(-ox, ox, x64, name + " sign")


def test_fp64_dropout_and_autograd():
    from test_gpu_train import compare
    name = "train_grads.npz"
    z, cfg = load(name), GRAD_CASES[name]
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    args = (int(z["T"]), 1e-5, z["t_int"].long())
    drop = dropout_from(z, cfg)
    _, _, g32 = O.training_grads(sd, cfg, batch, z["x0"], z["h0"], *args, z["eps_h"], z["eps_x"], dropout=drop)
    drop64 = [{nt: tuple(m.double() for m in d[nt]) for nt in d} for d in drop]
    l64, _, g64 = O.training_grads(O.state_dict64(sd), cfg, O.batch64(batch), z["x0"].double(), z["h0"].double(), *args,
                                   z["eps_h"].double(), z["eps_x"].double(), dropout=drop64)
    assert all(v.dtype == torch.float64 for v in l64.values())
    assert all(g.dtype == torch.float64 for g in g64.values())
    assert sum(float(g.abs().max()) > 0 for g in g64.values() if g.numel()) >= 150
    compare({k: g.double() for k, g in g32.items()}, g64, 1e-4, name)


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_live", os.path.join(GOLDEN, "make_golden_live.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_live_trajectory_fixture_first_steps_regenerate():
    """tests/golden/traj_live_c1_T500.npz from its committed generator: the first 20 steps in fp64 (to fp64 rounding) and in
    fp32 (within the budget the GPU test grants)."""
    G = _generator()
    fx = load(G.NAME)
    z, cfg, batch, sd_live, k, T, prec = G.setup()
    assert k == int(fx["k"]) and T == int(fx["T"]) == 500 and fx["pos_frames"].dtype == torch.float64
    assert fx["pos_frames"].shape == (T + 1, 4, 3) and fx["feat_frames"].shape == (T + 1, 4, 6)
    n = 20
    pos, feat, _, _ = G.run(sd_live, cfg, batch, T, prec, fx["noise"], n_steps=n)
    torch.testing.assert_close(pos, fx["pos_frames"][:n + 1], rtol=0, atol=1e-9)
    torch.testing.assert_close(feat, fx["feat_frames"][:n + 1], rtol=0, atol=1e-9)
    G.check_fair(cfg, batch, fx["pos_frames"])
    assert float((fx["x0"] - fx["x0_recorded_head"].double()).abs().max()) > 0.5
    p32, f32, _, _ = G.run(sd_live, cfg, batch, T, prec, fx["noise"], n_steps=n, double=False)
    for got, ref, e32 in ((p32, fx["pos_frames"], float(fx["e32_pos"])), (f32, fx["feat_frames"], float(fx["e32_feat"]))):
        for f in range(n + 1):
            bound = 8 * max(e32, 2.0 ** -22 * float(ref[f].abs().max()))
            assert float((got[f].double() - ref[f]).abs().max()) <= bound, f
