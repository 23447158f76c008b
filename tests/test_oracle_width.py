"""The CPU oracle against the reference model at hidden widths other than 128 / 16 (fixtures of
tests/golden/make_golden_width.py): edge sets, one conv layer with non-zero vectors, the dynamics call and a T = 50
trajectory, at the tolerances of test_oracle_golden.py.  This pins the oracle's width handling to the reference; the GPU
tests of the width-generic kernels (test_gpu_wide.py) check against both."""
import pytest
import torch

from oracle import pf_oracle as O
from helpers import batch_from, edge_set, load

# fixture -> config that generated it (tests/golden/make_golden_width.py)
WIDTH_DYN_CASES = {
    "dynamics_w256.npz": O.DynamicsConfig(n_hidden_scalars=256, vector_size=16),
    "dynamics_w64v32.npz": O.DynamicsConfig(n_hidden_scalars=64, vector_size=32, n_convs=3, message_norm=0, pf_k=0),
}
WIDTH_TRAJ_CASES = {"traj_w192v32_T50.npz": O.DynamicsConfig(n_hidden_scalars=192, vector_size=32)}


def close(a, b, rtol, atol):
    torch.testing.assert_close(a, b, rtol=rtol, atol=atol)


@pytest.mark.parametrize("name", list(WIDTH_DYN_CASES))
def test_edges_conv_dynamics_at_width(name):
    z, cfg = load(name), WIDTH_DYN_CASES[name]
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    assert z["conv_in_h_prot"].shape[1] == cfg.n_hidden_scalars and z["conv_in_v_prot"].shape[1] == cfg.vector_size
    edges = O.build_dynamic_edges(cfg, batch, z["prot_x"], z["x_t"])
    edges["pp"] = (batch.pp_src, batch.pp_dst)
    for et in O.ETYPES:
        assert edge_set(*edges[et]) == edge_set(z[f"e_{et}_src"].long(), z[f"e_{et}_dst"].long()), et
        assert len(edges[et][0]) == len(z[f"e_{et}_src"])
    li = int(z["conv_layer_index"])
    ref_edges = {et: (z[f"e_{et}_src"].long(), z[f"e_{et}_dst"].long()) for et in O.ETYPES}
    nf = {"pharm": (z["conv_in_h_pharm"], z["x_t"], z["conv_in_v_pharm"]),
          "prot": (z["conv_in_h_prot"], z["prot_x"], z["conv_in_v_prot"])}
    ec = O.dynamic_edge_counts(cfg, batch, ref_edges) if cfg.message_norm == 0 else None
    out = O.conv_layer(sd, f"dynamics.noise_predictor.conv_layers.{li}.", cfg, nf, ref_edges, batch, ec)
    for nt in ("pharm", "prot"):
        close(out[nt][0], z[f"conv_out_h_{nt}"], rtol=1e-4, atol=2e-5)
        close(out[nt][2], z[f"conv_out_v_{nt}"], rtol=1e-4, atol=2e-5)
    eps_h, eps_x = O.dynamics_forward(sd, cfg, batch, z["prot_x"], z["x_t"], z["h_t"], z["t"])
    close(eps_h, z["eps_h"], rtol=1e-4, atol=2e-5)
    close(eps_x, z["eps_x"], rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("name", list(WIDTH_TRAJ_CASES))
def test_trajectory_at_width(name):
    z, cfg = load(name), WIDTH_TRAJ_CASES[name]
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    res = O.sample_given_receptor(sd, cfg, batch, int(z["T"]), float(z["precision"]), z["noise"], return_traj=True)
    close(res[0], z["x0"], rtol=1e-3, atol=1e-3)
    close(res[1], z["h0"], rtol=1e-3, atol=1e-3)
    close(torch.stack([f[0] for f in res[2]]), z["pos_frames"], rtol=1e-3, atol=1e-3)
    close(torch.stack([f[1] for f in res[2]]), z["feat_frames"], rtol=1e-3, atol=1e-3)
