"""The CPU oracle's training gradients against the reference model at hidden widths other than 128 / 16 (fixtures of
tests/golden/make_golden_width_train.py: one reference training_step in train() mode, dropout 0.1, at (64, 32) and (96, 16)),
at the tolerances of test_oracle_golden.py::test_training_gradients.  This pins the oracle's autograd at other widths to the
reference; the GPU tests of the width-generic training leg (test_gpu_wide_train.py) check against both."""
import os

import pytest

from oracle import pf_oracle as O
from helpers import GOLDEN, batch_from, dropout_from, load

# fixture -> config that generated it (tests/golden/make_golden_width_train.py)
WIDTH_GRAD_CASES = {
    "train_grads_w64v32.npz": O.DynamicsConfig(n_hidden_scalars=64, vector_size=32, n_convs=3, message_norm=0, pf_k=0),
    "train_grads_w96v16.npz": O.DynamicsConfig(n_hidden_scalars=96, vector_size=16),
}


def load_parts(name):
    """a fixture written in parts (NAME.npz, NAME.p1.npz, ...: no committed file above the size limit) as one dict"""
    z = load(name)
    for i in range(1, int(z["n_parts"])):
        part = load(f"{name[:-4]}.p{i}.npz")
        assert not set(part) & set(z), name
        z.update(part)
    assert not os.path.exists(os.path.join(GOLDEN, f"{name[:-4]}.p{int(z['n_parts'])}.npz")), "a stale part file"
    return z


@pytest.mark.parametrize("name", sorted(WIDTH_GRAD_CASES))
def test_training_gradients_at_width(name):
    """Losses, metrics and every parameter gradient of one reference training_step (train() mode, dropout 0.1)."""
    z, cfg = load_parts(name), WIDTH_GRAD_CASES[name]
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    assert {k for k in z if k.startswith("grad_")} == {"grad_" + k for k, v in sd.items() if v.numel() > 0}
    assert z["drop_0_prot_msg_s"].shape[1] == cfg.n_hidden_scalars and z["drop_0_prot_msg_v"].shape[1] == cfg.vector_size
    losses, metrics, grads = O.training_grads(sd, cfg, batch, z["x0"], z["h0"], int(z["T"]), 1e-5,
                                              z["t_int"].long(), z["eps_h"], z["eps_x"],
                                              dropout=dropout_from(z, cfg), weighted_loss=bool(z["weighted_loss"]))
    for k, v in {**losses, **metrics}.items():
        ref = float(z["out_" + k.replace(" ", "_")])
        assert abs(float(v) - ref) <= 1e-5 * max(1.0, abs(ref)), (k, float(v), ref)
    live_ref = sum(float(z[k].abs().max()) > 0 for k in z if k.startswith("grad_"))
    live = 0
    for k, g in grads.items():
        if g.numel() == 0:
            continue
        ref = z["grad_" + k]
        scale = float(ref.abs().max())
        live += float(g.abs().max()) > 0
        assert float((g - ref).abs().max()) <= 2e-5 * scale + 1e-9, k
    # as many tensors with a gradient as the reference has (the last layer's prot-side parameters get exactly zero): not zeros
    assert live == live_ref and live_ref >= 100, (live, live_ref)
