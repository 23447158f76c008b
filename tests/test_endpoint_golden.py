"""The endpoint parameterisations of the training loss (pharmacodiff.py:204-215) without a GPU: the four forms that
k_loss_eval<EPC, EPF> evaluates, restated in torch on the oracle's dynamics, against the reference's own forward
(tests/golden/train_endpoint.npz, make_golden_endpoint.py).  Pins the fixture and the formulas."""
import pytest
import torch

from oracle import pf_oracle as O
from helpers import batch_from, load

KEYS = ("pos loss", "feat loss", "position error", "weighted position error", "accuracy", "weighted accuracy")


def endpoint_forward(sd, cfg, batch, x0_raw, h0_raw, T, t_int, eps_h, eps_x, ep_coord, ep_feat, remove_com, weighted,
                     feat_norm=1.0):
    """The kernel's formulas per center (include/pfdyn.h, pf_train_loss_forward_ep), on O.dynamics_forward."""
    bidx = batch.batch_idxs()
    bp, br = bidx["pharm"], bidx["prot"]
    Nf, nf = h0_raw.shape
    h0 = h0_raw / feat_norm
    com = O.segment_mean(x0_raw, batch.pharm_ptr)
    x0c = x0_raw - com[bp]
    prot_x = batch.prot_x - com[br]
    t = t_int.float() / T
    gamma_t = O.gamma_lookup(O.gamma_table(T, 1e-5), t, T)
    a, s = O.alpha(gamma_t)[bp][:, None], O.sigma(gamma_t)[bp][:, None]
    x_t, h_t = a * x0c + s * eps_x, a * h0 + s * eps_h
    m = torch.zeros(batch.batch_size, 3)
    if remove_com:
        m = O.segment_mean(x_t, batch.pharm_ptr)
        x_t, prot_x = x_t - m[bp], prot_x - m[br]
    dyn_h, dyn_x = O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, t)
    wm = 1 - t[bp]
    wl = wm if weighted else torch.ones_like(wm)
    it = h0_raw.argmax(dim=1)
    if ep_feat:
        mx = dyn_h.max(dim=1, keepdim=True).values
        hl = (dyn_h - mx).exp().sum(dim=1).log() + mx[:, 0] - dyn_h[torch.arange(Nf), it]
        ip = dyn_h.argmax(dim=1)
    else:
        hl = (eps_h - dyn_h).square().sum(dim=1)
        ip = ((h_t - s * dyn_h) / a).argmax(dim=1)
    if ep_coord:
        xl = (dyn_x + m[bp] - x0c).square().sum(dim=1)
        err = xl
    else:
        xl = (eps_x - dyn_x).square().sum(dim=1)
        err = ((x_t - s * dyn_x) / a - x0c).square().sum(dim=1)
    hit = (ip == it).float()
    return {"pos loss": (xl * wl).sum() / (3 * Nf), "feat loss": (hl * wl).sum() / (Nf * nf), "position error": err.mean(),
            "weighted position error": (wm * err).mean(), "accuracy": hit.mean(), "weighted accuracy": (wm * hit).mean()}


@pytest.mark.parametrize("prefix", ["both_", "feat_", "coord_"])
def test_four_forms_reproduce_the_reference_forward(prefix):
    z = load("train_endpoint.npz")
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    flags = {k: bool(int(z[prefix + k])) for k in ("endpoint_param_coord", "endpoint_param_feat", "remove_com", "weighted_loss")}
    with torch.no_grad():
        out = endpoint_forward(sd, cfg, batch_from(z), z["x0"], z["h0"], int(z["T"]), z["t_int"].long(), z["eps_h"], z["eps_x"],
                               flags["endpoint_param_coord"], flags["endpoint_param_feat"], flags["remove_com"],
                               flags["weighted_loss"])
    for k in KEYS:
        ref = float(z[prefix + "out_train_" + k.replace(" ", "_")])
        print(prefix, k, float(out[k]), ref)
        assert abs(float(out[k]) - ref) <= 2e-5 * max(1.0, abs(ref)), (k, float(out[k]), ref)


def test_fixture_holds_what_the_gpu_tests_need():
    z = load("train_endpoint.npz")
    assert [bool(int(z["both_" + k])) for k in ("endpoint_param_coord", "endpoint_param_feat", "remove_com", "weighted_loss")] == \
        [True, True, True, False]
    assert [bool(int(z["feat_" + k])) for k in ("endpoint_param_coord", "endpoint_param_feat", "remove_com", "weighted_loss")] == \
        [False, True, True, True]
    assert [bool(int(z["coord_" + k])) for k in ("endpoint_param_coord", "endpoint_param_feat", "remove_com", "weighted_loss")] == \
        [True, False, False, False]
    for p in ("both_", "feat_", "coord_"):
        assert float(z[p + "argmax_gap"]) >= 1e-2          # the accuracy cannot flip within fp32 error
    grads = {}
    for part in z["grad_parts"].tolist():
        grads.update({k: v for k, v in load(part).items() if k.startswith("both_grad_dynamics.")})
    live = sum(float(v.abs().max()) > 0 for v in grads.values())
    assert live >= 150, live
