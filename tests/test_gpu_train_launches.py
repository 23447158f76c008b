"""What one training step launches, counted per gradient-kernel class (pf_profile_read_train), on both training legs -- the
sequencing of pf_train_backward / wide_train_backward is host code that no parity test sees as long as the gradients come out
right -- and, at n_convs = 1, bitwise equality of the gradient under PFDYN_NO_PRUNE=1 and PFDYN_NO_FIX_FUSE=1: the one conv
layer is last and layer 0 at once, which no case of test_gpu_train.py reaches (its golden cases have two and three layers).

Run as a program (python tests/test_gpu_train_launches.py OUT.pt) it is the child process of the second test: one fp32
forward + backward at n_convs = 1, the flat gradient saved to OUT.pt."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pf_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GRAD_CLASSES = 0x1E00       # pf_profile_enable bits 9..12: the four gradient classes (bits 0 and 1 would change how the forward is launched)
T = 100


def small_batch(cfg):
    """two graphs: 12 and 20 atoms, 2 and 3 centers"""
    return O.synthetic_batch([21, 22], [12, 20], [2, 3], cfg)


def loss_step(eng, cfg, batch, dropout=0.1):
    """one pf_train_loss_forward_ep + pf_train_loss_backward on seeded inputs: the flat gradient"""
    gen = torch.Generator().manual_seed(7)
    Nf, B = int(batch.pharm_ptr[-1]), batch.batch_size
    com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    x0 = com[batch.batch_idxs()["pharm"]] + 2.0 * torch.randn(Nf, 3, generator=gen)
    h0 = torch.nn.functional.one_hot(torch.randint(0, cfg.pharm_nf, (Nf,), generator=gen), cfg.pharm_nf).float()
    t_int = torch.randint(0, T, (B,), generator=gen)
    e_x, e_h = torch.randn(Nf, 3, generator=gen), torch.randn(Nf, cfg.pharm_nf, generator=gen)
    gamma = O.gamma_table(T, 1e-5)
    out = eng.train_loss_forward(x0, h0, t_int, e_x, e_h, O.alpha(gamma), O.sigma(gamma), T, 1.0, True, False, dropout=dropout, seed=99)
    assert bool(torch.isfinite(out).all())
    return eng.train_loss_backward(torch.tensor(1.0), torch.tensor(1.0))


def launches_of_one_step(cfg, family):
    from test_gpu_wide import engine_for, set_batch
    eng = engine_for(cfg, O.make_state_dict(cfg, 3))
    eng.set_train_family(family)
    assert eng.train_family() == family
    set_batch(eng, small_batch(cfg))
    eng.profile_enable(GRAD_CLASSES)
    grad = loss_step(eng, cfg, small_batch(cfg))
    counts = {k: n for k, (ms, n) in eng.profile_read_train().items()}
    eng.profile_enable(0)
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    print(family, cfg.n_hidden_scalars, cfg.vector_size, "n_convs", cfg.n_convs, counts)
    return counts


@pytest.mark.parametrize("n_convs", [1, 2, 3])
def test_specialised_leg_launch_counts(n_convs):
    """One head launch (to_scalar_output and every head level in it), one node launch per conv layer (both LayerNorms and the
    update chain in it), one edge launch per conv layer and message-GVP level."""
    cfg = O.DynamicsConfig(n_convs=n_convs)
    counts = launches_of_one_step(cfg, "tuned")
    assert counts["bwd_head"] == 1
    assert counts["bwd_node"] == n_convs
    assert counts["bwd_edge_level"] == n_convs * cfg.n_message_gvps


@pytest.mark.parametrize("S,V", [(64, 32), (128, 16)], ids=["64_32", "forced_128_16"])
def test_wide_leg_launch_counts(S, V):
    """The width-generic leg differentiates one GVP level per launch: the head's levels, per conv layer the two LayerNorm
    launches and the update chain's levels, and the message chains' levels."""
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
    counts = launches_of_one_step(cfg, "wide")
    assert counts["bwd_head"] == cfg.n_noise_gvps
    assert counts["bwd_node"] == cfg.n_convs * (2 + cfg.n_update_gvps)
    assert counts["bwd_edge_level"] == cfg.n_convs * cfg.n_message_gvps


def test_single_layer_gradient_is_bitwise_the_same_without_pruning_and_with_the_two_launch_join(tmp_path):
    """n_convs = 1, each variant in a process of its own (the switches are read when the handle is created).
    PFDYN_NO_FIX_FUSE=1: k_fix_apply + k_enc_group instead of k_fix_enc_group -- the same per-element arithmetic in the same
    order, which test_gpu_train.py holds to bitwise equality at two and three layers.  PFDYN_NO_PRUNE=1: with one conv layer
    there is no second-to-last layer to prune, so the switch must change no launch, and repeated passes agree bit for bit
    (test_gpu_train.py: test_gradients_vs_oracle_more_configs)."""
    variants = {"default": {}, "no_prune": {"PFDYN_NO_PRUNE": "1"}, "no_fix_fuse": {"PFDYN_NO_FIX_FUSE": "1"}}
    procs = {}
    for name, extra in variants.items():
        env = {k: v for k, v in os.environ.items() if k not in ("PFDYN_NO_PRUNE", "PFDYN_NO_FIX_FUSE")}
        env.update(extra)
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), str(tmp_path / (name + ".pt"))], env=env, cwd=ROOT,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    grads = {}
    for name, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (name, log[-2000:])
        grads[name] = torch.load(str(tmp_path / (name + ".pt")))
    ref = grads["default"]
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    for name in ("no_prune", "no_fix_fuse"):
        assert torch.equal(grads[name], ref), (name, float((grads[name] - ref).abs().max()))


if __name__ == "__main__":
    import pharmacoforge_amd as pfa
    cfg1 = O.DynamicsConfig(n_convs=1)
    b1 = small_batch(cfg1)
    e1 = pfa.PfEngine(n_convs=1)
    e1.load_state_dict(O.make_state_dict(cfg1, 3))
    e1.set_batch(b1.prot_x, b1.prot_h, b1.prot_ptr, b1.pharm_ptr, b1.pp_src, b1.pp_dst)
    torch.save(loss_step(e1, cfg1, b1).cpu(), sys.argv[1])
