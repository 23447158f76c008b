"""The width-generic inference family (pf_wide.hip) on the GPU: dynamics calls at n_hidden_scalars / vector_size pairs other
than the specialised (128, 16) against the CPU oracle, the family forced onto (128, 16) with PFDYN_WIDE=1 against the reference
goldens and against the specialised kernels, sampling trajectories, run-to-run bit equality, and training refused.

Tolerances as tests/test_gpu_parity.py: one dynamics call |err| <= 2e-4 + 2e-4 |ref|; edge sets exact."""
import pytest
import torch

from oracle import pf_oracle as O
from helpers import DYN_CASES, batch_from, check_live, edge_set, golden_live, live_reference, load, with_head
from test_oracle_width import WIDTH_DYN_CASES, WIDTH_TRAJ_CASES

pytestmark = pytest.mark.gpu

SPEC_FAMILIES = {4, 8, 16, 17, 32, 128}     # pf_debug_kernel_family values of the specialised kernels

RTOL, ATOL = 2e-4, 2e-4
PAIRS = [(64, 16), (160, 16), (256, 16), (64, 32), (160, 32), (256, 32), (128, 32), (96, 16), (224, 32)]
CASES = {   # name -> (config fields, protein atoms per graph, centers per graph)
    "knn_mean_c2": (dict(), [64, 64], [4, 3]),
    "radius_value_c3": (dict(n_convs=3, n_noise_gvps=3, message_norm=10, pf_k=0, ff_k=0), [48, 64], [3, 5]),
    "knnff_c1": (dict(n_convs=1, ff_k=2, pf_k=3, message_norm=1), [64, 40], [4, 4]),
    "gnorm_radius_ragged": (dict(message_norm=0, pf_k=0), [40, 72, 56], [2, 6, 3]),
    "gnorm_knn_ragged": (dict(message_norm=0, pf_k=5), [64, 48, 72], [5, 2, 4]),
}


def engine_for(cfg: O.DynamicsConfig, sd):
    import pharmacoforge_amd as pfa
    eng = pfa.PfEngine(pharm_nf=cfg.pharm_nf, rec_nf=cfg.rec_nf, vector_size=cfg.vector_size,
                       n_hidden_scalars=cfg.n_hidden_scalars, n_convs=cfg.n_convs, n_message_gvps=cfg.n_message_gvps,
                       n_update_gvps=cfg.n_update_gvps, n_noise_gvps=cfg.n_noise_gvps, message_norm=cfg.message_norm,
                       ff_k=cfg.ff_k, pf_k=cfg.pf_k,
                       graph_cutoffs={"pp": cfg.cutoff_pp, "pf": cfg.cutoff_pf, "fp": cfg.cutoff_fp, "ff": cfg.cutoff_ff})
    eng.load_state_dict(sd)
    return eng


def set_batch(eng, batch, prot_x=None):
    eng.set_batch(batch.prot_x if prot_x is None else prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr,
                  batch.pp_src, batch.pp_dst)


def inputs(cfg, batch, seed):
    """x_t near each pocket's center, h_t, t per graph"""
    g = torch.Generator().manual_seed(seed)
    B, Nf = batch.batch_size, int(batch.pharm_ptr[-1])
    com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    x_t = com[batch.batch_idxs()["pharm"]] + 3.0 * torch.randn(Nf, 3, generator=g)
    h_t = torch.randn(Nf, cfg.pharm_nf, generator=g)
    t = torch.rand(B, generator=g)
    return x_t, h_t, t


def check_call(cfg, batch, seed=0, wseed=3):
    sd = O.make_state_dict(cfg, wseed)
    eng = engine_for(cfg, sd)
    set_batch(eng, batch)
    x_t, h_t, t = inputs(cfg, batch, seed)
    eps_h, eps_x = eng.dynamics(x_t, h_t, t)
    oh, ox, edges = O.dynamics_forward(sd, cfg, batch, batch.prot_x, x_t, h_t, t, return_edges=True)
    for i, et in enumerate(O.ETYPES):
        s, d = eng.get_edges(i)
        assert edge_set(s, d) == edge_set(edges[et][0], edges[et][1]), et
    torch.testing.assert_close(eps_h.cpu(), oh, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(eps_x.cpu(), ox, rtol=RTOL, atol=ATOL)
    for layer in range(cfg.n_convs):
        assert eng.kernel_family(layer) == 64
    # the live leg: the same call with the head scaled by 2**k (k from the oracle's fp32 eps_x above), eps_x of order one
    live = live_reference(sd, cfg, batch, batch.prot_x, x_t, h_t, t, eps_x_ref=ox)
    eng_live = engine_for(cfg, live.sd)
    set_batch(eng_live, batch)
    eps_h, eps_x = eng_live.dynamics(x_t, h_t, t)
    for layer in range(cfg.n_convs):
        assert eng_live.kernel_family(layer) == 64
    check_live(eps_h, eps_x, live, f"wide {cfg.n_hidden_scalars}/{cfg.vector_size} convs {cfg.n_convs} norm {cfg.message_norm} "
               f"pf_k {cfg.pf_k} ff_k {cfg.ff_k} atoms {int(batch.prot_ptr[-1])}", RTOL, ATOL)
    return eng


@pytest.mark.parametrize("S,V", PAIRS)
@pytest.mark.parametrize("case", list(CASES))
def test_dynamics_vs_oracle(S, V, case):
    fields, n_prot, n_pharm = CASES[case]
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V, **fields)
    batch = O.synthetic_batch(range(len(n_prot)), n_prot, n_pharm, cfg)
    check_call(cfg, batch)


@pytest.mark.parametrize("name,head", with_head(WIDTH_DYN_CASES))
def test_dynamics_vs_reference_fixtures(name, head):
    """the reference model's own outputs at (256, 16) and (64, 32) (tests/golden/make_golden_width.py) and the oracle; with the
    recorded head and with a live one (the recorded eps_x times 2**k is the reference's output for it)"""
    z, cfg = load(name), WIDTH_DYN_CASES[name]
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    live = None
    if head == "live":
        live = live_reference(sd, cfg, batch, z["prot_x"], z["x_t"], z["h_t"], z["t"], eps_x_ref=z["eps_x"])
        sd = live.sd
    eng = engine_for(cfg, sd)
    set_batch(eng, batch, z["prot_x"])
    eps_h, eps_x = eng.dynamics(z["x_t"], z["h_t"], z["t"])
    for i, et in enumerate(O.ETYPES):
        s, d = eng.get_edges(i)
        assert edge_set(s, d) == edge_set(z[f"e_{et}_src"].long(), z[f"e_{et}_dst"].long()), et
        assert s.numel() == z[f"e_{et}_src"].numel()
    for layer in range(cfg.n_convs):
        assert eng.kernel_family(layer) == 64
    if live is not None:
        check_live(eps_h, eps_x, live, f"wide fixture {name}", RTOL, ATOL, z=z)
        return
    torch.testing.assert_close(eps_h.cpu(), z["eps_h"], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(eps_x.cpu(), z["eps_x"], rtol=RTOL, atol=ATOL)
    oh, ox = O.dynamics_forward(sd, cfg, batch, z["prot_x"], z["x_t"], z["h_t"], z["t"])
    torch.testing.assert_close(eps_h.cpu(), oh, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(eps_x.cpu(), ox, rtol=RTOL, atol=ATOL)
    for layer in range(cfg.n_convs):
        assert eng.kernel_family(layer) == 64


@pytest.mark.parametrize("name", list(WIDTH_TRAJ_CASES))
def test_trajectory_vs_reference_fixture(name):
    """the reference's T = 50 trajectory at (192, 32), every frame, and the oracle's"""
    z, cfg = load(name), WIDTH_TRAJ_CASES[name]
    batch = batch_from(z)
    sd = O.make_state_dict(cfg, int(z["wseed"]))
    eng = engine_for(cfg, sd)
    set_batch(eng, batch)
    T = int(z["T"])
    coef = O.step_coefficients(O.gamma_table(T, float(z["precision"])), T)
    x0, h0, tx, th = eng.sample(eng.coef_array(coef, reversed(range(T))), T, z["noise"], trajectory=True)
    eng.sample_status()
    torch.testing.assert_close(x0.cpu(), z["x0"], rtol=0, atol=2e-2)
    torch.testing.assert_close(h0.cpu(), z["h0"], rtol=0, atol=2e-2)
    torch.testing.assert_close(tx.cpu(), z["pos_frames"], rtol=0, atol=2e-2)
    torch.testing.assert_close(th.cpu(), z["feat_frames"], rtol=0, atol=2e-2)
    ox, oh = O.sample_given_receptor(sd, cfg, batch, T, float(z["precision"]), z["noise"])
    torch.testing.assert_close(x0.cpu(), ox, rtol=0, atol=2e-2)
    torch.testing.assert_close(h0.cpu(), oh, rtol=0, atol=2e-2)


@pytest.mark.parametrize("S,V", [(256, 16), (64, 32)])
def test_pocket_above_512_atoms(S, V):
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
    batch = O.synthetic_batch([5, 6], [600, 64], [6, 3], cfg)
    check_call(cfg, batch)


@pytest.mark.parametrize("name,head", with_head(DYN_CASES))
def test_forced_wide_128_16_vs_goldens_and_specialised(name, head, monkeypatch):
    z, cfg = load(name), DYN_CASES[name]
    batch = batch_from(z)
    live = golden_live(name) if head == "live" else None
    sd = O.make_state_dict(cfg, int(z["wseed"])) if live is None else live.sd
    spec = engine_for(cfg, sd)
    set_batch(spec, batch, z["prot_x"])
    sh, sx = spec.dynamics(z["x_t"], z["h_t"], z["t"])
    fam = [spec.kernel_family(layer) for layer in range(cfg.n_convs)]
    assert all(f in SPEC_FAMILIES for f in fam), fam
    monkeypatch.setenv("PFDYN_WIDE", "1")
    eng = engine_for(cfg, sd)
    set_batch(eng, batch, z["prot_x"])
    eps_h, eps_x = eng.dynamics(z["x_t"], z["h_t"], z["t"])
    for layer in range(cfg.n_convs):
        assert eng.kernel_family(layer) == 64
    for i, et in enumerate(O.ETYPES):
        s, d = eng.get_edges(i)
        assert edge_set(s, d) == edge_set(z[f"e_{et}_src"].long(), z[f"e_{et}_dst"].long()), et
    if live is None:
        torch.testing.assert_close(eps_h.cpu(), z["eps_h"], rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(eps_x.cpu(), z["eps_x"], rtol=RTOL, atol=ATOL)
    else:
        check_live(eps_h, eps_x, live, f"forced wide 128/16 {name}", RTOL, ATOL, z=z)
    torch.testing.assert_close(eps_h, sh, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(eps_x, sx, rtol=2e-5, atol=2e-5)
    # without the variable a new handle is back on the specialised kernels, with the very families of the first one
    monkeypatch.delenv("PFDYN_WIDE")
    again = engine_for(cfg, sd)
    set_batch(again, batch, z["prot_x"])
    ah, ax = again.dynamics(z["x_t"], z["h_t"], z["t"])
    assert [again.kernel_family(layer) for layer in range(cfg.n_convs)] == fam
    assert torch.equal(ah, sh) and torch.equal(ax, sx)


@pytest.mark.parametrize("n_convs", [2, 3])
def test_forced_wide_128_16_still_trains(n_convs, monkeypatch):
    """PFDYN_WIDE=1 moves inference only: a (128, 16) handle under it trains on the specialised kernels (the dense conv
    layer 0 of n_convs = 3 takes the pp precompute, whose buffer must be there), bit for bit as a plain handle"""
    cfg = O.DynamicsConfig(n_convs=n_convs)
    sd = O.make_state_dict(cfg, 7)
    batch = O.synthetic_batch([60, 61], [48, 40], [4, 5], cfg)
    x_t, h_t, t = inputs(cfg, batch, 2)
    g = torch.Generator().manual_seed(5)
    w_h, w_x = torch.randn(x_t.shape[0], cfg.pharm_nf, generator=g), torch.randn(x_t.shape[0], 3, generator=g)
    res = []
    for wide in (False, True):
        if wide:
            monkeypatch.setenv("PFDYN_WIDE", "1")
        eng = engine_for(cfg, sd)
        monkeypatch.delenv("PFDYN_WIDE", raising=False)
        set_batch(eng, batch)
        eh, ex = eng.train_forward(x_t, h_t, t, dropout=0.0)
        grad = eng.train_backward(w_h, w_x)
        res.append((eh.cpu(), ex.cpu(), grad.cpu()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    oh, ox = O.dynamics_forward(sd, cfg, batch, batch.prot_x, x_t, h_t, t)
    torch.testing.assert_close(res[1][0], oh, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(res[1][1], ox, rtol=RTOL, atol=ATOL)


def sample_run(eng, T, noise, n_steps):
    coef = O.step_coefficients(O.gamma_table(T, 1e-5), T)
    return eng.sample(eng.coef_array(coef, reversed(range(T))), n_steps, noise)


@pytest.mark.parametrize("S,V", [(192, 32), (64, 16)])
def test_trajectory_vs_oracle_and_repeatable(S, V):
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
    batch = O.synthetic_batch([0, 1, 2], [64, 56, 72], [4, 3, 5], cfg)
    sd = O.make_state_dict(cfg, 1)
    eng = engine_for(cfg, sd)
    set_batch(eng, batch)
    T = 50
    noise = torch.randn(T + 1, int(batch.pharm_ptr[-1]), 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(9))
    x0, h0 = sample_run(eng, T, noise, T)
    eng.sample_status()                       # raises PfError on an invalid run
    ox, oh = O.sample_given_receptor(sd, cfg, batch, T, 1e-5, noise)
    torch.testing.assert_close(x0.cpu(), ox, rtol=0, atol=2e-2)
    torch.testing.assert_close(h0.cpu(), oh, rtol=0, atol=2e-2)
    x1, h1 = sample_run(eng, T, noise, T)
    assert torch.equal(x0, x1) and torch.equal(h0, h1)


def test_set_flat_params_reaches_the_packed_linears():
    """The family's packed Linears follow the flat parameter vector (the gather map of its packing, pf_pack.cpp): after
    pf_set_flat_params a (64, 32) handle computes, bit for bit, what a fresh handle committed with those weights computes -- and
    the first result again after the first weights come back."""
    fields, n_prot, n_pharm = CASES["knnff_c1"]
    cfg = O.DynamicsConfig(n_hidden_scalars=64, vector_size=32, **fields)
    batch = O.synthetic_batch(range(len(n_prot)), n_prot, n_pharm, cfg)
    x_t, h_t, t = inputs(cfg, batch, 0)
    sd1, sd2 = O.make_state_dict(cfg, 3), O.make_state_dict(cfg, 4)
    eng = engine_for(cfg, sd1)
    set_batch(eng, batch)
    h1, x1 = eng.dynamics(x_t, h_t, t)

    def flat(sd):
        return torch.cat([sd[n].reshape(-1) for n, _, _ in eng.param_layout()])
    eng.set_flat_params(flat(sd2))                  # as after an optimiser step
    h2, x2 = eng.dynamics(x_t, h_t, t)
    fresh = engine_for(cfg, sd2)
    set_batch(fresh, batch)
    fh, fx = fresh.dynamics(x_t, h_t, t)
    assert torch.equal(h2, fh) and torch.equal(x2, fx)
    assert not torch.equal(h2, h1)
    eng.set_flat_params(flat(sd1))
    h3, x3 = eng.dynamics(x_t, h_t, t)
    assert torch.equal(h3, h1) and torch.equal(x3, x1)


def test_pocket_groups_accepted_at_other_widths():
    cfg = O.DynamicsConfig(n_hidden_scalars=256, vector_size=16)
    pocket = O.synthetic_batch([4], [64], [3], cfg)
    batch = O.concat_pockets([pocket, pocket, pocket])
    sd = O.make_state_dict(cfg, 2)
    eng = engine_for(cfg, sd)
    eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst,
                  pocket_uid=[0, 0, 0])
    T = 20
    noise = torch.randn(T + 1, int(batch.pharm_ptr[-1]), 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(4))
    x0, h0 = sample_run(eng, T, noise, T)
    ox, oh = O.sample_given_receptor(sd, cfg, batch, T, 1e-5, noise)
    torch.testing.assert_close(x0.cpu(), ox, rtol=0, atol=2e-2)
    torch.testing.assert_close(h0.cpu(), oh, rtol=0, atol=2e-2)


def test_training_refused_at_other_widths():
    import pharmacoforge_amd as pfa
    cfg = O.DynamicsConfig(n_hidden_scalars=256, vector_size=32)
    batch = O.synthetic_batch([0], [48], [3], cfg)
    sd = O.make_state_dict(cfg, 0)
    eng = engine_for(cfg, sd)
    set_batch(eng, batch)
    assert sum(n for _, _, n in eng.param_layout()) == sum(v.numel() for v in sd.values())
    x_t, h_t, t = inputs(cfg, batch, 1)
    with pytest.raises(pfa.PfError, match="128 / vector_size 16"):
        eng.train_forward(x_t, h_t, t)
