"""The width-generic training leg (pf_train_set_family: the training form of pf_wide.hip's forward, the gradient kernels of
pf_wide_train.hip) on the GPU: parameter gradients at n_hidden_scalars / vector_size pairs other than (128, 16) against the
reference's own gradients (tests/golden/train_grads_w*.npz) and the oracle's autograd, the leg forced onto (128, 16) against
the reference's goldens and the specialised gradient kernels, the endpoint parameterisations, bitwise repeatability, the
switch's semantics, and a short training run.

Tolerances are the project's own: per gradient tensor 2e-3 max|ref| + 1e-7 (test_gpu_train.py: compare), the loss within
2e-4 max(1, |ref|), dynamics outputs within test_gpu_wide.py's RTOL / ATOL."""
import ctypes

import pytest
import torch

from oracle import pf_oracle as O
from helpers import GRAD_CASES, batch_from, load
from test_gpu_train import EXTRA_CASES, compare, flat_to_dict
from test_gpu_wide import ATOL, RTOL, engine_for, inputs, set_batch
from test_oracle_width_train import WIDTH_GRAD_CASES, load_parts

pytestmark = pytest.mark.gpu


def wide_engine(cfg, sd, batch):
    """an engine on the wide training leg"""
    eng = engine_for(cfg, sd)
    eng.set_train_family("wide")
    set_batch(eng, batch)
    return eng


def masks_from_engine(eng, cfg, p, seed, Np, Nf):
    S = cfg.n_hidden_scalars
    out = []
    for layer in range(cfg.n_convs):
        m0 = eng.dropout_mask(layer, 0, p, seed).cpu()
        m1 = eng.dropout_mask(layer, 1, p, seed).cpu()
        assert m0.shape == (Np + Nf, S + cfg.vector_size)
        out.append({nt: (m0[sl, :S], m0[sl, S:], m1[sl, :S], m1[sl, S:])
                    for nt, sl in (("prot", slice(0, Np)), ("pharm", slice(Np, Np + Nf)))})
    return out


def golden_masks(z, cfg, Np, Nf):
    """[n_convs, 2, N, S + V] multipliers in the engine's layout from the GVPDropout draws the reference made"""
    S = cfg.n_hidden_scalars
    out = torch.ones(cfg.n_convs, 2, Np + Nf, S + cfg.vector_size)
    for layer in range(cfg.n_convs):
        for w, which in enumerate(("msg", "res")):
            for nt, sl in (("prot", slice(0, Np)), ("pharm", slice(Np, Np + Nf))):
                out[layer, w, sl, :S] = z[f"drop_{layer}_{nt}_{which}_s"]
                out[layer, w, sl, S:] = z[f"drop_{layer}_{nt}_{which}_v"]
    return out


def model_for(cfg, T, wseed, family="wide", dropout=0.1):
    import pharmacoforge_amd as pfa
    dyn = dict(vector_size=cfg.vector_size, n_convs=cfg.n_convs, n_hidden_scalars=cfg.n_hidden_scalars,
               message_norm=cfg.message_norm, dropout=dropout, ff_k=cfg.ff_k, pf_k=cfg.pf_k, n_message_gvps=cfg.n_message_gvps,
               n_update_gvps=cfg.n_update_gvps, n_noise_gvps=cfg.n_noise_gvps)
    graph = {'graph_cutoffs': {'pp': cfg.cutoff_pp, 'pf': cfg.cutoff_pf, 'fp': cfg.cutoff_fp, 'ff': cfg.cutoff_ff}}
    m = pfa.PharmacophoreDiff(cfg.pharm_nf, cfg.rec_nf, pfa.analysis.ph_idx_to_type, None, n_timesteps=T, graph_config=graph,
                              dynamics_config=dyn, precision=1e-5)
    sd = dict(O.make_state_dict(cfg, wseed))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    m.dynamics.set_train_family(family)
    return m


def graph_from(b, x0, h0):
    import pharmacoforge_amd as pfa
    return pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, x0, h0)


def reference_step(m, z, cfg, what):
    """model.training_step with the fixture's draws and masks: total loss and every parameter gradient against the reference's"""
    m.train()
    m.weighted_loss = bool(int(z["weighted_loss"]))
    b = batch_from(z)
    g = graph_from(b, z["x0"], z["h0"]).to("cuda")
    Np, Nf = int(b.prot_ptr[-1]), int(b.pharm_ptr[-1])
    eng = m.dynamics.bind_graph(g)
    assert eng.train_family() == "wide"
    eng.set_dropout_masks(golden_masks(z, cfg, Np, Nf))
    loss = m.training_step(g, 0, t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    ref_total = float(z["out_train_pos_loss"]) + float(z["out_train_feat_loss"])
    print(what, "loss", float(loss.detach()), "reference", ref_total)
    assert abs(float(loss.detach()) - ref_total) <= 2e-4 * max(1.0, abs(ref_total))
    loss.backward()
    eng.set_dropout_masks(None)
    got, ref = {}, {}
    for k, p in m.named_parameters():
        if p.numel() == 0 or not k.startswith("dynamics."):
            continue
        ref[k] = z["grad_" + k]
        got[k] = torch.zeros_like(ref[k]) if p.grad is None else p.grad.cpu()
    assert sum(r.numel() > 0 and float(r.abs().max()) > 0 for r in ref.values()) >= 100
    compare(got, ref, 2e-3, what)


# 1. the reference's own gradients at (64, 32) and (96, 16)
@pytest.mark.parametrize("name", sorted(WIDTH_GRAD_CASES))
def test_training_step_gradients_match_reference_fixture(name):
    z, cfg = load_parts(name), WIDTH_GRAD_CASES[name]
    reference_step(model_for(cfg, int(z["T"]), int(z["wseed"])), z, cfg, name)


def oracle_check(cfg, batch, p_drop, seed, what, wseed=3, tol=2e-3):
    sd = O.make_state_dict(cfg, wseed)
    eng = wide_engine(cfg, sd, batch)
    Np, Nf, B = int(batch.prot_ptr[-1]), int(batch.pharm_ptr[-1]), batch.batch_size
    gen = torch.Generator().manual_seed(11)
    bidx = batch.batch_idxs()
    com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    prot_x = batch.prot_x - com[bidx["prot"]]
    x_t = 2.5 * torch.randn(Nf, 3, generator=gen)
    h_t = torch.randn(Nf, cfg.pharm_nf, generator=gen)
    t = torch.rand(B, generator=gen)
    w_h, w_x = torch.randn(Nf, cfg.pharm_nf, generator=gen), torch.randn(Nf, 3, generator=gen)
    eps_h, eps_x = eng.train_forward(x_t, h_t, t, prot_x=prot_x, dropout=p_drop, seed=seed)
    drop = masks_from_engine(eng, cfg, p_drop, seed, Np, Nf) if p_drop > 0 else None
    if drop is not None:
        keep = torch.cat([m.reshape(-1) for d in drop for nt in d for m in d[nt]])
        assert set(keep.unique().tolist()) <= {0.0, float(torch.tensor(1.0 / (1.0 - p_drop), dtype=torch.float32))}
        assert abs(float((keep == 0).float().mean()) - p_drop) < 0.02
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    with torch.enable_grad():
        oh, ox = O.dynamics_forward(leaf, cfg, batch, prot_x, x_t, h_t, t, dropout=drop)
        ((oh * w_h).sum() + (ox * w_x).sum()).backward()
    print(what, "max |eps_h - oracle|", float((eps_h.cpu() - oh.detach()).abs().max()),
          "max |eps_x - oracle|", float((eps_x.cpu() - ox.detach()).abs().max()))
    torch.testing.assert_close(eps_h.cpu(), oh.detach(), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(eps_x.cpu(), ox.detach(), rtol=RTOL, atol=ATOL)
    got = flat_to_dict(eng, eng.train_backward(w_h, w_x))
    ref = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leaf.items()}
    assert sum(r.numel() > 0 and float(r.abs().max()) > 0 for r in ref.values()) >= 50
    compare(got, ref, tol, what)
    return eng, (x_t, h_t, t, prot_x, w_h, w_x), got


# 2. the oracle's autograd at five width pairs, without and with dropout (the engine's own masks fed to the oracle)
@pytest.mark.parametrize("S,V", [(256, 32), (192, 16), (160, 32), (64, 16), (128, 32)])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_gradients_vs_oracle(S, V, p_drop):
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
    batch = O.synthetic_batch([13, 14, 15], 40, [4, 7, 5], cfg)
    oracle_check(cfg, batch, p_drop, 1234, f"wide train {S}/{V} dropout {p_drop}")


# 3. shapes that break structure, one width each
@pytest.mark.parametrize("case,S,V", [("large_radius", 64, 16), ("single_layer_single_center", 96, 32), ("deep", 64, 32),
                                      ("shallow_chains", 192, 32)])
def test_gradients_vs_oracle_more_configs(case, S, V):
    base, seeds, n_prot, n_pharm = EXTRA_CASES[case]
    cfg = O.DynamicsConfig(**{**base.__dict__, "n_hidden_scalars": S, "vector_size": V})
    batch = O.synthetic_batch(seeds, n_prot, n_pharm, cfg)
    oracle_check(cfg, batch, 0.2, 99, f"wide train {case} {S}/{V}")


# 4. 128 / 16 under the wide family: the reference's gradients, and the specialised gradient kernels on the same inputs
@pytest.mark.parametrize("name", sorted(GRAD_CASES))
def test_forced_128_16_gradients_match_reference_golden(name):
    z, cfg = load(name), GRAD_CASES[name]
    reference_step(model_for(cfg, int(z["T"]), int(z["wseed"])), z, cfg, "forced 128/16 " + name)


def test_forced_128_16_agrees_with_the_tuned_family():
    cfg = O.DynamicsConfig()
    batch = O.synthetic_batch([13, 14, 15], 40, [4, 7, 5], cfg)
    eng, (x_t, h_t, t, prot_x, w_h, w_x), got = oracle_check(cfg, batch, 0.1, 77, "wide train 128/16")
    tuned = engine_for(cfg, O.make_state_dict(cfg, 3))
    set_batch(tuned, batch)
    assert tuned.train_family() == "tuned"
    for layer in range(cfg.n_convs):
        for which in (0, 1):
            assert torch.equal(tuned.dropout_mask(layer, which, 0.1, 77), eng.dropout_mask(layer, which, 0.1, 77))
    th, tx = tuned.train_forward(x_t, h_t, t, prot_x=prot_x, dropout=0.1, seed=77)
    wh, wx = eng.train_forward(x_t, h_t, t, prot_x=prot_x, dropout=0.1, seed=77)
    torch.testing.assert_close(wh, th, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(wx, tx, rtol=RTOL, atol=ATOL)
    compare(got, flat_to_dict(tuned, tuned.train_backward(w_h, w_x)), 2e-3, "wide vs tuned 128/16")


# 5. the endpoint parameterisations on the reference's fixtures (loaded as test_gpu_endpoint_loss.py does), a 128 / 16 model on
# the wide family; endpoint_param_coord = endpoint_param_feat = False is the noise parameterisation of the tests above
@pytest.mark.parametrize("prefix", ["both_", "feat_", "coord_"])
def test_endpoint_parameterisations_match_reference_golden(prefix):
    from test_gpu_endpoint_loss import flags_of, inject, set_flags
    z = load("train_endpoint.npz")
    cfg = O.DynamicsConfig()
    m = model_for(cfg, int(z["T"]), int(z["wseed"]))
    set_flags(m, **flags_of(z, prefix))
    g = graph_from(batch_from(z), z["x0"], z["h0"]).to("cuda")
    assert m.dynamics.bind_graph(g).train_family() == "wide"
    losses, metrics = m.forward(g, 'train', **inject(z))          # autograd on: the training forward (eval mode: no dropout)
    for k, v in {**losses, **metrics}.items():
        ref = float(z[prefix + "out_" + k.replace(" ", "_")])
        v = float(v.detach())
        print(prefix, k, v, ref)
        assert abs(v - ref) <= 2e-4 * max(1.0, abs(ref)), (k, v, ref)
    if prefix != "both_":
        return
    grads = {}
    for part in z["grad_parts"].tolist():
        grads.update(load(part))
    m.zero_grad(set_to_none=True)
    loss = m.training_step(g, 0, **inject(z))
    ref_total = float(z["both_out_train_pos_loss"]) + float(z["both_out_train_feat_loss"])
    assert abs(float(loss.detach()) - ref_total) <= 2e-4 * max(1.0, abs(ref_total))
    loss.backward()
    got, ref = {}, {}
    for k, p in m.named_parameters():
        if p.numel() and k.startswith("dynamics."):
            ref[k] = grads["both_grad_" + k]
            got[k] = torch.zeros_like(ref[k]) if p.grad is None else p.grad.cpu()
    assert sum(float(r.abs().max()) > 0 for r in ref.values()) >= 150
    compare(got, ref, 2e-3, "endpoint both")


# 6. the same bits on every run; every element of the gradient vector is stored
@pytest.mark.parametrize("S,V", [(256, 32), (64, 16)])
def test_gradients_are_bitwise_repeatable(S, V):
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
    batch = O.synthetic_batch([13, 14, 15], 40, [4, 7, 5], cfg)
    sd = O.make_state_dict(cfg, 3)
    x_t, h_t, t = inputs(cfg, batch, 4)
    gen = torch.Generator().manual_seed(6)
    w_h, w_x = torch.randn(h_t.shape, generator=gen), torch.randn(x_t.shape, generator=gen)
    grads = []
    for _ in range(2):
        eng = wide_engine(cfg, sd, batch)
        eng.train_forward(x_t, h_t, t, dropout=0.1, seed=5)
        grads.append(eng.train_backward(w_h, w_x))
        grads.append(eng.train_backward(w_h, w_x))                # a second backward of the same forward
    for g in grads[1:]:
        assert torch.equal(g, grads[0])
    assert float(grads[0].abs().max()) > 0
    # the lazy-zero form (FlatAdam.zero_grad(lazy=True)): a buffer full of NaN comes back fully written
    buf = torch.full((eng.n_params,), float("nan"), device="cuda")
    gh, gx = w_h.cuda().contiguous(), w_x.cuda().contiguous()
    eng._ck(eng.lib.pf_train_backward(eng._h, ctypes.c_void_p(gh.data_ptr()), ctypes.c_void_p(gx.data_ptr()),
                                      ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "pf_train_backward")
    assert bool(torch.isfinite(buf).all())
    assert torch.equal(buf, grads[0])


# 7. the switch
def test_switch_semantics():
    import pharmacoforge_amd as pfa
    cfg = O.DynamicsConfig(n_hidden_scalars=64, vector_size=32)
    batch = O.synthetic_batch([0, 1], [48, 40], [3, 4], cfg)
    sd = O.make_state_dict(cfg, 0)
    eng = engine_for(cfg, sd)
    set_batch(eng, batch)
    x_t, h_t, t = inputs(cfg, batch, 1)
    assert eng.train_family() == "tuned"
    before = eng.dynamics(x_t, h_t, t)
    with pytest.raises(pfa.PfError, match="128 / vector_size 16"):
        eng.train_forward(x_t, h_t, t)
    eng.set_train_family("wide")
    assert eng.train_family() == "wide"
    eps_h, eps_x = eng.train_forward(x_t, h_t, t)
    w_h, w_x = torch.ones_like(eps_h), torch.ones_like(eps_x)
    assert bool(torch.isfinite(eng.train_backward(w_h, w_x)).all())
    after = eng.dynamics(x_t, h_t, t)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    # the wide leg is fp32 only, in either order
    with pytest.raises(pfa.PfError, match=r"\(-1\).*fp32 only"):              # PF_ERR_ARG
        eng.set_train_precision("bf16")
    eng.set_train_family("tuned")
    eng.set_train_precision("bf16")
    with pytest.raises(pfa.PfError, match=r"\(-1\).*fp32 only"):
        eng.set_train_family("wide")
    eng.set_train_precision("f32")
    # a backward after switching family has no forward of its own
    eng.set_train_family("wide")
    eng.train_forward(x_t, h_t, t)
    eng.set_train_family("tuned")
    eng.set_train_family("wide")
    with pytest.raises(pfa.PfError, match=r"\(-3\).*no pf_train_forward"):    # PF_ERR_STATE
        eng.train_backward(w_h, w_x)
    with pytest.raises(ValueError):
        eng.set_train_family("narrow")
    sx0 = eng.dynamics(x_t, h_t, t)
    assert torch.equal(before[0], sx0[0]) and torch.equal(before[1], sx0[1])


def test_switch_semantics_at_128_16():
    """a plain 128 / 16 handle takes the wide leg: inference stays on the tuned kernels, bit for bit and by kernel family; a
    backward whose forward ran under the other family is PF_ERR_STATE in both directions; a model keeps the leg across .to()
    and on its prefetch twin; masks of the wrong shape are refused before they reach the device"""
    import pharmacoforge_amd as pfa
    from test_gpu_wide import SPEC_FAMILIES, sample_run
    cfg = O.DynamicsConfig()
    batch = O.synthetic_batch([0, 1], [48, 40], [3, 4], cfg)
    eng = engine_for(cfg, O.make_state_dict(cfg, 0))
    set_batch(eng, batch)
    x_t, h_t, t = inputs(cfg, batch, 1)
    T = 20
    noise = torch.randn(T + 1, int(batch.pharm_ptr[-1]), 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(9))
    before = eng.dynamics(x_t, h_t, t, prot_x=batch.prot_x)
    fam = [eng.kernel_family(layer) for layer in range(cfg.n_convs)]
    assert all(f in SPEC_FAMILIES for f in fam), fam
    s_before = sample_run(eng, T, noise, T)
    set_batch(eng, batch)                     # (a sampling run leaves the pocket recentred: every leg below starts from a fresh bind)
    eps_h, eps_x = eng.train_forward(x_t, h_t, t)                     # tuned forward ...
    w_h, w_x = torch.ones_like(eps_h), torch.ones_like(eps_x)
    g_tuned = eng.train_backward(w_h, w_x)
    eng.train_forward(x_t, h_t, t)
    eng.set_train_family("wide")
    with pytest.raises(pfa.PfError, match=r"\(-3\).*no pf_train_forward"):    # ... is not the wide backward's
        eng.train_backward(w_h, w_x)
    wh, wx = eng.train_forward(x_t, h_t, t)
    torch.testing.assert_close(wh, eps_h, rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(wx, eps_x, rtol=RTOL, atol=ATOL)
    g_wide = eng.train_backward(w_h, w_x)
    compare(flat_to_dict(eng, g_wide), flat_to_dict(eng, g_tuned), 2e-3, "wide vs tuned, one handle")
    eng.train_forward(x_t, h_t, t)
    eng.set_train_family("tuned")
    with pytest.raises(pfa.PfError, match=r"\(-3\).*no pf_train_forward"):
        eng.train_backward(w_h, w_x)
    eng.train_forward(x_t, h_t, t)
    assert torch.equal(eng.train_backward(w_h, w_x), g_tuned)          # the tuned leg after the round trip: the same bits
    eng.set_train_family("wide")
    eng.train_forward(x_t, h_t, t, dropout=0.1, seed=3)
    set_batch(eng, batch)
    after = eng.dynamics(x_t, h_t, t, prot_x=batch.prot_x)
    assert [eng.kernel_family(layer) for layer in range(cfg.n_convs)] == fam
    s_after = sample_run(eng, T, noise, T)
    for a, b in zip(before + s_before, after + s_after):
        print("inference before / after the wide leg: max |difference|", float((a - b).abs().max()))
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="shape"):
        eng.set_dropout_masks(torch.ones(cfg.n_convs, 2, eng.Np + eng.Nf, 100))
    cfg64 = O.DynamicsConfig(n_hidden_scalars=64, vector_size=32)
    e64 = wide_engine(cfg64, O.make_state_dict(cfg64, 0), batch)
    with pytest.raises(ValueError, match="shape"):
        e64.set_dropout_masks(torch.ones(cfg64.n_convs, 2, e64.Np + e64.Nf, 144))
    # the model class: set before the engine exists, kept across .to(), carried to the prefetch twin
    m = model_for(cfg, 50, 0)
    m = m.to("cpu").to("cuda")
    Nf = int(batch.pharm_ptr[-1])
    g = graph_from(batch, torch.zeros(Nf, 3), torch.zeros(Nf, cfg.pharm_nf)).to("cuda")
    assert m.dynamics.bind_graph(g).train_family() == "wide"
    g2 = graph_from(O.synthetic_batch([5], [40], [3], cfg), torch.zeros(3, 3), torch.zeros(3, cfg.pharm_nf)).to("cuda")
    m.dynamics.prefetch_graph(g2)
    assert m.dynamics.bind_graph(g2).train_family() == "wide"


# 8. it trains
def fixed_batch_curve(m, g, steps, draws):
    import pharmacoforge_amd as pfa
    m.train()
    opt = pfa.FlatAdam(m.dynamics, lr=1e-3)
    curve = []
    for _ in range(steps):
        opt.zero_grad(lazy=True)
        loss = m.training_step(g, 0, **draws)
        loss.backward()
        opt.step()
        curve.append(float(loss.detach()))
    return curve


def test_it_trains_saves_loads_and_samples(tmp_path):
    import pharmacoforge_amd as pfa
    cfg = O.DynamicsConfig(n_hidden_scalars=64, vector_size=32)
    T = 100
    m = model_for(cfg, T, 2)
    batch = O.synthetic_batch([21, 22], [40, 36], [4, 5], cfg)
    Nf, B = int(batch.pharm_ptr[-1]), batch.batch_size
    gen = torch.Generator().manual_seed(3)
    x0 = 3.0 * torch.randn(Nf, 3, generator=gen)
    h0 = torch.nn.functional.one_hot(torch.randint(0, cfg.pharm_nf, (Nf,), generator=gen), cfg.pharm_nf).float()
    g = graph_from(batch, x0, h0).to("cuda")
    draws = dict(t_int=torch.randint(0, T, (B,), generator=gen), eps={'h': torch.randn(Nf, cfg.pharm_nf, generator=gen),
                                                                      'x': torch.randn(Nf, 3, generator=gen)})
    torch.manual_seed(0)
    curve = fixed_batch_curve(m, g, 30, draws)
    print("loss curve (64, 32):", curve[0], "->", curve[-1])
    assert all(c == c for c in curve) and curve[-1] < 0.9 * curve[0], curve
    path = tmp_path / "wide.ckpt"
    m.save_checkpoint(path)
    m2 = pfa.PharmacophoreDiff.load_from_checkpoint(str(path)).to("cuda").eval()
    m.eval()
    noise = torch.randn(T + 1, Nf, 3 + cfg.pharm_nf, generator=gen)
    a = m.sample_given_receptor(g, noise=noise)
    b = m2.sample_given_receptor(g, noise=noise)
    for pa, pb in zip(a, b):
        assert bool(torch.isfinite(pa.ph_coords).all())
        assert torch.equal(pa.ph_coords, pb.ph_coords)
    # torch's own optimiser on the module's parameters
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    opt.zero_grad()
    m.training_step(g, 0, **draws).backward()
    opt.step()


def test_wide_curve_tracks_the_tuned_one_at_128_16():
    cfg = O.DynamicsConfig()
    T = 100
    batch = O.synthetic_batch([21, 22], [40, 36], [4, 5], cfg)
    Nf, B = int(batch.pharm_ptr[-1]), batch.batch_size
    gen = torch.Generator().manual_seed(3)
    x0 = 3.0 * torch.randn(Nf, 3, generator=gen)
    h0 = torch.nn.functional.one_hot(torch.randint(0, cfg.pharm_nf, (Nf,), generator=gen), cfg.pharm_nf).float()
    g = graph_from(batch, x0, h0).to("cuda")
    draws = dict(t_int=torch.randint(0, T, (B,), generator=gen), eps={'h': torch.randn(Nf, cfg.pharm_nf, generator=gen),
                                                                      'x': torch.randn(Nf, 3, generator=gen)})
    curves = {}
    for family in ("tuned", "wide"):
        m = model_for(cfg, T, 2, family=family)
        torch.manual_seed(0)
        curves[family] = fixed_batch_curve(m, g, 30, draws)
    print("128/16 curves: tuned", curves["tuned"][0], "->", curves["tuned"][-1], "wide", curves["wide"][0], "->", curves["wide"][-1])
    for a, b in zip(curves["tuned"], curves["wide"]):
        assert abs(a - b) <= 0.02 * abs(a), (a, b)
