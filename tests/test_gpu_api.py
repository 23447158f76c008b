"""GPU tests of the reference-shaped Python API (PharmacophoreDiff / PharmRecDynamicsGVP mirror)
on top of the C ABI: sampling against the reference's golden trajectories and xyz output,
multi-pocket ragged sampling, training-loss forward, checkpoint round trip, and a full-size
config-2 trajectory through size-independent properties."""
import os
import sys

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O
from helpers import batch_from, load

pytestmark = pytest.mark.gpu

DEV_DYN = dict(vector_size=16, n_convs=2, n_hidden_scalars=128, message_norm='mean', dropout=0.1, ff_k=0, pf_k=5,
               n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4)
DEV_GRAPH = {'graph_cutoffs': {'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9}}


def make_model(T, wseed=0):
    m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=T, graph_config=DEV_GRAPH,
                              dynamics_config=DEV_DYN, precision=1e-5)
    sd = dict(O.make_state_dict(O.DynamicsConfig(), wseed))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    return m.to("cuda").eval()


def graph_from(b: O.PocketBatch, x0=None, h0=None):
    nf = int(b.pharm_ptr[-1])
    return pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst,
                           torch.zeros(nf, 3) if x0 is None else x0, torch.zeros(nf, 6) if h0 is None else h0)


def test_sample_given_receptor_matches_reference_golden():
    z = load("traj_c1.npz")
    m = make_model(int(z["T"]))
    g = graph_from(batch_from(z)).to("cuda")
    pharms = m.sample_given_receptor(g, visualize_trajectory=True, noise=z["noise"])
    assert len(pharms) == 1 and pharms[0].n_ph_centers == 4
    torch.testing.assert_close(pharms[0].ph_coords, z["x0"], rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(pharms[0].pos_frames, z["pos_frames"], rtol=5e-3, atol=5e-3)
    # the file the reference writes (generate_pharmacophores.py:357-392 -> pharms.xyz) to 3 decimals
    ours = [l.split() for l in pharms[0].to_xyz_file().splitlines()]
    ref = [l.split() for l in str(z["xyz"]).splitlines()]
    assert ours[0] == ref[0] and [r[0] for r in ours[1:]] == [r[0] for r in ref[1:]]
    for a, b in zip(ours[1:], ref[1:]):
        assert all(abs(float(u) - float(v)) <= 6e-3 for u, v in zip(a[1:], b[1:]))


def test_an_invalid_trajectory_is_never_returned():
    """An exchange time-out inside a step's merged last launch (forced: pf_debug_xchg_fault) raises from the very
    sample_given_receptor call whose results it spoiled -- nothing is built from x_0 / h_0 -- and the model goes on sampling
    (the handle falls back to the separate launches): same result as before the fault to the merged-vs-separate ulp."""
    z = load("traj_c1.npz")
    m = make_model(int(z["T"]))
    g = graph_from(batch_from(z)).to("cuda")
    good = m.sample_given_receptor(g, noise=z["noise"])
    eng = m.dynamics.engine()
    assert eng.kernel_family(2) == 2
    eng.xchg_fault(True, poll_max=64)
    with pytest.raises(pfa.PfError, match="time-out"):
        m.sample_given_receptor(g, noise=z["noise"])
    eng.xchg_fault(False)
    again = m.sample_given_receptor(g, noise=z["noise"])
    assert eng.kernel_family(2) == 0
    torch.testing.assert_close(again[0].ph_coords, good[0].ph_coords, rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(again[0].ph_coords, z["x0"], rtol=5e-3, atol=5e-3)


def test_dynamics_module_forward_signature():
    z = load("dynamics_ragged.npz")
    m = make_model(100)
    g = graph_from(batch_from(z)).to("cuda")
    g.prot_x = z["prot_x"].cuda()
    g.x_t, g.h_t = z["x_t"].cuda(), z["h_t"].cuda()
    eps_h, eps_x = m.dynamics(g, z["t"].cuda(), g.batch_idxs())
    torch.testing.assert_close(eps_h.cpu(), z["eps_h"], rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(eps_x.cpu(), z["eps_x"], rtol=2e-4, atol=2e-4)


def test_training_loss_forward_matches_reference_golden():
    z = load("train_fwd.npz")
    m = make_model(int(z["T"]))
    g = graph_from(batch_from(z), z["x0"], z["h0"]).to("cuda")
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    with torch.no_grad():                      # pruned inference kernels
        losses, metrics = m.forward(g, 'train', **inj)
    losses_g, _ = m.forward(g, 'train', **inj)  # autograd on: dense training forward (eval mode: no dropout)
    for k, v in {**losses, **metrics}.items():
        ref = float(z["out_" + k.replace(" ", "_")])
        assert abs(float(v) - ref) <= 2e-4 * max(1.0, abs(ref)), (k, float(v), ref)
    for k, v in losses_g.items():
        assert v.requires_grad
        assert abs(float(v.detach()) - float(losses[k])) <= 2e-5 * max(1.0, abs(float(losses[k])))


@pytest.mark.parametrize("remove_com,weighted", [(True, False), (False, True)])
def test_fused_loss_call_equals_the_framework_restatement(remove_com, weighted):
    """pf_train_loss_forward / _backward (one C-ABI call each) against forward()'s op-by-op restatement of
    pharmacodiff.py:162-243 around pf_train_forward / pf_train_backward: same draws, same losses, metrics and gradients."""
    z = load("train_fwd.npz")
    m = make_model(int(z["T"]))
    m.remove_com, m.weighted_loss = remove_com, weighted
    g = graph_from(batch_from(z), z["x0"], z["h0"]).to("cuda")
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    res = {}
    for fused in (True, False):
        m.fused_loss = fused
        m.zero_grad(set_to_none=True)
        losses, metrics = m.forward(g, 'train', **inj)
        (losses['train pos loss'] * 0.75 + losses['train feat loss'] * 1.5).backward()
        res[fused] = ({k: float(v.detach()) for k, v in {**losses, **metrics}.items()}, m.dynamics._last_flat_grad.clone())
    for k, v in res[True][0].items():
        assert abs(v - res[False][0][k]) <= 2e-5 * max(1.0, abs(v)), (k, v, res[False][0][k])
    ga, gb = res[True][1], res[False][1]
    assert float((ga - gb).abs().max()) <= 1e-4 * float(gb.abs().max())


def _golden_masks(z, cfg, Np, Nf):
    """[n_convs, 2, N, 144] multipliers in the engine's layout (global node ids: protein atoms first) from the
    GVPDropout draws the reference made (tests/golden/make_golden.py:golden_train_grads)."""
    out = torch.ones(cfg.n_convs, 2, Np + Nf, 144)
    for layer in range(cfg.n_convs):
        for w, which in enumerate(("msg", "res")):
            for nt, sl in (("prot", slice(0, Np)), ("pharm", slice(Np, Np + Nf))):
                out[layer, w, sl, :128] = z[f"drop_{layer}_{nt}_{which}_s"]
                out[layer, w, sl, 128:] = z[f"drop_{layer}_{nt}_{which}_v"]
    return out


def test_training_step_gradients_match_reference_golden():
    """One reference training_step in train() mode (dropout 0.1): loss.backward() through the HIP backward kernels
    gives the reference's own parameter gradients (its GVPDropout draws injected as masks)."""
    z = load("train_grads.npz")
    cfg = O.DynamicsConfig()
    m = make_model(int(z["T"]))
    m.train()
    b = batch_from(z)
    g = graph_from(b, z["x0"], z["h0"]).to("cuda")
    Np, Nf = int(b.prot_ptr[-1]), int(b.pharm_ptr[-1])
    eng = m.dynamics.bind_graph(g)
    eng.set_dropout_masks(_golden_masks(z, cfg, Np, Nf))
    loss = m.training_step(g, 0, t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    ref_total = float(z["out_train_pos_loss"]) + float(z["out_train_feat_loss"])
    assert abs(float(loss.detach()) - ref_total) <= 2e-4 * max(1.0, abs(ref_total))
    loss.backward()
    eng.set_dropout_masks(None)
    bad, live = [], 0
    for k, p in m.named_parameters():
        if p.numel() == 0 or not k.startswith("dynamics."):
            continue
        ref = z["grad_" + k]
        got = torch.zeros_like(ref) if p.grad is None else p.grad.cpu()
        scale = float(ref.abs().max())
        live += scale > 0
        if float((got - ref).abs().max()) > 2e-3 * scale + 1e-7:
            bad.append((k, float((got - ref).abs().max()), scale))
    assert not bad, (bad[:6], len(bad))
    assert live >= 150


def test_bf16_training_leg_gradients_against_the_reference_golden():
    """The same reference training_step through the bf16 leg (PharmRecDynamicsGVP.set_train_precision('bf16'); no reference
    counterpart, the reference trains in fp32): loss within 1e-3 relative of the reference's, every parameter gradient with
    cosine >= 0.999 and relative L2 error <= 2e-2 against the reference's own."""
    z = load("train_grads.npz")
    cfg = O.DynamicsConfig()
    m = make_model(int(z["T"]))
    m.train()
    m.dynamics.set_train_precision("bf16")
    b = batch_from(z)
    g = graph_from(b, z["x0"], z["h0"]).to("cuda")
    Np, Nf = int(b.prot_ptr[-1]), int(b.pharm_ptr[-1])
    eng = m.dynamics.bind_graph(g)
    assert eng.train_precision() == "bf16"
    eng.set_dropout_masks(_golden_masks(z, cfg, Np, Nf))
    loss = m.training_step(g, 0, t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    ref_total = float(z["out_train_pos_loss"]) + float(z["out_train_feat_loss"])
    assert abs(float(loss.detach()) - ref_total) <= 1e-3 * max(1.0, abs(ref_total))
    loss.backward()
    eng.set_dropout_masks(None)
    live = 0
    for k, p in m.named_parameters():
        if p.numel() == 0 or not k.startswith("dynamics."):
            continue
        ref = z["grad_" + k].double().reshape(-1)
        if float(ref.abs().max()) == 0.0:
            continue
        got = p.grad.cpu().double().reshape(-1)
        live += 1
        cos = float((ref * got).sum() / (ref.norm() * got.norm()))
        rel = float((ref - got).norm() / ref.norm())
        assert cos >= 0.999 and rel <= 2e-2, (k, cos, rel)
    assert live >= 150


def test_optimizer_steps_refresh_the_engine_and_reduce_the_loss():
    """Adam on the module's parameters (views of one flat device vector): after every step the engine sees the new
    values (device-side gather into the packed weights), the inference path agrees with the oracle on the updated
    state dict, and the loss of a fixed batch goes down."""
    z = load("train_grads.npz")
    cfg = O.DynamicsConfig()
    m = make_model(int(z["T"]))
    m.train()
    m.dynamics.dropout_rate = 0.0
    b = batch_from(z)
    g = graph_from(b, z["x0"], z["h0"]).to("cuda")
    opt = torch.optim.Adam(m.parameters(), lr=2e-3)
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    losses = []
    for _ in range(12):
        opt.zero_grad(set_to_none=True)
        loss = m.training_step(g, 0, **inj)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < 0.95 * losses[0] and all(torch.isfinite(torch.tensor(losses))), losses
    # engine state == module state == what the oracle computes with those weights
    eng = m.dynamics.engine()
    flat = eng.get_flat_params().cpu()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for name, off, n in eng.param_layout():
        assert torch.equal(flat[off:off + n], sd[name].reshape(-1)), name
    m.eval()
    with torch.no_grad():
        l_eng, _ = m.forward(g, 'val', **inj)
    l_ref, _ = O.training_forward(sd, cfg, b, z["x0"], z["h0"], int(z["T"]), 1e-5, z["t_int"].long(), z["eps_h"], z["eps_x"],
                                  phase="val")
    for k in l_ref:
        assert abs(float(l_eng[k]) - float(l_ref[k])) <= 5e-4 * max(1.0, abs(float(l_ref[k]))), (k, float(l_eng[k]), float(l_ref[k]))


def test_multi_pocket_ragged_sampling_and_checkpoint(tmp_path):
    """PharmacophoreDiff.sample (pharmacodiff.py:516-578): 3 pockets, ragged pharmacophore sizes,
    chunks of max_batch_size, regrouped per pocket; a checkpoint round trip gives the same samples."""
    cfg = O.DynamicsConfig()
    m = make_model(20)
    pockets = [graph_from(O.synthetic_batch([s], 48, 1, cfg)) for s in (21, 22, 23)]
    n_pharms = [[3, 4], [5], [8, 3, 6]]
    torch.manual_seed(0)
    out = m.sample(pockets, n_pharms, max_batch_size=4)
    assert [len(o) for o in out] == [2, 1, 3]
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    assert all(torch.isfinite(p.ph_coords).all() for o in out for p in o)
    ck = tmp_path / "m.ckpt"
    m.save_checkpoint(ck)
    m2 = pfa.PharmacophoreDiff.load_from_checkpoint(ck).to("cuda").eval()
    torch.manual_seed(0)
    out2 = m2.sample(pockets, n_pharms, max_batch_size=4)
    for a, b in zip(out, out2):
        for pa, pb in zip(a, b):
            assert torch.equal(pa.ph_coords, pb.ph_coords)          # deterministic kernels: bitwise repeatable
    # 2-way sharding of the same job: union of the ranks' samples == the single-rank result
    torch.manual_seed(0)
    r0 = m.sample(pockets, n_pharms, max_batch_size=4, rank=0, world_size=2)
    r1 = m.sample(pockets, n_pharms, max_batch_size=4, rank=1, world_size=2)
    assert [len(a) + len(b) for a, b in zip(r0, r1)] == [2, 1, 3]


def test_sample_multi_pocket_matches_reference_golden():
    """PharmacophoreDiff.sample + copy_graph against the reference's own run (tests/golden/sample_multi.npz:
    pharmacodiff.py:516-578 over three pockets of 40 / 52 / 33 atoms, requests [[3,4],[5],[8,3,6]], batches of 4, explicit
    init_pharm_com, its noise draws injected per batch): per-pocket grouping, sizes, coordinates, features, xyz text, and
    the protein frame the samples are returned in."""
    z = load("sample_multi.npz")
    cfg = O.DynamicsConfig()
    m = make_model(int(z["T"]), int(z["wseed"]))
    pockets = [graph_from(O.synthetic_batch([int(s)], int(n), 1, cfg)) for s, n in zip(z["pocket_seeds"], z["pocket_n_prot"])]
    sizes, per = z["n_pharms_flat"].tolist(), z["n_pharms_per_pocket"].tolist()
    n_pharms, k = [], 0
    for c in per:
        n_pharms.append(sizes[k:k + c]); k += c
    out = m.sample(pockets, n_pharms, max_batch_size=int(z["max_batch_size"]), init_pharm_com=z["init_pharm_com"],
                   noise=[z["noise_0"], z["noise_1"]])
    assert [len(o) for o in out] == per and [[p.n_ph_centers for p in o] for o in out] == n_pharms
    flat = [p for o in out for p in o]
    torch.testing.assert_close(torch.cat([p.ph_coords for p in flat]), z["x0"], rtol=5e-3, atol=5e-3)
    torch.testing.assert_close(torch.cat([p.g.pharm_h0 for p in flat]), z["h0"], rtol=5e-3, atol=5e-3)
    ours = [l.split() for l in "".join(p.to_xyz_file() for p in flat).splitlines()]
    ref = [l.split() for l in str(z["xyz"]).splitlines()]
    assert len(ours) == len(ref)
    for a, b in zip(ours, ref):
        assert a[0] == b[0] and all(abs(float(u) - float(v)) <= 6e-3 for u, v in zip(a[1:], b[1:])), (a, b)


def test_sample_lanes_edge_cases():
    """sample() with batches in flight on several handles: empty requests, fewer batches than lanes, trajectories -- counts,
    sizes, and bitwise the results of one lane."""
    m = make_model(20)
    cfg = O.DynamicsConfig()
    pockets = []
    for i in range(5):
        b = O.synthetic_batch([900 + i], 40 + 30 * i, 1, cfg)
        pockets.append(pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst, torch.zeros(1, 3), torch.zeros(1, 6)))
    cases = [("no pockets", [], [], 8, None),
             ("one pocket, one sample", pockets[:1], [[3]], 8, None),
             ("one pocket, empty request", pockets[:1], [[]], 8, None),
             ("mixed empty", pockets[:3], [[4, 5], [], [1]], 2, None),
             ("many tiny batches, four lanes", pockets, [[3, 4, 5, 6, 7, 8, 1]] * 5, 3, 4),
             ("more lanes than batches", pockets[:2], [[3], [4]], 1, 7),
             ("trajectories", pockets[:2], [[3, 4], [5]], 2, 2)]
    with torch.no_grad():
        for desc, ps, ns, mb, lanes in cases:
            traj = desc == "trajectories"
            torch.manual_seed(1)
            out = m.sample(ps, ns, max_batch_size=mb, lanes=lanes, visualize_trajectory=traj)
            assert [len(o) for o in out] == [len(n) for n in ns], desc
            assert all(p.n_ph_centers == k for o, n in zip(out, ns) for p, k in zip(o, n)), desc
            assert all(torch.isfinite(p.ph_coords).all() for o in out for p in o), desc
            torch.manual_seed(1)
            ref = m.sample(ps, ns, max_batch_size=mb, lanes=1, visualize_trajectory=traj)
            for o, r in zip(out, ref):
                for p, q in zip(o, r):
                    assert torch.equal(p.ph_coords, q.ph_coords) and torch.equal(p.ph_feats_idxs, q.ph_feats_idxs), desc
                    if traj:
                        assert torch.equal(p.pos_frames, q.pos_frames), desc


def test_bind_graph_rebinds_look_alike_batches():
    """Two batches with the same totals (same pocket, center counts [3, 5] vs [5, 3]) passed as temporaries: the second
    call must not run on the first batch's graph boundaries (the cache key holds the ptr contents and the module keeps
    the bound tensors alive, so addresses cannot be recycled into a false hit)."""
    cfg = O.DynamicsConfig()
    m = make_model(100)
    pocket = O.synthetic_batch([77], 48, 1, cfg)
    gen = torch.Generator().manual_seed(2)
    x_t, h_t = torch.randn(8, 3, generator=gen), torch.randn(8, 6, generator=gen)
    t = torch.tensor([0.3, 0.7])
    outs = []
    for sizes in ([3, 5], [5, 3]):
        b = O.concat_pockets([O.copy_pocket(pocket, n) for n in sizes])
        def call():
            g = graph_from(b).to("cuda")           # a temporary: freed when call() returns
            g.x_t, g.h_t = x_t.cuda(), h_t.cuda()
            return m.dynamics(g, t.cuda(), None)
        eh, ex = call()
        oh, ox = O.dynamics_forward(O.make_state_dict(cfg, 0), cfg, b, b.prot_x, x_t, h_t, t)
        torch.testing.assert_close(eh.cpu(), oh, rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(ex.cpu(), ox, rtol=2e-4, atol=2e-4)
        outs.append(eh.cpu())
    assert not torch.allclose(outs[0], outs[1])


def test_back_to_back_binds_keep_their_own_tables():
    """pf_set_pocket_batch uploads the table section on a copy stream into one of two alternating device buffers: six different
    batches are bound and run back to back WITHOUT any synchronisation in between (the upload of bind k + 1 overlaps the
    kernels of bind k, bind k + 2 reuses the buffer of bind k), and every result must equal that of a fresh engine that
    sees only its batch."""
    cfg = O.DynamicsConfig()
    sd = {k: v for k, v in pfa.synthetic.make_state_dict(0).items()}
    eng = pfa.PfEngine(device=torch.device("cuda", 0))
    eng.load_state_dict(sd)
    gen = torch.Generator().manual_seed(5)
    cases = []
    for i, (n_atoms, sizes) in enumerate([(64, [3, 5, 4]), (48, [6]), (80, [2, 2, 7, 3]), (64, [5, 3, 4]), (40, [8, 1]), (72, [4, 4, 4])]):
        b = O.concat_pockets([O.synthetic_batch([100 + 10 * i + j], n_atoms, n, cfg) for j, n in enumerate(sizes)])
        Nf = int(b.pharm_ptr[-1])
        cases.append((b, torch.randn(Nf, 3, generator=gen), torch.randn(Nf, 6, generator=gen), torch.rand(len(sizes), generator=gen)))
    outs = []
    for b, x, h, t in cases:                    # no synchronisation inside this loop
        eng.set_batch(b.prot_x.cuda(), b.prot_h.cuda(), b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst)
        outs.append(eng.dynamics(x.cuda(), h.cuda(), t.cuda()))
    torch.cuda.synchronize()
    for (b, x, h, t), (eh, ex) in zip(cases, outs):
        fresh = pfa.PfEngine(device=torch.device("cuda", 0))
        fresh.load_state_dict(sd)
        fresh.set_batch(b.prot_x.cuda(), b.prot_h.cuda(), b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst)
        fh, fx = fresh.dynamics(x.cuda(), h.cuda(), t.cuda())
        assert torch.equal(eh, fh) and torch.equal(ex, fx)
        oh, ox = O.dynamics_forward(O.make_state_dict(cfg, 0), cfg, b, b.prot_x, x, h, t)
        torch.testing.assert_close(eh.cpu(), oh, rtol=2e-4, atol=2e-4)
        torch.testing.assert_close(ex.cpu(), ox, rtol=2e-4, atol=2e-4)


def test_loss_vector_carries_the_sums_a_step_derives():
    """pf_train_loss_forward's entries 6..8 (total loss, total error, weighted total error) are what training_step reports, and
    pf_train_loss_backward_out with a gradient on entry 6 equals pf_train_loss_backward with that gradient on both losses."""
    z = load("train_fwd.npz")
    m = make_model(int(z["T"]))
    g = graph_from(batch_from(z), z["x0"], z["h0"]).to("cuda")
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    loss = m.training_step(g, 0, **inj)
    lm = m.last_metrics
    assert abs(float(loss.detach()) - (float(lm['train pos loss']) + float(lm['train feat loss']))) <= 1e-6 * max(1.0, abs(float(loss.detach())))
    assert abs(float(lm['train total error']) - (float(lm['train position error']) + 1 - float(lm['train accuracy']))) <= 1e-6
    assert abs(float(lm['train weighted total error'])
               - (float(lm['train weighted position error']) + 1 - float(lm['train weighted accuracy']))) <= 1e-6
    m.zero_grad(set_to_none=True)
    loss.backward()
    g_total = m.dynamics._last_flat_grad.clone()
    m.zero_grad(set_to_none=True)
    losses, _ = m.forward(g, 'train', **inj)
    (losses['train pos loss'] + losses['train feat loss']).backward()
    g_sum = m.dynamics._last_flat_grad
    assert torch.equal(g_total, g_sum)


def test_full_size_config2_batch_properties():
    """BASELINE config 2 at full size (B=32 x 256 atoms x 6 centers), 25 steps of the T=500 schedule:
    finite, bitwise reproducible, and invariant to a rigid motion of the whole input (the sampler's
    output frame is tied to the pocket)."""
    cfg = O.DynamicsConfig()
    m = make_model(500)
    b = O.synthetic_batch(range(400, 432), 256, 6, cfg)
    g = graph_from(b).to("cuda")
    eng = m.dynamics.bind_graph(g)
    coef = m.step_coefficients()
    arr = eng.coef_array(coef, reversed(range(25)))
    gen = torch.Generator().manual_seed(9)
    noise = torch.randn(26, 192, 9, generator=gen)
    x1, h1 = eng.sample(arr, 25, noise)
    x2, h2 = eng.sample(arr, 25, noise)
    assert torch.isfinite(x1).all() and torch.equal(x1, x2) and torch.equal(h1, h2)
    _, _, ne = eng.work()
    assert ne[1] == 32 * 6 * 5 and ne[2] == ne[1] and ne[3] == b.pp_src.numel()
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    # rotate pocket AND noise: outputs rotate with them (equivariance of the whole sampler)
    g2 = graph_from(O.PocketBatch(b.prot_x @ q.T + 3.0, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst)).to("cuda")
    eng2 = m.dynamics.bind_graph(g2)
    noise_r = noise.clone()
    noise_r[:, :, :3] = noise[:, :, :3] @ q.T
    x3, h3 = eng2.sample(arr, 25, noise_r)
    torch.testing.assert_close(x3.cpu(), x1.cpu() @ q.T + 3.0, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(h3.cpu(), h1.cpu(), rtol=2e-2, atol=2e-2)


def test_flat_adam_matches_torch_adam():
    """pf_adam_step (one fused kernel on the flat vector) == torch.optim.Adam on the 244 tensors, three steps."""
    z = load("train_grads.npz")
    b = batch_from(z)
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    outs = []
    for use_flat in (False, True):
        m = make_model(int(z["T"]))
        m.train()
        m.dynamics.dropout_rate = 0.0
        g = graph_from(b, z["x0"], z["h0"]).to("cuda")
        opt = (pfa.FlatAdam(m.dynamics, lr=1e-3, weight_decay=1e-2) if use_flat
               else torch.optim.Adam(m.dynamics.parameters(), lr=1e-3, weight_decay=1e-2))
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            m.training_step(g, 0, **inj).backward()
            opt.step()
        outs.append({k: v.detach().cpu().clone() for k, v in m.dynamics.state_dict().items()})
        with torch.no_grad():
            outs.append(m.eval().forward(g, 'val', **inj)[0])
    sd_t, l_t, sd_f, l_f = outs
    for k in sd_t:
        if sd_t[k].numel():
            torch.testing.assert_close(sd_f[k], sd_t[k], rtol=2e-4, atol=2e-6, msg=k)
    for k in l_t:
        assert abs(float(l_t[k]) - float(l_f[k])) <= 1e-4 * max(1.0, abs(float(l_t[k])))


def _write_pocket_files(tmp_path, n_res=24, seed=3):
    """A small synthetic receptor (standard residues around the origin + far ones) and a ligand at the origin."""
    rng = torch.Generator().manual_seed(seed)
    lines, serial = [], 1
    names = [("N", "N"), ("CA", "C"), ("C", "C"), ("O", "O"), ("CB", "C")]
    for r in range(n_res):
        centre = (6.0 if r < n_res - 4 else 40.0) * torch.nn.functional.normalize(torch.randn(3, generator=rng), dim=0)
        for name, el in names:
            x, y, z = (centre + 1.2 * torch.randn(3, generator=rng)).tolist()
            lines.append(f"ATOM  {serial:>5}  {name:<3} ALA A{r + 1:>4}    {x:8.3f}{y:8.3f}{z:8.3f}  1.00 20.00          {el:>2}")
            serial += 1
    (tmp_path / "rec.pdb").write_text("\n".join(lines) + "\nEND\n")
    sdf = ["lig", "  t", "", "  3  2  0  0  0  0  0  0  0  0999 V2000"]
    for x, el in ((-0.7, "C"), (0.0, "N"), (0.7, "O")):
        sdf.append(f"{x:10.4f}{0.0:10.4f}{0.0:10.4f} {el:<3} 0  0  0  0  0  0  0  0  0  0  0  0")
    sdf += ["  1  2  1  0", "  2  3  1  0", "M  END", "$$$$"]
    (tmp_path / "lig.sdf").write_text("\n".join(sdf) + "\n")


def test_generate_pharmacophores_cli_end_to_end(tmp_path):
    """The reference's CLI surface (generate_pharmacophores.py:29-66, 236-392): run dir with config.yaml + checkpoints/
    last.ckpt, PDB receptor + SDF ligand -> <out>/<receptor>/pharms.xyz, pocket.pdb, sample_time.txt, reference_files/."""
    import subprocess
    import sys
    import yaml
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_pocket_files(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    cfg['diffusion']['n_timesteps'] = 12
    cfg['dataset']['pocket_cutoff'] = 8
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True)
    yaml.dump(cfg, open(run / "config.yaml", "w"))
    m = pfa.model_from_config(cfg)
    sd = dict(O.make_state_dict(O.DynamicsConfig(), 0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m.save_checkpoint(run / "checkpoints" / "last.ckpt")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
           str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "5", "--pharm_sizes", "3", "4", "5", "6", "8",
           "--max_batch_size", "3", "--output_dir", str(out), "--seed", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    pdir = out / "rec"
    xyz = (pdir / "pharms.xyz").read_text().splitlines()
    counts, i = [], 0
    while i < len(xyz):
        n = int(xyz[i]); counts.append(n)
        for l in xyz[i + 1:i + 1 + n]:
            el, x, y, z = l.split()
            assert el in "PSFNOC" and all(abs(float(v)) < 1e4 for v in (x, y, z))
        i += n + 1
    # copy_graph always indexes pharm_sizes from 0 (the reference's quirk): chunks of 3 and 2 samples
    assert counts == [3, 4, 5, 3, 4]
    assert (pdir / "pocket.pdb").exists() and (pdir / "sample_time.txt").exists()
    assert (pdir / "reference_files" / "rec.pdb").exists() and (pdir / "reference_files" / "lig.sdf").exists()
    # 20 residues within 8 A of the ligand, 5 heavy atoms each
    assert sum(l.startswith("ATOM") for l in (pdir / "pocket.pdb").read_text().splitlines()) == 100
    # ---- value level: the file against the CPU oracle on the same pocket and the same draws.  The CLI seeds torch (--seed 1),
    # builds the model on the host and draws each chunk's noise on the device as one randn(T + 1, Nf, 9) (models.py:
    # _sample_enqueue) -- the same two draws here.  Pocket: pocket_io on the same files with the ORACLE's radius graph (so the
    # GPU radius graph, the ingestion, copy_graph, the sampler and the xyz writer are all inside the comparison).
    from pharmacoforge_amd import pocket_io as P
    emap, _ = P.get_prot_atom_ph_type_maps(cfg['dataset'])
    res = P.select_pocket_residues(P.read_pdb(tmp_path / "rec.pdb"), P.parse_ligand(tmp_path / "lig.sdf", True)[1], 8.0)
    pos = torch.tensor([a.coord.tolist() for r in res for a in r.atoms])
    e = O.radius_graph(pos, 3.5, torch.tensor([0, pos.shape[0]]), 100)
    pk = P.process_ligand_and_pocket(tmp_path / "rec.pdb", None, emap, cfg['graph']['graph_cutoffs'], 8.0, lig_file=tmp_path / "lig.sdf",
                                     pp_edges=(e[0], e[1]))
    pocket1 = O.PocketBatch(pk.prot_x, pk.prot_h, torch.tensor([0, pk.prot_x.shape[0]]), torch.tensor([0, 1]), pk.pp_src.long(), pk.pp_dst.long())
    T = 12
    torch.manual_seed(1)
    noises = [torch.randn(T + 1, n, 9, device="cuda").cpu() for n in (12, 7)]           # chunks [3, 4, 5] and [3, 4]
    want = []
    with torch.no_grad():
        for sizes, nz in zip(([3, 4, 5], [3, 4]), noises):
            b = O.concat_pockets([O.copy_pocket(pocket1, n) for n in sizes])
            x0, h0 = O.sample_given_receptor(sd, O.DynamicsConfig(), b, T, float(cfg['diffusion'].get('precision', 1e-5)), nz)
            want += list(zip(x0.tolist(), h0.argmax(1).tolist()))
    rows = [l.split() for l in xyz if len(l.split()) == 4]
    assert len(rows) == len(want) == 19
    scale = max(abs(float(v)) for r in rows for v in r[1:])
    for r, (xw, kw) in zip(rows, want):
        assert r[0] == "PSFNOC"[kw], (r, kw)
        assert all(abs(float(u) - v) <= 5e-3 * max(1.0, scale) for u, v in zip(r[1:], xw)), (r, xw)


def test_train_driver_smoke(tmp_path):
    """train.py on a tiny processed dataset in the reference's on-disk layout: a few optimiser steps, a validation
    pass and a checkpoint that load_from_checkpoint reads back."""
    import subprocess
    import sys
    import yaml
    import os
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(0)
    proc = tmp_path / "processed"
    for split in range(3):
        d = proc / f"split_{split}"
        d.mkdir(parents=True)
        n_g = 6
        np_, nf_ = np.full(n_g, 40), rng.integers(3, 8, n_g)
        pos = np.concatenate([O.synthetic_pocket(100 * split + i, 40)[0].numpy() for i in range(n_g)]).astype(np.float32)

        def idx(c):
            e = np.cumsum(c)
            return np.stack([e - c, e], 1)
        np.savez(d / 'prot_pharm_tensors.npz', prot_pos=pos, prot_feat=rng.integers(0, 4, np_.sum()), prot_idx=idx(np_),
                 pharm_pos=(rng.normal(size=(nf_.sum(), 3)) * 3).astype(np.float32), pharm_feat=rng.integers(0, 6, nf_.sum()),
                 pharm_idx=idx(nf_), prot_ph_pos=np.zeros((0, 3), np.float32), prot_ph_feat=np.zeros((0,), np.int64),
                 prot_ph_idx=np.zeros((n_g, 2), np.int64))
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    cfg['dataset'].update(processed_data_dir=str(proc), raw_data_dir=str(tmp_path), pocket_cutoff=8)
    cfg['training'].update(output_dir=str(tmp_path / "runs"), batch_size=4, num_workers=0, validation_splits=[2])
    cfg['training'].setdefault('trainer_args', {})['max_epochs'] = 1
    cfg.setdefault('wandb', {})['name'] = 'smoke'
    yaml.dump(cfg, open(tmp_path / "cfg.yml", "w"))
    r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "--config", str(tmp_path / "cfg.yml"), "--seed", "0",
                        "--bind_prefetch"],                  # (the look-ahead bind on the twin handle: same results, exercised here)
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "val total loss" in r.stdout
    ck = list((tmp_path / "runs").glob("*/checkpoints/last.ckpt"))
    assert len(ck) == 1 and (ck[0].parent.parent / "config.yaml").exists()
    m = pfa.PharmacophoreDiff.load_from_checkpoint(ck[0])
    ref = O.make_state_dict(O.DynamicsConfig(), 0)
    k = "dynamics.noise_predictor.noise_predictor.to_scalar_output.bias"
    assert m.state_dict()[k].shape == ref[k].shape and torch.isfinite(m.state_dict()[k]).all()


def _tiny_run_dir(tmp_path, T=10):
    """processed dataset in the reference layout (3 splits x 5 pockets of 40 atoms, 2-3 receptor pharmacophore points
    each) + a run directory (config.yaml, checkpoints/last.ckpt) with seeded weights."""
    import os
    import numpy as np
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(1)
    proc = tmp_path / "processed"
    for split in range(3):
        d = proc / f"split_{split}"
        d.mkdir(parents=True)
        n_g = 5
        np_, nf_, nh_ = np.full(n_g, 40), rng.integers(3, 8, n_g), rng.integers(2, 4, n_g)
        pos = np.concatenate([O.synthetic_pocket(200 * split + i, 40)[0].numpy() for i in range(n_g)]).astype(np.float32)

        def idx(c):
            e = np.cumsum(c)
            return np.stack([e - c, e], 1)
        np.savez(d / 'prot_pharm_tensors.npz', prot_pos=pos, prot_feat=rng.integers(0, 4, np_.sum()), prot_idx=idx(np_),
                 pharm_pos=(rng.normal(size=(nf_.sum(), 3)) * 3).astype(np.float32), pharm_feat=rng.integers(0, 6, nf_.sum()),
                 pharm_idx=idx(nf_), prot_ph_pos=(rng.normal(size=(nh_.sum(), 3)) * 4).astype(np.float32),
                 prot_ph_feat=rng.integers(0, 6, nh_.sum()), prot_ph_idx=idx(nh_))
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    cfg['diffusion']['n_timesteps'] = T
    cfg['dataset'].update(processed_data_dir=str(proc), raw_data_dir=str(tmp_path), pocket_cutoff=8)
    cfg['training'].update(output_dir=str(tmp_path / "runs"), batch_size=4, num_workers=0, validation_splits=[2])
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True)
    yaml.dump(cfg, open(run / "config.yaml", "w"))
    m = pfa.model_from_config(cfg)
    sd = dict(O.make_state_dict(O.DynamicsConfig(), 0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m.save_checkpoint(run / "checkpoints" / "last.ckpt")
    return root, run


@pytest.mark.parametrize("world", [1, 2])
def test_dataset_sampling_driver(tmp_path, world):
    """test.py (the reference's dataset-scale sampling driver, config 4's workflow): every validation pocket gets
    samples_per_pocket pharmacophores; with 2 ranks the pockets are dealt over the ranks and the metric counters are
    all-reduced."""
    import subprocess
    import sys
    import os
    root, run = _tiny_run_dir(tmp_path)
    out = tmp_path / "samples"
    base = [os.path.join(root, "test.py"), "--model_dir", str(run), "--samples_per_pocket", "3", "--pharm_sizes", "3", "5", "4",
            "--max_batch_size", "4", "--output_dir", str(out), "--metrics", "--pockets_per_call", "2"]
    if world == 1:
        cmd = [sys.executable] + base
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", "29677"] + base
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    for i in range(5):
        xyz = (out / f"pocket_{i}" / "pharms.xyz").read_text().splitlines()
        counts, j = [], 0
        while j < len(xyz):
            counts.append(int(xyz[j])); j += counts[-1] + 1
        assert counts == [3, 5, 4], (i, counts)
        assert (out / f"pocket_{i}" / "sample_time.txt").exists()
    metrics = dict(l.split(": ") for l in (out / "metrics.txt").read_text().splitlines())
    assert 0.0 <= float(metrics["validity"]) <= 1.0
    assert sum(eval((out / "pharm_counts_None.txt").read_text())) == 5 * 12


def test_train_driver_two_ranks_keep_identical_replicas(tmp_path):
    """train.py under torchrun with 2 ranks (sharing this box's one GPU: gloo collectives through the host; RCCL when the
    box has two): rank 0's weights are broadcast, gradients averaged every step, the validation loss all-reduced --
    --check_replicas verifies bitwise-identical parameters on all ranks after every epoch; the checkpoint carries the
    optimiser state and a resumed run continues from it."""
    import subprocess
    import sys
    import yaml
    import os
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(0)
    proc = tmp_path / "processed"
    for split in range(3):
        d = proc / f"split_{split}"
        d.mkdir(parents=True)
        n_g = 8
        np_, nf_ = np.full(n_g, 40), rng.integers(3, 8, n_g)
        pos = np.concatenate([O.synthetic_pocket(100 * split + i, 40)[0].numpy() for i in range(n_g)]).astype(np.float32)

        def idx(c):
            e = np.cumsum(c)
            return np.stack([e - c, e], 1)
        np.savez(d / 'prot_pharm_tensors.npz', prot_pos=pos, prot_feat=rng.integers(0, 4, np_.sum()), prot_idx=idx(np_),
                 pharm_pos=(rng.normal(size=(nf_.sum(), 3)) * 3).astype(np.float32), pharm_feat=rng.integers(0, 6, nf_.sum()),
                 pharm_idx=idx(nf_), prot_ph_pos=np.zeros((0, 3), np.float32), prot_ph_feat=np.zeros((0,), np.int64),
                 prot_ph_idx=np.zeros((n_g, 2), np.int64))
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    cfg['dataset'].update(processed_data_dir=str(proc), raw_data_dir=str(tmp_path), pocket_cutoff=8)
    cfg['training'].update(output_dir=str(tmp_path / "runs"), batch_size=4, num_workers=0, validation_splits=[2])
    cfg['training'].setdefault('trainer_args', {})['max_epochs'] = 2
    cfg['training']['evaluation']['sample_interval'] = 1000          # no sampling inside these few steps
    cfg.setdefault('wandb', {})['name'] = 'dp'
    yaml.dump(cfg, open(tmp_path / "cfg.yml", "w"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29687", os.path.join(root, "train.py"), "--config", str(tmp_path / "cfg.yml"), "--seed", "0",
           "--check_replicas"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("replicas identical on 2 ranks") == 2, r.stdout[-2000:]
    ck = list((tmp_path / "runs").glob("*/checkpoints/last.ckpt"))
    assert len(ck) == 1
    saved = torch.load(str(ck[0]), map_location="cpu", weights_only=False)
    assert saved['epoch'] == 1 and saved['global_step'] == 4
    st = saved['optimizer_states'][0]['state']
    assert st['step'] == 4 and float(st['exp_avg_sq'].abs().sum()) > 0 and 'best' in saved['lr_schedulers'][0]
    # resume: one more epoch from the saved optimiser state
    cfg['training']['trainer_args']['max_epochs'] = 3
    yaml.dump(cfg, open(tmp_path / "cfg.yml", "w"))
    r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "--config", str(tmp_path / "cfg.yml"), "--seed", "0",
                        "--resume", str(ck[0])], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "epoch 2:" in r.stdout and "epoch 0:" not in r.stdout
    newest = max((tmp_path / "runs").glob("*/checkpoints/last.ckpt"), key=lambda p: p.stat().st_mtime)
    again = torch.load(str(newest), map_location="cpu", weights_only=False)
    assert again['epoch'] == 2 and again['optimizer_states'][0]['state']['step'] > 4


def _rccl_rank_fn(rank, world, port, q):
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world, device_id=dev)
    z = load("train_grads.npz")
    m = make_model(int(z["T"])).to(dev)
    m.train()
    g = graph_from(batch_from(z), z["x0"], z["h0"]).to(dev)
    torch.manual_seed(3 + rank)                                     # different dropout draws per rank
    m.training_step(g, 0, t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]}).backward()
    own = m.dynamics._last_flat_grad.clone()
    flat = m.dynamics.allreduce_gradients(average=True)             # RCCL all-reduce of the flat gradient
    gathered = [torch.zeros_like(own) for _ in range(world)]
    dist.all_gather(gathered, own)
    ok = torch.allclose(flat, sum(gathered) / world, rtol=1e-6, atol=1e-9)
    ph = pfa.SampledPharmacophore(graph_from(batch_from(load("traj_c1.npz")), load("traj_c1.npz")["x0"], load("traj_c1.npz")["h0"]),
                                  pfa.analysis.ph_idx_to_type)
    freq = pfa.SampleAnalyzer().pharm_feat_freq([ph], process_group=dist.group.WORLD)      # NCCL branch: device buffer
    q.put((rank, bool(ok), float(freq.sum())))
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: RCCL is one rank per GPU (not substituted by gloo)")
def test_two_rank_rccl_gradient_allreduce_and_metrics():
    """A real 2-rank RCCL run (skipped on a one-GPU box): the flat-gradient all-reduce averages the two ranks' gradients,
    and the metric counters are reduced through a device buffer."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rccl_rank_fn, args=(r, 2, 29711, q)) for r in range(2)]
    [p.start() for p in procs]
    out = sorted(q.get(timeout=600) for _ in range(2))
    [p.join(60) for p in procs]
    assert all(ok for _, ok, _ in out) and out[0][2] == out[1][2] == 8.0


def test_gradient_views_accumulate_clear_and_allreduce_in_place():
    """The dynamics' parameters reach autograd as ONE flat leaf; every parameter's .grad is a view of the accumulated
    flat gradient.  Gradient accumulation over two backward passes, clearing parameter by parameter (what
    torch.optim's zero_grad does) and the single-vector all-reduce (one rank, RCCL) keep the usual semantics."""
    import torch.distributed as dist
    z = load("train_grads.npz")
    m = make_model(int(z["T"]))
    m.train()
    b = batch_from(z)
    g = graph_from(b, z["x0"], z["h0"]).to("cuda")
    kw = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})
    params = [p for k, p in m.named_parameters() if k.startswith("dynamics.") and p.numel() > 0]

    def grads():
        return torch.cat([p.grad.reshape(-1) for p in params]).clone()

    torch.manual_seed(3)
    m.training_step(g, 0, **kw).backward()
    g1 = grads()
    flat = m.dynamics._last_flat_grad
    assert all(p.grad.data_ptr() >= flat.data_ptr() and p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel() for p in params)
    torch.manual_seed(3)                                           # same dropout draws: the second pass adds the same gradient
    m.training_step(g, 0, **kw).backward()
    torch.testing.assert_close(grads(), 2 * g1, rtol=1e-5, atol=1e-7)
    for p in m.parameters():                                       # optimizer.zero_grad(set_to_none=True)
        p.grad = None
    torch.manual_seed(3)
    m.training_step(g, 0, **kw).backward()
    torch.testing.assert_close(grads(), g1, rtol=1e-5, atol=1e-7)
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29533", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        r = m.dynamics.allreduce_gradients(average=True)
        assert r.data_ptr() == m.dynamics._last_flat_grad.data_ptr()
        torch.testing.assert_close(grads(), g1, rtol=1e-5, atol=1e-7)
    finally:
        dist.destroy_process_group()


def test_flat_adam_lazy_clear_equals_the_eager_one():
    """FlatAdam.zero_grad(lazy=True) launches nothing; the next fused-loss backward stores its gradient into the bound flat vector
    (clear + accumulation in one).  Three optimiser steps give bitwise the parameters of the eager loop; a backward that accumulates
    through autograd instead (the framework-op loss) clears first; step() without a backward in between refuses."""
    z = load("train_grads.npz")
    b = batch_from(z)
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})

    def run(lazy):
        m = make_model(int(z["T"]))
        m.train()
        g = graph_from(b, z["x0"], z["h0"]).to("cuda")
        opt = pfa.FlatAdam(m.dynamics, lr=1e-3)
        for i in range(3):
            opt.zero_grad(lazy=lazy)
            torch.manual_seed(11 + i)
            m.training_step(g, 0, **inj).backward()
            opt.step()
        return m, opt, g

    m_e, _, _ = run(False)
    m_l, opt, g = run(True)
    for (k, a), (_, c) in zip(m_e.dynamics.state_dict().items(), m_l.dynamics.state_dict().items()):
        assert torch.equal(a, c), k
    # a deferred clear met by a backward that accumulates through autograd: cleared first, not added to the stale values
    params = [p for p in m_l.dynamics.parameters() if p.numel() > 0]
    opt.zero_grad(lazy=True)
    with pytest.raises(RuntimeError):
        opt.step()
    torch.manual_seed(5)
    m_l.training_step(g, 0, **inj).backward()
    ref = torch.cat([p.grad.reshape(-1) for p in params]).clone()
    opt.zero_grad(lazy=True)
    m_l.fused_loss = False
    torch.manual_seed(5)
    m_l.training_step(g, 0, **inj).backward()
    got = torch.cat([p.grad.reshape(-1) for p in params])
    torch.testing.assert_close(got, ref, rtol=2e-3, atol=1e-6)
    # a gradient that reaches a parameter directly (a regulariser on p: it never passes the flat leaf) next to the fused loss,
    # after a lazy clear: the sum of the two, not the sum plus the previous step's values
    m_l.fused_loss = True
    p_reg = params[3]
    opt.zero_grad(lazy=True)
    torch.manual_seed(5)
    (m_l.training_step(g, 0, **inj) + 0.5 * p_reg.pow(2).sum()).backward()
    got = torch.cat([p.grad.reshape(-1) for p in params])
    want = ref.clone()
    off = sum(p.numel() for p in params[:3])
    want[off:off + p_reg.numel()] += p_reg.detach().reshape(-1)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-7)
    opt.zero_grad(lazy=True)                            # and the regulariser alone
    (0.5 * p_reg.pow(2).sum()).backward()
    got = torch.cat([p.grad.reshape(-1) for p in params])
    want = torch.zeros_like(ref)
    want[off:off + p_reg.numel()] = p_reg.detach().reshape(-1)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0)


def test_bind_prefetch_on_the_twin_handle_equals_the_plain_loop():
    """PharmRecDynamicsGVP.prefetch_graph: the next batch is bound on a second handle by a worker thread while the current step's
    backward and optimiser step are enqueued, and the next step adopts that handle.  Six optimiser steps over three rotating
    batches (different graphs, sizes, pp edges), dropout on: parameters, Adam moments and every step's loss bitwise those of the
    loop that binds on its own thread; a prefetch that is not used (another batch comes next) and a prefetch of the batch that is
    already bound are harmless."""
    cfg = O.DynamicsConfig()
    parts = [O.synthetic_batch([900 + 7 * k + i for i in range(5)], [40, 52, 33, 61, 47][k % 5:] + [40, 52, 33, 61, 47][:k % 5],
                               [4 + (i + k) % 4 for i in range(5)], cfg) for k in range(3)]
    gen = torch.Generator().manual_seed(3)

    def graphs():
        out = []
        for b in parts:
            nf = int(b.pharm_ptr[-1])
            x0 = torch.randn(nf, 3, generator=torch.Generator().manual_seed(nf))
            h0 = torch.nn.functional.one_hot(torch.randint(0, 6, (nf,), generator=torch.Generator().manual_seed(nf + 1)), 6).float()
            out.append(graph_from(b, x0, h0).to("cuda"))
        return out

    def run(prefetch):
        m = make_model(100)
        m.train()
        gs = graphs()
        opt = pfa.FlatAdam(m.dynamics, lr=1e-3)
        losses = []
        for i in range(6):
            opt.zero_grad(lazy=True)
            torch.manual_seed(50 + i)
            loss = m.training_step(gs[i % 3], i)
            if prefetch:
                m.dynamics.prefetch_graph(gs[(i + 1) % 3])
                if i == 2:
                    m.dynamics.prefetch_graph(gs[i % 3])           # the batch that is bound already: nothing happens
                if i == 3:
                    m.dynamics.prefetch_graph(gs[(i + 2) % 3])     # not the batch that comes next: joined and dropped by the next bind
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return m, opt, losses

    m0, o0, l0 = run(False)
    m1, o1, l1 = run(True)
    assert l0 == l1
    for (k, a), (_, c) in zip(m0.dynamics.state_dict().items(), m1.dynamics.state_dict().items()):
        assert torch.equal(a, c), k
    assert torch.equal(o0.exp_avg, o1.exp_avg) and torch.equal(o0.exp_avg_sq, o1.exp_avg_sq)
    assert m1.dynamics.__dict__.get("_twin") is not None


def test_flat_adam_resumes_from_a_per_parameter_adam_state():
    """A checkpoint written by the reference's Lightning run carries torch.optim.Adam's per-parameter state
    (pharmacodiff.py:253-263); FlatAdam.load_state_dict maps it into the flat moment vectors (parameter i = tensor i of
    the flat layout) and the next steps equal torch.optim.Adam's own continuation."""
    z = load("train_grads.npz")
    b = batch_from(z)
    inj = dict(t_int=z["t_int"].long(), eps={'h': z["eps_h"], 'x': z["eps_x"]})

    def steps(m, opt, n):
        g = graph_from(b, z["x0"], z["h0"]).to("cuda")
        for _ in range(n):
            opt.zero_grad(set_to_none=True)
            m.training_step(g, 0, **inj).backward()
            opt.step()

    def fresh():
        m = make_model(int(z["T"]))
        m.train()
        m.dynamics.dropout_rate = 0.0
        return m
    m_t = fresh()
    opt_t = torch.optim.Adam(m_t.parameters(), lr=1e-3)
    steps(m_t, opt_t, 2)
    ck_state = {k: v.detach().cpu().clone() for k, v in m_t.state_dict().items()}
    import copy
    ck_opt = copy.deepcopy(opt_t.state_dict())                 # {'state': {i: {step, exp_avg, exp_avg_sq}}, 'param_groups': [...]}
    assert 'layout' not in ck_opt and isinstance(next(iter(ck_opt['state'].values())), dict)
    steps(m_t, opt_t, 2)                                       # the uninterrupted run
    m_f = fresh()
    m_f.load_state_dict(ck_state, strict=True)
    opt_f = pfa.FlatAdam(m_f.dynamics, lr=1e-3)
    opt_f.load_state_dict(ck_opt)
    assert opt_f.t == 2 and float(opt_f.exp_avg.abs().max()) > 0
    steps(m_f, opt_f, 2)
    for k, v in m_t.dynamics.state_dict().items():
        if v.numel():
            torch.testing.assert_close(m_f.dynamics.state_dict()[k].cpu(), v.cpu(), rtol=2e-4, atol=2e-6, msg=k)
    own = opt_f.state_dict()                                   # and its own format still round-trips
    opt_g = pfa.FlatAdam(m_f.dynamics, lr=1e-3)
    opt_g.load_state_dict(own)
    assert opt_g.t == opt_f.t and torch.equal(opt_g.exp_avg, opt_f.exp_avg)


def test_pocket_claims_device_resident_batches_and_failed_binds():
    """A pocket-group claim is verified for device-resident pocket tensors too (coordinates compared on the device), a
    rejected bind neither keeps its claim for the next batch nor destroys the batch that was bound before, and an
    injected t_int outside the schedule is refused."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    from test_gpu_fullsize import _copies_batch, _engine
    batch, uid = _copies_batch(cfg, [(601, 60), (602, 48)], [[3, 5, 4], [6, 4]])
    eng = _engine(cfg, sd)
    dev = lambda t: t.cuda()
    eng.set_batch(dev(batch.prot_x), dev(batch.prot_h), batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst, pocket_uid=uid)
    gen = torch.Generator().manual_seed(1)
    Nf = int(batch.pharm_ptr[-1])
    x_t, h_t, t = torch.randn(Nf, 3, generator=gen), torch.randn(Nf, 6, generator=gen), torch.full((5,), 0.4)
    ref = [v.cpu() for v in eng.dynamics(x_t, h_t, t)]
    px = batch.prot_x.clone(); px[70] += 0.01                 # an atom of the second copy of the first pocket, on the device
    with pytest.raises(pfa.PfError, match="coordinates / features differ"):
        eng.set_batch(dev(px), dev(batch.prot_h), batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst, pocket_uid=uid)
    # a bind the library rejects (a pp edge across two graphs) with a claim attached ...
    bad_src = batch.pp_src.clone(); bad_src[0] = int(batch.prot_ptr[1]) + 1
    with pytest.raises(pfa.PfError, match="crosses graphs"):
        eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, bad_src, batch.pp_dst, pocket_uid=uid)
    # (indices outside the batch, in the source and in the last destination: the vectorised pass hands them to the scalar one)
    for col, where, val in (("src", 5, int(batch.prot_ptr[-1]) + 3), ("src", 2, -1), ("dst", -1, int(batch.prot_ptr[-1]))):
        bs, bd = batch.pp_src.clone(), batch.pp_dst.clone()
        (bs if col == "src" else bd)[where] = val
        with pytest.raises(pfa.PfError, match="out of range"):
            eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, bs, bd)
    # ... leaves the previous batch usable, bitwise
    again = [v.cpu() for v in eng.dynamics(x_t, h_t, t)]
    assert torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1])
    # ... and the stale claim does not attach to the next, unrelated batch (another number of graphs)
    other = O.synthetic_batch([603, 604], 40, [4, 3], cfg)
    eng.set_batch(other.prot_x, other.prot_h, other.prot_ptr, other.pharm_ptr, other.pp_src, other.pp_dst)
    Nf2 = int(other.pharm_ptr[-1])
    eh, ex = eng.dynamics(torch.randn(Nf2, 3, generator=gen), torch.randn(Nf2, 6, generator=gen), torch.full((2,), 0.3))
    assert torch.isfinite(eh).all() and torch.isfinite(ex).all()
    # injected timesteps outside [0, T]
    z = load("train_grads.npz")
    m = make_model(int(z["T"]))
    g = graph_from(batch_from(z), z["x0"], z["h0"]).to("cuda")
    bad_t = z["t_int"].long().clone(); bad_t[0] = int(z["T"]) + 3
    with pytest.raises(ValueError, match="t_int must lie"):
        m.forward(g, 'val', t_int=bad_t, eps={'h': z["eps_h"], 'x': z["eps_x"]})


def test_a_false_claim_leaves_the_handle_without_a_batch():
    """A pocket-group claim is verified after the bind's point of no return (the plan is adopted, then the tables are filled): a
    claim that fails there -- same atoms, in-degrees and edge count, one pp source of a copy redirected inside its graph -- leaves
    the handle without a batch, loudly, never with the previous one's tables; binding the true batch again gives bitwise what it
    gave before."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    from test_gpu_fullsize import _copies_batch, _engine
    batch, uid = _copies_batch(cfg, [(621, 48), (622, 40)], [[3, 5], [4, 3]])
    eng = _engine(cfg, sd)
    args = (batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr)            # host rows
    eng.set_batch(*args, batch.pp_src, batch.pp_dst, pocket_uid=uid)
    gen = torch.Generator().manual_seed(6)
    Nf = int(batch.pharm_ptr[-1])
    x_t, h_t, t = torch.randn(Nf, 3, generator=gen), torch.randn(Nf, 6, generator=gen), torch.full((4,), 0.4)
    ref = [v.cpu() for v in eng.dynamics(x_t, h_t, t)]
    p1, p2 = int(batch.prot_ptr[1]), int(batch.prot_ptr[2])
    e = int((batch.pp_dst >= p1).nonzero()[0])                                      # the first pp edge of the first pocket's second copy
    bad_src = batch.pp_src.clone()
    bad_src[e] = p1 + (int(bad_src[e]) - p1 + 1) % (p2 - p1)
    assert bad_src[e] != batch.pp_src[e] and p1 <= int(bad_src[e]) < p2
    with pytest.raises(pfa.PfError, match="not a copy of graph"):
        eng.set_batch(*args, bad_src, batch.pp_dst, pocket_uid=uid)
    with pytest.raises(pfa.PfError, match="no pocket batch set"):
        eng.dynamics(x_t, h_t, t)
    eng.set_batch(*args, batch.pp_src, batch.pp_dst, pocket_uid=uid)
    again = [v.cpu() for v in eng.dynamics(x_t, h_t, t)]
    assert torch.equal(again[0], ref[0]) and torch.equal(again[1], ref[1])


def test_c_abi_verifies_a_pocket_claim_made_for_device_rows():
    """pf_set_pocket_groups + pf_set_pocket_batch with DEVICE coordinates / features, straight through the C ABI (the Python
    engine's own comparison bypassed): the bind compares every copy with its representative on the device, and the first call
    that would share conv-layer-0 messages fails with PF_ERR_ARG when the claim is false -- nothing is computed on it (VERDICT
    r4 weak #8).  A true claim samples as before."""
    import ctypes
    import numpy as np
    from pharmacoforge_amd.engine import _dptr, _stream_ptr
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    from test_gpu_fullsize import _copies_batch, _engine
    batch, uid = _copies_batch(cfg, [(611, 60)], [[3, 5, 4, 6, 4, 5, 3, 4]])
    eng = _engine(cfg, sd)
    B, Nf = 8, int(batch.pharm_ptr[-1])
    pptr = batch.prot_ptr.numpy().astype(np.int32); fptr = batch.pharm_ptr.numpy().astype(np.int32)
    src = batch.pp_src.numpy().astype(np.int32); dst = batch.pp_dst.numpy().astype(np.int32)
    rep = np.zeros(B, np.int32)                                   # every graph claims to be a copy of graph 0
    noise = torch.randn(4, Nf, 9, generator=torch.Generator().manual_seed(2))
    coef = O.step_coefficients(O.gamma_table(100, 1e-5), 100)
    arr = eng.coef_array(coef, [40, 39, 38])

    def bind(px):
        dx, dh = px.cuda().contiguous(), batch.prot_h.cuda().contiguous()
        eng._keep = [dx, dh]
        eng._ck(eng.lib.pf_set_pocket_groups(eng._h, B, rep.ctypes.data), "pf_set_pocket_groups")
        eng.B, eng.Np, eng.Nf = B, int(pptr[-1]), Nf
        eng._ck(eng.lib.pf_set_pocket_batch(eng._h, B, pptr.ctypes.data, fptr.ctypes.data, _dptr(dx), _dptr(dh), int(src.size),
                                            src.ctypes.data, dst.ctypes.data, _stream_ptr()), "pf_set_pocket_batch")
    bind(batch.prot_x)
    x_ok, h_ok = eng.sample(arr, 3, noise)
    assert eng.counts()["pp"] > 0
    px = batch.prot_x.clone(); px[60 * 5 + 7, 1] += 1e-3          # one atom of the sixth copy
    bind(px)                                                       # asynchronous: the bind itself cannot know yet
    with pytest.raises(pfa.PfError, match="claim made for this batch is false"):
        eng.sample(arr, 3, noise)
    bind(batch.prot_x)
    x2, h2 = eng.sample(arr, 3, noise)
    assert torch.equal(x2, x_ok) and torch.equal(h2, h_ok)


def _bench_child(args, timeout=300):
    """bench.py as a fresh child process (it starts its own ranks before touching the GPU); returns (returncode, last JSON line or None,
    stderr).  Output goes to files (a rank that outlives its launcher keeps a pipe open and would hold the reader forever); a child
    that does not finish in `timeout` seconds is killed with its whole process group and reported as a failure, never waited for."""
    import json
    import signal
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    with tempfile.TemporaryDirectory() as td:
        fo, fe = open(os.path.join(td, "out"), "w+"), open(os.path.join(td, "err"), "w+")
        pr = subprocess.Popen([sys.executable, os.path.join(root, "bench.py")] + args, stdout=fo, stderr=fe, cwd=root, env=env,
                              start_new_session=True)
        try:
            rc = pr.wait(timeout=timeout)
        except subprocess.TimeoutExpired:
            os.killpg(pr.pid, signal.SIGKILL)              # the launcher and the ranks it started (one session)
            pr.wait()
            rc = -9
        fo.seek(0); fe.seek(0)
        out, err = fo.read(), fe.read()
        fo.close(); fe.close()
    if rc == -9:
        err += f"\n[test] bench.py {' '.join(args)} did not finish in {timeout} s and was killed"
    line = None
    for ln in reversed(out.strip().splitlines()):
        if ln.strip().startswith("{"):
            line = json.loads(ln)
            break
    return rc, line, err


@pytest.mark.parametrize("leg", ["headline", "train", "sample_slice"])
def test_bench_two_rank_plumbing_on_one_gpu(leg):
    """The N > 1 code of bench.py -- rank launch, process group, barriers, max-over-ranks timing, per-rank gather, the
    work split of the config-4 slice, the gradient all-reduce of the training leg -- executed with TWO ranks on whatever
    GPUs are here (one card: the ranks share it and the process group is gloo, rccl_world 0; two or more: RCCL).  What an
    8-GPU driver pass runs, minus the hardware (pharmacodiff.py:516-578 for the slice's partitioning)."""
    light = ["--no-cpu-baseline", "--no-dense-leg", "--no-full-trajectory", "--no-secondary", "--no-traffic"]
    args = {"headline": ["--gpus", "2", "--steps", "10", "--warmup", "2"] + light,
            "train": ["--gpus", "2", "--train", "--steps", "4", "--warmup", "1", "--batch", "64"] + light,
            "sample_slice": ["--gpus", "2", "--sample-slice", "8", "--samples", "6", "--max-batch-size", "24"] + light}[leg]
    rc, j, err = _bench_child(args)
    assert rc == 0 and j is not None, err[-2000:]
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["value"] > 0
    assert len(j["per_rank_ms_per_step"]) == 2 and all(v > 0 for v in j["per_rank_ms_per_step"])
    assert j["rccl_world"] == (2 if torch.cuda.device_count() >= 2 else 0)
    if leg == "headline":
        assert j["config"]["batch_per_gpu"] == 32 and j["steps"] == 10 and j["warmup"] == 2


def test_bench_four_rank_training_keeps_the_host_off_the_critical_path():
    """Config 5 is a data-parallel TRAINING step, and a training step is as long on the host as on the device: with one process per
    GPU the ranks share the host, so each pins itself to its slice of the CPUs and sizes its thread pools to it before touching the
    GPU (sharding.pin_host_threads).  Four ranks on whatever GPUs are here (one card: they share it, gloo): the bench line names every
    rank's share, and a rank's mean host time per step -- enqueue only; the ranks queue up on the one card, which is not the
    point -- stays within 20 % of a single rank's (the unpinned form measured integer factors)."""
    light = ["--no-cpu-baseline", "--no-dense-leg", "--no-full-trajectory", "--no-secondary", "--no-traffic"]
    base = ["--train", "--steps", "12", "--warmup", "3", "--batch", "64"] + light
    rc, j1, err = _bench_child(["--gpus", "1"] + base)
    assert rc == 0 and j1 is not None, err[-2000:]
    rc, j4, err = _bench_child(["--gpus", "4"] + base, timeout=420)
    assert rc == 0 and j4 is not None, err[-2000:]
    assert j4["n_gpus"] == 4 and len(j4["per_rank_host_enqueue_ms"]) == 4
    h = j4["host"]
    assert h["local_world"] == 4 and h["host_threads_per_rank"] >= 1 and h["host_threads_per_rank"] <= max(1, h["host_cpus"] // 4)
    one = j1["per_rank_host_enqueue_ms"][0]
    # (when the four ranks share ONE card their steps queue up on it and the host blocks in the all-reduce / optimiser: compare
    # the enqueue part, which the per-step statistics carry as the median)
    med4, med1 = j4["per_step"]["host_enqueue_ms"]["median"], j1["per_step"]["host_enqueue_ms"]["median"]
    if torch.cuda.device_count() >= 4:
        assert max(j4["per_rank_host_enqueue_ms"]) <= 1.2 * one, (j4["per_rank_host_enqueue_ms"], one)
    else:
        assert med1 > 0 and med4 > 0


def test_bench_rejects_more_ranks_than_a_shared_gpu_takes():
    """`bench.py --gpus 8` where fewer than 8 GPUs are visible must fail at once with a message, not hang in a rendezvous or
    pile eight processes onto one card."""
    if torch.cuda.device_count() >= 8:
        pytest.skip("eight GPUs are visible here")
    rc, j, err = _bench_child(["--gpus", "8", "--steps", "2", "--warmup", "1"], timeout=120)
    assert rc != 0 and j is None
    assert "--gpus 8" in err and "GPU(s) visible" in err


def test_bench_plain_run_times_its_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` run: K timed steps, `ms_per_step` on the line, none of the legs --full adds;
    --dump-outputs writes the last timed step's samples (float32 .npy), and two runs with the same arguments compute the same
    samples (the pre-warm runs for a time, the noise of the warm-up and the timed steps starts from its seed again)."""
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        rc, j, err = _bench_child(["--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", str(d)])
        assert rc == 0 and j is not None, err[-2000:]
        assert j["steps"] == 7 and j["warmup"] == 3 and j["ms_per_step"] > 0 and j["unit"] == "sample-steps/s"
        assert abs(j["value"] - 32 * 1e3 / j["ms_per_step"]) <= 1e-6 * j["value"]
        assert not [leg for leg in ("roofline", "secondary", "full_trajectory", "cpu_baseline") if leg in j]
        dumps.append({n: np.load(d / f"{n}.npy") for n in ("pharm_x", "pharm_h")})
    for n, cols in (("pharm_x", 3), ("pharm_h", 6)):
        a, b = dumps[0][n], dumps[1][n]
        assert a.dtype == np.float32 and a.shape == (32 * 6, cols) and np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=n)
