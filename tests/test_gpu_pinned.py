"""Pinned centers (pf_sample_pinned / pf_sample_begin_pinned / pf_denoise_step_pinned): a pharmacophore completed around given
points by replacement conditioning, against a CPU composition of the oracle's own functions.

The reference for a pinned run is the loop of O.sample_given_receptor with the two selects of include/pfdyn.h ("pinned centers")
in front of the COM removal (`pinned_reference` below).  With all flags zero it is O.sample_given_receptor.

Shapes: five ragged pockets (the 300-atom one exercises the strided atom loops of the update), 23 centers, T = 50 at
precision 0.25 -- the bounded regime of tests/golden/traj_c1_T500_bounded.npz (centers stay within ~6 A of their pockets; the
frame offset |D| reaches ~5 A, so a wrong frame is an error of angstroms).  Tolerances are the project's own: the T-step
trajectory tolerance of test_gpu_parity.py (rtol = atol = 5e-3) and, for the width-generic family, that of test_gpu_wide.py
(atol = 2e-2, rtol = 0).  Given values must come back bit for bit."""
import functools

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O

pytestmark = pytest.mark.gpu

T, PREC = 50, 0.25


def pinned_reference(sd, cfg, batch, n_t, precision, noise, flags, pin_x, pin_h, init_pharm_com, fnorm=1.0, ep=False):
    """O.sample_given_receptor's loop (sample_step opened up) + the replacement selects.  Returns x_0, h_0, frames."""
    bidx, B = batch.batch_idxs(), batch.batch_size
    gamma = O.gamma_table(n_t, precision)
    coef = O.step_coefficients(gamma, n_t)
    px, ph = ((flags & 1) != 0)[:, None], ((flags & 2) != 0)[:, None]
    c_init = O.segment_mean(batch.prot_x, batch.prot_ptr)
    prot_x = batch.prot_x - init_pharm_com[bidx["prot"]]
    x_t, h_t = noise[0][:, :3].clone(), noise[0][:, 3:].clone()

    def frame(p, x, h):
        return x + (c_init - O.segment_mean(p, batch.prot_ptr))[bidx["pharm"]], h * fnorm
    a, b = frame(prot_x, x_t, h_t)
    fx, fh = [a], [b]
    for it, s in enumerate(reversed(range(n_t))):
        nz = noise[1 + it]
        D = (c_init - O.segment_mean(prot_x, batch.prot_ptr))[bidx["pharm"]]          # before this step's shift
        pred_h, pred_x = O.dynamics_forward(sd, cfg, batch, prot_x, x_t, h_t, coef["t"][s].expand(B).contiguous())
        a_ts, var, sig = coef["alpha_t_given_s"][s], coef["var_terms"][s], coef["sigma"][s]
        mu_x = coef["ep_zt"][s] * x_t + coef["ep_pred"][s] * pred_x if ep else x_t / a_ts - var * pred_x
        mu_h = coef["ep_zt"][s] * h_t + coef["ep_pred"][s] * pred_h if ep else h_t / a_ts - var * pred_h
        x_s, h_s = mu_x + sig * nz[:, :3], mu_h + sig * nz[:, 3:]
        g_s = O.gamma_lookup(gamma, coef["s"][s], n_t)
        al, sg = O.alpha(g_s), O.sigma(g_s)
        x_s = torch.where(px, al * (pin_x - D) + sg * nz[:, :3], x_s)
        h_s = torch.where(ph, al * (pin_h / fnorm) + sg * nz[:, 3:], h_s)
        com = O.segment_mean(x_s, batch.pharm_ptr)
        x_t, h_t, prot_x = x_s - com[bidx["pharm"]], h_s, prot_x - com[bidx["prot"]]
        a, b = frame(prot_x, x_t, h_t)
        fx.append(a); fh.append(b)
    x_0 = x_t - O.segment_mean(prot_x, batch.prot_ptr)[bidx["pharm"]] + c_init[bidx["pharm"]]      # (O.sample_given_receptor's order)
    x_0, h_0 = torch.where(px, pin_x, x_0), torch.where(ph, pin_h, h_t * fnorm)
    fx[-1], fh[-1] = torch.where(px, pin_x, fx[-1]), h_0
    return x_0, h_0, torch.stack(fx), torch.stack(fh)


def engine_for(cfg, sd):
    eng = pfa.PfEngine(pharm_nf=cfg.pharm_nf, rec_nf=cfg.rec_nf, vector_size=cfg.vector_size,
                       n_hidden_scalars=cfg.n_hidden_scalars, n_convs=cfg.n_convs, n_message_gvps=cfg.n_message_gvps,
                       n_update_gvps=cfg.n_update_gvps, n_noise_gvps=cfg.n_noise_gvps, message_norm=cfg.message_norm,
                       ff_k=cfg.ff_k, pf_k=cfg.pf_k,
                       graph_cutoffs={"pp": cfg.cutoff_pp, "pf": cfg.cutoff_pf, "fp": cfg.cutoff_fp, "ff": cfg.cutoff_ff})
    eng.load_state_dict(sd)
    return eng


def bound(eng, batch):
    eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst)
    return eng


def pins_for(batch, cfg, flags, seed=43):
    """given positions = the pocket's COM + 1.5 * randn, given rows = random one-hots (rows of free centers are ignored)"""
    gen = torch.Generator().manual_seed(seed)
    Nf = int(batch.pharm_ptr[-1])
    com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    pin_x = com[batch.batch_idxs()["pharm"]] + 1.5 * torch.randn(Nf, 3, generator=gen)
    pin_h = torch.nn.functional.one_hot(torch.randint(0, cfg.pharm_nf, (Nf,), generator=gen), cfg.pharm_nf).float()
    return torch.tensor(flags, dtype=torch.int32), pin_x, pin_h


@functools.lru_cache(maxsize=None)
def case():
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    batch = O.synthetic_batch([31, 32, 33, 34, 35], [48, 300, 40, 64, 32], [3, 8, 5, 1, 6], cfg)
    Nf = int(batch.pharm_ptr[-1])
    assert Nf == 23
    noise = torch.randn(T + 1, Nf, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(42))
    #        graph 0 | graph 1: 0, 1 both, 2 position, 3 row | graph 2: all | graph 3 | graph 4: the last
    flags = [0, 0, 0] + [3, 3, 1, 2, 0, 0, 0, 0] + [3] * 5 + [3] + [0, 0, 0, 0, 0, 3]
    pins = pins_for(batch, cfg, flags)
    com = O.segment_mean(batch.prot_x, batch.prot_ptr) + 0.5
    return cfg, sd, batch, noise, pins, com


@functools.lru_cache(maxsize=None)
def reference(ep):
    cfg, sd, batch, noise, pins, com = case()
    return pinned_reference(sd, cfg, batch, T, PREC, noise, *pins, com, ep=ep)


def arrays(eng, n_t=T, prec=PREC):
    gamma = O.gamma_table(n_t, prec)
    order = list(reversed(range(n_t)))
    return (eng.coef_array(O.step_coefficients(gamma, n_t), order),
            eng.pin_coef_array(pfa.schedule.pin_coefficients(gamma, n_t), order))


@pytest.mark.parametrize("ep", [False, True])
def test_pinned_run_vs_composition(ep):
    cfg, sd, batch, noise, pins, com = case()
    flags, pin_x, pin_h = pins
    rx, rh, rfx, rfh = reference(ep)
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr = arrays(eng)
    x0, h0, tx, th = (t.cpu() for t in eng.sample(arr, T, noise, init_pharm_com=com, ep_coord=ep, ep_feat=ep, trajectory=True,
                                                  pins=pins, pin_coef_arr=parr))
    assert eng.kernel_family(cfg.n_convs) == 0          # no tail, fused-tail or merged launch in a pinned run
    assert eng.xchg_timeouts() == 0
    eng.sample_status()
    print("worst |error|: x0 %.3g h0 %.3g frames x %.3g h %.3g" % tuple(float((a - b).abs().max()) for a, b in
                                                                         ((x0, rx), (h0, rh), (tx, rfx), (th, rfh))))
    for got, ref in ((x0, rx), (h0, rh), (tx, rfx), (th, rfh)):
        torch.testing.assert_close(got, ref, rtol=5e-3, atol=5e-3)
    mx, mh = (flags & 1) != 0, (flags & 2) != 0
    assert torch.equal(x0[mx], pin_x[mx]) and torch.equal(h0[mh], pin_h[mh])
    assert torch.equal(tx[-1][mx], pin_x[mx]) and torch.equal(th[-1][mh], pin_h[mh])
    assert torch.equal(tx[-1], x0) and torch.equal(th[-1], h0)
    # earlier frames show the noised state, not the given values
    assert not torch.equal(tx[T // 2][mx], pin_x[mx])


def test_all_zero_flags_equal_the_plain_run():
    cfg, sd, batch, noise, pins, com = case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr = arrays(eng)
    plain = eng.sample(arr, T, noise, init_pharm_com=com, trajectory=True)
    zero = (torch.zeros_like(pins[0]), pins[1], pins[2])
    got = eng.sample(arr, T, noise, init_pharm_com=com, trajectory=True, pins=zero, pin_coef_arr=parr)
    assert eng.kernel_family(cfg.n_convs) == 0 and eng.xchg_timeouts() == 0
    for a, b in zip(got, plain):
        torch.testing.assert_close(a.cpu(), b.cpu(), rtol=5e-3, atol=5e-3)


def test_pins_leave_nothing_behind():
    cfg, sd, batch, noise, pins, com = case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr = arrays(eng)
    a = eng.sample(arr, T, noise, init_pharm_com=com)
    form = eng.kernel_family(cfg.n_convs)
    eng.sample(arr, T, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr)
    assert eng.kernel_family(cfg.n_convs) == 0
    b = eng.sample(arr, T, noise, init_pharm_com=com)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert eng.kernel_family(cfg.n_convs) == form
    assert eng.xchg_timeouts() == 0


def test_step_api_equals_whole_loop_and_state_errors():
    cfg, sd, batch, noise, pins, com = case()
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr = arrays(eng)
    x0, h0 = eng.sample(arr, T, noise, init_pharm_com=com, pins=pins, pin_coef_arr=parr)
    eng.sample_begin(noise[0], init_pharm_com=com, pins=pins)
    with pytest.raises(pfa.PfError):                    # a plain step inside a pinned run
        eng.denoise_step(arr[0], noise[1])
    for i in range(T):
        eng.denoise_step(arr[i], noise[1 + i], pin_coef=parr[i])
    x1, h1 = eng.sample_end()
    assert torch.equal(x0, x1) and torch.equal(h0, h1)
    eng.sample_begin(noise[0], init_pharm_com=com)
    with pytest.raises(pfa.PfError):                    # a pinned step after a plain begin
        eng.denoise_step(arr[0], noise[1], pin_coef=parr[0])
    eng.denoise_step(arr[0], noise[1])                  # ... which the plain step continues


def test_width_generic_family():
    """(64, 32): the update runs alone (k_step_update<MovePinned>), the family launches its own encoders and edge build.  The given
    rows are divided by a feat_norm_constant of 2 here."""
    n_t, fnorm = 20, 2.0
    cfg = O.DynamicsConfig(n_hidden_scalars=64, vector_size=32)
    sd = O.make_state_dict(cfg, 0)
    batch = O.synthetic_batch([0, 1], [40, 56], [3, 5], cfg)
    noise = torch.randn(n_t + 1, 8, 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(42))
    pins = pins_for(batch, cfg, [3, 0, 0] + [0, 0, 3, 0, 0])
    flags, pin_x, pin_h = pins
    com = O.segment_mean(batch.prot_x, batch.prot_ptr) + 0.5
    rx, rh, rfx, rfh = pinned_reference(sd, cfg, batch, n_t, PREC, noise, *pins, com, fnorm=fnorm)
    eng = bound(engine_for(cfg, sd), batch)
    arr, parr = arrays(eng, n_t)
    x0, h0, tx, th = (t.cpu() for t in eng.sample(arr, n_t, noise, init_pharm_com=com, feat_norm_constant=fnorm, trajectory=True,
                                                  pins=pins, pin_coef_arr=parr))
    print("worst |error|: x0 %.3g h0 %.3g" % (float((x0 - rx).abs().max()), float((h0 - rh).abs().max())))
    for got, ref in ((x0, rx), (h0, rh), (tx, rfx), (th, rfh)):
        torch.testing.assert_close(got, ref, rtol=0, atol=2e-2)
    mx, mh = (flags & 1) != 0, (flags & 2) != 0
    assert torch.equal(x0[mx], pin_x[mx]) and torch.equal(h0[mh], pin_h[mh])


def test_model_level_sample_with_pins():
    """PharmacophoreDiff.sample: two pockets x three sizes, pins for the first pocket only.  Batches of three graphs: the copies
    of the pinned pocket form batch 0, those of the other pocket batch 1 -- which runs the plain path on the second lane, so
    its samples are the bits of a run without `pinned` (a batch holding a pinned graph takes the pinned step for all its graphs,
    which agrees with the plain step to rounding only)."""
    from test_gpu_api import graph_from, make_model
    n_t = 20
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[3, 5, 4], [4, 3, 6]]
    pin_x = (pockets[0].prot_x.mean(dim=0) + torch.tensor([[1.25, -0.5, 0.75], [-1.0, 1.5, 0.125]])).float()
    pin_x = torch.round(pin_x * 1000) / 1000            # what a user cuts from a pharms.xyz file: three decimals
    types = torch.tensor([2, 5])
    elems = pfa.SampledPharmacophore.type_idx_to_elem
    lines = ["%s %.3f %.3f %.3f" % (elems[int(k)], *xyz) for k, xyz in zip(types, pin_x.double().tolist())]
    torch.manual_seed(7)
    out = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2, pinned=[(pin_x, types, None), None])
    torch.manual_seed(7)
    plain = m.sample(pockets, n_pharms, max_batch_size=3, lanes=2)
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    for p in out[0]:
        assert p.pinned.tolist() == [3, 3] + [0] * (p.n_ph_centers - 2)
        assert torch.equal(p.ph_coords[:2], pin_x) and p.ph_feats_idxs[:2].tolist() == types.tolist()
        assert torch.equal(p.g.pharm_h0[:2], torch.nn.functional.one_hot(types, 6).float())
        assert p.to_xyz_file().splitlines()[1:3] == lines
        assert torch.isfinite(p.ph_coords).all()
    for p, q in zip(out[1], plain[1]):
        assert not p.pinned.any()
        assert torch.equal(p.ph_coords, q.ph_coords) and torch.equal(p.g.pharm_h0, q.g.pharm_h0)
    assert any(not torch.equal(p.ph_coords[2:], q.ph_coords[2:]) for p, q in zip(out[0], plain[0]))     # the free centers moved
    with pytest.raises(ValueError):
        m.sample(pockets, [[3, 1], [4]], max_batch_size=3, pinned=[(pin_x, types, None), None])
