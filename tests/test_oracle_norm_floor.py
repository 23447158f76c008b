"""The inputs of tests/test_gpu_norm_floor.py, checked on the CPU oracle alone: they put the 1e-8 floor of norm_no_nan
(gvp.py:12-19) to work in every chain family, keep every squared norm away from the threshold (so that an fp32 kernel, the fp32
oracle and the fp64 oracle all take the same side of the clamp), leave the fixed-point scatter of the gradient kernels its
headroom, and make a kernel without the floor -- or a gradient kernel that differentiates through the clamp -- miss the GPU
tests' tolerances by a factor of ten or more.  The wrong kernels are restated on the oracle (helpers.NORM_MUTANTS).

With the seeded weights alone the floor acts on about 1 % of the (row, channel) entries and a kernel without it stays inside
every tolerance of the suite; helpers.floor_weights puts about 45 % of them on it, helpers.twin_inputs puts nodes closer
together than the floor of the edge geometry."""
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import pf_oracle as O
from helpers import (NORM_EPS, floor_weights, live_reference, norm_census, norm_mutant, site_family, twin_inputs)

ATOL = 2e-4          # absolute tolerance of one dynamics call in the GPU parity tests
GRAD_TOL = 2e-3      # test_gpu_train.compare's tolerance in test_gradients_vs_oracle, relative to a tensor's max
BITE = 10.0          # a mutant has to miss a tolerance by this factor
SEEDS, N_PROT, N_PHARM = (81, 82, 83), 40, (5, 1, 6)
WSEED, ISEED = 3, 1
# (weight seed, input seed) per width pair, chosen so that no squared norm lies within 2**-10 of the threshold
# (test_distance_from_the_threshold): about one seed pair in five does at 100,000 entries
FLOOR_SEEDS = {(128, 16): (WSEED, ISEED), (64, 32): (7, 6)}
TWIN_CONFIGS = {
    "dev": dict(),
    "knnff_radiuspf_gnorm": dict(ff_k=2, pf_k=0, message_norm=0),
}


def _inputs(cfg, iseed=ISEED):
    batch = O.synthetic_batch(list(SEEDS), N_PROT, list(N_PHARM), cfg)
    com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    batch = O.PocketBatch(batch.prot_x - com[batch.batch_idxs()["prot"]], batch.prot_h, batch.prot_ptr, batch.pharm_ptr,
                          batch.pp_src, batch.pp_dst)            # the pocket's frame: prot_x is what the dynamics call gets
    gen = torch.Generator().manual_seed(iseed)
    Nf = int(batch.pharm_ptr[-1])
    x_t, h_t = 2.5 * torch.randn(Nf, 3, generator=gen), torch.randn(Nf, cfg.pharm_nf, generator=gen)
    t = torch.rand(batch.batch_size, generator=gen)
    w_h, w_x = torch.randn(Nf, cfg.pharm_nf, generator=gen), torch.randn(Nf, 3, generator=gen)
    return SimpleNamespace(cfg=cfg, batch=batch, prot_x=batch.prot_x, x_t=x_t, h_t=h_t, t=t, w_h=w_h, w_x=w_x)


@functools.lru_cache(maxsize=None)
def floor_case(S=128, V=16):
    """3 graphs of 40 atoms with 5, 1 and 6 centers; .sd: floor weights (plain head, for gradients), .live: live_reference on them"""
    wseed, iseed = FLOOR_SEEDS[(S, V)]
    c = _inputs(O.DynamicsConfig(n_hidden_scalars=S, vector_size=V), iseed)
    c.sd = floor_weights(O.make_state_dict(c.cfg, wseed))
    c.live = live_reference(c.sd, c.cfg, c.batch, c.prot_x, c.x_t, c.h_t, c.t)
    return c


@functools.lru_cache(maxsize=None)
def twin_case(name):
    """the same graphs with twin_inputs' coincident and near-coincident nodes, plain weights; .live: live_reference"""
    c = _inputs(O.DynamicsConfig(**TWIN_CONFIGS[name]))
    c.batch, c.x_t, c.planted = twin_inputs(c.batch, c.x_t, c.cfg)
    c.prot_x = c.batch.prot_x
    c.sd = O.make_state_dict(c.cfg, WSEED)
    c.live = live_reference(c.sd, c.cfg, c.batch, c.prot_x, c.x_t, c.h_t, c.t)
    return c


def forward(c, sd, fp64=False):
    f = O.dynamics_forward64 if fp64 else O.dynamics_forward
    return f(sd, c.cfg, c.batch, c.prot_x, c.x_t, c.h_t, c.t)


@functools.lru_cache(maxsize=None)
def floor_census(fp64=False):
    c = floor_case()
    with norm_census(lambda: forward(c, c.live.sd, fp64)) as census:
        pass
    return census


def oracle_gradients(c, sd, dropout, mutant=None, retain=None):
    """{name: gradient} of sum(eps_h * w_h) + sum(eps_x * w_x) by the oracle's autograd (in the dtype of ``sd``); retain: a list that
    receives the node features (h, v) entering every conv layer, with their gradients retained"""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    dt = next(iter(sd.values())).dtype
    batch = O.batch64(c.batch) if dt == torch.float64 else c.batch
    if dropout is not None:
        dropout = [{nt: tuple(m.to(dt) for m in d[nt]) for nt in d} for d in dropout]
    orig = O.conv_layer

    def spy(sd_, prefix, cfg, node, *a, **k):
        for nt in node:
            for q in (node[nt][0], node[nt][2]):
                if q.requires_grad:
                    q.retain_grad()
                    retain.append(q)
        return orig(sd_, prefix, cfg, node, *a, **k)

    if retain is not None:
        O.conv_layer = spy
    try:
        with torch.enable_grad():
            edges = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)
            args = (leaf, c.cfg, batch, c.prot_x.to(dt), c.x_t.to(dt), c.h_t.to(dt), c.t.to(dt))
            if mutant is None:
                oh, ox = O.dynamics_forward(*args, dropout=dropout, edges=edges)
            else:
                with norm_mutant(mutant):
                    oh, ox = O.dynamics_forward(*args, dropout=dropout, edges=edges)
            ((oh * c.w_h.to(dt)).sum() + (ox * c.w_x.to(dt)).sum()).backward()
    finally:
        O.conv_layer = orig
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad.detach()) for k, v in leaf.items()}
    return grads, oh.detach(), ox.detach()


def test_helpers_restore_the_oracle_and_scale_exactly():
    orig = O.norm_no_nan
    with norm_census() as census:
        assert O.norm_no_nan is not orig
        v = torch.tensor([[[3.0, 4.0, 0.0], [0.0, 0.0, 2.0 ** -17]]])
        assert torch.equal(O.norm_no_nan(v), torch.tensor([[5.0, float(torch.sqrt(torch.tensor(1e-8)))]]))
    assert O.norm_no_nan is orig and list(census.sites) == ["?"]
    assert torch.equal(census.squared("?"), torch.tensor([25.0, 2.0 ** -34]).double())
    assert census.clamped_share() == 0.5 and census.sides().tolist() == [False, True]
    with pytest.raises(ZeroDivisionError):
        with norm_census(lambda: 1 // 0):
            pass
    assert O.norm_no_nan is orig
    with norm_mutant("sqrt"):
        assert float(O.norm_no_nan(torch.zeros(1, 3))) == 0.0
    assert O.norm_no_nan is orig
    for S, V in ((128, 16), (64, 32)):
        cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
        sd = O.make_state_dict(cfg, 0)
        fw = floor_weights(sd)
        changed = [k for k in sd if not torch.equal(sd[k], fw[k])]
        n_gvp = sum(k.endswith(".Wh") for k in sd)
        assert len(changed) == 2 * n_gvp and all(k.endswith((".Wh", ".to_feats_out.0.weight")) for k in changed)
        k = "dynamics.noise_predictor.conv_layers.0.edge_message_fns.prot_pf_pharm.0."
        assert sd[k + "Wh"].shape == (V + 1, V + 1)
        assert torch.equal(fw[k + "Wh"][:, 1::2] * 2.0 ** 20, sd[k + "Wh"][:, 1::2])
        assert torch.equal(fw[k + "Wh"][:, 0::2], sd[k + "Wh"][:, 0::2])
        w, f = sd[k + "to_feats_out.0.weight"], fw[k + "to_feats_out.0.weight"]
        first = w.shape[1] - (V + 1)
        assert first == S + cfg.rbf_dim and torch.equal(f[:, :first], w[:, :first])
        assert torch.equal(f[:, first + 1::2], w[:, first + 1::2] * 2.0 ** 10) and torch.equal(f[:, first::2], w[:, first::2])


def test_twin_inputs_plant_what_they_say():
    for name in TWIN_CONFIGS:
        c = twin_case(name)
        q = 2.0 ** 12
        assert torch.equal(torch.round(c.prot_x * q), c.prot_x * q)
        src, dst = O.build_pp_edges(c.prot_x, c.batch.prot_ptr, c.cfg.cutoff_pp, 100)
        assert torch.equal(src, c.batch.pp_src) and torch.equal(dst, c.batch.pp_dst)
        gid = c.batch.batch_idxs()
        a, b = c.planted["exact twin"]
        assert torch.equal(c.x_t[a], c.x_t[b]) and a != b
        a, p = c.planted["on atom"]
        assert torch.equal(c.x_t[a], c.prot_x[p]) and int(gid["pharm"][a]) == int(gid["prot"][p])
        a, b = c.planted["near twin"]
        assert torch.equal(c.x_t[a] - c.x_t[b], torch.tensor([2.0 ** -15, 0.0, 2.0 ** -14]))
        a2, p = c.planted["near atom"]
        assert torch.equal(c.x_t[a2] - c.prot_x[p], torch.tensor([0.0, -2.0 ** -14, 2.0 ** -16]))
        assert int(gid["pharm"][a2]) == int(gid["prot"][p]) == int(gid["pharm"][a]) != int(gid["pharm"][c.planted["on atom"][0]])
        # the edges that carry the planted pairs exist, and their squared distances are below the floor (0 for the exact ones)
        edges = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)
        ff, pf = set(zip(*[e.tolist() for e in edges["ff"]])), set(zip(*[e.tolist() for e in edges["pf"]]))
        for what, (a, b) in c.planted.items():
            assert ((b, a) in ff and (a, b) in ff) if "twin" in what else (b, a) in pf, (name, what)
        with norm_census(lambda: forward(c, c.sd)) as census:
            pass
        for et, n_small in (("ff", 4), ("pf", 2), ("fp", 2), ("pp", 0)):
            ss = census.squared(f"dynamics.noise_predictor.conv_layers.0.distance.{et}")
            assert int((ss < NORM_EPS).sum()) == n_small and int((ss == 0).sum()) == n_small // 2, (name, et)


def test_coverage_of_the_floor():
    census = floor_census()
    share = {s: census.clamped_share(s) for s in census.sites}
    band = [s for s, v in share.items() if 0.25 <= v <= 0.75]
    fams = {}
    for s in census.sites:
        if site_family(s) not in ("norm", "distance"):
            fams.setdefault(site_family(s), []).append(s)
    print(f"norm floor coverage: {census.clamped_share():.3f} of {census.sides().numel()} entries clamped, "
          f"{len(band)} of {len(census.sites)} sites between 25 % and 75 %")
    for fam, sites in sorted(fams.items()):
        n = sum(census.squared(s).numel() for s in sites)
        k = sum(int((census.squared(s) < NORM_EPS).sum()) for s in sites)
        print(f"  family {fam}: clamped share {k / n:.3f}, {sum(s in band for s in sites)} of {len(sites)} sites in the band")
    assert len(census.sites) == 52
    assert census.clamped_share() >= 0.30
    assert len(band) >= 30
    assert sorted(fams) == ["head", "msg0", "msg1", "upd.pharm", "upd.prot"]
    for fam, sites in fams.items():
        assert any(s in band for s in sites), fam
    # the 64 / 32 model of the wide-family legs
    w = floor_case(64, 32)
    with norm_census(lambda: forward(w, w.live.sd)) as wide:
        pass
    with norm_census(lambda: forward(w, w.live.sd, True)) as wide64:
        pass
    near = min(wide.nearest_to_threshold(), wide64.nearest_to_threshold())
    print(f"  64 / 32 model: {wide.clamped_share():.3f} clamped, nearest to the threshold {near:.2e}")
    assert wide.clamped_share() >= 0.30 and near > 2.0 ** -10 and torch.equal(wide.sides(), wide64.sides())


def test_distance_from_the_threshold():
    c32, c64 = floor_census(), floor_census(True)
    near = c32.nearest_to_threshold()
    print(f"norm floor: nearest squared norm to 1e-8 is a relative {near:.3e} away (bound 2**-10 = {2.0 ** -10:.3e})")
    assert near > 2.0 ** -10 and c64.nearest_to_threshold() > 2.0 ** -10
    assert list(c32.sites) == list(c64.sites)
    assert torch.equal(c32.sides(), c64.sides())
    # The twin inputs run on plain weights.  Their planted squared distances are exact -- 0, 2**-30 + 2**-28 and 2**-28 + 2**-32,
    # less than half of 1e-8 -- in any arithmetic; the other sites hold the ~1 % of naturally small norms, which do come close to
    # the threshold (printed).  The clamp is continuous, so the side an implementation takes there moves a forward value by
    # that closeness times 1e-4 at most; only the backward indicator jumps, by one (row, channel) entry of a tensor's gradient
    # without the 2**up of the floor weights behind it: dropping the indicator on ALL such entries moves the worst tensor by
    # 1e-3 of its maximum.  So the two oracles' agreement is asserted for them, not the distance.
    for name in TWIN_CONFIGS:
        c = twin_case(name)
        with norm_census(lambda: forward(c, c.live.sd)) as a:
            pass
        with norm_census(lambda: forward(c, c.live.sd, True)) as b:
            pass
        print(f"twin inputs {name}: {a.clamped_share():.4f} clamped, nearest to the threshold {a.nearest_to_threshold():.2e}")
        assert torch.equal(a.sides(), b.sides()), name


def test_scatter_headroom():
    """The gradient kernels scatter node-feature gradients on fixed-point accumulators with 2**23 of headroom over the
    upstream gradient (pf_train.h: PFT_FIX_BITS); 2**up in floor_weights must not eat it."""
    c = floor_case()
    Nf, Np = int(c.batch.pharm_ptr[-1]), int(c.batch.prot_ptr[-1])
    kept = []
    oracle_gradients(c, c.sd, O.dropout_masks(c.cfg, Nf, Np, 0.1, 5), retain=kept)
    assert len(kept) >= 2 * c.cfg.n_convs
    worst = max(float(q.grad.abs().max()) for q in kept)
    up = max(float(c.w_h.abs().max()), float(c.w_x.abs().max()))
    print(f"norm floor: largest node-feature gradient {worst:.3e}, largest upstream gradient {up:.3e}, ratio 2**{torch.log2(torch.tensor(worst / up)):.1f}")
    assert worst < 2.0 ** 20 * up


def test_the_forward_tests_bite():
    c = floor_case()
    for mutant in ("sqrt", "floor_after_sqrt"):
        with norm_mutant(mutant):
            mh, mx = forward(c, c.live.sd)
        dh, dx = float((mh - c.live.oh).abs().max()), float((mx - c.live.ox).abs().max())
        print(f"norm floor mutant {mutant}: eps_h moves {dh:.3e}, eps_x {dx:.3e} (tolerance {ATOL:g})")
        assert max(dh, dx) > BITE * ATOL
    for name in TWIN_CONFIGS:
        t = twin_case(name)
        with norm_mutant("sqrt"):
            mh, mx = forward(t, t.live.sd)
        dx = float((mx - t.live.ox).abs().max())
        print(f"distance floor mutant sqrt, twin inputs {name}: eps_x moves {dx:.3e} of {float(t.live.ox.abs().max()):.2f}")
        assert bool(torch.isfinite(mx).all()) and dx > BITE * ATOL


def test_the_gradient_tests_bite():
    c = floor_case()
    Nf, Np = int(c.batch.pharm_ptr[-1]), int(c.batch.prot_ptr[-1])
    drop = O.dropout_masks(c.cfg, Nf, Np, 0.1, 5)
    g, oh, ox = oracle_gradients(c, c.sd, drop)
    gm, mh, mx = oracle_gradients(c, c.sd, drop, mutant="no_indicator")
    assert torch.equal(mh, oh) and torch.equal(mx, ox)            # the forward is the right one
    worst = {}
    for k in g:
        if k.endswith(".Wh"):
            fam = site_family(k[:-2] + "sh")
            fam = "msg" if fam.startswith("msg") else ("upd" if fam.startswith("upd") else fam)
            if float(g[k].abs().max()) == 0.0:          # (the last layer's protein side: no path to the outputs)
                continue
            r = float((gm[k] - g[k]).abs().max()) / float(g[k].abs().max())
            worst[fam] = max(worst.get(fam, (0.0, "")), (r, k))
    for fam, (r, k) in sorted(worst.items()):
        print(f"norm floor mutant no_indicator: worst {fam} Wh gradient moves {r:.3e} of its max ({k}; tolerance {GRAD_TOL:g})")
    assert sorted(worst) == ["head", "msg", "upd"]
    for fam, (r, k) in worst.items():
        assert r > BITE * GRAD_TOL, (fam, r, k)
