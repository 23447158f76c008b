"""The item fronts of the fused launch and of conv layer 0's "pa" items: what stands between a wave's start and its first gather.

k_n16_fused_u requests a group's edge records, its count and the first quads of its weights from preloaded arguments before its
first wait, and leaves -- for a group beyond the region's count -- only behind the shadowing of the records; every kernel-argument
field of the node update arrives in one block of scalar loads (n16_fused_args), also in k_n16_fused and in the store items;
k_n16_edge_u's "pa" items read the regions' counts, their starts and the kept prefixes in one batch through preloaded addresses.
None of it changes a value: eight denoising steps from the noisy end of a T = 50 schedule must equal, frame and eps after every
step and bit for bit, the same run without edge records (PFDYN_EDGE_REC=0: the chased front) and the same run without rows
computed ahead (PFDYN_NO_PA_SPEC=1: no kept prefixes) -- each on a handle of its own, created under that environment, which
pf_create reads per handle; that each environment took effect is asserted from the handle (the forms' record bit, pa_ahead) --
and agree with the oracle's steps at the tolerance test_gpu_n16.py holds step frames to (1e-3).

Which groups a case exercises.  The ff region of a graph with n centers has capacity n (n - 1) (pf_bind.cpp) and
ceil(capacity / 16) groups; the ff edges are a radius graph, so with the default 9 A cutoff and the bounded schedule (precision
0.25: the centers stay at the pocket) every region is FULL and no group is ever beyond the count -- the pf regions (kNN) always
are full.  The cases therefore shrink the ff cutoff to 2 A (counts change from step to step, below the capacity) or take the
unbounded schedule (precision 1e-5: the centers fly apart, the ff count is 0 from the second call on), and assert from the
oracle's own edge build -- whose totals eng.counts() must match in every step -- that the groups they are there for occurred.
Which item maps ran (k_n16_edge_u / k_n16_fused_u / records) is asserted from pf_debug_kernel_family(n_convs + 3)."""
import pytest
import torch

from oracle import pf_oracle as O
from test_gpu_parity import engine_for, set_batch

pytestmark = pytest.mark.gpu

T, N_STEPS = 50, 8
ENVS = {"default": {}, "chased": {"PFDYN_EDGE_REC": "0"}, "no_pa_spec": {"PFDYN_NO_PA_SPEC": "1"}}
EDGE_U, FUSED_U, RECORDS = 1, 2, 4           # bits of eng.kernel_family(n_convs + 3)

# name -> (centers per graph, atoms per pocket, pf_k, schedule precision, ff cutoff, item maps of the default run's last step,
#          what must occur among the ff groups of the run)
CASES = {
    # one center: the ff capacity is 0, the batch has no ff group at all and is not "uniform" for the arithmetic maps: the work lists
    # (k_n16_edge<true>, k_n16_fused and its store items) with the one-block arguments
    "B1_one_center": ([1], [28], 5, 0.25, 9.0, 0, ()),
    # one graph, two ff groups, ff count 0 from the second call on: both groups of k_n16_fused_u / k_n16_edge_u take the exit behind the
    # shadowing with the records' and the weights' loads in flight
    "B1_six_centers_no_ff_edges": ([6], [28], 5, 1e-5, 9.0, EDGE_U | FUSED_U | RECORDS, ("region_empty",)),
    # 4 centers: capacity 12, ONE group per region, ragged and changing (2..8 of 16 rows)
    "B2_four_centers": ([4, 4], [20, 36], 5, 0.25, 2.0, EDGE_U | FUSED_U | RECORDS, ("ragged",)),
    # 6 centers: capacity 30, two groups: graph 0 fills the first and leaves the second ragged, graph 1 leaves the first ragged and
    # the second EMPTY (beyond the count)
    "B2_six_centers_pfk1": ([6, 6], [24, 40], 1, 0.25, 2.0, EDGE_U | FUSED_U | RECORDS, ("ragged", "group_beyond_count", "second_ragged")),
    "B2_six_centers_pfk5": ([6, 6], [24, 40], 5, 0.25, 2.0, EDGE_U | FUSED_U | RECORDS, ("ragged", "group_beyond_count", "second_ragged")),
    # not uniform: k_n16_fused and k_n16_edge<true> (the work lists) instead of the _u forms
    "B3_ragged_centers": ([3, 6, 8], [20, 30, 40], 5, 0.25, 2.0, 0, ("ragged",)),
    # the "pa" scan of k_n16_edge_u over more than 32 lanes; the fused launch's XCD split takes at most 32 graphs, so it runs k_n16_fused
    "B33_six_centers": ([6] * 33, [24] * 33, 5, 0.25, 2.0, EDGE_U, ("ragged", "group_beyond_count")),
}


def _run(monkeypatch, cfg, sd, batch, noise, env, prec):
    """Eight steps on a handle created under env: frames and eps after every step, the counts of every step's dynamics call and the
    kernel families of the last."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_for(cfg, sd)
    for k in env:
        monkeypatch.delenv(k)
    set_batch(eng, batch)
    coef = O.step_coefficients(O.gamma_table(T, prec), T)
    order = list(range(T - 1, T - 1 - N_STEPS - 1, -1))            # (the plan one step past the last: that step computes ahead too)
    arr = eng.coef_array(coef, order)
    eng.prepare_timesteps(arr)
    eng.sample_begin(noise[0])
    out, counts, forms = [], [], []
    for i in range(N_STEPS):
        eng.denoise_step(arr[i], noise[i + 1])
        x, h = eng.sample_frame()
        eh, ex = eng.last_eps()
        out.append((x.cpu(), h.cpu(), eh.cpu(), ex.cpu()))
        counts.append(eng.counts())
        forms.append(eng.kernel_family(cfg.n_convs + 3))
    torch.cuda.synchronize()
    eng.sample_status()
    assert eng.xchg_timeouts() == 0
    fam = dict(fam0=eng.kernel_family(0), fam_last=eng.kernel_family(cfg.n_convs - 1), tail=eng.kernel_family(cfg.n_convs),
               pa_ahead=eng.ahead()["pa_ahead"], forms=forms)
    return out, counts, fam


def _oracle(cfg, sd, batch, noise, prec):
    """The oracle's eight steps: the frame after every step, and the per-graph ff / pf edge counts of every step's dynamics call and
    of the call that would follow the last (N_STEPS + 1 entries: a step ends with the next call's edge build)."""
    coef = O.step_coefficients(O.gamma_table(T, prec), T)
    bidx = batch.batch_idxs()
    init_com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    px = batch.prot_x - init_com[bidx["prot"]]
    x_t, h_t = noise[0][:, :3].clone(), noise[0][:, 3:].clone()
    frames, ff, pf = [], [], []
    for i in range(N_STEPS):
        edges = O.build_dynamic_edges(cfg, batch, px, x_t)
        ff.append(torch.bincount(bidx["pharm"][edges["ff"][1]], minlength=batch.batch_size).tolist())
        pf.append(int(edges["pf"][0].numel()))
        with torch.no_grad():
            px, x_t, h_t = O.sample_step(sd, cfg, batch, coef, T - 1 - i, px, x_t, h_t, noise[1 + i][:, :3], noise[1 + i][:, 3:])
        frames.append((x_t - O.segment_mean(px, batch.prot_ptr)[bidx["pharm"]] + init_com[bidx["pharm"]], h_t.clone()))
    edges = O.build_dynamic_edges(cfg, batch, px, x_t)
    ff.append(torch.bincount(bidx["pharm"][edges["ff"][1]], minlength=batch.batch_size).tolist())
    pf.append(int(edges["pf"][0].numel()))
    return frames, ff, pf


def _ff_groups(n_pharm, ff):
    """What occurred among the ff groups of a run (ff[step][graph] = the graph's ff edge count in that call)."""
    seen = set()
    for per_graph in ff:
        for nf, cnt in zip(n_pharm, per_graph):
            groups = (nf * (nf - 1) + 15) // 16
            used = (cnt + 15) // 16
            if groups > 0 and cnt == 0:
                seen.add("region_empty")
            if used < groups:
                seen.add("group_beyond_count")
            if cnt % 16:
                seen.add("ragged")
            if used == 2 and cnt % 16:
                seen.add("second_ragged")
    return seen


@pytest.mark.parametrize("name", list(CASES))
def test_item_fronts_equal_the_chased_and_the_plain_path_bitwise(name, monkeypatch):
    n_pharm, n_prot, pf_k, prec, cut, want_forms, want_groups = CASES[name]
    B = len(n_pharm)
    cfg = O.DynamicsConfig(pf_k=pf_k, cutoff_ff=cut)
    sd = O.make_state_dict(cfg, 300 + B)
    batch = O.synthetic_batch([9100 + 10 * B + i for i in range(B)], n_prot, n_pharm, cfg)
    Nf = int(batch.pharm_ptr[-1])
    noise = torch.randn(N_STEPS + 1, Nf, 9, generator=torch.Generator().manual_seed(600 + B + pf_k))
    runs = {k: _run(monkeypatch, cfg, sd, batch, noise, env, prec) for k, env in ENVS.items()}
    frames, ff, pf = _oracle(cfg, sd, batch, noise, prec)
    seen = _ff_groups(n_pharm, ff[:N_STEPS])                             # (the calls the run made)
    print(name, {k: r[2] for k, r in runs.items()}, "ff per graph and step:", ff if B <= 3 else [(min(f), max(f)) for f in ff], "groups seen:", sorted(seen))

    # the forms under test ran: the n16 kernels, the fused launch, the merged last launch with rows computed ahead; the item maps
    # the case is there for; and each environment took effect
    fam = runs["default"][2]
    assert fam["fam0"] == 16 and fam["fam_last"] == 17 and fam["tail"] == 2 and fam["pa_ahead"] > 0, (name, fam)
    assert all(f == want_forms for f in fam["forms"][1:]), (name, fam["forms"], want_forms)      # (the first call's edges come without records)
    assert all(f == want_forms & ~RECORDS for f in runs["chased"][2]["forms"]), (name, runs["chased"][2]["forms"])
    assert runs["no_pa_spec"][2]["pa_ahead"] == 0 and runs["no_pa_spec"][2]["forms"][1:] == fam["forms"][1:], (name, runs["no_pa_spec"][2])

    # the groups the case is there for: the counts a step's edge build leaves on the device (read after step i: those of call i + 1)
    # equal the oracle's edge build, and that build has them
    got = runs["default"][0]
    for i, c in enumerate(runs["default"][1]):
        assert c["ff"] == sum(ff[i + 1]) and c["pf"] == pf[i + 1] == pf_k * Nf, (name, i, c, ff[i + 1], pf[i + 1])
    assert set(want_groups) <= seen, (name, want_groups, sorted(seen), ff)
    if name == "B1_one_center":
        assert all(sum(f) == 0 for f in ff) and not seen                 # no ff group at all
    if name == "B1_six_centers_no_ff_edges":
        assert all(sum(f) == 0 for f in ff[1:N_STEPS])                   # two groups, both beyond the count, in seven of the eight calls

    # bit for bit: frames and eps after every step
    for other in ("chased", "no_pa_spec"):
        for i, (a, b) in enumerate(zip(got, runs[other][0])):
            for what, u, v in zip(("x", "h", "eps_h", "eps_x"), a, b):
                assert torch.equal(u, v), f"{name}: step {i}, {what} differs from the {other} run, max |d| = {(u - v).abs().max().item():.3g}"

    # and the oracle's steps
    for i, (ox, oh) in enumerate(frames):
        torch.testing.assert_close(got[i][0], ox, rtol=1e-3, atol=1e-3, msg=lambda m: f"{name}: step {i} x: {m}")
        torch.testing.assert_close(got[i][1], oh, rtol=1e-3, atol=1e-3, msg=lambda m: f"{name}: step {i} h: {m}")
