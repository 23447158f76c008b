"""Work done ahead in the merged last launch of a step (k_rg_node_hs_build<HsbExtra>) at the limits its host gates admit:
speculative "pa" rows (BuildParams::pa_same / EdgeParams::pa_skip), edge records (BuildParams::rec) and the center hoist, at up to 64
graphs, pockets of up to 512 atoms, up to PF_MAXF centers per graph and pf_k up to PF_MAXK.

The rows computed ahead and the records must reproduce the plain path (PFDYN_NO_PA_SPEC=1 PFDYN_EDGE_REC=0) bit for bit.  Every run
also proves that the forms engaged (kernel families, pf_debug_ahead, the exchange's time-outs) and runs the consumer-side check
(PFDYN_PA_CHECK=1: every "pa" group the next call skips must carry the serial of the speculative launch that computed it).
PFDYN_PA_SPEC_SPLIT runs the speculative items partly before and partly after the merged launch: the mixed view of the kind-3 counts
that items dispatched late in the launch can see, on every step, without depending on timing.

Sizes above 24,000 active edge rows leave the n16 kernels (and with them every form of work done ahead) under the default policy
(pf_host.cpp: n16_rows_max); the envelope tests raise that limit with PFDYN_N16_ROWS_MAX in both arms of each comparison, and
test_default_policy_at_the_envelope pins what the default does there."""
import random

import pytest
import torch

from oracle import pf_oracle as O
from test_gpu_parity import engine_for, set_batch

pytestmark = pytest.mark.gpu

T = 500
PF_MAXF = 64
WIDE = {"PFDYN_N16_ROWS_MAX": "100000000"}          # the n16 kernels (and the work done ahead) at every size of these tests
PLAIN = {"PFDYN_NO_PA_SPEC": "1", "PFDYN_EDGE_REC": "0"}
CHECK = {"PFDYN_PA_CHECK": "1"}


def _coef():
    return O.step_coefficients(O.gamma_table(T, 0.25), T)        # (bounded schedule: the centers stay inside the pocket)


def _segments(n):
    """n steps at the noisy end, in the middle and at the quiet end of the schedule (s descending)."""
    mid = T // 2 + n // 2
    return [list(range(T - 1, T - 1 - n, -1)), list(range(mid, mid - n, -1)), list(range(n - 1, -1, -1))]


def _noise(Nf, segs, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(len(o) + 1, Nf, 9, generator=gen) for o in segs]


def _run(monkeypatch, cfg, sd, batch, segs, noise, env):
    """One handle created under env; every segment as sample_begin + denoise_step with the plan announced one step past its end (so
    that its last step computes ahead too).  Returns the frame after every step, per segment what the policy reported, and the handle."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine_for(cfg, sd)
    for k in env:
        monkeypatch.delenv(k)
    set_batch(eng, batch)
    coef = _coef()
    frames, info = [], []
    for order, nz in zip(segs, noise):
        arr = eng.coef_array(coef, order + ([order[-1] - 1] if order[-1] > 0 else []))
        eng.prepare_timesteps(arr)
        eng.sample_begin(nz[0])
        ahead, skipped = 0, 0
        for i in range(len(order)):
            eng.denoise_step(arr[i], nz[i + 1])
            x, h = eng.sample_frame()
            frames += [x.cpu(), h.cpu()]
            ahead = max(ahead, eng.ahead()["pa_ahead"])
            skipped = max(skipped, eng.kernel_family(cfg.n_convs + 2))
        torch.cuda.synchronize()
        eng.sample_status()
        info.append(dict(fam0=eng.kernel_family(0), fam_last=eng.kernel_family(cfg.n_convs - 1), tail=eng.kernel_family(cfg.n_convs),
                         cen=eng.kernel_family(cfg.n_convs + 1), skipped=skipped, pa_ahead=ahead))
    assert eng.xchg_timeouts() == 0
    return frames, info, eng


def _first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if not torch.equal(x, y):
            return f"frame {i // 2} ({'xh'[i % 2]}) differs, max |d| = {(x - y).abs().max().item():.3g}"
    return None


def _equal(a, b, what):
    d = _first_difference(a, b)
    assert d is None, f"{what}: {d}"


def _equal_and_checked(a, b, chk, what):
    """Bit for bit the plain path, and the check found every kept group computed (both reported when either fails)."""
    d = _first_difference(a, b)
    assert d is None and chk["checked"] > 0 and chk["violations"] == 0, f"{what}: {d}; check {chk}"


def _assert_engaged(info, what):
    """The forms under test ran: conv layer 0 on the n16 kernels, the merged launch ending every step, rows computed ahead, and the
    quiet segment's calls skipping rows computed ahead."""
    for k, seg in enumerate(info):
        assert seg["fam0"] == 16 and seg["fam_last"] == 17 and seg["tail"] == 2, (what, k, seg)
        assert seg["pa_ahead"] > 0, (what, k, seg)
    assert info[-1]["skipped"] == 1, (what, info[-1])


def _shape(B, seed):
    rng = random.Random(seed)
    if B == 48:                                      # uniform: every graph 512 atoms, 16 centers (the arithmetic item maps)
        n_prot, n_pharm = [512] * B, [16] * B
    else:                                            # ragged up to exactly 512 atoms, 1..16 centers, two graphs at PF_MAXF
        n_prot = [rng.choice([200, 300, 384, 448, 512]) for _ in range(B)]
        n_prot[rng.randrange(B)] = 512
        n_pharm = [rng.randint(1, 16) for _ in range(B)]
        for g in rng.sample(range(B), 2):
            n_pharm[g] = PF_MAXF
    return n_prot, n_pharm


@pytest.mark.parametrize("B,pf_k", [(33, 16), (48, 5), (64, 1)])
def test_work_done_ahead_at_the_gate_limits_bitwise(B, pf_k, monkeypatch):
    """Rows computed ahead, kept prefixes and edge records at 33 / 48 / 64 graphs (the speculation's gate is B <= 64), pockets up to
    exactly 512 atoms (the merged launch's), 1..16 centers with graphs at PF_MAXF, pf_k 1 / 5 / PF_MAXK: three 16-step segments of the
    bounded T = 500 schedule equal PFDYN_NO_PA_SPEC=1 PFDYN_EDGE_REC=0 bit for bit, frames after every step included; the forms
    engaged, and the consumer-side check found every kept group computed by the previous step's speculative items."""
    cfg = O.DynamicsConfig(pf_k=pf_k)
    sd = O.make_state_dict(cfg, 40 + B)
    n_prot, n_pharm = _shape(B, 1000 + B)
    batch = O.synthetic_batch([3000 + 100 * B + i for i in range(B)], n_prot, n_pharm, cfg)
    segs = _segments(16)
    noise = _noise(int(batch.pharm_ptr[-1]), segs, B)
    fa, ia, eng = _run(monkeypatch, cfg, sd, batch, segs, noise, {**WIDE, **CHECK})
    chk = eng.pa_check_counts()
    fp, ip, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, {**WIDE, **PLAIN})
    what = f"B {B}, pf_k {pf_k}, atoms {sorted(set(n_prot))}, centers max {max(n_pharm)}"
    _assert_engaged(ia, what)
    assert all(seg["pa_ahead"] == 0 and seg["skipped"] == 0 for seg in ip), (what, ip)
    _equal_and_checked(fa, fp, chk, what)


@pytest.mark.parametrize("B", [48, 64])
def test_split_speculative_items_equal_the_plain_path(B, monkeypatch):
    """PFDYN_PA_SPEC_SPLIT: items w < k see the kind-3 counts before the build, items w >= k the counts after it -- the mixed view a
    map over the live counts gives items dispatched late in the merged launch.  With k fixed, at half of the non-empty groups and at a
    fraction of them the host picks per step, 300..512-atom pockets: bit for bit the plain path over all three segments, no violation of
    the check, and at least one step in which an earlier graph's group count changed in front of a graph whose rows were kept (the case
    the test is for).  Before the fix the check counted 1-20 missed groups per run here while the frames still agreed: the check is the
    sharper of the two."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 70 + B)
    rng = random.Random(B)
    n_prot = [rng.choice([300, 384, 448, 512]) for _ in range(B)]
    n_pharm = [rng.randint(2, 10) for _ in range(B)]
    batch = O.synthetic_batch([5000 + 100 * B + i for i in range(B)], n_prot, n_pharm, cfg)
    segs = _segments(16)
    noise = _noise(int(batch.pharm_ptr[-1]), segs, 7 * B)
    fp, _, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, {**WIDE, **PLAIN})
    exposed, failed = 0, []
    for split in ("24", "mid", "step"):
        fs, info, eng = _run(monkeypatch, cfg, sd, batch, segs, noise, {**WIDE, **CHECK, "PFDYN_PA_SPEC_SPLIT": split})
        chk = eng.pa_check_counts()
        _assert_engaged(info, f"B {B}, split {split}")
        d = _first_difference(fs, fp)
        if d is not None or chk["checked"] == 0 or chk["violations"] != 0:
            failed.append(f"split {split}: {d}; check {chk}")
        exposed += chk["exposed"]
    assert not failed, f"B {B}: " + " | ".join(failed)
    assert exposed > 0


def _pair(monkeypatch, cfg, sd, batch, n, seed):
    """n middle-of-schedule steps with the defaults of the envelope tests and on the plain path: (frames, info) of both."""
    segs = [_segments(n)[1]]
    noise = _noise(int(batch.pharm_ptr[-1]), segs, seed)
    fa, ia, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, dict(WIDE))
    fp, ip, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, {**WIDE, **PLAIN})
    _equal(fa, fp, f"B {len(batch.prot_ptr) - 1}")
    return ia[0], ip[0]


def test_gate_edge_64_against_65_graphs(monkeypatch):
    """64 graphs compute rows ahead; at 65 the speculation and the edge records are off (B <= 64) and the merged launch runs without
    them; both equal the plain path bit for bit."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 81)
    for B in (64, 65):
        batch = O.synthetic_batch([6000 + i for i in range(B)], 300, [4] * B, cfg)
        ia, ip = _pair(monkeypatch, cfg, sd, batch, 8, B)
        assert ia["fam0"] == 16 and ia["tail"] == 2, (B, ia)
        assert (ia["pa_ahead"] > 0) == (B <= 64), (B, ia)
        assert ip["pa_ahead"] == 0 and ip["skipped"] == 0, (B, ip)


def test_gate_edge_512_against_513_atoms(monkeypatch):
    """The merged launch takes pockets of at most 512 atoms (pf_host.cpp: max_np <= 512): a 512-atom pocket ends every step in it
    with rows computed ahead, a 513-atom pocket in the separate launches without them; both equal the plain path bit for bit."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 82)
    for big in (512, 513):
        n_prot = [256] * 31 + [big]
        batch = O.synthetic_batch([6200 + i for i in range(32)], n_prot, [6] * 32, cfg)
        ia, ip = _pair(monkeypatch, cfg, sd, batch, 8, big)
        assert ia["fam0"] == 16, (big, ia)
        if big == 512:
            assert ia["tail"] == 2 and ia["pa_ahead"] > 0, (big, ia)
        else:
            assert ia["tail"] != 2 and ia["pa_ahead"] == 0, (big, ia)


def test_gate_edge_16_against_17_centers(monkeypatch):
    """At 32 graphs a graph with 17 centers switches the fused launch's XCD split off (pf_host.cpp: max_nf <= 16) and nothing else: both
    end in the merged launch with rows computed ahead, and both equal the plain path bit for bit."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 83)
    for nf in (16, 17):
        n_pharm = [6] * 31 + [nf]
        batch = O.synthetic_batch([6400 + i for i in range(32)], 256, n_pharm, cfg)
        ia, _ = _pair(monkeypatch, cfg, sd, batch, 8, nf)
        assert ia["fam0"] == 16 and ia["fam_last"] == 17 and ia["tail"] == 2 and ia["pa_ahead"] > 0, (nf, ia)


def test_center_hoist_at_64_graphs_equals_on_the_fly_encoding(monkeypatch):
    """The center hoist at 64 graphs x 16 centers, 8 steps at the quiet end of the schedule: equal to PFDYN_NO_CENTER_HOIST=1 at the
    tolerance of test_center_hoist_equals_on_the_fly_encoding, and the hoist's tables were used."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 84)
    B = 64
    batch = O.synthetic_batch([6600 + i for i in range(B)], 384, [16] * B, cfg)
    segs = [_segments(8)[2]]
    noise = _noise(int(batch.pharm_ptr[-1]), segs, 84)
    fh, ih, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, dict(WIDE))
    fe, ie, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, {**WIDE, "PFDYN_NO_CENTER_HOIST": "1"})
    assert ih[0]["cen"] == 1 and ie[0]["cen"] == 0, (ih, ie)
    for a, b in zip(fh, fe):
        torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-3)


def test_default_policy_at_the_envelope(monkeypatch):
    """64 graphs x 512 atoms x 16 centers under the DEFAULT policy: more active edge rows than the n16 kernels take (n16_rows_max), so
    conv layer 0 runs the row-group kernels and nothing is computed ahead; the run equals the plain path bit for bit."""
    import os
    assert not [k for k in os.environ if k.startswith("PFDYN_") and k != "PFDYN_LIB"]
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 85)
    B = 64
    batch = O.synthetic_batch([6800 + i for i in range(B)], 512, [16] * B, cfg)
    segs = [_segments(4)[1]]
    noise = _noise(int(batch.pharm_ptr[-1]), segs, 85)
    fa, ia, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, {})
    fp, ip, _ = _run(monkeypatch, cfg, sd, batch, segs, noise, dict(PLAIN))
    assert ia[0]["fam0"] in (4, 8) and ia[0]["pa_ahead"] == 0 and ia[0]["skipped"] == 0, ia
    _equal(fa, fp, "default policy")


def test_64_graphs_512_atoms_steps_vs_oracle(monkeypatch):
    """The oracle anchor at the envelope: 64 graphs x 512 atoms x 16 centers, the n16 kernels with the work done ahead, three steps
    from the noisy end of the T = 500 schedule against O.sample_step after every step (1e-3, as the config-2 test), the kNN pf and
    the pp edge counts exact."""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    B, n = 64, 3
    batch = O.synthetic_batch(range(7000, 7000 + B), 512, [16] * B, cfg)
    Nf = int(batch.pharm_ptr[-1])
    noise = torch.randn(n + 1, Nf, 9, generator=torch.Generator().manual_seed(42))
    coef = O.step_coefficients(O.gamma_table(T, 1e-5), T)
    for k, v in WIDE.items():
        monkeypatch.setenv(k, v)
    eng = engine_for(cfg, sd)
    set_batch(eng, batch)
    order = list(range(T - 1, T - 1 - n - 1, -1))                  # (the plan one step past the last: that step computes ahead too)
    arr = eng.coef_array(coef, order)
    eng.prepare_timesteps(arr)
    eng.sample_begin(noise[0])
    bidx = batch.batch_idxs()
    init_com = O.segment_mean(batch.prot_x, batch.prot_ptr)
    px = batch.prot_x - init_com[bidx["prot"]]
    x_t, h_t = noise[0][:, :3].clone(), noise[0][:, 3:].clone()
    for i in range(n):
        eng.denoise_step(arr[i], noise[i + 1])
        x, h = eng.sample_frame()
        with torch.no_grad():
            px, x_t, h_t = O.sample_step(sd, cfg, batch, coef, order[i], px, x_t, h_t, noise[1 + i][:, :3], noise[1 + i][:, 3:])
        ox = x_t - O.segment_mean(px, batch.prot_ptr)[bidx["pharm"]] + init_com[bidx["pharm"]]
        torch.testing.assert_close(x.cpu(), ox, rtol=1e-3, atol=1e-3)
        torch.testing.assert_close(h.cpu(), h_t, rtol=1e-3, atol=1e-3)
        assert eng.kernel_family(0) == 16 and eng.kernel_family(cfg.n_convs) == 2, (i, eng.kernel_family(0), eng.kernel_family(cfg.n_convs))
        assert eng.ahead()["pa_ahead"] > 0
    ne = eng.work()[2]
    assert ne[1] == cfg.pf_k * Nf and ne[2] == ne[1] and ne[3] == batch.pp_src.numel()
    assert eng.xchg_timeouts() == 0
