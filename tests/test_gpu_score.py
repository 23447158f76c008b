"""Scoring given pharmacophores on the device (pf_score; k_score_prepare / k_score_eval around the inference forward): the
per-level terms and the weighted score against the CPU composition (tests/score_ref.py) inside the fp64 error budget, the
reference's own eval-mode forward and the training call rebuilt from the terms, batch independence and pocket sharing, level
handling, what the call leaves on the handle, and the Python / CLI surface end to end.

Measured on an MI355X, worst ratio err / max(e32, 2**-22) (the bound is 8).  Test 1, over both widths, both heads, remove_com
on and off and the four parameterisations: pos 0.51, feat 0.35, err 0.48, score columns 0.33 / 0.33.  Test 4: with the claim
0.31 / 0.34 / 0.24, without 0.54 / 0.34 / 0.43, the candidate alone 0.54 / 0.34 / 0.14 (pos / feat / err).  hits equal
everywhere.  e32, the fp32 composition's own distance from the fp64 one, is computed by the CPU oracle wherever the test runs:
tests/test_score_host.py asserts it within one floor for every case (at most 0.87 floors where that suite was run); on the
GPU machine's host, whose CPU rounds some sums differently, the same quantity came out at up to 1.12 floors (2.68e-7, the
cross-entropy feat term at 64 / 32) -- the budget takes max(e32, floor) either way, so the bound was 8 to 9 floors."""
import os
import subprocess
import sys

import pytest
import torch

import pharmacoforge_amd as pfa
from pharmacoforge_amd.engine import _dptr, _f32, _stream_ptr
from oracle import pf_oracle as O
from helpers import batch_from, load, with_head, within_budget
import score_ref as R
from test_gpu_api import graph_from, make_model
from test_gpu_wide import engine_for, set_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_POS, W_FEAT = [0.5, 0.25, 2.0], [1.0, 0.125, 0.75]
OUT_KEYS = ("pos loss", "feat loss", "position error", "weighted position error", "accuracy", "weighted accuracy")


def bound_engine(width, head):
    c = R.inputs(width)
    eng = engine_for(c.cfg, R.weights(width, head))
    set_batch(eng, c.batch)
    return c, eng


def run_score(eng, c, levels=R.LEVELS, noise=None, w=(W_POS, W_FEAT), T=R.T, **kw):
    _, al, sg = R.tables()
    return eng.score(c.x0, c.h0, levels, c.noise if noise is None else noise, w[0], w[1], al, sg, T, **kw)


# -- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", list(R.WIDTHS))
@pytest.mark.parametrize("remove_com,head", with_head([True, False]))
def test_terms_and_score_match_the_composition(width, remove_com, head):
    c, eng = bound_engine(width, head)
    ref32, ref64 = R.reference(width, head, remove_com, False), R.reference(width, head, remove_com, True)
    for ep_coord, ep_feat in R.PARAMS:
        score, terms = run_score(eng, c, remove_com=remove_com, ep_coord=ep_coord, ep_feat=ep_feat)
        t32, t64 = ref32[(ep_coord, ep_feat)][0], ref64[(ep_coord, ep_feat)][0]
        what = f"{width} {head} com={remove_com} ep=({int(ep_coord)},{int(ep_feat)})"
        for q, name in enumerate(("pos", "feat", "err")):
            within_budget(terms[:, :, q], t32[:, :, q], t64[:, :, q], f"{what} {name}")
        assert torch.equal(terms[:, :, 3].cpu().double(), t64[:, :, 3]), (what, terms[:, :, 3].cpu(), t64[:, :, 3])
        s32, s64 = R.score_of(t32, W_POS, W_FEAT), R.score_of(t64, W_POS, W_FEAT)
        for q, name in enumerate(("score pos", "score feat")):
            within_budget(score[:, q], s32[:, q], s64[:, q], f"{what} {name}")


# -- 2 ------------------------------------------------------------------------------------------------------------------
def rebuild_outputs(terms, own, t_int, T, n_per_graph, nf):
    """the six outputs of PharmacophoreDiff.forward from per-graph sums: terms [L, B, 4], own[g] = index of graph g's level"""
    B = len(own)
    row = torch.stack([terms[own[g], g] for g in range(B)]).double()
    Nf = float(sum(n_per_graph))
    wm = 1.0 - torch.as_tensor(t_int).double() / T
    return {"pos loss": float(row[:, 0].sum()) / (Nf * 3), "feat loss": float(row[:, 1].sum()) / (Nf * nf),
            "position error": float(row[:, 2].sum()) / Nf, "weighted position error": float((wm * row[:, 2]).sum()) / Nf,
            "accuracy": float(row[:, 3].sum()) / Nf, "weighted accuracy": float((wm * row[:, 3]).sum()) / Nf}


def test_the_reference_forward_is_rebuilt_from_the_terms():
    z = load("train_fwd.npz")
    T = int(z["T"])
    m = make_model(T)
    batch = batch_from(z)
    eng = m.dynamics.bind_graph(graph_from(batch, z["x0"], z["h0"]).to("cuda"))
    tabs = m._loss_tables()
    t_int = [int(t) for t in z["t_int"]]
    levels = sorted(set(t_int))
    eps = torch.cat([z["eps_x"], z["eps_h"]], dim=1)
    noise = eps[None].expand(len(levels), -1, -1).contiguous()
    w = [1.0 / len(levels)] * len(levels)
    _, terms = eng.score(z["x0"], z["h0"], levels, noise, w, w, tabs[0], tabs[1], T)
    sizes = (batch.pharm_ptr[1:] - batch.pharm_ptr[:-1]).tolist()
    got = rebuild_outputs(terms.cpu(), [levels.index(t) for t in t_int], t_int, T, sizes, 6)
    for k in OUT_KEYS:
        ref = float(z["out_train_" + k.replace(" ", "_")])
        print(k, got[k], ref)
        assert abs(got[k] - ref) <= 2e-4 * max(1.0, abs(ref)), (k, got[k], ref)


# -- 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ep_coord,ep_feat", R.PARAMS)
def test_one_level_equals_the_training_call(ep_coord, ep_feat):
    c, eng = bound_engine("128x16", "live")
    _, al, sg = R.tables()
    B, level = c.batch.batch_size, R.LEVELS[1]
    out = eng.train_loss_forward(c.x0, c.h0, torch.full((B,), level, dtype=torch.int32), c.noise[1][:, :3], c.noise[1][:, 3:], al, sg,
                                 R.T, 1.0, True, False, dropout=0.0, ep_coord=ep_coord, ep_feat=ep_feat).cpu()
    _, terms = run_score(eng, c, levels=[level], noise=c.noise[1:2], w=([1.0], [1.0]), ep_coord=ep_coord, ep_feat=ep_feat)
    got = rebuild_outputs(terms.cpu(), [0] * B, [level] * B, R.T, R.N_PHARM, c.cfg.pharm_nf)
    for i, k in enumerate(OUT_KEYS):
        print(k, got[k], float(out[i]))
        assert abs(got[k] - float(out[i])) <= 2e-4 * max(1.0, abs(float(out[i]))), (k, got[k], float(out[i]))


# -- 4 ------------------------------------------------------------------------------------------------------------------
def one_pocket_case():
    cfg = O.DynamicsConfig()
    sizes = [2, 5, 9, 4]
    pocket = O.synthetic_batch([21], 96, [1], cfg)
    batch = O.concat_pockets([O.copy_pocket(pocket, n) for n in sizes])
    gen = torch.Generator().manual_seed(5)
    Nf = sum(sizes)
    x0 = 3.0 * torch.randn(Nf, 3, generator=gen)
    h0 = torch.nn.functional.one_hot(torch.randint(0, 6, (Nf,), generator=gen), 6).float()
    noise = torch.randn(len(R.LEVELS), Nf, 9, generator=gen)
    return cfg, pocket, batch, sizes, x0, h0, noise


def test_batch_independence_and_pocket_sharing():
    cfg, pocket, batch, sizes, x0, h0, noise = one_pocket_case()
    c = R.inputs("128x16")
    sd = R.weights("128x16", "live")
    _, al, sg = R.tables()
    ref = {dbl: R.compose(sd, cfg, batch, x0, h0, R.LEVELS, noise, R.T, al, sg, double=dbl)[(False, False)][0] for dbl in (False, True)}
    eng = engine_for(cfg, sd)
    got, edges = {}, {}
    for claim in (False, True):
        eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst,
                      pocket_uid=torch.full((len(sizes),), 7) if claim else None)
        runs = [eng.score(x0, h0, R.LEVELS, noise, W_POS, W_FEAT, al, sg, R.T) for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])       # the same call twice: equal bits
        got[claim] = runs[0]
        edges[claim] = eng.work_detail()["executed_edges_per_layer"][0]
        for q, name in enumerate(("pos", "feat", "err")):
            within_budget(got[claim][1][:, :, q], ref[False][:, :, q], ref[True][:, :, q], f"claim={claim} {name}")
        assert torch.equal(got[claim][1][:, :, 3].cpu().double(), ref[True][:, :, 3])
    print("conv layer 0 edges computed without / with the claim:", edges)
    # the claim was honoured: conv layer 0 ran on the shared edge list (the union of what the copies need of the pocket's pp edges,
    # computed once, instead of each copy's own -- with four small candidates the union need not be the shorter list)
    assert edges[True] != edges[False], edges
    # candidate 2 alone: the same candidate inside the batch
    k = 2
    f0, f1 = sum(sizes[:k]), sum(sizes[:k + 1])
    alone = O.copy_pocket(pocket, sizes[k])
    set_batch(eng, alone)
    _, t1 = eng.score(x0[f0:f1], h0[f0:f1], R.LEVELS, noise[:, f0:f1].contiguous(), W_POS, W_FEAT, al, sg, R.T)
    for q, name in enumerate(("pos", "feat", "err")):
        within_budget(t1[:, 0, q], ref[False][:, k, q], ref[True][:, k, q], f"alone {name}")
    assert torch.equal(t1[:, 0, 3].cpu().double(), ref[True][:, k, 3])


# -- 5 ------------------------------------------------------------------------------------------------------------------
def test_level_handling():
    c, eng = bound_engine("128x16", "live")
    _, al, sg = R.tables()
    levels = [(7 * i) % R.T + 1 for i in range(65)]                   # 65 levels: crosses the 64-timestep chunk of the tables
    levels[64] = levels[3]
    levels[40] = levels[3]
    gen = torch.Generator().manual_seed(2)
    Nf = int(c.batch.pharm_ptr[-1])
    noise = torch.randn(65, Nf, 9, generator=gen)
    noise[64] = noise[3]
    noise[40] = noise[3]
    w = [1.0 / 65] * 65
    dev = eng.device
    x0, h0, nz, ald, sgd = (_f32(t, dev) for t in (c.x0, c.h0, noise, al, sg))
    arr = (pfa._lib.PfScoreLevel * 65)(*[pfa._lib.PfScoreLevel(t, a, b) for t, a, b in zip(levels, w, w)])
    score = torch.full((c.batch.batch_size, 2), float("nan"), device=dev)          # pre-filled: the first level stores
    terms = torch.empty(65, c.batch.batch_size, 4, device=dev)
    score2 = torch.full((c.batch.batch_size, 2), float("nan"), device=dev)
    with torch.cuda.device(dev):
        for sc, tm in ((score, terms), (score2, None)):
            rc = eng.lib.pf_score(eng._h, _dptr(x0), _dptr(h0), 65, arr, _dptr(nz), _dptr(ald), _dptr(sgd), R.T, 1.0, 1, 0, 0, _dptr(sc),
                                  _dptr(tm), _stream_ptr())
            assert rc == 0, eng.lib.pf_last_error(eng._h)
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(terms).all())
    assert torch.equal(terms[3], terms[64]) and torch.equal(terms[3], terms[40])
    assert not torch.equal(terms[3], terms[4])
    assert torch.equal(score, score2)                                  # dev_terms = NULL: the same score bits
    acc = torch.zeros_like(score)
    for l in range(65):                                                # the score is the terms added in level order
        acc += torch.tensor(w[l], device=dev) * terms[l, :, :2]
    assert torch.equal(acc, score)


# -- 6 ------------------------------------------------------------------------------------------------------------------
def test_what_a_score_call_leaves_on_the_handle():
    c, eng = bound_engine("128x16", "live")
    _, al, sg = R.tables()
    T = R.T
    Nf = int(c.batch.pharm_ptr[-1])
    gen = torch.Generator().manual_seed(8)
    noise = torch.randn(T + 1, Nf, 9, generator=gen)
    coef = eng.coef_array(O.step_coefficients(O.gamma_table(T, R.PRECISION), T), reversed(range(T)))
    plain = eng.sample(coef, 6, noise)
    torch.cuda.synchronize()
    eng.sample_status()
    set_batch(eng, c.batch)
    run_score(eng, c)
    after = eng.sample(coef, 6, noise)
    torch.cuda.synchronize()
    eng.sample_status()
    assert torch.equal(plain[0], after[0]) and torch.equal(plain[1], after[1])
    # inside a run: refused, and the run goes on with the bits it has without the refusal
    eng.sample_begin(noise[0])
    eng.denoise_step(coef[0], noise[1])
    with pytest.raises(pfa._lib.PfError, match="pf_score inside a plain run"):
        run_score(eng, c)
    for i in range(1, 6):
        eng.denoise_step(coef[i], noise[i + 1])
    x, h = eng.sample_end()
    assert torch.equal(x, plain[0]) and torch.equal(h, plain[1])
    # a kept training forward does not survive a score call (include/pfdyn.h)
    set_batch(eng, c.batch)
    x_t, h_t, t = torch.randn(Nf, 3, generator=gen), torch.randn(Nf, 6, generator=gen), torch.rand(c.batch.batch_size, generator=gen)
    eng.train_forward(x_t, h_t, t)
    run_score(eng, c)
    with pytest.raises(pfa._lib.PfError, match="no pf_train_forward"):
        eng.train_backward(torch.zeros(Nf, 6), torch.zeros(Nf, 3))
    # a seed armed with pf_sample_seed_next stays armed across a score call: the next begin starts from it
    a = 6
    seed_x, seed_h = c.x0 + 0.25, c.h0
    seed_coef = pfa.schedule.seed_coefficients(O.gamma_table(T, R.PRECISION), T, a)
    coef_a = eng.coef_array(O.step_coefficients(O.gamma_table(T, R.PRECISION), T), reversed(range(a)))
    set_batch(eng, c.batch)
    seeded = eng.sample(coef_a, a, noise, seed=(seed_x, seed_h, seed_coef))
    set_batch(eng, c.batch)
    eng.seed_next(seed_x, seed_h, seed_coef)
    run_score(eng, c)
    behind = eng.sample(coef_a, a, noise)
    torch.cuda.synchronize()
    eng.sample_status()
    assert torch.equal(seeded[0], behind[0]) and torch.equal(seeded[1], behind[1])
    assert not torch.equal(behind[0], eng.sample(coef_a, a, noise)[0])          # (consumed by that begin: this run is unseeded)


def test_a_refused_score_call_launches_nothing():
    """Every refusal leaves the row / edge counts of the last dynamics call (pf_debug_counts: device memory that every edge build
    of a level rewrites) and a kept training forward as they were.  The counts in front of the refusals are those of a training
    forward on OTHER coordinates than the candidates', so a level launched by a refused call would change them."""
    c, eng = bound_engine("128x16", "live")
    _, al, sg = R.tables()
    T, Nf, B = R.T, int(c.batch.pharm_ptr[-1]), c.batch.batch_size
    run_score(eng, c)
    of_a_score = eng.counts()
    gen = torch.Generator().manual_seed(12)
    x_t, h_t, t = 0.5 * torch.randn(Nf, 3, generator=gen), torch.randn(Nf, 6, generator=gen), torch.rand(B, generator=gen)
    w_h, w_x = torch.randn(Nf, 6, generator=gen), torch.randn(Nf, 3, generator=gen)
    eng.train_forward(x_t, h_t, t)
    want_grad = eng.train_backward(w_h, w_x).clone()
    eng.train_forward(x_t, h_t, t)
    before = eng.counts()
    assert before != of_a_score, (before, of_a_score)
    dev = eng.device
    x0, h0, nz, ald, sgd = (_f32(t_, dev) for t_ in (c.x0, c.h0, c.noise, al, sg))
    score = torch.zeros(B, 2, device=dev)
    Lv = pfa._lib.PfScoreLevel
    good = (Lv * 3)(*[Lv(t_, 1.0, 1.0) for t_ in R.LEVELS])

    def call(e=eng, x0=x0, h0=h0, n=3, arr=good, nz=nz, al_=ald, sg_=sgd, T_=T, fn=1.0, sc=score):
        with torch.cuda.device(dev):
            return e.lib.pf_score(e._h, _dptr(x0), _dptr(h0), n, arr, _dptr(nz), _dptr(al_), _dptr(sg_), T_, fn, 1, 0, 0, _dptr(sc), None,
                                  _stream_ptr())
    bad_levels = [(Lv * 3)(Lv(1, 1.0, 1.0), Lv(T + 1, 1.0, 1.0), Lv(2, 1.0, 1.0)), (Lv * 3)(Lv(-1, 1.0, 1.0), Lv(1, 1.0, 1.0), Lv(2, 1.0, 1.0))]
    cases = [dict(x0=None), dict(h0=None), dict(arr=None), dict(nz=None), dict(al_=None), dict(sg_=None), dict(sc=None), dict(n=0), dict(n=-2),
             dict(arr=bad_levels[0]), dict(arr=bad_levels[1]), dict(fn=0.0), dict(fn=-1.0), dict(fn=float("nan")), dict(T_=0)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert eng.counts() == before, kw
    # the kept forward is still good: its backward gives the bits it gave in front of the refusals
    assert torch.equal(eng.train_backward(w_h, w_x), want_grad)
    assert eng.counts() == before
    # a batch without centers
    empty = O.synthetic_batch([31], 40, [0], c.cfg)
    set_batch(eng, empty)
    of_the_bind = eng.counts()
    assert call(x0=torch.zeros(1, 3, device=dev), h0=torch.zeros(1, 6, device=dev), nz=torch.zeros(3, 1, 9, device=dev)) == -1
    assert "no pharmacophore centers" in eng.lib.pf_last_error(eng._h).decode()
    assert eng.counts() == of_the_bind
    # no batch
    fresh = engine_for(c.cfg, R.weights("128x16", "live"))
    assert call(e=fresh) == -3
    # more feature columns than the evaluation kernel holds
    cfg9 = O.DynamicsConfig(pharm_nf=9)
    wide9 = engine_for(cfg9, O.make_state_dict(cfg9, 0))
    b9 = O.synthetic_batch([32], 40, [3], cfg9)
    set_batch(wide9, b9)
    of_the_bind = wide9.counts()
    assert call(e=wide9, x0=torch.zeros(3, 3, device=dev), h0=torch.zeros(3, 9, device=dev), nz=torch.zeros(3, 3, 12, device=dev),
                sc=torch.zeros(1, 2, device=dev)) == -1
    assert "pharm_nf 9" in wide9.lib.pf_last_error(wide9._h).decode()
    assert wide9.counts() == of_the_bind
    # and the handle still scores
    set_batch(eng, c.batch)
    assert call() == 0 and bool(torch.isfinite(score).all())


# -- 7 ------------------------------------------------------------------------------------------------------------------
def synthetic_pocket_graph(seed=41, n=80):
    b = O.synthetic_batch([seed], n, [1], O.DynamicsConfig())
    return pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, torch.tensor([0, 0]), b.pp_src, b.pp_dst, torch.zeros(0, 3), torch.zeros(0, 6))


def test_model_score_equals_the_engine_call_and_sample_attaches_scores():
    T = 12
    m = make_model(T)
    g = synthetic_pocket_graph()
    gen = torch.Generator().manual_seed(4)
    cands = [(3.0 * torch.randn(n, 3, generator=gen), torch.randint(0, 6, (n,), generator=gen)) for n in (3, 6, 4)]
    levels = pfa.schedule.score_levels(T, 4)
    scores = m.score([g], [cands], levels=levels, seed=9)[0]
    assert len(scores) == 3 and [s.n_centers for s in scores] == [3, 6, 4]
    # the same batch through the engine
    batch = O.concat_pockets([O.copy_pocket(O.PocketBatch(g.prot_x, g.prot_h, g.prot_ptr, torch.tensor([0, 1]), g.pp_src, g.pp_dst), n)
                              for n in (3, 6, 4)])
    eng = m.dynamics.engine()
    eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst, pocket_uid=torch.full((3,), 5))
    m.dynamics._batch_key = None
    x0 = torch.cat([c[0] for c in cands])
    h0 = torch.cat([torch.nn.functional.one_hot(c[1], 6).float() for c in cands])
    nz = torch.randn(4, 13, 9, generator=torch.Generator().manual_seed(9))
    w = pfa.schedule.score_weights(m.gamma.gamma, T, levels, "uniform")
    tabs = m._loss_tables()
    sc, tm = eng.score(x0, h0, levels, nz, w[0], w[1], tabs[0], tabs[1], T)
    for k, s in enumerate(scores):
        assert s.pos == float(sc[k, 0]) and s.feat == float(sc[k, 1]) and torch.equal(s.terms, tm[:, k].cpu())
        assert s.total == s.pos + s.feat and s.per_center == s.total / s.n_centers and 0.0 <= s.type_accuracy <= 1.0
    with pytest.raises(ValueError, match="pharmacophore 1: 65 centers"):
        m.score([g], [[cands[0], (torch.zeros(65, 3), torch.zeros(65, dtype=torch.int64))]])
    with pytest.raises(ValueError, match="pharmacophore 0: 0 centers"):
        m.score([g], [[(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int64))]])
    # sample(..., score_levels=4): scores attached, the samples bit for bit what they are without
    runs = []
    for k in (None, 4):
        torch.manual_seed(3)
        runs.append(m.sample([g], [[4, 5, 4]], max_batch_size=8, score_levels=k)[0])
    for a, b in zip(*runs):
        assert torch.equal(a.ph_coords, b.ph_coords) and torch.equal(a.g.pharm_h0, b.g.pharm_h0)
        assert a.score is None and b.score is not None and b.score.n_centers == b.n_ph_centers and len(b.score.levels) == 4
        assert b.score.total == b.score.total and b.score.total > 0
    again = m.score([g], [[(p.ph_coords, p.ph_feats_idxs) for p in runs[1]]], levels=levels, max_batch_size=8)[0]
    assert [s.total for s in again] == [p.score.total for p in runs[1]]


def test_cli_scores_samples_and_given_pharmacophores(tmp_path):
    from test_gpu_api import _tiny_run_dir, _write_pocket_files
    _, run_dir = _tiny_run_dir(tmp_path, T=12)
    _write_pocket_files(tmp_path)

    def cli(out, *extra):
        cmd = [sys.executable, os.path.join(ROOT, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
               str(tmp_path / "lig.sdf"), "--model_dir", str(run_dir), "--output_dir", str(out), "--seed", "5", *extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        return out / "rec"

    def rows(path):
        lines = path.read_text().splitlines()
        assert lines[0].split("\t") == ["index", "centers", "total", "per_center", "pos", "feat", "position_error", "type_accuracy"]
        return [ln.split("\t") for ln in lines[1:]]
    # (the sizes are given: drawn sizes come from numpy's unseeded generator, as in the reference, and differ from run to run)
    draw = ("--samples_per_pocket", "4", "--pharm_sizes", "3", "6", "4", "5")
    full = cli(tmp_path / "full", *draw, "--score_samples", "4")
    frames = pfa.analysis.read_pharmacophores(full / "pharms.xyz")
    table = rows(full / "scores.tsv")
    assert len(frames) == 4 and [int(r[0]) for r in table] == [0, 1, 2, 3] and [int(r[1]) for r in table] == [f[0].shape[0] for f in frames]
    best = cli(tmp_path / "best", *draw, "--score_samples", "4", "--keep_best", "2")
    kept, kept_table = pfa.analysis.read_pharmacophores(best / "pharms.xyz"), rows(best / "scores.tsv")
    print("scores of the four samples:", table, "kept:", kept_table)
    assert all(float(v) == float(v) and abs(float(v)) != float("inf") for r in table for v in r[2:])
    order = sorted(range(4), key=lambda i: (float(table[i][3]), i))[:2]
    assert len(kept) == 2 and len(kept_table) == 2
    for (x, t), row, i in zip(kept, kept_table, order):                 # best first, ordered as scores.tsv
        assert torch.equal(x, frames[i][0]) and torch.equal(t, frames[i][1]) and row[1:] == table[i][1:]
    assert float(kept_table[0][3]) <= float(kept_table[1][3])
    # the frames of the first run, scored from the file: the same seed and levels give that run's scores
    again = cli(tmp_path / "again", "--score_pharmacophores", str(full / "pharms.xyz"), "--score_samples", "4")
    assert not (again / "pharms.xyz").exists()
    assert rows(again / "scores.tsv") == table           # (scores.tsv describes the frames as pharms.xyz holds them)
