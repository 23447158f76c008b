"""Sample-set analysis on the device (pf_sample_set_analyze: k_sset_overlap, k_sset_cluster, k_sset_consensus)
against the CPU composition of tests/sample_set_ref.py.

Inputs: the planted groups (3 groups of 5 / 4 / 3 samples with 5 / 4 / 7 centers, interleaved) and, in one call, random sets of
S = 1, 2, 17 and 33 samples with center counts drawn from {1, 2, 6, 63, 64} in a 6 A box, at pharm_nf 6 and 11.  At the default
options those random sets have no similarity above 0.28, so every sample is its own cluster: the "wide" case is the same kind of
input at sigma 1.5, tolerance 2.0, threshold 0.3, where the 33-sample set has a cluster of 16 large samples.  Similarities and
consensus positions go through helpers.within_budget against fp64 with the fp32 composition as ref32; supports, labels, centroids,
sizes, cluster counts and consensus counts are exact -- the clusters against butina run on the device's own matrix read back, so
that no threshold tie can decide the test.  The conditions on the inputs (no distance within 1e-3 A of the tolerance, no
nearest / second-nearest gap of a consensus under 1e-3 A) are asserted by the builders.

Measured on the MI355X, ratio of the error against fp64 to max(e32, 2**-22), of the allowed 8: similarity 0.44 (planted), at most
0.24 / 0.16 (random, nf 6 / 11), 0.60 (wide), 0.95 (S = 1024), 0.23 (4 x 64 centers); consensus positions at most 0.55."""
import functools

import numpy as np
import pytest
import torch

import pharmacoforge_amd as pfa
import sample_set_ref as R
from helpers import within_budget
from oracle import pf_oracle as O

pytestmark = pytest.mark.gpu

ERR_ARG = r"\(-1\)"
OUT = ("similarity", "support", "label", "centroid", "size", "n_clusters", "cons_x", "cons_cnt")


@functools.lru_cache(maxsize=None)
def engine(nf=6):
    return pfa.PfEngine(pharm_nf=nf, device="cuda:0")


@functools.lru_cache(maxsize=None)
def planted_sets():
    samples, group = R.planted()
    return (tuple(samples),), group


WIDE = dict(sigma=1.5, tolerance=2.0, threshold=0.3)


def options(kind):
    return WIDE if kind == "wide" else dict(sigma=R.SIGMA, tolerance=R.TOLERANCE, threshold=R.THRESHOLD)


@functools.lru_cache(maxsize=None)
def random_sets(nf, kind="random"):
    return tuple(R.random_sets(nf=nf, seed=21 if kind == "wide" else nf, **options(kind)))


def inputs(kind, nf):
    return planted_sets()[0] if kind == "planted" else random_sets(nf, kind)


@functools.lru_cache(maxsize=None)
def reference(kind, nf, dtype):
    """per set of the input: sample_set_ref.analyze at one precision (computed once, shared, never changed)"""
    return tuple(R.analyze(*R.flat(list(st)), dtype=np.float64 if dtype == 64 else np.float32, **options(kind)) for st in inputs(kind, nf))


def run(eng, sets, **kw):
    x, t, sp, cp = R.pack_sets(sets)
    out = eng.sample_set(torch.from_numpy(x), torch.from_numpy(t), sp, cp, **kw)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}, sp, cp


def split(out, sp, cp):
    """the call's outputs per set: dicts of sim [S, S], support / cons_cnt [n], cons_x [n, 3], label, centroid, size [S], n_clusters"""
    per, at = [], 0
    for p in range(len(sp) - 1):
        s0, s1 = int(sp[p]), int(sp[p + 1])
        S, c0, c1 = s1 - s0, int(cp[s0]), int(cp[s1])
        per.append(dict(sim=out["similarity"][at:at + S * S].reshape(S, S), support=out["support"][c0:c1], cons_x=out["cons_x"][c0:c1],
                        cons_cnt=out["cons_cnt"][c0:c1], label=out["label"][s0:s1], centroid=out["centroid"][s0:s1],
                        size=out["size"][s0:s1], n_clusters=int(out["n_clusters"][p])))
        at += S * S
    return per


CASES = [("planted", 6), ("random", 6), ("random", 11), ("wide", 6)]


@functools.lru_cache(maxsize=None)
def device_result(kind, nf):
    out, sp, cp = run(engine(nf), inputs(kind, nf), **options(kind))
    return tuple(split(out, sp, cp)), out


# 1. similarity
@pytest.mark.parametrize("kind,nf", CASES)
def test_similarity_vs_fp64(kind, nf):
    got, _ = device_result(kind, nf)
    for p, (g, r32, r64) in enumerate(zip(got, reference(kind, nf, 32), reference(kind, nf, 64))):
        sim = g["sim"]
        assert np.array_equal(sim.view(np.uint32), sim.T.view(np.uint32)), f"set {p}: the matrix is not bitwise symmetric"
        assert np.array_equal(np.diagonal(sim).view(np.uint32), np.full(sim.shape[0], 1.0, np.float32).view(np.uint32))
        assert sim.min() >= 0.0 and sim.max() <= 1.0
        within_budget(sim, r32["sim"], r64["sim"], f"similarity, {kind} nf {nf} set {p} (S = {sim.shape[0]})")


# 2. support
@pytest.mark.parametrize("kind,nf", CASES)
def test_support_exact(kind, nf):
    got, _ = device_result(kind, nf)
    for g, r64 in zip(got, reference(kind, nf, 64)):
        assert np.array_equal(g["support"], r64["support"])
    if kind == "planted":
        sets, group = planted_sets()
        sizes = np.bincount(group)
        want = np.concatenate([np.full(len(s[1]), sizes[k] - 1) for s, k in zip(sets[0], group)])
        assert np.array_equal(got[0]["support"], want)


def check_clusters(g, labels, centroids, sizes):
    k = len(centroids)
    assert g["n_clusters"] == k
    assert np.array_equal(g["label"], labels)
    assert np.array_equal(g["centroid"][:k], centroids) and np.array_equal(g["size"][:k], sizes)
    assert (g["centroid"][k:] == -1).all() and (g["size"][k:] == -1).all()


# 3. clusters
@pytest.mark.parametrize("kind,nf", CASES)
def test_clusters_exact_on_the_device_matrix(kind, nf):
    got, _ = device_result(kind, nf)
    for g in got:
        labels, centroids, sizes, _ = R.butina(g["sim"], options(kind)["threshold"])
        check_clusters(g, labels, centroids, sizes)
    if kind == "wide":
        assert max(got[3]["size"]) >= 8          # (a real cluster: the consensus test walks its members)
    if kind == "planted":
        _, group = planted_sets()
        lab = got[0]["label"]
        assert got[0]["n_clusters"] == len(set(group.tolist()))
        for a in range(len(group)):
            for b in range(len(group)):
                assert (lab[a] == lab[b]) == (group[a] == group[b])
        assert sorted(got[0]["size"][:3].tolist(), reverse=True) == got[0]["size"][:3].tolist() == [5, 4, 3]


# 4. consensus
@pytest.mark.parametrize("kind,nf", CASES)
def test_consensus(kind, nf):
    got, _ = device_result(kind, nf)
    sets, tol = inputs(kind, nf), options(kind)["tolerance"]
    for p, (g, st) in enumerate(zip(got, sets)):
        x, t, cptr = R.flat(list(st))
        k = g["n_clusters"]
        c64, n64 = R.consensus(x, t, cptr, g["label"], g["centroid"][:k].tolist(), tol, dtype=np.float64)
        c32, _ = R.consensus(x, t, cptr, g["label"], g["centroid"][:k].tolist(), tol, dtype=np.float32)
        assert np.array_equal(g["cons_cnt"], n64)
        within_budget(g["cons_x"], c32, c64, f"consensus positions, {kind} nf {nf} set {p}")
        filled = np.zeros(len(t), dtype=bool)
        for m in g["centroid"][:k]:
            filled[cptr[m]:cptr[m + 1]] = True
        assert (g["cons_cnt"][filled] >= 1).all() and (g["cons_cnt"][~filled] == 0).all() and (g["cons_x"][~filled] == 0).all()
    if kind == "planted":
        # within the jitter of the motif: the mean of positions within 0.2 A of a point is within 0.2 A of it
        g, (x, t, cptr) = got[0], R.flat(list(sets[0]))
        for c in range(g["n_clusters"]):
            m = g["centroid"][c]
            assert np.abs(g["cons_x"][cptr[m]:cptr[m + 1]] - x[cptr[m]:cptr[m + 1]]).max() <= 0.4
            assert (g["cons_cnt"][cptr[m]:cptr[m + 1]] == g["size"][c]).all()


# 5. caps
def check_whole_set(st, what):
    """one set against the reference: similarity under the budget, support exact, clusters exact on the device's matrix, consensus
    counts exact and positions under the budget on the device's clusters -- whose choices have no runner-up within 1e-3 A (asserted)"""
    out, sp, cp = run(engine(), [st])
    g = split(out, sp, cp)[0]
    x, t, cptr = R.flat(st)
    within_budget(g["sim"], R.similarity(x, t, cptr, dtype=np.float32), R.similarity(x, t, cptr), f"similarity, {what}")
    assert np.array_equal(g["sim"].view(np.uint32), g["sim"].T.view(np.uint32))
    assert np.array_equal(g["support"], R.support(x, t, cptr))
    labels, centroids, sizes, _ = R.butina(g["sim"])
    check_clusters(g, labels, centroids, sizes)
    gaps = []
    c64, n64 = R.consensus(x, t, cptr, g["label"], centroids, dtype=np.float64, gaps=gaps)
    c32, _ = R.consensus(x, t, cptr, g["label"], centroids, dtype=np.float32)
    assert all(gap >= 1e-3 for gap, _ in gaps), "the input has a consensus choice with a runner-up within 1e-3 A: choose another seed"
    assert np.array_equal(g["cons_cnt"], n64)
    within_budget(g["cons_x"], c32, c64, f"consensus positions, {what}")
    return g


def test_cap_1024_samples():
    rng = np.random.default_rng(5)
    # (a 3 A box and three types: a few hundred clusters, the largest of some twenty samples)
    st = [(rng.uniform(0.0, 3.0, (2, 3)).astype(np.float32), rng.integers(0, 3, 2)) for _ in range(1024)]
    g = check_whole_set(R.clear_of_tolerance(st, rng, 0.0, 3.0), "S = 1024")
    assert 100 < g["n_clusters"] < 600 and g["size"].max() >= 10


def test_cap_64_centers():
    """4 samples x 64 centers: full LDS rows, bit 63 of the partner mask, a full tile of the consensus kernel"""
    rng = np.random.default_rng(6)
    base = rng.uniform(0.0, 9.0, (64, 3))
    types = rng.integers(0, 6, 64)
    st = [((base + rng.uniform(-0.3, 0.3, base.shape)).astype(np.float32), types.copy()) for _ in range(4)]
    g = check_whole_set(R.clear_of_tolerance(st, rng, 0.0, 9.0), "4 x 64 centers")
    assert g["n_clusters"] == 1 and g["support"][63::64].max() == 3 and g["cons_cnt"].max() == 4


def test_identical_samples_have_similarity_one():
    """duplicates (frames are written to three decimals): O(a,b) is summed in O(a,a)'s order, so the similarity is exactly 1.0f and the
    two are neighbours at threshold 1; no value of the matrix leaves [0, 1]"""
    rng = np.random.default_rng(8)
    for n in (1, 7, 8, 9, 64):
        one = (rng.uniform(0.0, 5.0, (n, 3)).astype(np.float32), rng.integers(0, 3, n))
        near = (np.nextafter(one[0], np.float32(9.0)), one[1])
        other = (rng.uniform(0.0, 5.0, (n, 3)).astype(np.float32), one[1])
        st = [one, other, (one[0].copy(), one[1].copy()), near] + [one] * 15          # (the copies span two tiles)
        out, sp, cp = run(engine(), [st], threshold=1.0)
        g = split(out, sp, cp)[0]
        same = [0, 2] + list(range(4, 19))
        assert (g["sim"][np.ix_(same, same)].view(np.uint32) == np.float32(1.0).view(np.uint32)).all(), n
        assert g["sim"].max() <= 1.0 and g["sim"].min() >= 0.0
        assert g["label"][same].tolist() == [0] * 17 and g["size"][0] >= 17


def test_caps_refused_before_any_launch():
    eng = engine()
    one = (np.zeros((1, 3), np.float32), np.zeros(1, np.int64))
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*set 0 has 1025 samples"):
        run(eng, [[one] * 1025])
    big = (np.zeros((65, 3), np.float32), np.zeros(65, np.int64))
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*sample 1 has 65 centers"):
        run(eng, [[one, big]])
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*sigma"):
        run(eng, [[one]], sigma=0.0)
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*threshold"):
        run(eng, [[one]], threshold=1.5)


def test_type_out_of_range_reported():
    eng = engine()
    st = [(np.zeros((2, 3), np.float32), np.array([0, 6])), (np.ones((1, 3), np.float32), np.array([-1]))]
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*2 centers have a type outside \[0, 6\)"):
        run(eng, [st])
    out, sp, cp = run(engine(11), [[(np.zeros((2, 3), np.float32), np.array([0, 6]))]])        # in range at pharm_nf 11
    assert out["n_clusters"][0] == 1
    run(eng, list(planted_sets()[0]))           # and the handle goes on


# 6. repeatable
def test_two_calls_same_bytes():
    sets = random_sets(6)
    a, _, _ = run(engine(), sets)
    b, _, _ = run(engine(), sets)
    for k in OUT:
        assert a[k].tobytes() == b[k].tobytes(), k


# 7. alone and among others
def test_a_set_alone_equals_the_set_among_others():
    sets = random_sets(6)
    among, _ = device_result("random", 6)
    for p in (2, 3):
        out, sp, cp = run(engine(), [sets[p]])
        alone = split(out, sp, cp)[0]
        for k, v in alone.items():
            assert np.asarray(v).tobytes() == np.asarray(among[p][k]).tobytes(), (p, k)


def test_similarity_kept_in_the_workspace():
    sets = random_sets(6)
    _, full = device_result("random", 6)
    out, _, _ = run(engine(), sets, want_similarity=False)
    assert out["similarity"] is None
    for k in OUT[1:]:
        assert out[k].tobytes() == full[k].tobytes(), k


# 8. the handle's run state is untouched
def test_sampling_run_unchanged_by_a_call():
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    batch = O.synthetic_batch([0, 1], 64, [4, 3], cfg)
    T = 20
    noise = torch.randn(4, int(batch.pharm_ptr[-1]), 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(7))
    coef = O.step_coefficients(O.gamma_table(T, 1e-5), T)

    def sample(eng):
        return eng.sample(eng.coef_array(coef, reversed(range(T))), 3, noise)

    eng = pfa.PfEngine(device="cuda:0")
    eng.load_state_dict(sd)
    eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst)
    x_a, h_a = (t.cpu() for t in sample(eng))
    eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst)
    before, _, _ = run(eng, random_sets(6))
    x_b, h_b = (t.cpu() for t in sample(eng))
    assert torch.equal(x_a, x_b) and torch.equal(h_a, h_b)
    ref, _ = device_result("random", 6)[1], None
    for k in OUT:
        assert before[k].tobytes() == ref[k].tobytes(), k


# 9. the surface
def as_torch(samples):
    return [(torch.from_numpy(np.asarray(x)), torch.from_numpy(np.asarray(t))) for x, t in samples]


def test_model_consensus_device_equals_host():
    from test_gpu_api import make_model
    m = make_model(12)
    pockets = [as_torch(planted_sets()[0][0]), [], as_torch(random_sets(6, "wide")[3])]
    dev = m.consensus(pockets, **WIDE, min_support=0.25)
    host = m.consensus(pockets, **WIDE, min_support=0.25, device="cpu")
    assert dev[1] is None and host[1] is None
    for p in (0, 2):
        d, h = dev[p], host[p]
        x, t, cptr = R.flat([(a.numpy(), b.numpy()) for a, b in pockets[p]])
        within_budget(d.similarity, h.similarity, R.similarity(x, t, cptr, WIDE["sigma"]), f"model.consensus similarity, pocket {p}")
        assert torch.equal(d.labels, h.labels) and d.centroids == h.centroids and torch.equal(d.neighbour_counts, h.neighbour_counts)
        assert all(torch.equal(a, b) for a, b in zip(d.support, h.support))
        assert [c.cluster for c in d.clusters] == [c.cluster for c in h.clusters]
        r64 = R.consensus(x, t, cptr, h.labels.numpy(), h.centroids, WIDE["tolerance"])[0]
        for cd, ch in zip(d.clusters, h.clusters):
            assert cd.members == ch.members and torch.equal(cd.counts, ch.counts) and torch.equal(cd.types, ch.types)
            rows = slice(cptr[cd.centroid], cptr[cd.centroid + 1])
            within_budget(cd.positions, ch.positions, r64[rows], f"model.consensus positions, pocket {p} cluster {cd.cluster}")
        assert d.pick_diverse(4) == h.pick_diverse(4)
        assert d.options == h.options and d.options["min_support"] == 0.25
    assert max(c.size for c in dev[2].clusters) >= 8


def test_sample_returns_the_sets():
    from test_gpu_api import graph_from, make_model
    n_t = 12
    cfg = O.DynamicsConfig()
    m = make_model(n_t)
    pockets = [graph_from(O.synthetic_batch([s], n, 1, cfg)) for s, n in ((60, 48), (61, 40))]
    n_pharms = [[3, 5, 4], [4, 3]]
    gen = torch.Generator().manual_seed(11)
    nz = [torch.randn(n_t + 1, 12, 9, generator=gen), torch.randn(n_t + 1, 7, 9, generator=gen)]
    kw = dict(max_batch_size=3, lanes=2, noise=nz)
    plain = m.sample(pockets, n_pharms, **kw)
    samples, sets = m.sample(pockets, n_pharms, consensus=dict(threshold=0.25), **kw)
    for a, b in zip([p for o in plain for p in o], [p for o in samples for p in o]):
        assert torch.equal(a.ph_coords, b.ph_coords) and torch.equal(a.g.pharm_h0, b.g.pharm_h0)
    assert [s.n_samples for s in sets] == [3, 2] and all(s.options["threshold"] == 0.25 for s in sets)
    again = m.consensus(samples, threshold=0.25)
    for s, t in zip(sets, again):
        assert torch.equal(s.similarity, t.similarity) and torch.equal(s.labels, t.labels)
    assert m.sample(pockets, n_pharms, consensus=True, **kw)[1][0].options["threshold"] == 0.5


def test_cli_consensus_files(tmp_path):
    """generate_pharmacophores.py --consensus --keep_diverse on a tiny seeded run: consensus.xyz and clusters.tsv are those of the
    host analysis of the frames the run drew (as written: three decimals), pharms.xyz holds the max-min picks, and the same run
    without the flags writes the same first files and no new ones"""
    import os
    import subprocess
    import sys
    import yaml
    from test_gpu_api import _write_pocket_files
    from test_sample_set_host import parse_consensus_xyz
    from pharmacoforge_amd import analysis as A
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
    base = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
            str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "6", "--pharm_sizes", "3", "4", "5", "3", "4", "5",
            "--max_batch_size", "6", "--seed", "1"]
    # (this fixture's seeded random weights throw the centers far apart: a wide Gaussian and tolerance make the samples neighbours)
    flags = ["--consensus", "--keep_diverse", "2", "--consensus_sigma", "400", "--consensus_tolerance", "800", "--consensus_threshold",
             "0.05", "--min_support", "0.2"]
    for out, extra in ((tmp_path / "plain", []), (tmp_path / "cons", flags)):
        r = subprocess.run(base + ["--output_dir", str(out)] + extra, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
    plain, cons = tmp_path / "plain" / "rec", tmp_path / "cons" / "rec"
    assert not (plain / "consensus.xyz").exists() and not (plain / "clusters.tsv").exists()
    frames = A.read_pharmacophores(plain / "pharms.xyz")
    assert len(frames) == 6
    want = A.analyze_sample_set(frames, sigma=400.0, tolerance=800.0, threshold=0.05, min_support=0.2)
    got_frames, want_frames = parse_consensus_xyz((cons / "consensus.xyz").read_text()), parse_consensus_xyz(want.consensus_xyz())
    assert len(got_frames) == len(want_frames) == len(want.clusters)
    for (ge, gx, gs), (we, wx, ws) in zip(got_frames, want_frames):
        assert ge == we and gs == ws and np.abs(gx - wx).max() <= 1.5e-3
    rows = [ln.split("\t") for ln in (cons / "clusters.tsv").read_text().splitlines()]
    ref_rows = [ln.split("\t") for ln in want.clusters_tsv().splitlines()]
    assert rows[0] == ref_rows[0] + ["pick"] and [r[:4] for r in rows[1:]] == [r[:4] for r in ref_rows[1:]]
    assert all(abs(float(a[4]) - float(b[4])) <= 1e-4 for a, b in zip(rows[1:], ref_rows[1:]))
    picks = want.pick_diverse(2)
    assert [int(r[5]) for r in rows[1:]] == [picks.index(a) if a in picks else -1 for a in range(6)]
    kept = A.read_pharmacophores(cons / "pharms.xyz")
    assert len(kept) == 2
    for k, a in enumerate(picks):
        assert torch.equal(kept[k][0], frames[a][0]) and torch.equal(kept[k][1], frames[a][1])


def test_dataset_driver_consensus(tmp_path):
    """test.py --consensus on two ranks: per pocket consensus.xyz and clusters.tsv are those of the host analysis of the pocket's
    frames as written, and consensus_summary.txt holds the means over all pockets of all ranks (the counters are all-reduced)"""
    import os
    import subprocess
    import sys
    from test_gpu_api import _tiny_run_dir
    from test_sample_set_host import parse_consensus_xyz
    from pharmacoforge_amd import analysis as A
    root, run_dir = _tiny_run_dir(tmp_path)
    out = tmp_path / "samples"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29683", os.path.join(root, "test.py"), "--model_dir", str(run_dir), "--samples_per_pocket", "3", "--pharm_sizes",
           "3", "5", "4", "--max_batch_size", "4", "--output_dir", str(out), "--pockets_per_call", "2", "--consensus"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    n_clusters, supports = [], []
    for i in range(5):
        want = A.analyze_sample_set(A.read_pharmacophores(out / f"pocket_{i}" / "pharms.xyz"))
        got, ref = parse_consensus_xyz((out / f"pocket_{i}" / "consensus.xyz").read_text()), parse_consensus_xyz(want.consensus_xyz())
        assert len(got) == len(ref) == len(want.clusters)
        for (ge, gx, gs), (we, wx, ws) in zip(got, ref):
            assert ge == we and gs == ws and np.abs(gx - wx).max() <= 1.5e-3
        rows = [ln.split("\t") for ln in (out / f"pocket_{i}" / "clusters.tsv").read_text().splitlines()]
        ref_rows = [ln.split("\t") for ln in want.clusters_tsv().splitlines()]
        assert [r_[:4] for r_ in rows] == [r_[:4] for r_ in ref_rows] and len(rows) == 4
        n_clusters.append(len(want.clusters))
        supports += want.mean_support()
    summary = dict(ln.split(": ") for ln in (out / "consensus_summary.txt").read_text().splitlines())
    assert abs(float(summary["clusters_per_pocket"]) - sum(n_clusters) / 5) <= 5e-4
    assert abs(float(summary["mean_support"]) - sum(supports) / 15) <= 5e-4
