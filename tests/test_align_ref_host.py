"""The pharmacophore alignment on the host (analysis.align_pair / align_pharmacophores, PharmacophoreLibrary, ScreenHit;
models.screen_library without an engine; the command line's --screen_queries) against tests/align_ref.py, the numpy composition
of the same definition with SVD Kabsch -- both in fp64, where the two rotation solvers agree to rounding.  No GPU."""
import functools
import math

import numpy as np
import pytest
import torch

import pharmacoforge_amd as pfa
import align_ref as R
from pharmacoforge_amd import analysis as A


def as_torch(ph):
    return torch.from_numpy(np.asarray(ph[0])), torch.from_numpy(np.asarray(ph[1]))


@functools.lru_cache(maxsize=None)
def library_slice():
    """the three queries of the library input against its first 40 entries (centers 1 to 8, the collinear entry among them)"""
    queries, library = R.library_case()
    return queries, library[:40]


@functools.lru_cache(maxsize=None)
def library_reference():
    return R.align_all(*library_slice(), np.float64, want_margin=True)


def assert_host_matches(queries, library, r64=None, **kw):
    r64 = R.align_all(queries, library, np.float64, want_margin=True, **kw) if r64 is None else r64
    assert r64["margin"] >= R.MARGIN
    got = A.align_pharmacophores([as_torch(q) for q in queries], [as_torch(e) for e in library], dtype=torch.float64, **kw)
    assert np.array_equal(got["n_seeds"].numpy(), r64["n_seeds"]) and np.array_equal(got["n_matched"].numpy(), r64["n_matched"])
    assert np.abs(got["sim"].numpy() - r64["sim"]).max() <= 1e-9
    assert np.abs(got["transform"].numpy() - r64["transform"]).max() <= 1e-7
    return got, r64


def test_host_path_matches_the_reference():
    got, r64 = assert_host_matches(*library_slice(), r64=library_reference())
    n = r64["n_seeds"]
    assert (n == 0).any() and (n == 1).any() and (n > 64).any() and (n[:, 7] == 0).all()
    none = torch.from_numpy(n == 0)
    assert (got["sim"][none] == 0).all() and (got["transform"][none] == torch.tensor([1., 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64)).all()


def test_host_path_other_options():
    queries, library = library_slice()
    assert_host_matches(queries, library[:16], sigma=1.5, tolerance=2.0, refine=16, min_area=2.0)
    assert_host_matches(queries, library[:16], refine=0)


def test_host_path_one_type_mirror_and_rigid_copies():
    assert_host_matches(*R.one_type_case())
    got, _ = assert_host_matches(*R.mirror_case())
    assert 0.3 < float(got["sim"][0, 0]) < 0.8                      # an improper rotation would give 1
    for n in (3, 4, 6):
        (q,), (e,) = R.rigid_case(n)
        got, _ = assert_host_matches([q], [e])
        assert int(got["n_matched"][0, 0]) == n and float(got["sim"][0, 0]) >= 1 - 1e-9
        hit = A.ScreenHit(0, "copy", got["sim"][0, 0], n, got["transform"][0, 0], as_torch(e))
        moved, types = hit.aligned()
        d = torch.cdist(as_torch(q)[0].double(), moved.double())
        d[as_torch(q)[1][:, None] != types[None, :]] = float("inf")
        assert float(d.min(dim=1).values.max()) <= 1e-3
    R_ = got["transform"][0, 0][:9].reshape(3, 3)
    assert abs(float(torch.linalg.det(R_)) - 1) < 1e-9


def test_fp32_host_path_within_the_device_bound():
    queries, library = library_slice()
    r64 = library_reference()
    got = A.align_pharmacophores([as_torch(q) for q in queries], [as_torch(e) for e in library])
    assert got["sim"].dtype == torch.float32
    assert np.array_equal(got["n_seeds"].numpy(), r64["n_seeds"]) and np.array_equal(got["n_matched"].numpy(), r64["n_matched"])
    assert np.abs(got["sim"].double().numpy() - r64["sim"]).max() <= R.SIM_BOUND


def test_bad_arguments():
    one = (torch.zeros(1, 3), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"query 1 has 17 centers \(1 to 16 per query\)"):
        pfa.screen_library([one, (torch.zeros(17, 3), torch.zeros(17, dtype=torch.int64))], [one])
    with pytest.raises(ValueError, match=r"entry 0 has 33 centers \(1 to 32 per library entry\)"):
        A.PharmacophoreLibrary([(torch.zeros(33, 3), torch.zeros(33, dtype=torch.int64))])
    for kw, what in ((dict(sigma=0.0), "sigma"), (dict(tolerance=-1.0), "tolerance"), (dict(refine=17), "refine"), (dict(min_area=0.0), "min_area")):
        with pytest.raises(ValueError, match=what):
            A.align_pharmacophores([one], [one], **kw)
    with pytest.raises(ValueError, match="min_match"):
        pfa.screen_library([one], [one], min_match=1.5)
    with pytest.raises(ValueError, match="2 names for 1 entries"):
        A.PharmacophoreLibrary([one], names=["a", "b"])


def planted(seed=23):
    rng = np.random.default_rng(seed)
    (query,), entries = R.random_case(rng, [6], [3 + b % 6 for b in range(24)], 6)
    for b in (5, 17):
        entries[b] = R.rigid_copy(rng, query[0], query[1], jitter=0.2)
    return query, entries


def test_screen_order_filter_and_chunks():
    query, entries = planted()
    r64 = R.align_all([query, entries[3]], entries)
    lib = A.PharmacophoreLibrary([as_torch(e) for e in entries], names=[f"lig{b}" for b in range(len(entries))])
    queries = [as_torch(query), as_torch(entries[3])]
    hits = pfa.screen_library(queries, lib, top_k=len(entries))
    for a, hs in enumerate(hits):
        want = sorted(range(len(entries)), key=lambda b: (-r64["sim"][a, b], b))
        # the fp32 host path against the fp64 reference: the same order wherever two similarities are apart
        for h, b in zip(hs, want):
            assert h.entry == b or abs(r64["sim"][a, h.entry] - r64["sim"][a, b]) <= 2 * R.SIM_BOUND
            assert h.n_matched == r64["n_matched"][a, h.entry] and abs(h.sim - r64["sim"][a, h.entry]) <= R.SIM_BOUND
            assert h.name == f"lig{h.entry}"
        assert all(x.sim > y.sim or (x.sim == y.sim and x.entry < y.entry) for x, y in zip(hs, hs[1:]))
    assert [h.entry for h in hits[0][:2]] in ([5, 17], [17, 5]) and hits[1][0].entry == 3 and hits[1][0].sim >= 1 - 1e-6
    # entries without a seed are listed last with sim 0, in entry order
    tail = [h for h in hits[0] if h.sim == 0.0]
    assert tail and [h.entry for h in tail] == sorted(h.entry for h in tail) and hits[0][-len(tail):] == tail
    # the filter: n_matched >= ceil(min_match * n_q)
    for mm in (0.5, 0.67, 1.0):
        need = math.ceil(mm * 6 - 1e-9)
        got = pfa.screen_library(queries[:1], lib, top_k=100, min_match=mm)[0]
        assert [h.entry for h in got] == [h.entry for h in hits[0] if h.n_matched >= need] and all(h.n_matched >= need for h in got)
    assert [h.entry for h in pfa.screen_library(queries[:1], lib, top_k=3)[0]] == [h.entry for h in hits[0][:3]]
    # chunks: whatever the pair cap of a call, the same lists bit for bit
    for cap in (1, 7, 24, 25):
        again = pfa.screen_library(queries, lib, top_k=len(entries), max_pairs=cap)
        for hs, gs in zip(hits, again):
            assert [(h.entry, h.sim, h.n_matched) for h in hs] == [(h.entry, h.sim, h.n_matched) for h in gs]
            assert all(torch.equal(h.transform, g.transform) for h, g in zip(hs, gs))
    assert pfa.screen_library([], lib) == [] and pfa.screen_library(queries, A.PharmacophoreLibrary([])) == [[], []]


def test_queries_of_every_kind():
    query, entries = planted()
    lib = A.PharmacophoreLibrary([as_torch(e) for e in entries])
    x, t = as_torch(query)
    cons = A.ConsensusPharmacophore(0, 0, [0], x, t, torch.ones(6))

    class Sample:                                   # what screen reads of a SampledPharmacophore
        ph_coords, ph_feats_idxs = x, t
    a, b, c = pfa.screen_library([(x, t), cons, Sample()], lib, top_k=4)
    assert [(h.entry, h.sim) for h in a] == [(h.entry, h.sim) for h in b] == [(h.entry, h.sim) for h in c]
    assert lib.names[5] == "entry_5" and len(lib) == 24 and lib.dropped == 0


def write_xyz(path, phs):
    path.write_text("".join(A._xyz_block([A._XYZ_ELEMENTS[int(k)] for k in t], x) for x, t in phs))


def test_library_from_file_and_cli_screen_queries(tmp_path):
    import generate_pharmacophores as gp
    query, entries = planted()
    big = (np.zeros((33, 3), np.float32) + np.arange(33, dtype=np.float32)[:, None], np.zeros(33, dtype=np.int64))
    write_xyz(tmp_path / "ligands.xyz", entries[:10] + [big] + entries[10:])
    write_xyz(tmp_path / "queries.xyz", [query, entries[3]])
    lib = A.PharmacophoreLibrary.from_file(tmp_path / "ligands.xyz")
    assert len(lib) == 24 and lib.dropped == 1 and lib.names[0] == "ligands:0" and lib.names[10] == "ligands:11"
    queries = A.read_pharmacophores(tmp_path / "queries.xyz")
    want = pfa.screen_library(queries, lib, top_k=5, min_match=0.5, sigma=1.2, tolerance=1.4, refine=2)
    gp.main(["--screen_queries", str(tmp_path / "queries.xyz"), "--screen_library", str(tmp_path / "ligands.xyz"), "--output_dir", str(tmp_path / "out"),
             "--receptor_name", "pocket", "--screen_top", "5", "--screen_min_match", "0.5", "--screen_sigma", "1.2", "--screen_tolerance", "1.4",
             "--screen_refine", "2"])
    rows = [ln.split("\t") for ln in (tmp_path / "out" / "pocket" / "hits.tsv").read_text().splitlines()]
    assert rows[0] == ["query", "rank", "entry", "sim", "matched", "n_q"]
    flat = [(a, k, h) for a, hs in enumerate(want) for k, h in enumerate(hs)]
    assert len(rows) - 1 == len(flat) and len(flat) > 2
    for row, (a, k, h) in zip(rows[1:], flat):
        assert (int(row[0]), int(row[1]), row[2], int(row[4]), int(row[5])) == (a, k, h.name, h.n_matched, len(queries[a][0]))
        assert abs(float(row[3]) - h.sim) <= 1e-5
    frames = A.read_pharmacophores(tmp_path / "out" / "pocket" / "hits_aligned.xyz")
    assert len(frames) == len(flat)
    for (x, t), (_, _, h) in zip(frames, flat):
        moved, types = h.aligned()
        assert torch.equal(t, types) and float((x - moved).abs().max()) <= 2e-3          # three decimals, and fp32 on another device
    # the best hit of the first query lies on it
    d = torch.cdist(queries[0][0].double(), frames[0][0].double())
    d[queries[0][1][:, None] != frames[0][1][None, :]] = float("inf")
    assert float(d.min(dim=1).values.max()) < 1.0


@pytest.mark.parametrize("argv,needle", [
    (["--screen_queries", "q.xyz"], "--screen_queries needs --screen_library"),
    (["r.pdb", "--screen_top", "3"], "--screen_top needs --screen_library"),
    (["--screen_queries", "q.xyz", "--screen_library", "/nonexistent/l.xyz"], "--screen_library / --screen_queries:"),
])
def test_cli_refuses(argv, needle, capsys):
    import generate_pharmacophores as gp
    with pytest.raises(SystemExit):
        gp.parse_arguments(argv)
    assert needle in capsys.readouterr().err


def test_self_rank_of_test_cli():
    """test.py --screen_self: the rank of a pocket's own ligand among the hits of its best sample (the helper, on the host path)"""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("pf_test_cli", os.path.join(root, "test.py"))     # (`test` is also a stdlib package)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    query, entries = planted()
    lib = A.PharmacophoreLibrary([as_torch(e) for e in entries])

    class Sample:
        def __init__(self, ph):
            self.ph_coords, self.ph_feats_idxs = as_torch(ph)
            self.n_ph_centers = len(ph[1])

    class Model:                                    # what self_rank calls of a PharmacophoreDiff
        @staticmethod
        def screen(queries, library, top_k):
            return pfa.screen_library(queries, library, None, top_k=top_k)

    far = (np.zeros((17, 3), np.float32), np.zeros(17, dtype=np.int64))                            # too large to be a query
    samples = [Sample(far), Sample(entries[2]), Sample(query)]
    # the pocket's ligand is entry 5, a jittered copy of the query: sample 2 is its best sample, and it ranks first or second there
    rank, best, sim = cli.self_rank(pfa, Model, lib, 5, samples)
    assert best == 2 and rank in (1, 2) and sim > 0.9
    hits = pfa.screen_library([as_torch(query)], lib, top_k=len(lib))[0]
    assert hits[rank - 1].entry == 5 and hits[rank - 1].sim == sim
    assert cli.self_rank(pfa, Model, lib, 2, samples)[:2] == (1, 1)                                # entry 2 itself is sample 1
    assert cli.self_rank(pfa, Model, lib, None, samples) is None and cli.self_rank(pfa, Model, lib, 5, samples[:1]) is None
