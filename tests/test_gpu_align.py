"""Pharmacophore alignment on the device (pf_pharm_align: k_align_self, k_align_pairs) against the numpy reference of
tests/align_ref.py (SVD Kabsch, fp64).

Integers (n_seeds, n_matched) are exact for every pair.  sim is held to align_ref.SIM_BOUND = 8 x the largest |fp32 - fp64| of the
reference itself over these inputs (1.62e-7 -> 1.30e-6); a pair may be left out only when the reference's own fp32 and fp64 runs
differ by more than the bound, and align_ref.checked asserts that no input has such a pair.  The conditions on the inputs (no seed
filter and no matched distance within 1e-3 of its bound in fp64, at most 2e5 seeds per input) are asserted there too.

Inputs (align_ref.gpu_cases): Q = 3 queries of 3 / 5 / 6 centers against L = 130 entries of 1 to 8 centers, six and two types --
sub-libraries of 1, 63, 64 and 65 entries and Q = 1 are calls over its slices; 16 x 32 and 16 x 4 centers with six types; 8 x 8
centers of one type; rigid copies of 3, 4, 6 and 16 centers tens of angstroms away; a chiral query against its mirror image."""
import functools

import numpy as np
import pytest
import torch

import pharmacoforge_amd as pfa
import align_ref as R
from oracle import pf_oracle as O

pytestmark = pytest.mark.gpu

ERR_ARG = r"\(-1\)"
OUT = ("sim", "n_matched", "n_seeds", "transform")


@functools.lru_cache(maxsize=None)
def engine(nf=6):
    return pfa.PfEngine(pharm_nf=nf, device="cuda:0")


@functools.lru_cache(maxsize=None)
def cases():
    return R.gpu_cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(fp64, fp32) reference of one input, with the input's conditions asserted (computed once, shared, never changed)"""
    return R.checked(*cases()[name])


def run(eng, queries, library, want_transform=True, **kw):
    qx, qt, qp = R.pack(queries)
    lx, lt, lp = R.pack(library)
    out = eng.align(torch.from_numpy(qx), torch.from_numpy(qt), qp, torch.from_numpy(lx), torch.from_numpy(lt), lp,
                    want_transform=want_transform, **kw)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def device_result(name):
    return run(engine(), *cases()[name])


def assert_matches(got, r64, what):
    assert np.array_equal(got["n_seeds"], r64["n_seeds"]), what
    assert np.array_equal(got["n_matched"], r64["n_matched"]), what
    err = np.abs(got["sim"].astype(np.float64) - r64["sim"])
    print(f"{what}: max |sim - fp64| = {err.max():.3e} of the allowed {R.SIM_BOUND:.3e}")
    assert err.max() <= R.SIM_BOUND, (what, float(err.max()), np.argwhere(err > R.SIM_BOUND)[:5].tolist())
    assert (got["sim"] >= 0).all() and (got["sim"] <= 1).all()


# 1. against the reference
@pytest.mark.parametrize("name", ["library", "caps", "one_type"])
def test_against_the_reference(name):
    r64, _ = reference(name)
    assert_matches(device_result(name), r64, name)


def test_library_covers_the_seed_counts():
    """the library input has pairs without a seed, with one, with fewer than the 64 lanes that share a pair and with more; entries
    of one and two centers and the collinear entry have none"""
    r64, _ = reference("library")
    n = r64["n_seeds"]
    assert (n == 0).any() and (n == 1).any() and ((n > 1) & (n < R.LANES)).any() and (n > R.LANES).any()
    sizes = np.array([len(t) for _, t in cases()["library"][1]])
    assert (n[:, sizes <= 2] == 0).all() and (n[:, 7] == 0).all() and sizes[7] == 3
    got = device_result("library")
    none = n == 0
    assert (got["sim"][none] == 0).all() and (got["n_matched"][none] == 0).all()
    assert (got["transform"][none] == np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)).all()
    assert reference("one_type")[0]["n_seeds"][0, 0] > 1000 and reference("caps")[0]["n_seeds"][0, 0] > 1000


def test_transforms_are_proper_rotations():
    for name in ("library", "caps", "one_type", "mirror"):
        xf = device_result(name)["transform"].reshape(-1, 12).astype(np.float64)
        Rm = xf[:, :9].reshape(-1, 3, 3)
        assert np.abs(np.linalg.det(Rm) - 1).max() < 1e-5, name
        assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5, name


# 2. rigid copies
@pytest.mark.parametrize("n", [3, 4, 6, 16])
def test_rigid_copy_found(n):
    name = f"rigid{n}"
    (q,), (e,) = cases()[name]
    r64, _ = reference(name)
    assert r64["n_matched"][0, 0] == n and r64["sim"][0, 0] >= 1 - 1e-5
    got = device_result(name)
    assert_matches(got, r64, name)
    assert got["n_matched"][0, 0] == n and got["sim"][0, 0] >= 1 - 1e-5
    xf = got["transform"][0, 0].astype(np.float64)
    moved = e[0].astype(np.float64) @ xf[:9].reshape(3, 3).T + xf[9:]
    # every query center has its copy on it: a wrong correspondence misses by angstroms
    d = np.linalg.norm(q[0].astype(np.float64)[:, None] - moved[None], axis=-1)
    d[q[1][:, None] != e[1][None, :]] = np.inf
    print(f"{name}: max |R y + s - x| = {d.min(axis=1).max():.2e} A")
    assert d.min(axis=1).max() <= 1e-3


# 3. proper rotations only
def test_mirror_image_is_another_pharmacophore():
    r64, _ = reference("mirror")
    got = device_result("mirror")
    assert_matches(got, r64, "mirror")
    assert got["sim"][0, 0] < 0.8 and r64["sim"][0, 0] < 0.8          # an improper rotation would give 1


# 4. order and batch
def test_permuted_entry():
    queries, library = cases()["library"]
    r64, _ = reference("library")
    rng = np.random.default_rng(3)
    pick = [b for b in range(len(library)) if len(library[b][1]) >= 4][:16]
    perm = []
    for b in pick:
        p = rng.permutation(len(library[b][1]))
        perm.append((library[b][0][p], library[b][1][p]))
    got = run(engine(), queries, perm)
    sub = {k: r64[k][:, pick] for k in ("sim", "n_matched", "n_seeds")}
    assert_matches(got, sub, "permuted entries")


@pytest.mark.parametrize("L", [1, 63, 64, 65])
@pytest.mark.parametrize("Q", [1, 3])
def test_sub_library_same_bytes(Q, L):
    queries, library = cases()["library"]
    whole = device_result("library")
    q0 = 2 if Q == 1 else 0                        # Q = 1: the last query alone
    l0 = len(library) - L if Q == 1 else 0         # ... against the library's tail
    got = run(engine(), queries[q0:q0 + Q], library[l0:l0 + L])
    for k in OUT:
        assert got[k].tobytes() == np.ascontiguousarray(whole[k][q0:q0 + Q, l0:l0 + L]).tobytes(), k


def test_two_calls_same_bytes():
    for name in ("library", "one_type"):
        again = run(engine(), *cases()[name])
        for k in OUT:
            assert again[k].tobytes() == device_result(name)[k].tobytes(), (name, k)


def test_without_the_transform():
    got = run(engine(), *cases()["library"], want_transform=False)
    assert got["transform"] is None
    for k in OUT[:3]:
        assert got[k].tobytes() == device_result("library")[k].tobytes(), k


def test_options_reach_the_kernel():
    """refine = 0 stops at the best seed; a wide tolerance admits more seeds: both as the reference has them"""
    queries, library = cases()["library"]
    library = library[:24]
    for kw in (dict(refine=0), dict(sigma=1.5, tolerance=2.0, refine=16, min_area=2.0)):
        r64 = R.align_all(queries, library, np.float64, want_margin=True, **kw)
        got = run(engine(), queries, library, **kw)
        far = r64["margin"] >= R.MARGIN
        assert far, "an input of this test sits on a bound"
        assert_matches(got, r64, str(kw))


# 5. the contract
def test_host_checks_refuse_before_any_launch():
    eng = engine()
    one = (np.zeros((1, 3), np.float32), np.zeros(1, np.int64))
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*query 1 has 17 centers \(1 to 16 per query\)"):
        run(eng, [one, (np.zeros((17, 3), np.float32), np.zeros(17, np.int64))], [one])
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*entry 0 has 33 centers \(1 to 32 per entry\)"):
        run(eng, [one], [(np.zeros((33, 3), np.float32), np.zeros(33, np.int64))])
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*16781312 pairs \(at most 16777216 per call"):
        run(eng, [one] * 4097, [one] * 4096)
    for kw, what in ((dict(sigma=0.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(tolerance=-1.0), "tolerance"),
                     (dict(refine=17), "refine"), (dict(refine=-1), "refine"), (dict(min_area=0.0), "min_area"),
                     (dict(min_area=float("inf")), "min_area")):
        with pytest.raises(pfa.PfError, match=ERR_ARG + r".*" + what):
            run(eng, [one], [one], **kw)
    # the pointer arrays and null pointers, at the C entry itself
    import ctypes
    L = pfa._lib
    x = torch.zeros(8, 3, device="cuda:0")
    t = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    o = torch.zeros(4, 12, device="cuda:0")
    oi = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    opts = L.PfAlignOpts(1.0, 1.5, 4, 1.0)

    def call(qp, lp, qx=x, sim=o, Q=None, Lc=None, popts=opts):
        qp, lp = (None if p is None else np.asarray(p, dtype=np.int32) for p in (qp, lp))
        rc = eng.lib.pf_pharm_align(eng._h, (len(qp) - 1) if Q is None else Q, None if qp is None else qp.ctypes.data,
                                    (len(lp) - 1) if Lc is None else Lc, None if lp is None else lp.ctypes.data,
                                    None if qx is None else qx.data_ptr(), t.data_ptr(), x.data_ptr(), t.data_ptr(),
                                    None if popts is None else ctypes.byref(popts), None if sim is None else sim.data_ptr(),
                                    oi.data_ptr(), oi.data_ptr(), None, None)
        return rc, eng.lib.pf_last_error(eng._h).decode()

    for args, what in ((dict(qp=[1, 3], lp=[0, 2]), "q_ptr[0] must be 0"), (dict(qp=[0, 3], lp=[2, 4]), "l_ptr[0] must be 0"),
                       (dict(qp=[0, 3, 2], lp=[0, 2]), "q_ptr decreases at query 1"), (dict(qp=[0, 3], lp=[0, 4, 3]), "l_ptr decreases at entry 1"),
                       (dict(qp=[0, 3, 3], lp=[0, 2]), "query 1 has 0 centers"), (dict(qp=[0, 3], lp=[0, 0]), "entry 0 has 0 centers"),
                       (dict(qp=None, lp=[0, 2], Q=1), "null pointer array or options"), (dict(qp=[0, 3], lp=None, Lc=1), "null pointer array or options"),
                       (dict(qp=[0, 3], lp=[0, 2], popts=None), "null pointer array or options"),
                       (dict(qp=[0, 3], lp=[0, 2], Q=0), "0 queries"), (dict(qp=[0, 3], lp=[0, 2], Lc=0), "0 library entries"),
                       (dict(qp=[0, 3], lp=[0, 2], qx=None), "null device array"), (dict(qp=[0, 3], lp=[0, 2], sim=None), "null device array")):
        rc, msg = call(**args)
        assert rc == -1 and "pf_pharm_align" in msg and what in msg, (args, rc, msg)
    rc, _ = call([0, 3], [0, 2])
    assert rc == 0
    run(eng, *cases()["mirror"])                  # and the handle goes on


def test_type_out_of_range_reported():
    eng = engine()
    q = [(np.zeros((2, 3), np.float32), np.array([0, 6]))]
    e = [(np.ones((1, 3), np.float32), np.array([-1])), (np.ones((3, 3), np.float32), np.array([1, 2, 3]))]
    with pytest.raises(pfa.PfError, match=ERR_ARG + r".*2 centers have a type outside \[0, 6\)"):
        run(eng, q, e)
    out = run(engine(11), q, e[1:])               # in range at pharm_nf 11
    assert out["n_seeds"][0, 0] == 0
    got = run(eng, *cases()["mirror"])            # and the handle goes on
    assert got["sim"].tobytes() == device_result("mirror")["sim"].tobytes()


def test_sampling_run_unchanged_by_a_call():
    """a call with a batch bound, and one between the steps of a sampling run, leave the run's outputs bitwise what they are"""
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    batch = O.synthetic_batch([0, 1], 64, [4, 3], cfg)
    T = 20
    noise = torch.randn(4, int(batch.pharm_ptr[-1]), 3 + cfg.pharm_nf, generator=torch.Generator().manual_seed(7))
    coef = O.step_coefficients(O.gamma_table(T, 1e-5), T)
    eng = pfa.PfEngine(device="cuda:0")
    eng.load_state_dict(sd)
    bind = lambda: eng.set_batch(batch.prot_x, batch.prot_h, batch.prot_ptr, batch.pharm_ptr, batch.pp_src, batch.pp_dst)
    arr = eng.coef_array(coef, reversed(range(T)))

    def sample(call_inside):
        bind()
        got = None
        if call_inside:
            got = run(eng, *cases()["one_type"])                       # a batch is bound
        eng.sample_begin(noise[0])
        for k in range(3):
            eng.denoise_step(arr[k], noise[k + 1])
            if call_inside and k == 0:
                inside = run(eng, *cases()["one_type"])                # inside the run
                for name in OUT:
                    assert inside[name].tobytes() == got[name].tobytes(), name
        x, h = eng.sample_end()
        return x.cpu(), h.cpu(), got

    x_a, h_a, _ = sample(False)
    x_b, h_b, got = sample(True)
    assert torch.equal(x_a, x_b) and torch.equal(h_a, h_b)
    for name in OUT:
        assert got[name].tobytes() == device_result("one_type")[name].tobytes(), name


# 6. the surface
def planted_library(seed=23):
    """a query of 6 centers; a library of 40 random entries (3 to 8 centers, six types) with rigid copies of the query, jittered by
    0.2 A, at places 5, 17 and 31"""
    rng = np.random.default_rng(seed)
    (query,), entries = R.random_case(rng, [6], [3 + b % 6 for b in range(40)], 6)
    for b in (5, 17, 31):
        entries[b] = R.rigid_copy(rng, query[0], query[1], jitter=0.2)
    return query, entries, (5, 17, 31)


def as_torch(ph):
    return torch.from_numpy(np.asarray(ph[0])), torch.from_numpy(np.asarray(ph[1]))


def test_model_screen_device_equals_host():
    from test_gpu_api import make_model
    query, entries, copies = planted_library()
    r64 = R.align_all([query], entries)
    others = [b for b in range(len(entries)) if b not in copies]
    assert r64["sim"][0, list(copies)].min() > r64["sim"][0, others].max()         # on the reference first
    m = make_model(12)
    lib = pfa.PharmacophoreLibrary([as_torch(e) for e in entries], names=[f"lig{b}" for b in range(len(entries))])
    queries = [as_torch(query), as_torch(entries[0])]
    host = m.screen(queries, lib, top_k=8, device="cpu")
    dev = m.screen(queries, lib.to("cuda"), top_k=8)
    small = pfa.screen_library(queries, lib, m.dynamics.engine(), top_k=8, max_pairs=7)          # many small calls
    for hs, ds, ss in zip(host, dev, small):
        assert [h.entry for h in ds] == [h.entry for h in hs] == [h.entry for h in ss] and len(ds) == 8
        assert [h.n_matched for h in ds] == [h.n_matched for h in hs] and [h.name for h in ds] == [h.name for h in hs]
        assert max(abs(a.sim - b.sim) for a, b in zip(ds, hs)) <= 2 * R.SIM_BOUND
        assert all(a.sim == b.sim and torch.equal(a.transform, b.transform) for a, b in zip(ds, ss))
    assert sorted(h.entry for h in dev[0][:3]) == list(copies) and dev[0][0].name.startswith("lig")
    assert dev[1][0].entry == 0 and dev[1][0].sim >= 1 - 1e-5
    moved, types = dev[0][0].aligned()
    d = torch.cdist(as_torch(query)[0].double(), moved.double())
    d[as_torch(query)[1][:, None] != types[None, :]] = float("inf")
    assert float(d.min(dim=1).values.max()) < 1.0                                  # the jittered copy lies on the query
    strict = m.screen(queries[:1], lib, top_k=50, min_match=1.0)
    assert sorted(h.entry for h in strict[0]) == list(copies)


def test_library_from_dataset(tmp_path):
    from test_io_dataset import CUTOFFS, PROT_ELEMENTS, make_split, oracle_pp
    from pharmacoforge_amd import dataset as D
    root = tmp_path / "processed"
    _, nf_a, _ = make_split(root / "split_0", 0, 3)
    _, nf_b, _ = make_split(root / "split_1", 1, 2)
    ds = D.ProteinPharmacophoreDataset('train', [0, 1], raw_data_dir=str(tmp_path), processed_data_dir=str(root), graph_cutoffs=CUTOFFS,
                                       prot_elements=PROT_ELEMENTS, ph_type_map=pfa.analysis.ph_idx_to_type, pp_edges_fn=oracle_pp)
    lib = pfa.PharmacophoreLibrary.from_dataset(ds)
    sizes = np.concatenate([nf_a, nf_b]).tolist()
    assert len(lib) == 5 and lib.dropped == 0 and [len(t) for _, t in lib.entries] == sizes
    assert lib.names == ds.prot_file_names and lib.index == list(range(5))
    # screened against its own entries on the device: the host path's hit lists
    host = pfa.screen_library([lib[k] for k in range(5)], lib, None, top_k=3)
    dev = pfa.screen_library([lib[k] for k in range(5)], lib.to("cuda"), engine(), top_k=3)
    for hs, ds in zip(host, dev):
        assert [h.entry for h in ds] == [h.entry for h in hs] and [h.n_matched for h in ds] == [h.n_matched for h in hs]
    assert any(ds[0].sim >= 1 - 1e-5 and ds[0].entry == k for k, ds in enumerate(dev))
