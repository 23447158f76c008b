"""Test infrastructure of the pharmacophore alignment (include/pfdyn.h "pharmacophore alignment"), written independently
of the package's analysis.py: the definition in numpy at a chosen dtype -- seeds by brute-force masks, every rotation by SVD Kabsch
with the determinant correction -- and the input builders of the alignment tests.

The bound on sim.  The fp32 and the fp64 run of this reference over every input of tests/test_gpu_align.py (`measure()` below,
398 pairs, 3.6e4 seeds) differ by at most SIM_FP32_FP64_MAX in sim, with no pair above 1e-4 and no integer differing; the device is
held to SIM_BOUND = 8 x that maximum against the fp64 run: the margin covers its different rotation solver, expf and summation order.
"""
import numpy as np

SIM_FP32_FP64_MAX = 1.62e-7       # measured by measure() on the inputs of gpu_cases(); see the module docstring
SIM_BOUND = 8 * SIM_FP32_FP64_MAX
MARGIN = 1e-3                     # no seed filter and no matched distance of a built input is closer than this to its bound (fp64)
MAX_SEEDS_PER_TEST = 200_000
LANES = 64                        # lanes that share a pair on the device (one wave)

DEFAULTS = dict(sigma=1.0, tolerance=1.5, refine=4, min_area=1.0)


def _opts(kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def _kabsch(Y, X, W, dtype):
    """Batched weighted Kabsch: Y, X [n, m, 3] corresponding points, W [n, m] weights -> R [n, 3, 3], s [n, 3] with X ~ R Y + s,
    R proper (the determinant correction on the smallest singular direction)."""
    Wn = W / W.sum(axis=1, keepdims=True)
    yc = (Wn[..., None] * Y).sum(axis=1)
    xc = (Wn[..., None] * X).sum(axis=1)
    Yc, Xc = Y - yc[:, None, :], X - xc[:, None, :]
    H = np.einsum("nm,nma,nmb->nab", W, Yc, Xc).astype(dtype)          # sum w y x^T
    U, _, Vt = np.linalg.svd(H)
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, 1, 2))).astype(dtype)
    d[d == 0] = 1
    D = np.zeros((H.shape[0], 3, 3), dtype=dtype)
    D[:, 0, 0] = 1
    D[:, 1, 1] = 1
    D[:, 2, 2] = d
    R = (V @ D @ np.swapaxes(U, 1, 2)).astype(dtype)
    s = xc - np.einsum("nab,nb->na", R, yc)
    return R, s.astype(dtype)


def _overlap(x, same, y, R, s, inv_2s2):
    """O [n] for transforms R [n,3,3], s [n,3]; also the squared distances [n, nq, nl]"""
    ry = np.einsum("nab,lb->nla", R, y) + s[:, None, :]
    d = x[None, :, None, :] - ry[:, None, :, :]
    d2 = (d * d).sum(axis=-1)
    return (np.exp(-d2 * inv_2s2) * same[None]).sum(axis=(1, 2)), d2


def self_overlap(x, t, sigma, dtype):
    x = np.asarray(x, dtype=dtype)
    d = x[:, None, :] - x[None, :, :]
    return ((np.exp(-(d * d).sum(-1) * dtype(1.0 / (2.0 * sigma * sigma)))) * (t[:, None] == t[None, :])).sum()


def seeds_of(x, t, y, u, tolerance, min_area, want_margin=False):
    """The seeds of a pair in enumeration order: (qi [n, 3], li [n, 3]) index arrays; with want_margin also the smallest distance
    of any filter value from its bound (distance differences of type-compatible candidates, the areas of all triplets)."""
    nq, nl = len(t), len(u)
    margin = np.inf
    dq = np.linalg.norm(x[:, None] - x[None], axis=-1)
    dl = np.linalg.norm(y[:, None] - y[None], axis=-1)
    a, b, c = np.meshgrid(np.arange(nl), np.arange(nl), np.arange(nl), indexing="ij")
    distinct = (a != b) & (a != c) & (b != c)
    area_l = np.linalg.norm(np.cross(y[b] - y[a], y[c] - y[a]), axis=-1) if nl else np.zeros((0, 0, 0))
    if want_margin and distinct.any():
        margin = min(margin, np.abs(area_l[distinct] - min_area).min())
    qi, li = [], []
    for i in range(nq):
        for j in range(i + 1, nq):
            for k in range(j + 1, nq):
                area_q = np.linalg.norm(np.cross(x[j] - x[i], x[k] - x[i]))
                if want_margin:
                    margin = min(margin, abs(area_q - min_area))
                ty = distinct & (u[a] == t[i]) & (u[b] == t[j]) & (u[c] == t[k])
                if not ty.any():
                    continue
                diffs = [np.abs(dq[i, j] - dl[a, b]), np.abs(dq[i, k] - dl[a, c]), np.abs(dq[j, k] - dl[b, c])]
                if want_margin:
                    margin = min(margin, min(np.abs(df[ty] - 2 * tolerance).min() for df in diffs))
                if area_q < min_area:
                    continue
                ok = ty & (diffs[0] <= 2 * tolerance) & (diffs[1] <= 2 * tolerance) & (diffs[2] <= 2 * tolerance) & (area_l >= min_area)
                hit = np.argwhere(ok)                      # row-major: (a, b, c) ascending
                if len(hit):
                    li.append(hit)
                    qi.append(np.tile(np.array([i, j, k]), (len(hit), 1)))
    if not qi:
        return (np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3), dtype=np.int64)), margin
    return (np.concatenate(qi), np.concatenate(li)), margin


def align_pair(x, t, y, u, dtype=np.float64, want_margin=False, **kw):
    """One pair by the definition.  Returns a dict: sim, n_matched, n_seeds, transform [12] (R row-major, s), and with want_margin
    `margin`: the smallest distance of a seed filter or a matched distance from its bound."""
    o = _opts(kw)
    dtype = np.dtype(dtype).type
    t, u = np.asarray(t, dtype=np.int64), np.asarray(u, dtype=np.int64)
    x64, y64 = np.asarray(x, dtype=np.float64).reshape(-1, 3), np.asarray(y, dtype=np.float64).reshape(-1, 3)
    x, y = x64.astype(dtype), y64.astype(dtype)
    # the filters are evaluated at the dtype too; the inputs the tests build keep every filter MARGIN away from its bound
    (qi, li), margin = seeds_of(x, t, y, u, dtype(o["tolerance"]), dtype(o["min_area"]), want_margin)
    n = len(qi)
    out = dict(sim=0.0, n_matched=0, n_seeds=n, transform=np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=dtype), margin=margin)
    if n == 0:
        return out
    inv = dtype(1.0 / (2.0 * o["sigma"] ** 2))
    same = (t[:, None] == u[None, :])
    best_o, best = -1.0, None
    for c0 in range(0, n, 4096):
        q_, l_ = qi[c0:c0 + 4096], li[c0:c0 + 4096]
        R, s = _kabsch(y[l_], x[q_], np.ones(q_.shape, dtype=dtype), dtype)
        O, _ = _overlap(x, same, y, R, s, inv)
        m = int(np.argmax(O))                              # the first of equals
        if O[m] > best_o:
            best_o, best = O[m], (R[m], s[m])
    R, s = best
    O = best_o
    for _ in range(int(o["refine"])):
        _, d2 = _overlap(x, same, y, R[None], s[None], inv)
        w = (np.exp(-d2[0] * inv) * same).astype(dtype)    # [nq, nl]
        p_, q_ = np.nonzero(same)
        R2, s2 = _kabsch(y[q_][None], x[p_][None], w[p_, q_][None], dtype)
        O2, _ = _overlap(x, same, y, R2, s2, inv)
        if not O2[0] >= O:
            break
        R, s, O = R2[0], s2[0], O2[0]
    oqq, oll = self_overlap(x, t, o["sigma"], dtype), self_overlap(y, u, o["sigma"], dtype)
    _, d2 = _overlap(x, same, y, R[None], s[None], inv)
    dist = np.sqrt(d2[0])
    out["sim"] = float(min(O / (oqq + oll - O), dtype(1.0)))
    out["n_matched"] = int(((dist <= dtype(o["tolerance"])) & same).any(axis=1).sum())
    out["transform"] = np.concatenate([R.reshape(-1), s]).astype(dtype)
    if want_margin and same.any():
        out["margin"] = min(margin, float(np.abs(dist[same] - o["tolerance"]).min()))
    return out


def align_all(queries, library, dtype=np.float64, want_margin=False, **kw):
    """Every pair: dict of sim [Q, L] float64, n_matched, n_seeds [Q, L] int64, transform [Q, L, 12], margin (the smallest)."""
    Q, L = len(queries), len(library)
    res = dict(sim=np.zeros((Q, L)), n_matched=np.zeros((Q, L), dtype=np.int64), n_seeds=np.zeros((Q, L), dtype=np.int64),
               transform=np.zeros((Q, L, 12)), margin=np.inf)
    for a, (x, t) in enumerate(queries):
        for b, (y, u) in enumerate(library):
            r = align_pair(x, t, y, u, dtype=dtype, want_margin=want_margin, **kw)
            res["sim"][a, b], res["n_matched"][a, b], res["n_seeds"][a, b], res["transform"][a, b] = r["sim"], r["n_matched"], r["n_seeds"], r["transform"]
            res["margin"] = min(res["margin"], r["margin"])
    return res


# ---- input builders -------------------------------------------------------------------------------------------------------------

def pack(phs):
    """[(x [n, 3], t [n])] -> (X [N, 3] float32, T [N] int32, ptr [len + 1] int32)"""
    X = np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1, 3) for x, _ in phs])
    T = np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for _, t in phs])
    ptr = np.concatenate([[0], np.cumsum([len(t) for _, t in phs])]).astype(np.int32)
    return X, T, ptr


def random_pharmacophore(rng, n, n_types, box=8.0):
    """n centers uniform in the box, rounded to fp32 (what the device reads is what the reference reads)"""
    return rng.uniform(0.0, box, size=(n, 3)).astype(np.float32), rng.integers(0, n_types, size=n).astype(np.int64)


def random_case(rng, nq, nl, n_types, **kw):
    """Queries of nq[k] centers and entries of nl[k] centers.  An entry (or, when a query triplet's area offends, a query) is drawn
    again until every pair keeps MARGIN from every bound in fp64 -- asserted on what is returned by checked()."""
    queries = [random_pharmacophore(rng, n, n_types) for n in nq]
    for a in range(len(queries)):
        while seeds_of(queries[a][0].astype(np.float64), queries[a][1], np.zeros((0, 3)), np.zeros(0, dtype=np.int64), 1.5, _opts(kw)["min_area"], True)[1] < MARGIN:
            queries[a] = random_pharmacophore(rng, len(queries[a][1]), n_types)
    library = []
    for n in nl:
        while True:
            e = random_pharmacophore(rng, n, n_types)
            if all(align_pair(x, t, e[0], e[1], want_margin=True, **kw)["margin"] >= MARGIN for x, t in queries):
                break
        library.append(e)
    return queries, library


def random_rotation(rng):
    """a proper rotation, uniform"""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rigid_copy(rng, x, t, shift=30.0, jitter=0.0, permute=True):
    """(y, u) with x ~ R y + s: the pharmacophore under the inverse of a random proper rotation and a translation of up to `shift`
    per axis, its centers permuted, optionally jittered; y is rounded to fp32"""
    R, s = random_rotation(rng), rng.uniform(-shift, shift, size=3)
    y = (np.asarray(x, dtype=np.float64) - s) @ R                          # R^T (x - s)
    if jitter:
        y = y + rng.normal(scale=jitter / np.sqrt(3.0), size=y.shape)
    perm = rng.permutation(len(t)) if permute else np.arange(len(t))
    return y[perm].astype(np.float32), np.asarray(t)[perm]


def mirror(x, t):
    y = np.array(x, dtype=np.float32)
    y[:, 0] = -y[:, 0]
    return y, np.asarray(t)


def checked(queries, library, **kw):
    """The fp64 and the fp32 reference of a test's inputs, with what every test input must satisfy asserted: the margins, the seed
    budget, and no pair whose fp32 and fp64 reference differ by more than SIM_BOUND or in an integer."""
    r64 = align_all(queries, library, np.float64, want_margin=True, **kw)
    r32 = align_all(queries, library, np.float32, **kw)
    assert r64["margin"] >= MARGIN, f"an input is {r64['margin']:.2e} from a bound"
    assert r64["n_seeds"].sum() <= MAX_SEEDS_PER_TEST, int(r64["n_seeds"].sum())
    assert np.array_equal(r64["n_seeds"], r32["n_seeds"]) and np.array_equal(r64["n_matched"], r32["n_matched"])
    assert np.abs(r64["sim"] - r32["sim"]).max() <= SIM_BOUND, np.abs(r64["sim"] - r32["sim"]).max()
    return r64, r32


# ---- the inputs of tests/test_gpu_align.py (built once per process; the host tests use some of them too) -------------------------

def collinear_entry(t):
    """three centers on a line, types t: type-compatible with a query triplet of those types, and every seed fails the area test"""
    return np.array([[1.0, 1.0, 1.0], [2.5, 1.5, 1.0], [4.0, 2.0, 1.0]], dtype=np.float32), np.asarray(t, dtype=np.int64)


def library_case(seed=5):
    """Q = 3 queries of 3, 5 and 6 centers (six types, two types, two types) against L = 130 entries of 1 to 8 centers, six and two
    types alternating; entry 7 is collinear with the types of query 0's centers"""
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 3, 4, 5, 6, 8, 7]
    q, _ = random_case(np.random.default_rng(seed), [3], [], 6)
    q2, _ = random_case(np.random.default_rng(seed + 1), [5, 6], [], 2)
    queries = q + q2
    library = []
    for b in range(130):
        n, nt = sizes[b % 8], (6 if (b // 8) % 2 == 0 else 2)
        while True:
            e = collinear_entry(queries[0][1]) if b == 7 else random_pharmacophore(rng, n, nt)
            if all(align_pair(x, t, e[0], e[1], want_margin=True)["margin"] >= MARGIN for x, t in queries):
                break
        library.append(e)
    return queries, library


def build_caps_case(seed=9):
    """one query of 16 centers against entries of 32 and 4 centers, six types.  With ~8 x 10^4 type-compatible candidates most draws
    of the large entry have a filter value within MARGIN of its bound: some ten draws (as many seconds) until one has none"""
    return random_case(np.random.default_rng(seed), [16], [32, 4], 6)


def caps_case():
    """build_caps_case() as stored in tests/golden/align_caps.npz (written by `python align_ref.py golden`); checked() asserts the
    conditions on what is loaded like on any other input"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_caps.npz"))
    return [(z["qx"], z["qt"])], [(z["l0x"], z["l0t"]), (z["l1x"], z["l1t"])]


def one_type_case(seed=13):
    """8 x 8 centers, all of one type: every triple of the entry is type-compatible with every triplet of the query"""
    return random_case(np.random.default_rng(seed), [8], [8], 1)


def rigid_case(n, seed=17):
    """a query of n centers (six types) and its rigid copy far away, centers permuted"""
    rng = np.random.default_rng(seed + n)
    (q,), _ = random_case(rng, [n], [], 6)
    return [q], [rigid_copy(rng, q[0], q[1])]


def mirror_case():
    """a chiral query -- five centers of distinct types, not coplanar -- and its reflection"""
    x = np.array([[0.0, 0.0, 0.0], [3.0, 0.2, 0.1], [0.5, 2.8, -0.3], [1.1, 0.9, 2.6], [-1.7, 1.4, 1.2]], dtype=np.float32)
    t = np.arange(5, dtype=np.int64)
    return [(x, t)], [mirror(x, t)]


def gpu_cases():
    """name -> (queries, library) of every input tests/test_gpu_align.py compares against this reference"""
    cases = {"library": library_case(), "caps": caps_case(), "one_type": one_type_case(), "mirror": mirror_case()}
    for n in (3, 4, 6, 16):
        cases[f"rigid{n}"] = rigid_case(n)
    return cases


def measure():
    """max |sim fp32 - sim fp64| of this reference over gpu_cases(): the figure SIM_FP32_FP64_MAX records"""
    worst, pairs, seeds, ints = 0.0, 0, 0, 0
    for name, (qs, lib) in gpu_cases().items():
        r64, r32 = align_all(qs, lib, np.float64), align_all(qs, lib, np.float32)
        d = np.abs(r64["sim"] - r32["sim"])
        ints += int((r64["n_seeds"] != r32["n_seeds"]).sum() + (r64["n_matched"] != r32["n_matched"]).sum())
        pairs, seeds, worst = pairs + d.size, seeds + int(r64["n_seeds"].sum()), max(worst, float(d.max()))
        print(f"{name}: {d.size} pairs, {int(r64['n_seeds'].sum())} seeds, max |fp32 - fp64| = {d.max():.3e}, pairs above 1e-4: {int((d > 1e-4).sum())}")
    print(f"all: {pairs} pairs, {seeds} seeds, max {worst:.3e}, integers differing: {ints}")
    return worst


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["golden"]:
        import os
        (q,), (l0, l1) = build_caps_case()
        np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_caps.npz"), qx=q[0], qt=q[1], l0x=l0[0], l0t=l0[1],
                 l1x=l1[0], l1t=l1[1])
    measure()
