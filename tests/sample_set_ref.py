"""CPU yardstick of the sample-set analysis (pf_sample_set_analyze, analysis.py's sample_set_* functions): the four definitions of
include/pfdyn.h, "sample sets", in numpy at a chosen precision, written on flat center arrays and independently of analysis.py,
and the builders of the test inputs.

A set here is (x [N, 3] float32, t [N] int, cptr [S + 1]): the centers of its S samples one after the other."""
import numpy as np

SIGMA, TOLERANCE, THRESHOLD = 1.0, 1.5, 0.5


def flat(samples):
    """[(x, t)] -> (x [N, 3] float32, t [N] int64, cptr [S + 1])"""
    x = np.concatenate([np.asarray(s[0], dtype=np.float32).reshape(-1, 3) for s in samples])
    t = np.concatenate([np.asarray(s[1], dtype=np.int64).reshape(-1) for s in samples])
    return x, t, np.concatenate([[0], np.cumsum([len(np.asarray(s[1]).reshape(-1)) for s in samples])]).astype(np.int64)


def unflat(x, t, cptr):
    return [(x[cptr[a]:cptr[a + 1]], t[cptr[a]:cptr[a + 1]]) for a in range(len(cptr) - 1)]


def _d2(x, dtype):
    x = x.astype(dtype)
    d = x[:, None, :] - x[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def overlap(x, t, cptr, sigma=SIGMA, dtype=np.float64):
    """O [S, S]: every operation in `dtype`"""
    g = np.exp(-(_d2(x, dtype) / dtype(2.0 * float(sigma) ** 2)))
    g = np.where(t[:, None] == t[None, :], g, dtype(0)).astype(dtype)
    rows = np.add.reduceat(g, cptr[:-1], axis=0)
    return np.add.reduceat(rows, cptr[:-1], axis=1).astype(dtype)


def similarity(x, t, cptr, sigma=SIGMA, dtype=np.float64):
    """sim [S, S] in `dtype`: each unordered pair from the upper triangle of O, the diagonal 1"""
    O = overlap(x, t, cptr, sigma, dtype)
    O = np.triu(O) + np.triu(O, 1).T
    s = np.diagonal(O)
    sim = (O / ((s[:, None] + s[None, :]) - O)).astype(dtype)
    np.fill_diagonal(sim, dtype(1))
    return sim


def support(x, t, cptr, tolerance=TOLERANCE):
    """support [N] int64, distances in fp64"""
    hit = (t[:, None] == t[None, :]) & (np.sqrt(_d2(x, np.float64)) <= float(tolerance))
    per = np.logical_or.reduceat(hit, cptr[:-1], axis=1)                # [N, S]
    own = np.repeat(np.arange(len(cptr) - 1), np.diff(cptr))
    per[np.arange(len(t)), own] = False
    return per.sum(axis=1).astype(np.int64)


def butina(sim, threshold=THRESHOLD):
    """(labels [S], centroids, sizes, counts [S]) of Taylor-Butina without re-counting; the comparison is made in sim's dtype"""
    sim = np.asarray(sim)
    S = sim.shape[0]
    thr = sim.dtype.type(threshold)
    counts = [sum(1 for b in range(S) if b != a and sim[a, b] >= thr) for a in range(S)] if S <= 64 else \
        list(((sim >= thr).sum(axis=1) - (np.diagonal(sim) >= thr)).astype(int))
    labels, centroids, sizes = [-1] * S, [], []
    for a in sorted(range(S), key=lambda a: (-counts[a], a)):
        if labels[a] >= 0:
            continue
        c = len(centroids)
        members = [b for b in range(S) if labels[b] < 0 and (b == a or sim[a, b] >= thr)]
        for b in members:
            labels[b] = c
        centroids.append(a)
        sizes.append(len(members))
    return np.asarray(labels), centroids, sizes, np.asarray(counts)


def consensus(x, t, cptr, labels, centroids, tolerance=TOLERANCE, dtype=np.float64, gaps=None):
    """(cons_x [N, 3] `dtype`, cons_cnt [N]): filled for the centers of centroid samples, zero elsewhere.  Distances in fp64 decide;
    the sum runs over the members ascending in `dtype`.  gaps: a list that receives (second nearest - nearest distance, member's
    second-nearest center index) of every choice that had a second candidate of the type (inside the tolerance or not)."""
    N = len(t)
    cx, cc = np.zeros((N, 3), dtype=dtype), np.zeros(N, dtype=np.int64)
    xd = x.astype(np.float64)
    for c, m in enumerate(centroids):
        for i in range(cptr[m], cptr[m + 1]):
            acc = np.zeros(3, dtype=dtype)
            for b in np.nonzero(np.asarray(labels) == c)[0]:
                js = np.arange(cptr[b], cptr[b + 1])
                js = js[t[js] == t[i]]
                if len(js) == 0:
                    continue
                dist = np.sqrt(((xd[js] - xd[i]) ** 2).sum(axis=1))
                k = np.argsort(dist, kind="stable")
                if gaps is not None and len(js) > 1 and dist[k[0]] <= float(tolerance):
                    gaps.append((float(dist[k[1]] - dist[k[0]]), int(js[k[1]])))
                if dist[k[0]] <= float(tolerance):
                    acc = (acc + x[js[k[0]]].astype(dtype)).astype(dtype)
                    cc[i] += 1
            cx[i] = acc / dtype(cc[i])
    return cx, cc


def analyze(x, t, cptr, sigma=SIGMA, tolerance=TOLERANCE, threshold=THRESHOLD, dtype=np.float64):
    """all of it at one precision: dict(sim, support, labels, centroids, sizes, counts, cons_x, cons_cnt)"""
    sim = similarity(x, t, cptr, sigma, dtype)
    labels, centroids, sizes, counts = butina(sim, threshold)
    cx, cc = consensus(x, t, cptr, labels, centroids, tolerance, dtype)
    return dict(sim=sim, support=support(x, t, cptr, tolerance), labels=labels, centroids=centroids, sizes=sizes, counts=counts,
                cons_x=cx, cons_cnt=cc)


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def planted(group_sizes=(5, 4, 3), group_centers=(5, 4, 7), nf=6, seed=0, jitter=0.2, interleave=True):
    """G motif groups: fixed center positions at least 4 A apart (over all motifs) and fixed types; every sample of a group is its
    motif plus uniform jitter in +-`jitter` A.  Returns (samples [(x, t)], group [S]): with sigma 1, tolerance 1.5, threshold 0.5
    same-motif-center distances are <= 0.7 A and all others > 3 A, so same-group similarities are >= 0.65 and cross-group ones
    about 0 (both asserted)."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < sum(group_centers):
        p = rng.uniform(-12.0, 12.0, 3)
        if all(np.linalg.norm(p - q) >= 4.0 for q in pts):
            pts.append(p)
    pts, motifs, at = np.asarray(pts), [], 0
    for n in group_centers:
        motifs.append((pts[at:at + n], rng.integers(0, nf, n)))
        at += n
    group = np.repeat(np.arange(len(group_sizes)), group_sizes)
    if interleave:
        group = group[rng.permutation(len(group))]
    samples = [((motifs[g][0] + rng.uniform(-jitter, jitter, motifs[g][0].shape)).astype(np.float32), motifs[g][1].copy()) for g in group]
    x, t, cptr = flat(samples)
    dist = np.sqrt(_d2(x, np.float64))
    motif_of = np.concatenate([np.arange(len(s[1])) + 1000 * g for s, g in zip(samples, group)])
    same = motif_of[:, None] == motif_of[None, :]
    assert dist[same].max() <= 0.7 and dist[~same].min() > 3.0
    sim = similarity(x, t, cptr)
    same_group = group[:, None] == group[None, :]
    assert sim[same_group].min() >= 0.65 and (sim[~same_group].max() if (~same_group).any() else 0.0) < 1e-3
    return samples, group


def random_sets(set_sizes=(1, 2, 17, 33), center_counts=(1, 2, 6, 63, 64), nf=6, seed=0, box=6.0, tolerance=TOLERANCE,
                threshold=THRESHOLD, sigma=SIGMA, margin=1e-3):
    """One list of samples per set: centers uniform in a `box` A cube with random types, center counts drawn from
    `center_counts`.  Centers are drawn again (the offending ones, from the same generator) until, in fp64 and within each set,
    no distance between centers of one type in two samples is within `margin` of the tolerance, no similarity is within 1e-4 of
    the threshold, and no nearest / second-nearest gap used by a consensus is under `margin`.  All three are asserted on what is
    returned."""
    rng = np.random.default_rng(seed)
    sets = []
    for S in set_sizes:
        samples = []
        for _ in range(S):
            n = int(rng.choice(center_counts))
            samples.append((rng.uniform(0.0, box, (n, 3)).astype(np.float32), rng.integers(0, nf, n)))
        x, t, cptr = flat(samples)
        for _ in range(200):
            bad = _violations(x, t, cptr, sigma, tolerance, threshold, margin)
            if bad is None:
                raise AssertionError("a similarity sits on the threshold: choose another seed")
            if len(bad) == 0:
                break
            x[bad] = rng.uniform(0.0, box, (len(bad), 3)).astype(np.float32)
        assert len(_violations(x, t, cptr, sigma, tolerance, threshold, margin)) == 0
        sets.append(unflat(x, t, cptr))
    return sets


def near_tolerance(x, t, cptr, tolerance, margin):
    """the later center of every pair of one type in two samples whose fp64 distance is within `margin` of the tolerance"""
    own = np.repeat(np.arange(len(cptr) - 1), np.diff(cptr))
    dist = np.sqrt(_d2(x, np.float64))
    i, j = np.nonzero((np.abs(dist - tolerance) < margin) & (t[:, None] == t[None, :]) & (own[:, None] != own[None, :]))
    return sorted(set(i[i > j].tolist()))


def clear_of_tolerance(samples, rng, lo, hi, tolerance=TOLERANCE, margin=1e-3):
    """the samples with the offending centers drawn again, uniform in [lo, hi)^3, until near_tolerance finds none (asserted):
    for inputs too large for random_sets' other two conditions, which tests then assert on what they use"""
    x, t, cptr = flat(samples)
    for _ in range(200):
        bad = near_tolerance(x, t, cptr, tolerance, margin)
        if not bad:
            break
        x[bad] = rng.uniform(lo, hi, (len(bad), 3)).astype(np.float32)
    assert not near_tolerance(x, t, cptr, tolerance, margin)
    return unflat(x, t, cptr)


def _violations(x, t, cptr, sigma, tolerance, threshold, margin):
    """indices of centers to draw again (one per violated condition); None: a similarity within 1e-4 of the threshold"""
    bad = set(near_tolerance(x, t, cptr, tolerance, margin))
    sim = similarity(x, t, cptr, sigma)
    off = ~np.eye(len(cptr) - 1, dtype=bool)
    if off.any() and np.abs(sim[off] - threshold).min() < 1e-4:
        return None
    labels, centroids, _, _ = butina(sim, threshold)
    gaps = []
    consensus(x, t, cptr, labels, centroids, tolerance, np.float64, gaps)
    bad |= {j for gap, j in gaps if gap < margin}
    return sorted(bad)


def pack_sets(sets):
    """sets (lists of samples) -> (x [N, 3], t [N], set_ptr [P + 1], center_ptr [S + 1]) of one call"""
    samples = [s for st in sets for s in st]
    x, t, cptr = flat(samples)
    return x, t, np.concatenate([[0], np.cumsum([len(st) for st in sets])]).astype(np.int32), cptr.astype(np.int32)
