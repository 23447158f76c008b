"""Output objects and sample metrics of the path (pharmacoforge/analysis/pharm_builder.py:7-71,
pharmacoforge/analysis/metrics.py:9-86, pharmacoforge/utils/unorganized_utils.py:111-128).
Host code on small per-pharmacophore tensors; the only multi-GPU exchange on the sampling path is
the all-reduce of the validity numerator/denominator and the type counts (8 numbers)."""
from pathlib import Path
from typing import List, Optional

import torch

ph_idx_to_type = ['Aromatic', 'HydrogenDonor', 'HydrogenAcceptor', 'PositiveIon', 'NegativeIon', 'Hydrophobic']


_XYZ_ELEMENTS = ('P', 'S', 'F', 'N', 'O', 'C')      # file format of pharms.xyz: one pseudo-element per pharmacophore type


def _xyz_block(elements, coords) -> str:
    """One xyz frame: the center count, then `element x y z` with three decimals per center (the text
    pharm_builder.py:35-42 / unorganized_utils.py:111-128 emit; this is the file format)."""
    rows = torch.as_tensor(coords, dtype=torch.float64).reshape(-1, 3).tolist()
    if len(rows) != len(elements):
        raise ValueError(f"{len(elements)} element symbols for {len(rows)} positions")
    body = "".join(f"{e} {x:.3f} {y:.3f} {z:.3f}\n" for e, (x, y, z) in zip(elements, rows))
    return f"{len(rows)}\n" + body


def read_pinned_centers(filename):
    """One xyz frame in the pharms.xyz format (the center count, then `element x y z` per center, elements P S F N O C)
    -> (positions [k,3] fp32, type indices [k]): centers a user cut from an earlier output, to be pinned."""
    lines = [ln.strip() for ln in Path(filename).read_text().splitlines() if ln.strip()]
    if not lines:
        raise ValueError(f"{filename}: empty file")
    try:
        k = int(lines[0])
    except ValueError:
        raise ValueError(f"{filename}: the first line must be the center count, got {lines[0]!r}") from None
    if k < 1 or len(lines) != k + 1:
        raise ValueError(f"{filename}: one frame of {k} center lines expected, found {len(lines) - 1} lines")
    pos, types = [], []
    for ln in lines[1:]:
        tok = ln.split()
        if len(tok) != 4 or tok[0] not in _XYZ_ELEMENTS:
            raise ValueError(f"{filename}: bad center line {ln!r} (element x y z, elements {' '.join(_XYZ_ELEMENTS)})")
        try:
            pos.append([float(v) for v in tok[1:]])
        except ValueError:
            raise ValueError(f"{filename}: bad coordinates in {ln!r}") from None
        types.append(_XYZ_ELEMENTS.index(tok[0]))
    return torch.tensor(pos, dtype=torch.float32), torch.tensor(types, dtype=torch.int64)


def read_pharmacophores(filename):
    """Every frame of a file in the pharms.xyz format (consecutive frames: the center count, then `element x y z` per center;
    blank lines are ignored) -> [(positions [k,3] fp32, type indices [k])], in file order: pharmacophores to be scored.
    read_pinned_centers stays the one-frame reader."""
    lines = [ln.strip() for ln in Path(filename).read_text().splitlines() if ln.strip()]
    if not lines:
        raise ValueError(f"{filename}: empty file")
    frames, i = [], 0
    while i < len(lines):
        try:
            k = int(lines[i])
        except ValueError:
            raise ValueError(f"{filename}: frame {len(frames)} must start with its center count, got {lines[i]!r}") from None
        if k < 1 or i + 1 + k > len(lines):
            raise ValueError(f"{filename}: frame {len(frames)} announces {k} centers, {len(lines) - i - 1} lines follow")
        pos, types = [], []
        for ln in lines[i + 1:i + 1 + k]:
            tok = ln.split()
            if len(tok) != 4 or tok[0] not in _XYZ_ELEMENTS:
                raise ValueError(f"{filename}: bad center line {ln!r} (element x y z, elements {' '.join(_XYZ_ELEMENTS)})")
            try:
                pos.append([float(v) for v in tok[1:]])
            except ValueError:
                raise ValueError(f"{filename}: bad coordinates in {ln!r}") from None
            types.append(_XYZ_ELEMENTS.index(tok[0]))
        frames.append((torch.tensor(pos, dtype=torch.float32), torch.tensor(types, dtype=torch.int64)))
        i += 1 + k
    return frames


class PharmacophoreScore:
    """How plausible the trained model finds one pharmacophore for its pocket (PharmacophoreDiff.score, pf_score): the candidate
    is noised to L levels and the error of the network's prediction at each is a term of the model's variational bound.
    ``terms`` [L, 4]: per level the sums over the centers of the position term, the feature term, the squared error of the
    predicted clean centers and the number of centers whose predicted type is the given one.  ``pos`` / ``feat``: the weighted sums
    of the first two over the levels; ``total`` their sum; ``per_center`` = total / centers -- LOWER IS BETTER.  Totals compare
    candidates of one size only (there is no size prior in them): across sizes use per_center.  ``position_error`` and
    ``type_accuracy``: means over levels and centers."""
    __slots__ = ("n_centers", "levels", "pos", "feat", "total", "per_center", "position_error", "type_accuracy", "terms")

    def __init__(self, n_centers: int, levels, pos: float, feat: float, terms: torch.Tensor):
        self.n_centers, self.levels = int(n_centers), [int(t) for t in levels]
        self.pos, self.feat = float(pos), float(feat)
        self.total = self.pos + self.feat
        self.per_center = self.total / self.n_centers
        self.terms = terms
        denom = float(self.n_centers * max(len(self.levels), 1))
        self.position_error = float(terms[:, 2].double().sum()) / denom
        self.type_accuracy = float(terms[:, 3].double().sum()) / denom

    def __repr__(self):
        return (f"PharmacophoreScore(centers={self.n_centers}, levels={len(self.levels)}, total={self.total:.6g}, "
                f"per_center={self.per_center:.6g}, position_error={self.position_error:.6g}, type_accuracy={self.type_accuracy:.4f})")


def _emit(text: str, filename):
    """Return the text, or write it when a file name is given (the reference's writers do the same)."""
    if filename is None:
        return text
    Path(filename).write_text(text)
    return None


class SampledPharmacophore:
    """One generated pharmacophore: the final graph, its argmax feature types and, optionally, the frames of its
    reverse-diffusion trajectory.  Attribute and method names follow pharmacoforge/analysis/pharm_builder.py:7-71
    (callers and the metrics read them); the bodies are this repository's."""
    type_idx_to_elem = list(_XYZ_ELEMENTS)

    def __init__(self, g, pharm_type_map: List[str], traj_frames=None, ref_prot_file: Path = None, ref_rdkit_lig=None):
        if len(pharm_type_map) != len(_XYZ_ELEMENTS):
            raise AssertionError(f"a pharmacophore type map of {len(_XYZ_ELEMENTS)} entries is required, got {len(pharm_type_map)}")
        self.g = g                                       # single-graph PocketGraph with x_0 / h_0 of the centers
        self.pharm_type_map = list(pharm_type_map)
        self.ph_type_to_elem = dict(zip(self.pharm_type_map, _XYZ_ELEMENTS))
        self.ref_prot_file, self.ref_rdkit_lig = ref_prot_file, ref_rdkit_lig
        self.ph_coords = g.pharm_x0
        self.ph_feats_idxs = torch.argmax(g.pharm_h0, dim=1)
        self.ph_types = self._names(self.ph_feats_idxs)
        self.n_ph_centers = int(self.ph_coords.shape[0])
        # the 2-bit pin flag of every center (bit 0: its position was given, bit 1: its type); all zero for an unpinned sample
        pin = getattr(g, "pharm_pin", None)
        self.pinned = torch.zeros(self.n_ph_centers, dtype=torch.int32) if pin is None else pin.to("cpu", torch.int32)
        self.pos_frames, self.feat_frames = traj_frames if traj_frames is not None else (None, None)
        self.score: Optional[PharmacophoreScore] = None  # set by PharmacophoreDiff.sample(..., score_levels=K)
        # set by PharmacophoreDiff.sample(..., pair_restraints= / min_separation=): pair_restraint_energy of the final centers
        self.pair_energy: Optional[float] = None
        self.pair_violations: Optional[int] = None

    def _names(self, type_indices) -> List[str]:
        return [self.pharm_type_map[k] for k in torch.as_tensor(type_indices).tolist()]

    def pharm_to_xyz(self, pos: torch.Tensor, types: List[str]) -> str:
        return _xyz_block([self.ph_type_to_elem[t] for t in types], pos)

    def to_xyz_file(self, filename: str = None):
        return _emit(self.pharm_to_xyz(self.ph_coords, self.ph_types), filename)

    def as_written(self):
        """(positions [n,3] fp32, type indices [n]) as to_xyz_file writes them and read_pharmacophores reads them back: three
        decimals per coordinate, argmax types"""
        rows = torch.as_tensor(self.ph_coords, dtype=torch.float64).reshape(-1, 3).tolist()
        return (torch.tensor([[float(f"{v:.3f}") for v in r] for r in rows], dtype=torch.float32).reshape(-1, 3),
                self.ph_feats_idxs.to(torch.int64).clone())

    def traj_to_xyz(self, filename: str = None):
        if self.pos_frames is None or self.feat_frames is None:
            raise ValueError("this SampledPharmacophore holds no trajectory: sample with visualize_trajectory=True to record one")
        per_frame_types = torch.argmax(self.feat_frames, dim=2)
        frames = (self.pharm_to_xyz(x, self._names(k)) for x, k in zip(self.pos_frames, per_frame_types))
        return _emit("".join(frames), filename)


def write_pharmacophore_file(coords_list, atom_types_list, pharm_type_map: list, filename: str = None):
    """Several pharmacophores, given as coordinates and type INDICES, as consecutive xyz frames (unorganized_utils.py:111-128)."""
    frames = []
    for coords, type_indices in zip(coords_list, atom_types_list):
        frames.append(_xyz_block([_XYZ_ELEMENTS[int(k)] for k in type_indices], coords))
    return _emit("".join(frames), filename)


_MATCHING_TYPES = {'Aromatic': ['Aromatic', 'PositiveIon'], 'HydrogenDonor': ['HydrogenAcceptor'],
                   'HydrogenAcceptor': ['HydrogenDonor'], 'PositiveIon': ['NegativeIon', 'Aromatic'],
                   'NegativeIon': ['PositiveIon'], 'Hydrophobic': ['Hydrophobic']}
_MATCHING_DIST = {"Aromatic": 7, "Hydrophobic": 5, "HydrogenAcceptor": 4, "HydrogenDonor": 4, "NegativeIon": 5,
                  "PositiveIon": 5}


def complementarity_tables():
    """(match [6, 6] int32, dist [6] float32) in ph_idx_to_type's order: match[t][u] == 1 where a center of type t is matched by
    a receptor feature of type u, dist[t] the distance within which it counts -- _MATCHING_TYPES / _MATCHING_DIST as the
    tables the pocket field's complementarity term takes (PfEngine.field_next)."""
    match = torch.tensor([[int(u in _MATCHING_TYPES[t]) for u in ph_idx_to_type] for t in ph_idx_to_type], dtype=torch.int32)
    dist = torch.tensor([float(_MATCHING_DIST[t]) for t in ph_idx_to_type], dtype=torch.float32)
    return match, dist


def clash_energy(ph_coords, prot_x, radius=2.0, weight=1.0):
    """(energy, clashing pairs) of centers [n, 3] against atoms [m, 3], both in the pocket's frame, in fp64: the pocket field's
    clash term, weight * max(0, radius - distance)^2 over all (center, atom) pairs, and the number of pairs inside the radius.
    ``radius``: a float or a per-atom tensor [m]."""
    x, a = torch.as_tensor(ph_coords).double().reshape(-1, 3), torch.as_tensor(prot_x).double().reshape(-1, 3).cpu()
    if x.shape[0] == 0 or a.shape[0] == 0:
        return 0.0, 0
    r = torch.as_tensor(radius).double().reshape(-1).cpu()
    gap = torch.clamp(r[None] - torch.cdist(x.cpu(), a), min=0)
    return float(weight) * float((gap * gap).sum()), int((gap > 0).sum())


def type_restraint_energy(ph_coords, ph_feats, type_restraints, sharpness=4.0):
    """Energy of type restraints on centers [n, 3] (the pocket's frame) with feature rows [n, nf] (one-hot scale: a sample's
    h_0), in fp64: the sum over restraints (type index, center or None, point, radius, weight) and the centers each applies to of
    weight * omega * -log softmax(sharpness * row)[type], omega = 1 for radius 0, else max(0, 1 - rho^2 / radius^2)^2 with rho the
    distance to the point -- the type guidance's restraint term (include/pfdyn.h) on final values."""
    x = torch.as_tensor(ph_coords).double().reshape(-1, 3).cpu()
    h = torch.as_tensor(ph_feats).double().cpu().reshape(x.shape[0], -1)
    if x.shape[0] == 0:
        return 0.0
    ce = -torch.log_softmax(float(sharpness) * h, dim=1)
    total = 0.0
    for t, center, point, radius, weight in (type_restraints or []):
        rows = range(x.shape[0]) if center is None or center == "*" or int(center) < 0 else [int(center)]
        p = torch.as_tensor([float(v) for v in point], dtype=torch.float64)
        for f in rows:
            omega = 1.0
            if float(radius) > 0:
                q = max(0.0, 1.0 - float(((x[f] - p) ** 2).sum()) / float(radius) ** 2)
                omega = q * q
            total += float(weight) * omega * float(ce[f, int(t)])
    return total


def pair_restraint_energy(ph_coords, pair_restraints):
    """(energy, violated pairs) of pair restraints on centers [n, 3], in fp64: the sum over restraints (i, j, lo, hi, weight) --
    i, j center indices, or None / '*' / a negative index for every center -- and the unordered pairs {a, b}, a != b, each covers
    ({i, j}; with one wildcard {i, b} for every b != i; with two every a < b) of weight * (max(0, lo - rho)^2 + max(0, rho - hi)^2),
    rho the pair's distance, hi = inf: no upper bound -- the pair guidance's energy (include/pfdyn.h) on final values -- and the
    number of (restraint, pair) combinations whose distance lies outside lo .. hi.  Fewer than two centers: (0.0, 0)."""
    x = torch.as_tensor(ph_coords).double().reshape(-1, 3).cpu()
    n = x.shape[0]
    if n < 2 or not pair_restraints:
        return 0.0, 0
    rho = (x[:, None, :] - x[None, :, :]).pow(2).sum(dim=2).sqrt()
    upper = torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1)
    index = lambda c: -1 if c is None or c == "*" or int(c) < 0 else int(c)
    total, violated = 0.0, 0
    for i, j, lo, hi, weight in pair_restraints:
        i, j = index(i), index(j)
        if max(i, j) >= n:
            raise ValueError(f"a pair restraint names center {max(i, j)} of {n}")
        cover = torch.zeros(n, n, dtype=torch.bool)
        if i >= 0 and j >= 0:
            cover[min(i, j), max(i, j)] = i != j
        elif i >= 0 or j >= 0:
            c = max(i, j)
            cover[c, :] = True
            cover[:, c] = True
        else:
            cover[:, :] = True
        cover &= upper
        m_lo, m_hi = (float(lo) - rho).clamp(min=0), (rho - float(hi)).clamp(min=0)
        total += float(weight) * float((m_lo * m_lo + m_hi * m_hi)[cover].sum())
        violated += int(((m_lo > 0) | (m_hi > 0))[cover].sum())
    return total, violated


def compute_complementarity(pharm_types, pharm_pos, prot_ph_types, prot_ph_pos, return_count=False):
    """metrics.py:53-86: number (or fraction) of centers with a complementary receptor feature within
    the type-specific distance."""
    if len(prot_ph_types) == 0 or len(pharm_types) == 0:
        count = torch.tensor(0)
    else:
        distances = torch.cdist(pharm_pos, prot_ph_pos)
        lim = torch.tensor([_MATCHING_DIST[t] for t in pharm_types], dtype=distances.dtype).reshape(-1, 1)
        matching = torch.tensor([[r in _MATCHING_TYPES[p] for r in prot_ph_types] for p in pharm_types])
        count = ((distances <= lim) & matching).any(dim=1).sum()
    if return_count:
        return count
    return count / max(len(pharm_types), 1)          # (the reference divides by an undefined name here, metrics.py:85)


def _allreduce_sum(counts: torch.Tensor, process_group, device=None) -> torch.Tensor:
    """Sum a small host vector over the ranks.  The buffer lives where the group's backend needs it: RCCL ("nccl")
    reduces device memory only, so the buffer goes to ``device`` (default: this process's current GPU); gloo reduces the
    host tensor directly."""
    import torch.distributed as dist
    if dist.get_backend(process_group) == "nccl":
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        buf = counts.to(dev)
    else:
        buf = counts.clone()
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=process_group)
    return buf.cpu()


class SampleAnalyzer:
    def analyze(self, sample: List[SampledPharmacophore], process_group=None, device=None):
        """metrics.py:9-35.  With ``process_group`` the numerator / denominator are all-reduced (sum)
        before the division, so every rank reports the validity of the whole job."""
        num = den = 0
        for ph in sample:
            g = ph.g
            if g.prot_ph_h is None or g.prot_ph_x is None:
                prot_types, prot_pos = [], torch.zeros(0, 3)
            else:
                prot_types = [ph_idx_to_type[int(i)] for i in g.prot_ph_h.argmax(dim=1)]
                prot_pos = g.prot_ph_x
            num += int(compute_complementarity(ph.ph_types, ph.ph_coords, prot_types, prot_pos, return_count=True))
            den += ph.n_ph_centers
        counts = torch.tensor([float(num), float(den)], dtype=torch.float64)
        if process_group is not None:
            counts = _allreduce_sum(counts, process_group, device)
        return {'validity': float(counts[0] / counts[1]) if counts[1] > 0 else 0.0}

    def pharm_feat_freq(self, sample: List[SampledPharmacophore], process_group=None, device=None):
        """metrics.py:37-51: counts of each predicted feature type (optionally summed over ranks)."""
        counts = torch.zeros(6, dtype=torch.float64)
        for ph in sample:
            for val in ph.ph_feats_idxs:
                counts[int(val)] += 1
        if process_group is not None:
            counts = _allreduce_sum(counts, process_group, device)
        return counts


# ---- sample sets: what the samples of one pocket agree on (include/pfdyn.h "sample sets") ----------------------------
# The CPU product path of pf_sample_set_analyze, same definitions, usable without a GPU.  A set is a list of samples, each
# (positions [n, 3], type indices [n]) in the pocket's frame; nothing is aligned, and type identity is exact.

SSET_MAX_SAMPLES, SSET_MAX_CENTERS = 1024, 64


def _sset_samples(samples, dtype=torch.float32):
    """[(x [n, 3] dtype, types [n] int64)] on the host from (x, types) pairs or SampledPharmacophore objects, limits checked."""
    out = []
    for s in samples:
        x, t = (s.ph_coords, s.ph_feats_idxs) if hasattr(s, "ph_coords") else s
        x = torch.as_tensor(x).detach().to("cpu", dtype).reshape(-1, 3)
        t = torch.as_tensor(t).detach().to("cpu", torch.int64).reshape(-1)
        if x.shape[0] != t.shape[0]:
            raise ValueError(f"sample {len(out)}: {x.shape[0]} positions for {t.shape[0]} types")
        if not 1 <= x.shape[0] <= SSET_MAX_CENTERS:
            raise ValueError(f"sample {len(out)} has {x.shape[0]} centers (1 to {SSET_MAX_CENTERS} per sample)")
        out.append((x, t))
    if not 1 <= len(out) <= SSET_MAX_SAMPLES:
        raise ValueError(f"a sample set has {len(out)} samples (1 to {SSET_MAX_SAMPLES} per set)")
    return out


def _sset_options(sigma=1.0, tolerance=1.5, threshold=0.5):
    import math
    sigma, tolerance, threshold = float(sigma), float(tolerance), float(threshold)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0")
    if not (math.isfinite(tolerance) and tolerance >= 0):
        raise ValueError("tolerance must be finite and >= 0")
    if not 0.0 <= threshold <= 1.0:
        raise ValueError("threshold must be in [0, 1]")
    return sigma, tolerance, threshold


def _sset_padded(samples):
    """x [S, m, 3], types [S, m] (padding: -1 - sample index, equal to no type), n [S]"""
    S, m = len(samples), max(x.shape[0] for x, _ in samples)
    X = torch.zeros(S, m, 3, dtype=samples[0][0].dtype)
    T = -1 - torch.arange(S, dtype=torch.int64)[:, None].repeat(1, m)
    for a, (x, t) in enumerate(samples):
        X[a, :x.shape[0]], T[a, :x.shape[0]] = x, t
    return X, T, torch.tensor([x.shape[0] for x, _ in samples])


def _sset_rows(X, T, rows):
    """squared distances [r, S, m, m] and same-type mask between the centers of samples `rows` and those of every sample; a padded
    center (a negative type) matches nothing, not even itself"""
    d = X[rows][:, None, :, None, :] - X[None, :, None, :, :]
    same = (T[rows][:, None, :, None] == T[None, :, None, :]) & (T[rows] >= 0)[:, None, :, None]
    return (d * d).sum(dim=-1), same


def sample_set_similarity(samples, sigma=1.0, dtype=torch.float32):
    """The typed Gaussian-overlap Tanimoto matrix [S, S] of a set: O(a,b) = sum_i sum_j [t_ai == t_bj] exp(-|x_ai - x_bj|^2 /
    (2 sigma^2)), sim(a,b) = O(a,b) / (O(a,a) + O(b,b) - O(a,b)).  Each unordered pair is computed once and stored to both
    places; the diagonal is exactly 1."""
    samples = _sset_samples(samples, dtype)
    sigma = _sset_options(sigma=sigma)[0]
    X, T, _ = _sset_padded(samples)
    S, m = X.shape[0], X.shape[1]
    O = torch.zeros(S, S, dtype=dtype)
    step = max(1, (1 << 22) // (S * m * m))
    for a0 in range(0, S, step):
        rows = torch.arange(a0, min(a0 + step, S))
        d2, same = _sset_rows(X, T, rows)
        O[rows] = (torch.exp(-d2 / (2.0 * sigma * sigma)) * same).sum(dim=(2, 3))
    self_o = torch.diagonal(O).clone()
    up = torch.triu(O, diagonal=1)
    sim = (up / (self_o[:, None] + self_o[None, :] - up)).clamp(max=1.0)       # (an ulp of rounding between near-identical samples)
    sim = torch.triu(sim, diagonal=1)
    sim = sim + sim.T
    sim.fill_diagonal_(1.0)
    return sim


def sample_set_support(samples, tolerance=1.5):
    """One int64 tensor [n_a] per sample: support(a, i) = the number of samples b != a of the set with a center of type t_ai within
    `tolerance` (<=) of x_ai."""
    samples = _sset_samples(samples, torch.float64)
    tol = _sset_options(tolerance=tolerance)[1]
    X, T, n = _sset_padded(samples)
    S, m = X.shape[0], X.shape[1]
    sup = torch.zeros(S, m, dtype=torch.int64)
    step = max(1, (1 << 22) // (S * m * m))
    for a0 in range(0, S, step):
        rows = torch.arange(a0, min(a0 + step, S))
        d2, same = _sset_rows(X, T, rows)
        hit = ((d2 <= tol * tol) & same).any(dim=3)                     # [r, S, m]: center i of row sample has a partner in sample b
        hit[torch.arange(rows.shape[0]), rows] = False
        sup[rows] = hit.sum(dim=1)
    return [sup[a, :int(n[a])].clone() for a in range(S)]


def butina_clusters(sim, threshold=0.5):
    """Taylor-Butina on a similarity matrix [S, S], the values compared as they are: adj(a,b) = a != b and sim(a,b) >= threshold,
    count(a) = sum_b adj(a,b); samples are visited in the order (-count, index); an unassigned sample becomes the centroid of a
    new cluster (ids in order of creation) and takes every still unassigned neighbour.  Counts are not updated as samples
    leave: the result depends on that order by design.  Returns (labels [S] int64, centroids, sizes, counts [S])."""
    sim = torch.as_tensor(sim).detach().cpu()
    S = sim.shape[0]
    if sim.dim() != 2 or sim.shape[1] != S or S < 1:
        raise ValueError(f"a square similarity matrix is required, got {tuple(sim.shape)}")
    thr = torch.tensor(_sset_options(threshold=threshold)[2], dtype=sim.dtype)
    adj = sim >= thr
    adj.fill_diagonal_(False)
    counts = adj.sum(dim=1)
    order = sorted(range(S), key=lambda a: (-int(counts[a]), a))
    labels = torch.full((S,), -1, dtype=torch.int64)
    centroids, sizes = [], []
    for a in order:
        if labels[a] >= 0:
            continue
        take = adj[a] & (labels < 0)
        take[a] = True
        labels[take] = len(centroids)
        centroids.append(a)
        sizes.append(int(take.sum()))
    return labels, centroids, sizes, counts


def cluster_consensus(samples, labels, centroids, tolerance=1.5, dtype=torch.float32):
    """Per cluster c (centroid sample m = centroids[c]) and center i of m: the members of c in ascending index (m included) each
    give their nearest center of type t_mi within `tolerance` of x_mi (ties: the lowest index); their positions are summed in
    that order in `dtype` and divided by their number.  Returns one (positions [n_m, 3], types [n_m], counts [n_m] int64) per
    cluster; counts / cluster size is the consensus support."""
    samples = _sset_samples(samples, dtype)
    tol = _sset_options(tolerance=tolerance)[1]
    tol2 = torch.tensor(tol * tol, dtype=dtype)
    labels = torch.as_tensor(labels).cpu()
    out = []
    for c, m in enumerate(centroids):
        xm, tm = samples[int(m)]
        pos, cnt = torch.zeros_like(xm), torch.zeros(xm.shape[0], dtype=torch.int64)
        for b in torch.nonzero(labels == c).reshape(-1).tolist():
            xb, tb = samples[b]
            d = xm[:, None, :] - xb[None, :, :]
            d2 = (d * d).sum(dim=-1)
            ok = (tm[:, None] == tb[None, :]) & (d2 <= tol2)
            j = torch.where(ok, d2, torch.full_like(d2, float("inf"))).argmin(dim=1)        # (argmin: the first of equals)
            got = ok.any(dim=1)
            pos = pos + torch.where(got[:, None], xb[j], torch.zeros_like(xm))
            cnt = cnt + got.to(torch.int64)
        out.append((pos / cnt.clamp(min=1).to(dtype)[:, None], tm.clone(), cnt))
    return out


def pick_diverse(sim, k, first=None):
    """Max-min selection of k samples on a similarity matrix: after `first`, the next pick is the sample with the largest minimum
    distance 1 - sim to those chosen (ties: the lowest index).  `first` defaults to the centroid of the largest Butina cluster at
    the default threshold (ties: the first made).  Returns the chosen indices in order of choice; at most S of them."""
    sim = torch.as_tensor(sim).detach().cpu().double()
    S = sim.shape[0]
    if int(k) < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    if first is None:
        _, centroids, sizes, _ = butina_clusters(sim)
        first = centroids[max(range(len(sizes)), key=lambda c: (sizes[c], -c))]
    first = int(first)
    if not 0 <= first < S:
        raise ValueError(f"first = {first} is not a sample of the set ({S})")
    chosen = [first]
    far = 1.0 - sim[first]
    far[first] = -1.0
    while len(chosen) < min(int(k), S):
        nxt = int(torch.argmax(far))            # (argmax: the first of equals)
        chosen.append(nxt)
        far = torch.minimum(far, 1.0 - sim[nxt])
        far[chosen] = -1.0
    return chosen


class ConsensusPharmacophore:
    """The consensus of one cluster of a sample set: the centers of the cluster's centroid sample, each moved to the mean of its
    nearest same-type partners in the members, with the fraction of members that have one.  ``centroid``: the centroid's sample
    index within the set; ``members``: the cluster's sample indices, ascending; ``positions`` [n, 3], ``types`` [n] (indices),
    ``counts`` [n] and ``support`` [n] = counts / len(members).  It is the centroid's consensus, not a re-fit."""
    __slots__ = ("cluster", "centroid", "members", "positions", "types", "counts", "support")

    def __init__(self, cluster, centroid, members, positions, types, counts):
        self.cluster, self.centroid, self.members = int(cluster), int(centroid), [int(b) for b in members]
        self.positions = torch.as_tensor(positions).detach().to("cpu", torch.float32).reshape(-1, 3)
        self.types = torch.as_tensor(types).detach().to("cpu", torch.int64).reshape(-1)
        self.counts = torch.as_tensor(counts).detach().to("cpu", torch.int64).reshape(-1)
        self.support = self.counts.double() / max(len(self.members), 1)

    @property
    def size(self):
        return len(self.members)

    def to_xyz_file(self, filename: str = None, min_support: float = 0.0):
        """One frame in the pharms.xyz format with the support as a trailing column: the number of centers written, then
        `element x y z support` per center whose support is at least ``min_support``."""
        keep = [i for i in range(self.types.shape[0]) if float(self.support[i]) >= float(min_support)]
        rows = self.positions.double().tolist()
        body = "".join(f"{_XYZ_ELEMENTS[int(self.types[i])]} {rows[i][0]:.3f} {rows[i][1]:.3f} {rows[i][2]:.3f} {float(self.support[i]):.3f}\n"
                       for i in keep)
        return _emit(f"{len(keep)}\n" + body, filename)

    def __repr__(self):
        return f"ConsensusPharmacophore(cluster={self.cluster}, centroid={self.centroid}, size={self.size}, centers={self.types.shape[0]})"


class SampleSet:
    """What the S samples of one pocket agree on.  ``similarity`` [S, S] fp32; ``support``: one int64 tensor per sample, the
    number of other samples that hold each of its centers; ``labels`` [S]: the Butina cluster id of each sample (ids in order
    of creation); ``neighbour_counts`` [S]; ``clusters``: ConsensusPharmacophore objects, largest first, ties by id;
    ``pick_diverse(k)``: max-min selection starting from the largest cluster's centroid.  ``options``: sigma, tolerance,
    threshold, min_support."""

    def __init__(self, similarity, support, labels, centroids, consensus, neighbour_counts=None, options=None):
        self.similarity = torch.as_tensor(similarity).detach().to("cpu", torch.float32)
        self.support = [torch.as_tensor(s).detach().to("cpu", torch.int64) for s in support]
        self.labels = torch.as_tensor(labels).detach().to("cpu", torch.int64)
        self.options = dict(options or {})
        if neighbour_counts is None:
            adj = self.similarity >= torch.tensor(float(self.options.get("threshold", 0.5)), dtype=torch.float32)
            adj.fill_diagonal_(False)
            neighbour_counts = adj.sum(dim=1)
        self.neighbour_counts = torch.as_tensor(neighbour_counts).detach().to("cpu", torch.int64)
        made = [ConsensusPharmacophore(c, m, torch.nonzero(self.labels == c).reshape(-1).tolist(), *consensus[c])
                for c, m in enumerate(centroids)]
        self.clusters = sorted(made, key=lambda c: (-c.size, c.cluster))

    @property
    def n_samples(self):
        return int(self.labels.shape[0])

    @property
    def centroids(self):
        """centroid sample index of every cluster, by cluster id"""
        return [c.centroid for c in sorted(self.clusters, key=lambda c: c.cluster)]

    def mean_support(self):
        """one float per sample: the mean support of its centers, as a fraction of the other samples (0 for a set of one)"""
        other = max(self.n_samples - 1, 1)
        return [float(s.double().mean()) / other for s in self.support]

    def pick_diverse(self, k, first=None):
        return pick_diverse(self.similarity, k, first=self.clusters[0].centroid if first is None else first)

    def consensus_xyz(self, min_support=None):
        """every cluster's frame (ConsensusPharmacophore.to_xyz_file), largest cluster first"""
        f = float(self.options.get("min_support", 0.5)) if min_support is None else float(min_support)
        return "".join(c.to_xyz_file(min_support=f) for c in self.clusters)

    def clusters_tsv(self):
        """sample index, cluster, is-centroid, neighbour count, mean center support -- one row per sample"""
        cents, ms = set(self.centroids), self.mean_support()
        rows = ["sample\tcluster\tis_centroid\tneighbours\tmean_support\n"]
        for a in range(self.n_samples):
            rows.append(f"{a}\t{int(self.labels[a])}\t{int(a in cents)}\t{int(self.neighbour_counts[a])}\t{ms[a]:.4f}\n")
        return "".join(rows)

    def __repr__(self):
        return f"SampleSet(samples={self.n_samples}, clusters={len(self.clusters)}, largest={self.clusters[0].size})"


def analyze_sample_set(samples, sigma=1.0, tolerance=1.5, threshold=0.5, min_support=0.5):
    """The SampleSet of one pocket's samples, computed on the host (the device path: PharmacophoreDiff.consensus)."""
    sigma, tolerance, threshold = _sset_options(sigma, tolerance, threshold)
    samples = _sset_samples(samples)
    sim = sample_set_similarity(samples, sigma)
    labels, centroids, _, counts = butina_clusters(sim, threshold)
    return SampleSet(sim, sample_set_support(samples, tolerance), labels, centroids,
                     cluster_consensus(samples, labels, centroids, tolerance), counts,
                     dict(sigma=sigma, tolerance=tolerance, threshold=threshold, min_support=float(min_support)))


# ---- pharmacophore alignment: superpose a library onto queries and rank it (include/pfdyn.h "pharmacophore alignment")
# The CPU product path of pf_pharm_align, same definition, usable without a GPU: per (query, entry) pair the best of the three-point
# superpositions by typed Gaussian overlap, refined by weighted least squares.  Proper rotations only (Horn's quaternion), types
# match exactly; the result is the best of a discrete seed set plus a local refinement, not a global optimum.

ALIGN_MAX_QUERY_CENTERS, ALIGN_MAX_ENTRY_CENTERS, ALIGN_MAX_PAIRS, ALIGN_MAX_REFINE = 16, 32, 1 << 24, 16


def _align_options(sigma=1.0, tolerance=1.5, refine=4, min_area=1.0):
    import math
    sigma, tolerance, min_area = float(sigma), float(tolerance), float(min_area)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError("sigma must be finite and > 0")
    if not (math.isfinite(tolerance) and tolerance >= 0):
        raise ValueError("tolerance must be finite and >= 0")
    if int(refine) != refine or not 0 <= int(refine) <= ALIGN_MAX_REFINE:
        raise ValueError(f"refine must be an integer in [0, {ALIGN_MAX_REFINE}]")
    if not (math.isfinite(min_area) and min_area > 0):
        raise ValueError("min_area must be finite and > 0")
    return sigma, tolerance, int(refine), min_area


def _align_item(s, dtype=torch.float32):
    """(x [n, 3] dtype, types [n] int64) on the host from a SampledPharmacophore, a ConsensusPharmacophore or an (x, types) pair"""
    if hasattr(s, "ph_coords"):
        x, t = s.ph_coords, s.ph_feats_idxs
    elif hasattr(s, "positions") and hasattr(s, "types"):
        x, t = s.positions, s.types
    else:
        x, t = s
    x = torch.as_tensor(x).detach().to("cpu", dtype).reshape(-1, 3)
    t = torch.as_tensor(t).detach().to("cpu", torch.int64).reshape(-1)
    if x.shape[0] != t.shape[0]:
        raise ValueError(f"{x.shape[0]} positions for {t.shape[0]} types")
    return x, t


def _align_queries(queries, dtype=torch.float32):
    out = [_align_item(s, dtype) for s in queries]
    for k, (x, _) in enumerate(out):
        if not 1 <= x.shape[0] <= ALIGN_MAX_QUERY_CENTERS:
            raise ValueError(f"query {k} has {x.shape[0]} centers (1 to {ALIGN_MAX_QUERY_CENTERS} per query)")
    return out


def _horn_rotation(S):
    """S [n, 3, 3] = sum w (y - yc)(x - xc)^T -> the proper rotations R [n, 3, 3] with x ~ R y: the unit quaternion is the
    eigenvector of the largest eigenvalue of Horn's symmetric 4 x 4 matrix"""
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (S[:, a, b] for a in range(3) for b in range(3))
    N = torch.stack([torch.stack([Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], -1),
                     torch.stack([Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz], -1),
                     torch.stack([Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy], -1),
                     torch.stack([Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz], -1)], -2)
    w, x, y, z = torch.linalg.eigh(N)[1][:, :, -1].unbind(-1)              # eigenvalues ascend: the last column
    return torch.stack([torch.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                        torch.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)


def _align_fit(Y, X, W):
    """weighted least squares over corresponding points Y, X [n, m, 3] with weights W [n, m]: R [n, 3, 3], s [n, 3], X ~ R Y + s"""
    Wn = W / W.sum(dim=1, keepdim=True)
    yc, xc = (Wn[..., None] * Y).sum(dim=1), (Wn[..., None] * X).sum(dim=1)
    S = torch.einsum("nm,nma,nmb->nab", W, Y - yc[:, None], X - xc[:, None])
    R = _horn_rotation(S)
    return R, xc - torch.einsum("nab,nb->na", R, yc)


def _align_overlap(x, y, same, R, s, inv_2s2):
    d2 = ((x[None, :, None, :] - (torch.einsum("nab,lb->nla", R, y) + s[:, None, :])[:, None, :, :]) ** 2).sum(-1)
    return (torch.exp(-d2 * inv_2s2) * same[None]).sum(dim=(1, 2)), d2


def _align_seeds(x, t, y, u, tolerance, min_area):
    """(query triplets [n, 3], entry triples [n, 3]) in enumeration order (i, j, k, a, b, c)"""
    nq = t.shape[0]
    dq, dl = torch.cdist(x, x), torch.cdist(y, y)
    where = [torch.nonzero(u == k).reshape(-1) for k in range(int(max(t.max(), u.max())) + 1)] if nq else []
    qs, ls = [], []
    for i in range(nq):
        for j in range(i + 1, nq):
            for k in range(j + 1, nq):
                A, B, C = where[int(t[i])], where[int(t[j])], where[int(t[k])]
                if not (len(A) and len(B) and len(C)):
                    continue
                if torch.linalg.cross(x[j] - x[i], x[k] - x[i]).norm() < min_area:
                    continue
                a, b, c = (v.reshape(-1) for v in torch.meshgrid(A, B, C, indexing="ij"))
                ok = (a != b) & (a != c) & (b != c)
                ok &= ((dq[i, j] - dl[a, b]).abs() <= 2 * tolerance) & ((dq[i, k] - dl[a, c]).abs() <= 2 * tolerance) & ((dq[j, k] - dl[b, c]).abs() <= 2 * tolerance)
                a, b, c = a[ok], b[ok], c[ok]
                ok = torch.linalg.cross(y[b] - y[a], y[c] - y[a]).norm(dim=-1) >= min_area
                if ok.any():
                    ls.append(torch.stack([a[ok], b[ok], c[ok]], -1))
                    qs.append(torch.tensor([i, j, k]).expand(ls[-1].shape[0], 3))
    if not qs:
        return torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3, dtype=torch.int64)
    return torch.cat(qs), torch.cat(ls)


def align_pair(x, t, y, u, sigma=1.0, tolerance=1.5, refine=4, min_area=1.0, dtype=torch.float64):
    """One (query, entry) pair by the definition of pf_pharm_align, on the host at `dtype`: returns (sim, n_matched, n_seeds,
    transform [12] = R row-major then s, entry frame -> query frame).  No seed: (0.0, 0, 0, identity)."""
    sigma, tolerance, refine, min_area = _align_options(sigma, tolerance, refine, min_area)
    (x, t), (y, u) = _align_item((x, t), dtype), _align_item((y, u), dtype)
    qs, ls = _align_seeds(x, t, y, u, tolerance, min_area)
    n = int(qs.shape[0])
    if n == 0:
        return 0.0, 0, 0, torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=dtype)
    inv = 1.0 / (2.0 * sigma * sigma)
    same = t[:, None] == u[None, :]
    O, R, s = None, None, None
    for c0 in range(0, n, 8192):
        q_, l_ = qs[c0:c0 + 8192], ls[c0:c0 + 8192]
        Rc, sc = _align_fit(y[l_], x[q_], torch.ones(q_.shape, dtype=dtype))
        Oc, _ = _align_overlap(x, y, same, Rc, sc, inv)
        m = int(torch.nonzero(Oc == Oc.max())[0])                           # the first of equals
        if O is None or Oc[m] > O:
            O, R, s = Oc[m], Rc[m], sc[m]
    p_, q_ = torch.nonzero(same, as_tuple=True)
    for _ in range(refine):
        _, d2 = _align_overlap(x, y, same, R[None], s[None], inv)
        w = torch.exp(-d2[0] * inv)[p_, q_]
        R2, s2 = _align_fit(y[q_][None], x[p_][None], w[None])
        O2, _ = _align_overlap(x, y, same, R2, s2, inv)
        if not bool(O2[0] >= O):
            break
        O, R, s = O2[0], R2[0], s2[0]
    eye = torch.eye(3, dtype=dtype)[None]
    zero = torch.zeros(1, 3, dtype=dtype)
    oqq = _align_overlap(x, x, t[:, None] == t[None, :], eye, zero, inv)[0][0]
    oll = _align_overlap(y, y, u[:, None] == u[None, :], eye, zero, inv)[0][0]
    _, d2 = _align_overlap(x, y, same, R[None], s[None], inv)
    matched = int(((d2[0] <= tolerance * tolerance) & same).any(dim=1).sum())
    return min(float(O / (oqq + oll - O)), 1.0), matched, n, torch.cat([R.reshape(-1), s])


def align_pharmacophores(queries, library, sigma=1.0, tolerance=1.5, refine=4, min_area=1.0, dtype=torch.float32):
    """Every query against every library entry on the host (the device path: PfEngine.align, PharmacophoreDiff.screen).  `queries`:
    samples, ConsensusPharmacophore objects or (x, types) pairs of 1 to 16 centers; `library`: a PharmacophoreLibrary or such a
    list, entries of 1 to 32 centers.  Returns a dict: sim [Q, L] (dtype), n_matched [Q, L], n_seeds [Q, L] int64, transform
    [Q, L, 12]."""
    opts = _align_options(sigma, tolerance, refine, min_area)
    qs = _align_queries(queries, dtype)
    lib = library if isinstance(library, PharmacophoreLibrary) else PharmacophoreLibrary(library)
    Q, L = len(qs), len(lib)
    out = dict(sim=torch.zeros(Q, L, dtype=dtype), n_matched=torch.zeros(Q, L, dtype=torch.int64), n_seeds=torch.zeros(Q, L, dtype=torch.int64),
               transform=torch.zeros(Q, L, 12, dtype=dtype))
    for a, (x, t) in enumerate(qs):
        for b in range(L):
            y, u = lib[b]
            out["sim"][a, b], out["n_matched"][a, b], out["n_seeds"][a, b], out["transform"][a, b] = align_pair(x, t, y, u, *opts, dtype=dtype)
    return out


class PharmacophoreLibrary:
    """Known pharmacophores to screen against: entries (positions [n, 3] fp32, type indices [n]) of 1 to 32 centers each, with
    ``names``.  ``dropped``: how many offered entries lay outside 1..32 centers (from_dataset / from_file drop them and count;
    the constructor refuses them).  ``to(device)`` packs the centers once and uploads them, for many screening calls."""

    def __init__(self, entries, names=None, dropped=0):
        self.entries = [_align_item(e) for e in entries]
        for k, (x, _) in enumerate(self.entries):
            if not 1 <= x.shape[0] <= ALIGN_MAX_ENTRY_CENTERS:
                raise ValueError(f"entry {k} has {x.shape[0]} centers (1 to {ALIGN_MAX_ENTRY_CENTERS} per library entry)")
        self.names = [str(n) for n in names] if names is not None else [f"entry_{k}" for k in range(len(self.entries))]
        if len(self.names) != len(self.entries):
            raise ValueError(f"{len(self.names)} names for {len(self.entries)} entries")
        self.dropped = int(dropped)
        self._packed = None

    @staticmethod
    def _kept(entries, names):
        keep = [k for k, (x, _) in enumerate(entries) if 1 <= torch.as_tensor(x).reshape(-1, 3).shape[0] <= ALIGN_MAX_ENTRY_CENTERS]
        return PharmacophoreLibrary([entries[k] for k in keep], [names[k] for k in keep], dropped=len(entries) - len(keep))

    @classmethod
    def from_file(cls, path):
        """the frames of a file in the pharms.xyz format (read_pharmacophores), named <file stem>:<frame index>"""
        frames = read_pharmacophores(path)
        return cls._kept(frames, [f"{Path(path).stem}:{k}" for k in range(len(frames))])

    @classmethod
    def from_dataset(cls, dataset):
        """each pocket's ligand pharmacophore of a ProteinPharmacophoreDataset (pharm_pos / pharm_feat), named by the pocket's
        protein file where the dataset has the names, else pocket_<index>.  ``index``: the pocket index of every kept entry."""
        entries, names = [], []
        for i in range(int(dataset.pharm_idx.shape[0])):
            ps, pe = (int(v) for v in dataset.pharm_idx[i])
            entries.append((dataset.pharm_pos[ps:pe].float(), dataset.pharm_feat[ps:pe].long()))
            have = getattr(dataset, "prot_file_names", None)
            names.append(str(have[i]) if have and i < len(have) else f"pocket_{i}")
        lib = cls._kept(entries, names)
        lib.index = [k for k, (x, _) in enumerate(entries) if 1 <= x.shape[0] <= ALIGN_MAX_ENTRY_CENTERS]
        return lib

    def __len__(self):
        return len(self.entries)

    def __getitem__(self, k):
        return self.entries[k]

    def packed(self):
        """(x [N, 3] fp32, types [N] int32, ptr [L + 1] int32 on the host): the library as pf_pharm_align takes it"""
        if self._packed is None:
            ptr = torch.zeros(len(self) + 1, dtype=torch.int32)
            if len(self):
                ptr[1:] = torch.cumsum(torch.tensor([x.shape[0] for x, _ in self.entries]), 0)
                self._packed = (torch.cat([x for x, _ in self.entries]), torch.cat([t for _, t in self.entries]).to(torch.int32), ptr)
            else:
                self._packed = (torch.zeros(0, 3), torch.zeros(0, dtype=torch.int32), ptr)
        return self._packed

    def to(self, device):
        x, t, ptr = self.packed()
        self._packed = (x.to(device), t.to(device), ptr)
        return self

    def __repr__(self):
        return f"PharmacophoreLibrary(entries={len(self)}, dropped={self.dropped})"


class ScreenHit:
    """One library entry superposed onto a query: ``entry`` (index in the library), ``name``, ``sim``, ``n_matched`` and
    ``transform`` [12] (R row-major, then s: entry frame -> query frame).  ``aligned()`` gives the entry's centers in the query's
    frame."""
    __slots__ = ("entry", "name", "sim", "n_matched", "transform", "_centers")

    def __init__(self, entry, name, sim, n_matched, transform, centers=None):
        self.entry, self.name, self.sim, self.n_matched = int(entry), str(name), float(sim), int(n_matched)
        self.transform = torch.as_tensor(transform).detach().to("cpu", torch.float32).reshape(12)
        self._centers = centers

    def aligned(self):
        """(positions [n, 3] fp32 in the query's frame, type indices [n])"""
        if self._centers is None:
            raise ValueError("this hit does not hold its entry's centers")
        y, u = self._centers
        R, s = self.transform[:9].reshape(3, 3).double(), self.transform[9:].double()
        return (y.double() @ R.T + s).float(), u.clone()

    def to_xyz_file(self, filename: str = None):
        y, u = self.aligned()
        return _emit(_xyz_block([_XYZ_ELEMENTS[int(k)] for k in u], y), filename)

    def __repr__(self):
        return f"ScreenHit(entry={self.entry}, name={self.name!r}, sim={self.sim:.4f}, n_matched={self.n_matched})"
