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
