#!/usr/bin/env python3
"""Dataset-scale sampling (BASELINE config 4): for every pocket of a data split draw ``samples_per_pocket``
pharmacophores and write <output_dir>/pocket_<idx>/{pharms.xyz | pharm_<k>_traj.xyz, sample_time.txt,
reference_files/}, plus validity / type-frequency metrics over the whole job.

Flag names, types, defaults and the output tree are those of the reference's test.py (:23-60, :113-262).  The execution
model is this repository's: the (pocket, sample) graphs of ``--pockets_per_call`` pockets share device batches of
``--max_batch_size`` (PharmacophoreDiff.sample; the reference runs one pocket per batch), and under
``torchrun --nproc-per-node N test.py ...`` the pockets are dealt over the GPUs by work -- greedy on
(pp edges x samples), pharmacoforge_amd.sharding -- with no data-path collective; only the eight metric counters are
all-reduced (RCCL when every rank has its own GPU)."""
import argparse
import os
import pickle
import shutil
import time
from pathlib import Path

import torch
import yaml

_FLAGS = [
    ('--ckpt', dict(type=Path, default=None, help='checkpoint file at <run>/checkpoints/<name>.ckpt')),
    ('--model_dir', dict(type=Path, default=None, help='training run directory; checkpoints/last.ckpt is used')),
    ('--samples_per_pocket', dict(type=int, default=1, help='pharmacophores drawn for each pocket')),
    ('--pharm_sizes', dict(nargs='*', type=int, default=[], help='centers per pharmacophore, one integer per sample (default: uniform 3..8)')),
    ('--max_batch_size', dict(type=int, default=128, help='graphs per device batch')),
    ('--seed', dict(type=int, default=42, help='torch seed (each rank adds its rank)')),
    ('--output_dir', dict(type=Path, default=None, help='default: <run>/samples')),
    ('--max_tries', dict(type=int, default=1, help='accepted for compatibility; every requested sample is produced in one pass')),
    ('--dataset_size', dict(type=int, default=None, help='use only this many pockets')),
    ('--dataset_idx', dict(type=int, default=None, help='a single pocket, or the first one with --dataset_idx_as_start')),
    ('--dataset_idx_as_start', dict(action='store_true', help='sample --dataset_size pockets beginning at --dataset_idx')),
    ('--split', dict(type=str, default='val', help="'val' or 'train'")),
    ('--use_ref_pharm_com', dict(action='store_true', help='start the centers at the reference pharmacophore\'s mean position')),
    ('--visualize_trajectory', dict(action='store_true', help='write every denoising frame, one xyz file per sample')),
    ('--metrics', dict(action='store_true', help='validity and feature-type counts over all samples of all ranks')),
    ('--sample_steps', dict(type=int, default=None, help='few-step sampling: visit only this many of the T levels; how good such samples are depends on the trained weights')),
    ('--sampler', dict(choices=['ancestral', 'ddim', 'multistep'], default=None, help='with --sample_steps: ancestral (default), ddim (--eta, default 0) or multistep (second-order multistep solver)')),
    ('--eta', dict(type=float, default=None, help='with --sample_steps --sampler ddim: share of the posterior noise injected, 0..1 (default 0)')),
    ('--spacing', dict(choices=['uniform', 'quadratic', 'logsnr'], default=None, help='with --sample_steps: how the visited levels are spread (default uniform)')),
    ('--avoid_clashes', dict(type=float, nargs='?', const=2.0, default=None, metavar='R', help='guided sampling: keep the centers out of the pocket\'s own atoms, R angstroms around each (default 2.0); a guided step costs several times a default one')),
    ('--clash_weight', dict(type=float, default=None, help='with --avoid_clashes: weight of the clash energy (default 1)')),
    ('--guide_complementarity', dict(type=float, default=None, metavar='W', help='guided sampling: pull every center to within the matching distance of a complementary receptor feature of the dataset graph, with weight W (what --metrics counts as validity)')),
    ('--guide_scale', dict(type=float, default=None, help='with --avoid_clashes or --guide_complementarity: strength of the guidance (default 1)')),
    ('--guide_clip', dict(type=float, default=None, help='with --avoid_clashes or --guide_complementarity: largest shift of a center per step in angstroms (default 0: no clip)')),
    ('--guide_family', dict(choices=['wide', 'tuned'], default=None, help='with --avoid_clashes or --guide_complementarity: the kernels of a guided step (wide: every model width, the default; tuned: models of n_hidden_scalars 128 / vector_size 16)')),
    ('--pair_restraints', dict(type=Path, default=None, help='guided sampling: a text file with one pair restraint per line, "pair I|* J|* LO HI|inf WEIGHT" (# starts a comment): the two centers (*: every center) of one sample are held LO to HI angstroms apart, applied to every pocket')),
    ('--min_separation', dict(type=float, default=None, metavar='D', help='guided sampling: no two centers of a sample closer than D angstroms (the pair restraint "* * D inf W"); every batch then runs guided, which costs several times a default step')),
    ('--separation_weight', dict(type=float, default=None, metavar='W', help='with --min_separation: weight of its energy (default 1)')),
    ('--type_restraints', dict(type=Path, default=None, help='guided sampling of the types: a text file with one type restraint per line, "type NAME|INDEX x y z radius weight [center|*]" (# starts a comment), applied to every pocket in its own frame (radius 0: no spatial condition)')),
    ('--guide_type_scale', dict(type=float, default=None, help='with --type_restraints or --guide_complementarity_types: strength of the guidance of the feature rows (default 1)')),
    ('--guide_type_clip', dict(type=float, default=None, help='with --type_restraints or --guide_complementarity_types: largest Euclidean norm of a feature row\'s shift per step (default 0: no clip)')),
    ('--type_sharpness', dict(type=float, default=None, help='with --type_restraints or --guide_complementarity_types: sharpness of the soft type assignment on one-hot-scaled features (default 4)')),
    ('--guide_complementarity_types', dict(action='store_true', help='with --guide_complementarity: the complementarity energy steers the centers\' types too, so that a center next to an acceptor can become a donor')),
    ('--comp_unmatched', dict(type=float, default=None, metavar='U', help='with --guide_complementarity_types: what a type without any partner in the pocket costs, as a distance beyond its matching distance (default 0)')),
    ('--pockets_per_call', dict(type=int, default=64, help='pockets whose samples are batched together (not in the reference)')),
    ('--use_ema', dict(action='store_true', help="sample from the checkpoint's EMA weights ('ema_state_dict') instead of the training weights")),
    ('--screen_self', dict(action='store_true', help='screen the ligand pharmacophores of the split (1 to 32 centers each) against every pocket\'s samples (rigid superposition, default options): per pocket the rank of the pocket\'s own ligand among the hits of its best sample -- the sample most similar to that ligand -- and self_rank_median and self_top10 over all ranks, written to screen_self.tsv and screen_summary.txt')),
    ('--consensus', dict(action='store_true', help='analyse the samples of every pocket as a set (similarity, clusters, consensus; default options): writes consensus.xyz and clusters.tsv per pocket and adds clusters_per_pocket and mean_support to the summary over all ranks')),
]


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    a = parser.parse_args(argv)
    if a.ckpt is None and a.model_dir is None:
        raise ValueError('no model given: pass --ckpt or --model_dir')
    if a.pharm_sizes and len(a.pharm_sizes) != a.samples_per_pocket:
        raise ValueError(f'--pharm_sizes lists {len(a.pharm_sizes)} sizes for --samples_per_pocket {a.samples_per_pocket}')
    if a.consensus and a.samples_per_pocket > 1024:
        raise ValueError(f'--consensus: --samples_per_pocket {a.samples_per_pocket} (a set has at most 1024 samples)')
    if a.sample_steps is None and (a.sampler is not None or a.eta is not None or a.spacing is not None):
        raise ValueError('--sampler, --eta and --spacing need --sample_steps')
    if a.sample_steps is not None and a.sample_steps < 1:
        raise ValueError(f'--sample_steps must be at least 1, got {a.sample_steps}')
    if a.eta is not None and (a.sampler != 'ddim' or not 0.0 <= a.eta <= 1.0):
        raise ValueError('--eta needs --sampler ddim and a value in 0..1')
    typed = a.type_restraints is not None or a.guide_complementarity_types
    paired = a.pair_restraints is not None or a.min_separation is not None
    guided = a.avoid_clashes is not None or a.guide_complementarity is not None or a.type_restraints is not None or paired
    if a.separation_weight is not None and a.min_separation is None:
        raise ValueError('--separation_weight needs --min_separation')
    for flag in ('min_separation', 'separation_weight'):
        v = getattr(a, flag)
        if v is not None and not (v >= 0 and v < float('inf')):
            raise ValueError(f'--{flag} must be finite and not negative, got {v}')
    a.separation_weight = 1.0 if a.separation_weight is None else a.separation_weight
    a.pair_restraint_list = None
    if a.pair_restraints is not None:
        from pharmacoforge_amd.pocket_io import read_pair_restraints
        a.pair_restraint_list = read_pair_restraints(a.pair_restraints)
        named = [c for i, j, _, _, _ in a.pair_restraint_list for c in (i, j) if c is not None]
        small = [n for n in (a.pharm_sizes or []) if named and n <= max(named)]
        if small:
            raise ValueError(f'--pharm_sizes {small} do not reach center {max(named)} named in --pair_restraints')
    for flag in ('guide_type_scale', 'guide_type_clip', 'type_sharpness'):
        if getattr(a, flag) is not None and not typed:
            raise ValueError(f'--{flag} needs --type_restraints or --guide_complementarity_types')
    if a.guide_complementarity_types and not (a.guide_complementarity is not None and a.guide_complementarity > 0):
        raise ValueError('--guide_complementarity_types needs --guide_complementarity with a positive weight')
    if a.comp_unmatched is not None and not a.guide_complementarity_types:
        raise ValueError('--comp_unmatched needs --guide_complementarity_types')
    for flag in ('guide_type_scale', 'guide_type_clip', 'type_sharpness', 'comp_unmatched'):
        v = getattr(a, flag)
        if v is not None and not (v >= 0 and v < float('inf')):
            raise ValueError(f'--{flag} must be finite and not negative, got {v}')
    a.type_restraint_list, a.type_guidance = None, None
    if a.type_restraints is not None:
        from pharmacoforge_amd.pocket_io import read_type_restraints
        a.type_restraint_list = read_type_restraints(a.type_restraints)
        named = [c for _, c, _, _, _ in a.type_restraint_list if c is not None]
        small = [n for n in (a.pharm_sizes or []) if named and n <= max(named)]
        if small:
            raise ValueError(f'--pharm_sizes {small} do not reach center {max(named)} named in --type_restraints')
    if typed:
        a.type_guidance = dict(scale=1.0 if a.guide_type_scale is None else a.guide_type_scale,
                               clip=0.0 if a.guide_type_clip is None else a.guide_type_clip,
                               sharpness=4.0 if a.type_sharpness is None else a.type_sharpness,
                               complementarity=bool(a.guide_complementarity_types),
                               unmatched=0.0 if a.comp_unmatched is None else a.comp_unmatched)
    for flag in ('guide_scale', 'guide_clip', 'guide_family'):
        if getattr(a, flag) is not None and not guided:
            raise ValueError(f'--{flag} needs --avoid_clashes, --guide_complementarity, --type_restraints, --pair_restraints or --min_separation')
    if a.clash_weight is not None and a.avoid_clashes is None:
        raise ValueError('--clash_weight needs --avoid_clashes')
    for flag in ('avoid_clashes', 'clash_weight', 'guide_complementarity', 'guide_scale', 'guide_clip'):
        v = getattr(a, flag)
        if v is not None and not (v >= 0 and v < float('inf')):
            raise ValueError(f'--{flag} must be finite and not negative, got {v}')
    if guided and a.sampler == 'multistep':
        raise ValueError('--sampler multistep takes no guidance: no --avoid_clashes, --guide_complementarity, --type_restraints, --pair_restraints or --min_separation')
    a.pocket_field = None
    if a.avoid_clashes is not None or a.guide_complementarity is not None:
        a.pocket_field = dict(clash_radius=a.avoid_clashes, clash_weight=1.0 if a.clash_weight is None else a.clash_weight,
                              comp_weight=0.0 if a.guide_complementarity is None else a.guide_complementarity)
    a.guide_scale = 1.0 if a.guide_scale is None else a.guide_scale
    a.guide_clip = 0.0 if a.guide_clip is None else a.guide_clip
    a.guide_family = 'wide' if a.guide_family is None else a.guide_family
    if a.dataset_idx_as_start and (a.dataset_idx is None or a.dataset_size is None):
        raise ValueError('--dataset_idx_as_start needs both --dataset_idx and --dataset_size')
    return a


def selected_pockets(args, n_total):
    if args.dataset_idx is None:
        return list(range(n_total if args.dataset_size is None else args.dataset_size))
    if args.dataset_idx_as_start:
        return list(range(args.dataset_idx, args.dataset_idx + args.dataset_size))
    return [args.dataset_idx]


def init_ranks():
    """-> (rank, world, device, process group or None).  RCCL when every rank owns a GPU, gloo for dry runs on fewer."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    from pharmacoforge_amd.sharding import pin_host_threads
    pin_host_threads(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))       # before anything touches the GPU
    ndev = torch.cuda.device_count()
    torch.cuda.set_device(local % ndev)
    device = torch.device('cuda', local % ndev)
    if world == 1:
        return rank, world, device, None
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29551")
    if world <= ndev:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return rank, world, device, dist.group.WORLD


def write_pocket(out_root, dataset, idx, pharms, seconds, trajectories):
    pocket_dir = out_root / f'pocket_{idx}'
    pocket_dir.mkdir(exist_ok=True)
    (pocket_dir / 'sample_time.txt').write_text(f'{seconds:.2f}')
    raw_dir, prot_file, _ = dataset.get_files(idx)
    if prot_file is not None and (Path(raw_dir) / prot_file).exists():
        ref_dir = pocket_dir / 'reference_files'
        ref_dir.mkdir(exist_ok=True)
        shutil.copy(Path(raw_dir) / prot_file, ref_dir / Path(prot_file).name)
    if trajectories:
        for k, ph in enumerate(pharms):
            ph.traj_to_xyz(pocket_dir / f'pharm_{k}_traj.xyz')
    else:
        (pocket_dir / 'pharms.xyz').write_text(''.join(ph.to_xyz_file() for ph in pharms))


def self_rank(pfa, model, library, own, pharms):
    """--screen_self: (rank, sample, sim) of library entry `own` -- the pocket's own ligand pharmacophore -- among the hits of the
    pocket's best sample: the sample (of 1 to 16 centers) most similar to that entry after the superposition; the rank is 1-based
    over the whole library.  None when the ligand is not in the library or no sample can be a query."""
    usable = [k for k, ph in enumerate(pharms) if 1 <= ph.n_ph_centers <= 16]
    if own is None or not usable:
        return None
    hits = model.screen([pharms[k] for k in usable], library, top_k=len(library))
    place = [next(r for r, h in enumerate(hs) if h.entry == own) for hs in hits]
    best = max(range(len(usable)), key=lambda a: (hits[a][place[a]].sim, -a))
    return place[best] + 1, usable[best], hits[best][place[best]].sim


def main(argv=None):
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd.dataset import data_module_from_config
    from pharmacoforge_amd.sharding import shard_by_work
    from generate_pharmacophores import load_model, locate_run

    args = parse_arguments(argv)
    if not torch.cuda.is_available():
        raise SystemExit("test.py needs an MI355X: the denoising kernels have no CPU fallback")
    rank, world, device, group = init_ranks()
    run_dir, ckpt, config = locate_run(args)
    out_root = args.output_dir if args.output_dir is not None else run_dir / 'samples'
    out_root.mkdir(exist_ok=True)
    if rank == 0:
        print(f'{device=}', flush=True)
    torch.manual_seed(args.seed + rank)
    dm = data_module_from_config(config)
    dm.setup('fit' if args.split == 'train' else 'test')
    dataset = dm.train_dataset if args.split == 'train' else dm.val_dataset
    model = load_model(pfa, ckpt, config, device, use_ema=args.use_ema)

    pockets = selected_pockets(args, len(dataset))
    # pockets are independent units; a pocket's cost is its pp edge count times its sample count (sizes 3-8 change it by
    # < 5 %): every rank computes the same greedy assignment, nothing is communicated
    epp = dataset.pp_edge_counts()
    mine = [pockets[j] for j in shard_by_work([float(epp[i] + 1) * args.samples_per_pocket for i in pockets], world)[rank]]
    all_pharms = []
    set_counts = torch.zeros(4, dtype=torch.float64)       # --consensus: pockets, clusters, samples, sum of the samples' mean support
    library, self_rows = None, []
    if args.screen_self:                                   # the split's ligand pharmacophores, uploaded once
        library = pfa.PharmacophoreLibrary.from_dataset(dataset).to(device)
        entry_of = {pocket: k for k, pocket in enumerate(library.index)}
        rank_hist = torch.zeros(len(library) + 1, dtype=torch.float64)      # rank_hist[r]: pockets whose own ligand has rank r (1-based)
        if rank == 0:
            print(f'--screen_self: {len(library)} library entries, {library.dropped} ligand pharmacophores outside 1..32 centers dropped', flush=True)
    for c0 in range(0, len(mine), args.pockets_per_call):
        chunk = mine[c0:c0 + args.pockets_per_call]
        t0 = time.time()
        graphs = [dataset[i] for i in chunk]
        sizes = [list(args.pharm_sizes) or model.pharm_size_dist.sample_uniformly(args.samples_per_pocket).tolist()
                 for _ in chunk]
        coms = torch.stack([g.pharm_x0.mean(dim=0) for g in graphs]) if args.use_ref_pharm_com else None
        with torch.no_grad():
            per_pocket = model.sample(graphs, sizes, max_batch_size=args.max_batch_size, init_pharm_com=coms,
                                      visualize_trajectory=args.visualize_trajectory, sample_steps=args.sample_steps,
                                      sampler=args.sampler, eta=args.eta, spacing=args.spacing,
                                      pocket_field=None if args.pocket_field is None else pfa.PocketField(**args.pocket_field),
                                      guide_scale=args.guide_scale, guide_clip=args.guide_clip, guide_family=args.guide_family,
                                      type_restraints=[args.type_restraint_list] * len(graphs) if args.type_restraint_list else None,
                                      type_guidance=None if args.type_guidance is None else pfa.TypeGuidance(**args.type_guidance),
                                      pair_restraints=[args.pair_restraint_list] * len(graphs) if args.pair_restraint_list else None,
                                      min_separation=args.min_separation, separation_weight=args.separation_weight,
                                      consensus=args.consensus)
        sets = None
        if args.consensus:
            per_pocket, sets = per_pocket
        seconds = (time.time() - t0) / len(chunk)
        for idx, pharms in zip(chunk, per_pocket):
            write_pocket(out_root, dataset, idx, pharms, seconds, args.visualize_trajectory)
            all_pharms += pharms
            if sets is not None and sets[chunk.index(idx)] is not None:
                sset = sets[chunk.index(idx)]
                (out_root / f'pocket_{idx}' / 'consensus.xyz').write_text(sset.consensus_xyz())
                (out_root / f'pocket_{idx}' / 'clusters.tsv').write_text(sset.clusters_tsv())
                set_counts += torch.tensor([1.0, len(sset.clusters), sset.n_samples, sum(sset.mean_support())], dtype=torch.float64)
            if library is not None:
                r = self_rank(pfa, model, library, entry_of.get(idx), pharms)
                if r is not None:
                    rank_hist[r[0]] += 1
                    self_rows.append(f'{idx}\t{r[0]}\t{r[1]}\t{r[2]:.6f}')
            if args.avoid_clashes is not None and rank == 0:       # the final clash energy and clashing pairs of every sample
                from pharmacoforge_amd.analysis import clash_energy
                cl = [clash_energy(ph.ph_coords, ph.g.prot_x, args.avoid_clashes, args.pocket_field['clash_weight']) for ph in pharms]
                print(f'pocket {idx}: clash energy per sample ' + ' '.join(f'{e:.3g}' for e, _ in cl)
                      + '; clashing pairs ' + ' '.join(str(c) for _, c in cl), flush=True)
            if args.type_restraint_list and rank == 0:             # the final type energy of every sample
                from pharmacoforge_amd.analysis import type_restraint_energy
                rows = [(model._type_index(t), c, p, r, w) for t, c, p, r, w in args.type_restraint_list]
                te = [type_restraint_energy(ph.ph_coords, ph.g.pharm_h0, rows, args.type_guidance['sharpness']) for ph in pharms]
                print(f'pocket {idx}: type energy per sample ' + ' '.join(f'{e:.3g}' for e in te), flush=True)
            if (args.pair_restraint_list or args.min_separation is not None) and rank == 0:     # the final pair energy of every sample
                print(f'pocket {idx}: pair energy per sample ' + ' '.join(f'{ph.pair_energy:.3g}' for ph in pharms)
                      + '; violated pairs ' + ' '.join(str(ph.pair_violations) for ph in pharms), flush=True)
        if rank == 0:
            print(f'pockets {chunk[0]}..{chunk[-1]}: {seconds:.3f} s per pocket, '
                  f'{seconds / max(args.samples_per_pocket, 1):.4f} s per pharmacophore', flush=True)
    if args.metrics:
        analyzer = pfa.SampleAnalyzer()
        metrics = analyzer.analyze(all_pharms, process_group=group, device=device)
        freqs = analyzer.pharm_feat_freq(all_pharms, process_group=group, device=device)
        if rank == 0:
            print(metrics)
            (out_root / 'metrics.txt').write_text('\n'.join(f'{k}: {v:.3f}' for k, v in metrics.items()))
            with open(out_root / 'metrics.pkl', 'wb') as f:
                pickle.dump(metrics, f)
            (out_root / f'pharm_counts_{args.dataset_idx}.txt').write_text(str(freqs.tolist()))
    if args.consensus:
        if group is not None:
            from pharmacoforge_amd.analysis import _allreduce_sum
            set_counts = _allreduce_sum(set_counts, group, device)
        summary = {'clusters_per_pocket': float(set_counts[1] / set_counts[0]) if set_counts[0] > 0 else 0.0,
                   'mean_support': float(set_counts[3] / set_counts[2]) if set_counts[2] > 0 else 0.0}
        if rank == 0:
            print(summary)
            (out_root / 'consensus_summary.txt').write_text('\n'.join(f'{k}: {v:.3f}' for k, v in summary.items()))
    if library is not None:
        (out_root / f'screen_self_rank{rank}.tsv' if world > 1 else out_root / 'screen_self.tsv').write_text(
            'pocket\tself_rank\tbest_sample\tsim\n' + ''.join(row + '\n' for row in self_rows))
        if group is not None:
            from pharmacoforge_amd.analysis import _allreduce_sum
            rank_hist = _allreduce_sum(rank_hist, group, device)
        n = float(rank_hist.sum())
        below = torch.cumsum(rank_hist, 0)
        summary = {'self_rank_median': float(torch.nonzero(below >= n / 2)[0]) if n > 0 else 0.0,        # the lower median
                   'self_top10': float(rank_hist[:11].sum() / n) if n > 0 else 0.0, 'pockets_ranked': n}
        if rank == 0:
            print(summary)
            (out_root / 'screen_summary.txt').write_text('\n'.join(f'{k}: {v:.3f}' for k, v in summary.items()))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
