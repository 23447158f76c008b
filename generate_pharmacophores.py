#!/usr/bin/env python3
"""Pharmacophore sampling for one receptor pocket on the MI355X library.

Command-line contract of the reference's generate_pharmacophores.py (flag names, types and defaults of its :29-46; the
run-directory convention <run>/config.y[a]ml + <run>/checkpoints/last.ckpt; the output tree
<output_dir>/<receptor>/{pharms.xyz | pharm_<i>_traj.xyz, pocket.pdb, sample_time.txt, sample_time.pkl,
reference_files/}), so scripts written against the reference keep working.  Everything behind the flags is this
repository's: receptor parsing without Biopython / rdkit (pharmacoforge_amd.pocket_io: PDB or mmCIF receptor, SDF
ligand), PharmacophoreDiff.sample_given_receptor -> pf_sample (the whole reverse process enqueued on the GPU)."""
import argparse
import pickle
import shutil
import sys
import time
from pathlib import Path

import torch
import yaml

# (flag, argparse keywords): names / types / defaults are the reference's, the descriptions are ours
_FLAGS = [
    ('receptor_file', dict(type=Path, help='receptor structure, .pdb or .cif / .mmcif')),
    ('--ref_ligand_file', dict(type=Path, help='SDF ligand; residues with an atom within the config\'s pocket_cutoff of it form the pocket')),
    ('--residue_list', dict(nargs='+', type=str, default=[], help='pocket given explicitly instead: entries CHAIN:RESSEQ, e.g. A:105 A:106')),
    ('--ckpt', dict(type=Path, default=None, help='checkpoint file at <run>/checkpoints/<name>.ckpt (the config is looked up in <run>)')),
    ('--model_dir', dict(type=Path, default=None, help='training run directory <run>; its checkpoints/last.ckpt is loaded')),
    ('--samples_per_pocket', dict(type=int, default=1, help='how many pharmacophores to draw')),
    ('--pharm_sizes', dict(nargs='+', type=int, default=[], help='centers per pharmacophore, one integer per sample (default: uniform 3..8)')),
    ('--output_dir', dict(type=str, default='generated_pharms/', help='root of the output tree')),
    ('--receptor_name', dict(type=str, default=None, help='sub-directory name (default: receptor file stem)')),
    ('--max_batch_size', dict(type=int, default=128, help='graphs per device batch')),
    ('--seed', dict(type=int, default=42, help='torch seed of the run')),
    ('--use_ref_lig_com', dict(action='store_true', help='start the centers at the ligand\'s mean position instead of the pocket\'s')),
    ('--visualize_trajectory', dict(action='store_true', help='write every denoising frame, one xyz file per sample')),
    ('--pinned_centers', dict(type=Path, default=None, help='one xyz frame in the pharms.xyz format (elements P S F N O C): centers every sample must contain; the model places the others around them')),
    ('--pin_what', dict(choices=['both', 'position', 'type'], default='both', help='what of the pinned centers is fixed')),
    ('--pin_resamples', dict(type=int, default=None, help='with --pinned_centers: denoise every stretch of --pin_jump levels this many times, re-noising it in between, so that the free centers can react to the pinned ones (default 1: no resampling; a run costs about this many times the steps)')),
    ('--pin_jump', dict(type=int, default=None, help='with --pinned_centers: levels per resampled stretch (default 10)')),
    ('--restraints', dict(type=Path, default=None, help='guided sampling: a text file with one restraint per line, "attract|repel x y z radius weight [center|*]" in the receptor\'s frame (# starts a comment): keep centers out of / pull a center into a sphere; a guided step costs several times a default one')),
    ('--type_restraints', dict(type=Path, default=None, help='guided sampling of the types: a text file with one type restraint per line, "type NAME|INDEX x y z radius weight [center|*]" in the receptor\'s frame (# starts a comment): a center inside the sphere takes that type or is pushed out (radius 0: no spatial condition); with an attract restraint on the same sphere: "a center of this type within radius of the point"')),
    ('--guide_type_scale', dict(type=float, default=None, help='with --type_restraints: strength of the guidance of the feature rows (default 1)')),
    ('--guide_type_clip', dict(type=float, default=None, help='with --type_restraints: largest Euclidean norm of a feature row\'s shift per step (default 0: no clip)')),
    ('--type_sharpness', dict(type=float, default=None, help='with --type_restraints: sharpness of the soft type assignment on one-hot-scaled features (default 4)')),
    ('--pair_restraints', dict(type=Path, default=None, help='guided sampling: a text file with one pair restraint per line, "pair I|* J|* LO HI|inf WEIGHT" (# starts a comment): the two centers (*: every center) of one sample are held LO to HI angstroms apart')),
    ('--min_separation', dict(type=float, default=None, metavar='D', help='guided sampling: no two centers of a sample closer than D angstroms (the pair restraint "* * D inf W"); every batch then runs guided, which costs several times a default step')),
    ('--separation_weight', dict(type=float, default=None, metavar='W', help='with --min_separation: weight of its energy (default 1)')),
    ('--avoid_clashes', dict(type=float, nargs='?', const=2.0, default=None, metavar='R', help='guided sampling: keep the centers out of the pocket\'s own atoms -- a center of the predicted clean sample within R angstroms of an atom (default 2.0) is pushed out; every batch then runs guided, which costs several times a default step')),
    ('--clash_weight', dict(type=float, default=None, help='with --avoid_clashes: weight of the clash energy (default 1)')),
    ('--guide_scale', dict(type=float, default=None, help='with --restraints or --avoid_clashes: strength of the guidance (default 1)')),
    ('--guide_clip', dict(type=float, default=None, help='with --restraints or --avoid_clashes: largest shift of a center per step in angstroms (default 0: no clip)')),
    ('--guide_family', dict(choices=['wide', 'tuned'], default=None, help='with --restraints or --avoid_clashes: the kernels of a guided step\'s training forward and input gradients -- wide (default; every model width) or tuned (models of n_hidden_scalars 128 / vector_size 16: the tuned gradient kernels)')),
    ('--seed_pharmacophore', dict(type=Path, default=None, help='seeded sampling: one xyz frame in the pharms.xyz format; every sample is a variation of it (the frame is noised forward to --seed_level and only the steps below that level are run)')),
    ('--seed_level', dict(type=int, default=None, help='with --seed_pharmacophore: the level 1..T the seed is noised to; small: close analogues, large: loose ones')),
    ('--seed_keep', dict(type=str, default=None, help='with --seed_pharmacophore: comma-separated indices of seed centers that stay fixed in position and type, e.g. 0,2')),
    ('--sample_steps', dict(type=int, default=None, help='few-step sampling: visit only this many of the T levels (from --seed_level down in a seeded run); how good such samples are depends on the trained weights')),
    ('--sampler', dict(choices=['ancestral', 'ddim', 'multistep'], default=None, help='with --sample_steps: ancestral (default; the posterior between the visited levels), ddim (--eta, default 0: no injected noise) or multistep (second-order multistep solver; composes with --seed_pharmacophore only)')),
    ('--eta', dict(type=float, default=None, help='with --sample_steps --sampler ddim: share of the posterior noise injected, 0..1 (default 0)')),
    ('--spacing', dict(choices=['uniform', 'quadratic', 'logsnr'], default=None, help='with --sample_steps: how the visited levels are spread (default uniform; quadratic is denser near level 0, logsnr uniform in the log signal-to-noise ratio)')),
    ('--score_samples', dict(type=int, default=None, help='score the drawn samples with the model at this many noise levels (stratified over 1..T) and write scores.tsv, one line per sample in the order of pharms.xyz; lower per-center score is better')),
    ('--keep_best', dict(type=int, default=None, help='with --score_samples: write only this many samples, best (lowest per-center score) first')),
    ('--score_pharmacophores', dict(type=Path, default=None, help='no sampling: score every frame of this file (pharms.xyz format) against the pocket and write scores.tsv; --score_samples gives the number of levels (default: every level); with the --seed, --score_samples, --score_weighting and --max_batch_size of the run that wrote the file, and its frames in their order, this reproduces that run\'s scores.tsv (the noise of a score is drawn per device batch)')),
    ('--score_weighting', dict(choices=['uniform', 'vlb'], default=None, help='weights of the levels in a score: uniform (default; the per-graph training loss) or vlb (the diffusion terms of the variational bound)')),
    ('--consensus', dict(action='store_true', help='analyse the drawn samples as a set: write consensus.xyz (one frame per cluster of similar samples, largest first: the cluster centroid\'s centers at the mean of their partners in the members, with the share of members that have one as a fifth column) and clusters.tsv (sample index, cluster, is-centroid, neighbour count, mean center support)')),
    ('--consensus_sigma', dict(type=float, default=None, metavar='A', help='with --consensus / --consensus_of / --keep_diverse: width of the Gaussians of the similarity between two samples, angstroms (default 1.0)')),
    ('--consensus_tolerance', dict(type=float, default=None, metavar='A', help='with --consensus / --consensus_of: two centers of one type within this distance are the same center (default 1.5)')),
    ('--consensus_threshold', dict(type=float, default=None, metavar='S', help='with --consensus / --consensus_of: samples at least this similar (0..1) are neighbours in the clustering (default 0.5)')),
    ('--min_support', dict(type=float, default=None, metavar='F', help='with --consensus / --consensus_of: consensus.xyz lists the centers found in at least this share of a cluster\'s members (default 0.5)')),
    ('--keep_diverse', dict(type=int, default=None, metavar='K', help='write only K samples chosen by max-min selection on the similarity (each next one the least similar to those chosen, starting from the largest cluster\'s centroid); with --keep_best: the best N first, then K diverse among them')),
    ('--consensus_of', dict(type=Path, default=None, metavar='FILE', help='no sampling, no receptor_file, no checkpoint: analyse the frames of this file (pharms.xyz format, all of one pocket) as --consensus does and write consensus.xyz and clusters.tsv')),
    ('--screen_library', dict(type=Path, default=None, metavar='FILE', help='screen a pharmacophore library (the frames of this file, pharms.xyz format, 1 to 32 centers each) against the written samples, or with --consensus against the consensus pharmacophores: every entry is superposed rigidly onto every query (proper rotations, exact types, at most 16 query centers); writes hits.tsv (query, rank, entry name, sim, matched, n_q) and hits_aligned.xyz (the hit entries in the pocket\'s frame, one frame per hit)')),
    ('--screen_top', dict(type=int, default=None, metavar='K', help='with --screen_library: hits listed per query (default 10)')),
    ('--screen_min_match', dict(type=float, default=None, metavar='F', help='with --screen_library: only entries that match at least this share (0..1) of the query\'s centers qualify (default 0)')),
    ('--screen_sigma', dict(type=float, default=None, metavar='A', help='with --screen_library: width of the Gaussians of the similarity, angstroms (default 1.0)')),
    ('--screen_tolerance', dict(type=float, default=None, metavar='A', help='with --screen_library: a query center is matched by a same-type entry center within this distance (default 1.5)')),
    ('--screen_refine', dict(type=int, default=None, metavar='R', help='with --screen_library: refinement rounds behind the best three-point superposition, 0..16 (default 4)')),
    ('--screen_queries', dict(type=Path, default=None, metavar='FILE', help='with --screen_library; no sampling, no receptor_file, no checkpoint: the frames of this file (pharms.xyz format) are the queries')),
    ('--metrics', dict(action='store_true', help='print the validity of the samples against receptor pharmacophore features')),
    ('--use_ema', dict(action='store_true', help="sample from the checkpoint's EMA weights (its 'ema_state_dict', written by train.py with ema_decay set) instead of the training weights")),
]


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    argv = sys.argv[1:] if argv is None else list(argv)
    file_only = any(str(v) == f or str(v).startswith(f + '=') for v in argv for f in ('--consensus_of', '--screen_queries'))
    for flag, kw in _FLAGS:
        if flag == 'receptor_file' and file_only:           # --consensus_of reads no receptor: the positional may be left out
            kw = dict(kw, nargs='?', default=None)
        parser.add_argument(flag, **kw)
    a = parser.parse_args(argv)
    analysed = a.consensus or a.consensus_of is not None
    for flag in ('consensus_sigma', 'consensus_tolerance', 'consensus_threshold', 'min_support'):
        v = getattr(a, flag)
        if v is not None and not (analysed or (flag == 'consensus_sigma' and a.keep_diverse is not None)):
            parser.error(f'--{flag} needs --consensus or --consensus_of' + (' or --keep_diverse' if flag == 'consensus_sigma' else ''))
        if v is not None and not (v >= 0 and v < float('inf')):
            parser.error(f'--{flag} must be finite and not negative, got {v}')
    if a.consensus_sigma is not None and not a.consensus_sigma > 0:
        parser.error(f'--consensus_sigma must be positive, got {a.consensus_sigma}')
    for flag in ('consensus_threshold', 'min_support'):
        if getattr(a, flag) is not None and getattr(a, flag) > 1:
            parser.error(f'--{flag} must lie in 0..1, got {getattr(a, flag)}')
    a.consensus_sigma = 1.0 if a.consensus_sigma is None else a.consensus_sigma
    a.consensus_tolerance = 1.5 if a.consensus_tolerance is None else a.consensus_tolerance
    a.consensus_threshold = 0.5 if a.consensus_threshold is None else a.consensus_threshold
    a.min_support = 0.5 if a.min_support is None else a.min_support
    if a.keep_diverse is not None and a.keep_diverse < 1:
        parser.error(f'--keep_diverse must be at least 1, got {a.keep_diverse}')
    for flag in ('screen_top', 'screen_min_match', 'screen_sigma', 'screen_tolerance', 'screen_refine', 'screen_queries'):
        if getattr(a, flag) is not None and a.screen_library is None:
            parser.error(f'--{flag} needs --screen_library')
    a.screen_top = 10 if a.screen_top is None else a.screen_top
    a.screen_min_match = 0.0 if a.screen_min_match is None else a.screen_min_match
    a.screen_sigma = 1.0 if a.screen_sigma is None else a.screen_sigma
    a.screen_tolerance = 1.5 if a.screen_tolerance is None else a.screen_tolerance
    a.screen_refine = 4 if a.screen_refine is None else a.screen_refine
    if a.screen_top < 1:
        parser.error(f'--screen_top must be at least 1, got {a.screen_top}')
    if not 0.0 <= a.screen_min_match <= 1.0:
        parser.error(f'--screen_min_match must lie in 0..1, got {a.screen_min_match}')
    if not (0 < a.screen_sigma < float('inf')):
        parser.error(f'--screen_sigma must be positive and finite, got {a.screen_sigma}')
    if not (0 <= a.screen_tolerance < float('inf')):
        parser.error(f'--screen_tolerance must be finite and not negative, got {a.screen_tolerance}')
    if not 0 <= a.screen_refine <= 16:
        parser.error(f'--screen_refine must lie in 0..16, got {a.screen_refine}')
    a.screen_lib, a.screen_query_frames = None, None
    if a.screen_library is not None:
        from pharmacoforge_amd.analysis import PharmacophoreLibrary, read_pharmacophores
        try:
            a.screen_lib = PharmacophoreLibrary.from_file(a.screen_library)
            if a.screen_queries is not None:
                a.screen_query_frames = read_pharmacophores(a.screen_queries)
        except (OSError, ValueError) as e:
            parser.error(f'--screen_library / --screen_queries: {e}')
        if len(a.screen_lib) == 0:
            parser.error(f'--screen_library: no frame of {a.screen_library} has 1 to 32 centers')
        if a.visualize_trajectory or a.score_pharmacophores is not None:
            parser.error('--screen_library together with --visualize_trajectory / --score_pharmacophores: no pharms.xyz is written to screen')
    if a.screen_query_frames is not None:
        given = [f for f in ('receptor_file', '--ckpt', '--model_dir', '--ref_ligand_file', '--residue_list', '--samples_per_pocket', '--pharm_sizes',
                             '--pinned_centers', '--restraints', '--type_restraints', '--pair_restraints', '--min_separation', '--avoid_clashes',
                             '--seed_pharmacophore', '--sample_steps', '--score_samples', '--use_ref_lig_com', '--metrics', '--use_ema', '--consensus',
                             '--consensus_of', '--keep_diverse')
                 if getattr(a, f.lstrip('-')) not in (parser.get_default(f.lstrip('-')), None)]
        if given:
            parser.error(f'--screen_queries samples nothing and reads no receptor or checkpoint: {" ".join(given)} make no sense with it')
        a.consensus_frames = None
        return a
    if a.screen_library is not None and a.consensus_of is not None:
        parser.error('--screen_library together with --consensus_of: screen the consensus.xyz it writes with --screen_queries')
    if a.keep_diverse is not None and a.visualize_trajectory:
        parser.error('--keep_diverse together with --visualize_trajectory: trajectories are written per sample index')
    if a.keep_diverse is not None and (a.score_pharmacophores is not None or a.consensus_of is not None):
        parser.error('--keep_diverse together with --score_pharmacophores / --consensus_of: nothing is sampled, every frame is listed')
    a.consensus_frames = None
    if a.consensus_of is not None:
        given = [f for f in ('receptor_file', '--ckpt', '--model_dir', '--ref_ligand_file', '--residue_list', '--samples_per_pocket', '--pharm_sizes',
                             '--visualize_trajectory', '--pinned_centers', '--restraints', '--type_restraints', '--pair_restraints',
                             '--min_separation', '--avoid_clashes', '--seed_pharmacophore', '--sample_steps', '--score_samples',
                             '--score_pharmacophores', '--use_ref_lig_com', '--metrics', '--use_ema', '--consensus')
                 if getattr(a, f.lstrip('-')) not in (parser.get_default(f.lstrip('-')), None)]
        if given:
            parser.error(f'--consensus_of samples nothing and reads no receptor or checkpoint: {" ".join(given)} make no sense with it')
        from pharmacoforge_amd.analysis import read_pharmacophores
        try:
            a.consensus_frames = read_pharmacophores(a.consensus_of)
        except (OSError, ValueError) as e:
            parser.error(f'--consensus_of: {e}')
        big = [i for i, (x, _) in enumerate(a.consensus_frames) if len(x) > 64]
        if big:
            parser.error(f'--consensus_of: frame(s) {big} have more than 64 centers')
        if len(a.consensus_frames) > 1024:
            parser.error(f'--consensus_of: {len(a.consensus_frames)} frames (a set has at most 1024 samples)')
        return a
    if (a.consensus or a.keep_diverse is not None) and a.samples_per_pocket > 1024:
        parser.error(f'--consensus / --keep_diverse: --samples_per_pocket {a.samples_per_pocket} (a set has at most 1024 samples)')
    if a.consensus and a.score_pharmacophores is not None:
        parser.error('--consensus together with --score_pharmacophores: nothing is sampled; --consensus_of analyses a file')
    for flag in ('pin_resamples', 'pin_jump'):
        v = getattr(a, flag)
        if v is not None and a.pinned_centers is None and a.seed_keep is None:     # (a seeded run with --seed_keep is a pinned run)
            parser.error(f'--{flag} needs --pinned_centers')
        if v is not None and v < 1:
            parser.error(f'--{flag} must be at least 1, got {v}')
    paired = a.pair_restraints is not None or a.min_separation is not None
    guided = a.restraints is not None or a.avoid_clashes is not None or a.type_restraints is not None or paired
    if a.separation_weight is not None and a.min_separation is None:
        parser.error('--separation_weight needs --min_separation')
    for flag in ('min_separation', 'separation_weight'):
        v = getattr(a, flag)
        if v is not None and not (v >= 0 and v < float('inf')):
            parser.error(f'--{flag} must be finite and not negative, got {v}')
    if paired and a.pin_resamples is not None and a.pin_resamples > 1:
        parser.error('--pair_restraints / --min_separation together with --pin_resamples > 1: guidance with resampling jumps is not supported')
    a.separation_weight = 1.0 if a.separation_weight is None else a.separation_weight
    for flag in ('guide_type_scale', 'guide_type_clip', 'type_sharpness'):
        v = getattr(a, flag)
        if v is not None and a.type_restraints is None:
            parser.error(f'--{flag} needs --type_restraints')
        if v is not None and not (v >= 0 and v < float('inf')):
            parser.error(f'--{flag} must be finite and not negative, got {v}')
    if a.type_restraints is not None and a.pin_resamples is not None and a.pin_resamples > 1:
        parser.error('--type_restraints together with --pin_resamples > 1: guidance with resampling jumps is not supported')
    a.guide_type_scale = 1.0 if a.guide_type_scale is None else a.guide_type_scale
    a.guide_type_clip = 0.0 if a.guide_type_clip is None else a.guide_type_clip
    a.type_sharpness = 4.0 if a.type_sharpness is None else a.type_sharpness
    for flag in ('guide_scale', 'guide_clip'):
        v = getattr(a, flag)
        if v is not None and not guided:
            parser.error(f'--{flag} needs --restraints, --avoid_clashes, --type_restraints, --pair_restraints or --min_separation')
        if v is not None and not v >= 0:
            parser.error(f'--{flag} must not be negative, got {v}')
    if a.guide_family is not None and not guided:
        parser.error('--guide_family needs --restraints, --avoid_clashes, --type_restraints, --pair_restraints or --min_separation')
    if a.clash_weight is not None and a.avoid_clashes is None:
        parser.error('--clash_weight needs --avoid_clashes')
    for flag in ('avoid_clashes', 'clash_weight'):
        v = getattr(a, flag)
        if v is not None and not (v >= 0 and v < float('inf')):
            parser.error(f'--{flag} must be finite and not negative, got {v}')
    a.clash_weight = 1.0 if a.clash_weight is None else a.clash_weight
    if a.avoid_clashes is not None and a.pin_resamples is not None and a.pin_resamples > 1:
        parser.error('--avoid_clashes together with --pin_resamples > 1: guidance with resampling jumps is not supported')
    a.guide_family = 'wide' if a.guide_family is None else a.guide_family
    a.guide_scale = 1.0 if a.guide_scale is None else a.guide_scale
    a.guide_clip = 0.0 if a.guide_clip is None else a.guide_clip
    if a.restraints is not None and a.pin_resamples is not None and a.pin_resamples > 1:
        parser.error('--restraints together with --pin_resamples > 1: guidance with resampling jumps is not supported')
    a.seed_centers = None
    a.seed_keep_list = None
    if a.seed_pharmacophore is None:
        for flag in ('seed_level', 'seed_keep'):
            if getattr(a, flag) is not None:
                parser.error(f'--{flag} needs --seed_pharmacophore')
    else:
        if a.seed_level is None:
            parser.error('--seed_pharmacophore needs --seed_level')
        if a.seed_level < 1:
            parser.error(f'--seed_level must be at least 1, got {a.seed_level}')
        if a.pinned_centers is not None:
            parser.error('--seed_pharmacophore together with --pinned_centers: use --seed_keep')
        from pharmacoforge_amd.analysis import read_pinned_centers
        a.seed_centers = read_pinned_centers(a.seed_pharmacophore)
        n_seed = len(a.seed_centers[1])
        if any(n != n_seed for n in a.pharm_sizes):
            parser.error(f'--pharm_sizes {a.pharm_sizes} differ from the {n_seed} centers of --seed_pharmacophore')
        if a.seed_keep is not None:
            try:
                a.seed_keep_list = [int(v) for v in a.seed_keep.split(',') if v.strip()]
            except ValueError:
                parser.error(f'--seed_keep is a comma-separated list of center indices, got {a.seed_keep!r}')
            bad = [i for i in a.seed_keep_list if not 0 <= i < n_seed]
            if bad:
                parser.error(f'--seed_keep {bad} outside the {n_seed} centers of --seed_pharmacophore')
    if a.sample_steps is None:
        for flag in ('sampler', 'eta', 'spacing'):
            if getattr(a, flag) is not None:
                parser.error(f'--{flag} needs --sample_steps')
    else:
        if a.sample_steps < 1:
            parser.error(f'--sample_steps must be at least 1, got {a.sample_steps}')
        if a.seed_level is not None and a.sample_steps > a.seed_level:
            parser.error(f'--sample_steps {a.sample_steps} exceeds --seed_level {a.seed_level}')
        if a.pin_resamples is not None and a.pin_resamples > 1:
            parser.error('--sample_steps together with --pin_resamples > 1: resampling jumps over a strided plan are not supported')
        if a.eta is not None and a.sampler != 'ddim':
            parser.error('--eta needs --sampler ddim')
        if a.eta is not None and not 0.0 <= a.eta <= 1.0:
            parser.error(f'--eta must lie in 0..1, got {a.eta}')
        if a.sampler == 'multistep' and (a.pinned_centers is not None or guided or a.seed_keep is not None):
            parser.error('--sampler multistep composes with --seed_pharmacophore only: no --pinned_centers, --seed_keep, --restraints, --type_restraints, --pair_restraints, --min_separation or --avoid_clashes')
    a.pin_resamples = 1 if a.pin_resamples is None else a.pin_resamples
    a.pin_jump = 10 if a.pin_jump is None else a.pin_jump
    for flag in ('score_samples', 'keep_best'):
        v = getattr(a, flag)
        if v is not None and v < 1:
            parser.error(f'--{flag} must be at least 1, got {v}')
    if a.keep_best is not None and a.score_samples is None:
        parser.error('--keep_best needs --score_samples')
    if a.keep_best is not None and a.score_pharmacophores is not None:
        parser.error('--keep_best together with --score_pharmacophores: nothing is sampled, scores.tsv lists every frame')
    if a.keep_best is not None and a.visualize_trajectory:
        parser.error('--keep_best together with --visualize_trajectory: trajectories are written per sample index')
    if a.score_weighting is not None and a.score_samples is None and a.score_pharmacophores is None:
        parser.error('--score_weighting needs --score_samples or --score_pharmacophores')
    a.score_weighting = 'uniform' if a.score_weighting is None else a.score_weighting
    a.score_frames = None
    if a.score_pharmacophores is not None:
        given = [f for f in ('--samples_per_pocket', '--pharm_sizes', '--visualize_trajectory', '--pinned_centers', '--restraints',
                             '--type_restraints', '--pair_restraints', '--min_separation',
                             '--seed_pharmacophore', '--use_ref_lig_com', '--metrics')
                 if getattr(a, f[2:]) not in (parser.get_default(f[2:]), None)]
        if given:
            parser.error(f'--score_pharmacophores samples nothing: {" ".join(given)} make no sense with it')
        from pharmacoforge_amd.analysis import read_pharmacophores
        try:
            a.score_frames = read_pharmacophores(a.score_pharmacophores)
        except (OSError, ValueError) as e:
            parser.error(f'--score_pharmacophores: {e}')
        big = [i for i, (x, _) in enumerate(a.score_frames) if len(x) > 64]
        if big:
            parser.error(f'--score_pharmacophores: frame(s) {big} have more than 64 centers')
    problems = []
    if (a.ckpt is None) == (a.model_dir is None):
        problems.append('give exactly one of --ckpt and --model_dir')
    if a.pharm_sizes and len(a.pharm_sizes) != a.samples_per_pocket:
        problems.append(f'--pharm_sizes lists {len(a.pharm_sizes)} sizes for --samples_per_pocket {a.samples_per_pocket}')
    if a.ref_ligand_file is None and not a.residue_list:
        problems.append('the pocket is undefined: pass --ref_ligand_file or --residue_list')
    a.pinned = None
    if a.pinned_centers is not None:
        from pharmacoforge_amd.analysis import read_pinned_centers
        a.pinned = read_pinned_centers(a.pinned_centers)
        k = len(a.pinned[1])
        small = [n for n in a.pharm_sizes if n < k]
        if small:
            problems.append(f'--pharm_sizes {small} below the {k} centers of --pinned_centers')
    a.restraint_list = None
    if a.restraints is not None:
        from pharmacoforge_amd.pocket_io import read_restraints
        a.restraint_list = read_restraints(a.restraints)
        named = [c for _, c, _, _, _ in a.restraint_list if c is not None]
        small = [n for n in a.pharm_sizes if named and n <= max(named)]
        if small:
            problems.append(f'--pharm_sizes {small} do not reach center {max(named)} named in --restraints')
    a.type_restraint_list = None
    if a.type_restraints is not None:
        from pharmacoforge_amd.pocket_io import read_type_restraints
        a.type_restraint_list = read_type_restraints(a.type_restraints)
        named = [c for _, c, _, _, _ in a.type_restraint_list if c is not None]
        small = [n for n in a.pharm_sizes if named and n <= max(named)]
        if small:
            problems.append(f'--pharm_sizes {small} do not reach center {max(named)} named in --type_restraints')
    a.pair_restraint_list = None
    if a.pair_restraints is not None:
        from pharmacoforge_amd.pocket_io import read_pair_restraints
        a.pair_restraint_list = read_pair_restraints(a.pair_restraints)
        named = [c for i, j, _, _, _ in a.pair_restraint_list for c in (i, j) if c is not None]
        small = [n for n in a.pharm_sizes if named and n <= max(named)]
        if small:
            problems.append(f'--pharm_sizes {small} do not reach center {max(named)} named in --pair_restraints')
    if problems:
        raise ValueError('; '.join(problems))
    if a.ref_ligand_file is not None and a.residue_list:
        print('note: --residue_list is ignored because --ref_ligand_file defines the pocket', file=sys.stderr)
    return a


def pinned_sizes(sizes, k, what='pinned centers'):
    """Sizes drawn uniformly may fall below the k pinned centers (or the centers --restraints names): those are raised to k, with a note."""
    sizes = [int(n) for n in sizes]
    raised = sum(n < k for n in sizes)
    if raised:
        print(f'note: {raised} drawn size(s) below the {k} {what} raised to {k}', file=sys.stderr)
    return [max(n, k) for n in sizes]


def locate_run(args):
    """-> (run directory, checkpoint file, parsed config)."""
    if args.ckpt is not None:
        run_dir, ckpt = args.ckpt.parent.parent, args.ckpt
    else:
        run_dir, ckpt = args.model_dir, args.model_dir / 'checkpoints' / 'last.ckpt'
    for name in ('config.yaml', 'config.yml'):
        if (run_dir / name).exists():
            with open(run_dir / name) as f:
                return run_dir, ckpt, yaml.load(f, Loader=yaml.FullLoader)
    raise FileNotFoundError(f'{run_dir} holds neither config.yaml nor config.yml')


def load_model(pfa, ckpt, config, device, use_ema=False):
    try:
        model = pfa.PharmacophoreDiff.load_from_checkpoint(ckpt)
    except TypeError:              # checkpoints written before ph_type_map became a hyper-parameter
        model = pfa.PharmacophoreDiff.load_from_checkpoint(ckpt, ph_type_map=config['dataset']['ph_type_map'])
    if use_ema:
        model.load_ema_weights(ckpt)
        print(f"sampling from the EMA weights of {ckpt}", flush=True)
    return model.to(device).eval()


def score_frames(pfa, model, pocket, frames, args):
    """PharmacophoreScore of every (positions, types) frame against the pocket: --score_samples levels stratified over 1..T (every
    level without it), --score_weighting, noise seeded by --seed."""
    T = model.n_timesteps
    k = T if args.score_samples is None else min(args.score_samples, T)
    with torch.no_grad():
        return model.score([pocket], [frames], levels=pfa.schedule.score_levels(T, k), weighting=args.score_weighting, seed=args.seed,
                           max_batch_size=args.max_batch_size)[0]


def write_scores(path, indices, scores, clashes=None, type_energies=None, pair_energies=None):
    """scores.tsv: one line per pharmacophore, in the order of pharms.xyz (or of the scored file).  clashes (a pocket field was on):
    per pharmacophore (final clash energy, clashing (center, atom) pairs), two more columns; type_energies (type restraints were
    given): per pharmacophore the final type energy, one more column; pair_energies (pair restraints or a minimum separation were
    given): per pharmacophore the final pair energy, one more column"""
    head = ('index', 'centers', 'total', 'per_center', 'pos', 'feat', 'position_error', 'type_accuracy')
    lines = ['\t'.join(head + (('clash_energy', 'clashes') if clashes is not None else ())
                       + (('type_energy',) if type_energies is not None else ())
                       + (('pair_energy',) if pair_energies is not None else ()))]
    for k, (i, s) in enumerate(zip(indices, scores)):
        row = (str(i), str(s.n_centers), f'{s.total:.6g}', f'{s.per_center:.6g}', f'{s.pos:.6g}', f'{s.feat:.6g}',
               f'{s.position_error:.6g}', f'{s.type_accuracy:.4f}')
        if clashes is not None:
            row += (f'{clashes[k][0]:.6g}', str(clashes[k][1]))
        if type_energies is not None:
            row += (f'{type_energies[k]:.6g}',)
        if pair_energies is not None:
            row += (f'{pair_energies[k]:.6g}',)
        lines.append('\t'.join(row))
    Path(path).write_text('\n'.join(lines) + '\n')


def analyse_set(pfa, frames, args, engine=None):
    """The SampleSet of (positions, types) frames of one pocket under the --consensus_* options: on the engine's device, or on
    the host without one."""
    return pfa.sample_sets([frames], engine, sigma=args.consensus_sigma, tolerance=args.consensus_tolerance,
                           threshold=args.consensus_threshold, min_support=args.min_support)[0]


def write_consensus(pocket_dir, sset, picks=None):
    """consensus.xyz and clusters.tsv of a SampleSet; picks (--keep_diverse): one more column, the rank of each sample among the
    picks or -1"""
    (pocket_dir / 'consensus.xyz').write_text(sset.consensus_xyz())
    rows = sset.clusters_tsv().splitlines()
    if picks is not None:
        rank = {a: k for k, a in enumerate(picks)}
        rows = [rows[0] + '\tpick'] + [f'{row}\t{rank.get(a, -1)}' for a, row in enumerate(rows[1:])]
    (pocket_dir / 'clusters.tsv').write_text('\n'.join(rows) + '\n')


def screen_and_write(pfa, pocket_dir, queries, labels, args, engine=None):
    """--screen_library: the library against `queries` ((positions, types) pairs, named by `labels`) on the engine's device, or on
    the host without one; writes hits.tsv and hits_aligned.xyz and returns the hit lists.  Queries outside 1..16 centers are left
    out (reported)."""
    keep = [k for k, (x, _) in enumerate(queries) if 1 <= len(x) <= 16]
    if len(keep) < len(queries):
        print(f'--screen_library: {len(queries) - len(keep)} queries outside 1..16 centers are not screened')
    hits = pfa.screen_library([queries[k] for k in keep], args.screen_lib, engine, top_k=args.screen_top, min_match=args.screen_min_match,
                              sigma=args.screen_sigma, tolerance=args.screen_tolerance, refine=args.screen_refine)
    rows, frames = ['query\trank\tentry\tsim\tmatched\tn_q'], []
    for k, hs in zip(keep, hits):
        for rank, h in enumerate(hs):
            rows.append(f'{labels[k]}\t{rank}\t{h.name}\t{h.sim:.6f}\t{h.n_matched}\t{len(queries[k][0])}')
            frames.append(h.to_xyz_file())
    (pocket_dir / 'hits.tsv').write_text('\n'.join(rows) + '\n')
    (pocket_dir / 'hits_aligned.xyz').write_text(''.join(frames))
    if args.screen_lib.dropped:
        print(f'--screen_library: {args.screen_lib.dropped} frames outside 1..32 centers were dropped')
    return hits


def main(argv=None):
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd.pocket_io import get_prot_atom_ph_type_maps, process_ligand_and_pocket

    args = parse_arguments(argv)
    if args.screen_query_frames is not None:    # no sampling, no receptor, no checkpoint: the frames of the file are the queries
        name = args.receptor_name or args.screen_queries.name.split('.')[0]
        pocket_dir = Path(args.output_dir) / name
        pocket_dir.mkdir(parents=True, exist_ok=True)
        engine = pfa.PfEngine(pharm_nf=len(pfa.SampledPharmacophore.type_idx_to_elem)) if torch.cuda.is_available() else None
        hits = screen_and_write(pfa, pocket_dir, args.screen_query_frames, list(range(len(args.screen_query_frames))), args, engine)
        print(f'{name}: {len(args.screen_query_frames)} queries against {len(args.screen_lib)} library entries, {sum(len(h) for h in hits)} hits listed')
        return
    if args.consensus_frames is not None:       # no sampling, no receptor, no checkpoint: the frames of the file as one set
        name = args.receptor_name or args.consensus_of.name.split('.')[0]
        pocket_dir = Path(args.output_dir) / name
        pocket_dir.mkdir(parents=True, exist_ok=True)
        engine = pfa.PfEngine(pharm_nf=len(pfa.SampledPharmacophore.type_idx_to_elem)) if torch.cuda.is_available() else None
        sset = analyse_set(pfa, args.consensus_frames, args, engine)
        write_consensus(pocket_dir, sset)
        print(f'{name}: {sset.n_samples} pharmacophores in {len(sset.clusters)} clusters, sizes ' + ' '.join(str(c.size) for c in sset.clusters))
        return
    for path, what in ((args.receptor_file, 'receptor'), (args.ref_ligand_file, 'ligand')):
        if path is not None and not path.exists():
            raise ValueError(f'{what} file {path} not found')
    if not torch.cuda.is_available():
        raise SystemExit("generate_pharmacophores.py needs an MI355X: the denoising kernels have no CPU fallback")
    _, ckpt, config = locate_run(args)
    device = torch.device('cuda')
    print(f'{device=}', flush=True)
    torch.manual_seed(args.seed)
    prot_element_map, _ = get_prot_atom_ph_type_maps(config['dataset'])
    model = load_model(pfa, ckpt, config, device, use_ema=args.use_ema)

    name = args.receptor_name or args.receptor_file.name.split('.')[0]
    pocket_dir = Path(args.output_dir) / name
    pocket_dir.mkdir(parents=True, exist_ok=True)
    pocket = process_ligand_and_pocket(args.receptor_file, pocket_dir, lig_file=args.ref_ligand_file,
                                       residue_list=args.residue_list, prot_element_map=prot_element_map,
                                       graph_cutoffs=config['graph']['graph_cutoffs'],
                                       pocket_cutoff=config['dataset']['pocket_cutoff'], remove_hydrogen=True).to(device)

    if args.score_frames is not None:            # no sampling: the frames of the file against this pocket
        scores = score_frames(pfa, model, pocket, args.score_frames, args)
        write_scores(pocket_dir / 'scores.tsv', range(len(scores)), scores)
        print(f'{name}: {len(scores)} pharmacophores scored')
        return

    k_pin = 0
    if args.pinned is not None:              # the pinned centers ride on the pocket graph: the first k centers of every copy
        import dataclasses
        pin_x, pin_types = args.pinned
        k_pin = len(pin_types)
        flag = {'both': 3, 'position': 1, 'type': 2}[args.pin_what]
        pocket = dataclasses.replace(pocket, pharm_pin=torch.full((k_pin,), flag, dtype=torch.int32, device=device),
                                     pharm_pin_x=pin_x.to(device),
                                     pharm_pin_h=torch.nn.functional.one_hot(pin_types, model.n_pharm_feats).float().to(device))

    k_named = 0
    if args.restraint_list:
        k_named = 1 + max([c for _, c, _, _, _ in args.restraint_list if c is not None], default=-1)
    type_guidance = None
    if args.type_restraint_list:
        k_named = max(k_named, 1 + max([c for _, c, _, _, _ in args.type_restraint_list if c is not None], default=-1))
        type_guidance = pfa.TypeGuidance(scale=args.guide_type_scale, clip=args.guide_type_clip, sharpness=args.type_sharpness)
    if args.pair_restraint_list:
        k_named = max(k_named, 1 + max([c for i, j, _, _, _ in args.pair_restraint_list for c in (i, j) if c is not None], default=-1))
    field = None
    if args.avoid_clashes is not None:       # PDB input has no receptor features: the clash term alone
        field = pfa.PocketField(clash_radius=args.avoid_clashes, clash_weight=args.clash_weight, comp_weight=0.0)
    t0 = time.time()
    pharms = []
    while len(pharms) < args.samples_per_pocket:
        n = min(args.samples_per_pocket - len(pharms), args.max_batch_size)
        sizes = args.pharm_sizes or model.pharm_size_dist.sample_uniformly(args.samples_per_pocket)
        if args.seed_centers is not None:                # every sample has the seed's size
            sizes = [len(args.seed_centers[1])] * args.samples_per_pocket
        elif max(k_pin, k_named) and not args.pharm_sizes:
            sizes = pinned_sizes(sizes, max(k_pin, k_named), 'pinned centers' if k_pin >= k_named else 'centers named in --restraints')
        # like the reference (:329-333, utils/unorganized_utils.py:48) every chunk reads the size list from its start
        copies = pfa.batch(pfa.copy_graph(pocket, n, pharm_feats_per_copy=sizes))
        com = pocket.pharm_x0.repeat(n, 1) if args.use_ref_lig_com else None
        with torch.no_grad():
            pharms += model.sample_given_receptor(copies, init_pharm_com=com, visualize_trajectory=args.visualize_trajectory,
                                                  pin_resamples=args.pin_resamples, pin_jump=args.pin_jump,
                                                  restraints=[args.restraint_list] * n if args.restraint_list else None,
                                                  guide_scale=args.guide_scale, guide_clip=args.guide_clip, guide_family=args.guide_family,
                                                  seeds=[args.seed_centers] * n if args.seed_centers is not None else None, seed_level=args.seed_level,
                                                  seed_keep=[args.seed_keep_list] * n if args.seed_keep_list else None,
                                                  sample_steps=args.sample_steps, sampler=args.sampler, eta=args.eta, spacing=args.spacing,
                                                  pocket_field=field,
                                                  type_restraints=[args.type_restraint_list] * n if args.type_restraint_list else None,
                                                  type_guidance=type_guidance,
                                                  pair_restraints=[args.pair_restraint_list] * n if args.pair_restraint_list else None,
                                                  min_separation=args.min_separation, separation_weight=args.separation_weight)
    elapsed = time.time() - t0

    (pocket_dir / 'sample_time.txt').write_text(f'{elapsed:.2f}')
    with open(pocket_dir / 'sample_time.pkl', 'wb') as f:
        pickle.dump([elapsed], f)
    print(f'{name}: {len(pharms)} pharmacophores in {elapsed:.2f} s ({elapsed / len(pharms):.3f} s each)')
    clashes = None
    if field is not None:                    # the final clash energy and the clashing (center, atom) pairs of every sample
        from pharmacoforge_amd.analysis import clash_energy
        clashes = [clash_energy(ph.ph_coords, pocket.prot_x, args.avoid_clashes, args.clash_weight) for ph in pharms]
        print(f'{name}: clash energy per sample ' + ' '.join(f'{e:.3g}' for e, _ in clashes)
              + '; clashing pairs ' + ' '.join(str(c) for _, c in clashes))
    type_energies = None
    if args.type_restraint_list:             # the final type energy of every sample
        from pharmacoforge_amd.analysis import type_restraint_energy
        rows = [(model._type_index(t), c, p, r, w) for t, c, p, r, w in args.type_restraint_list]
        type_energies = [type_restraint_energy(ph.ph_coords, ph.g.pharm_h0, rows, args.type_sharpness) for ph in pharms]
        print(f'{name}: type energy per sample ' + ' '.join(f'{e:.3g}' for e in type_energies))
    pair_energies = None
    if args.pair_restraint_list or args.min_separation is not None:     # the final pair energy of every sample
        pair_energies = [ph.pair_energy for ph in pharms]
        print(f'{name}: pair energy per sample ' + ' '.join(f'{e:.3g}' for e in pair_energies)
              + '; violated pairs ' + ' '.join(str(ph.pair_violations) for ph in pharms))
    ref_dir = pocket_dir / 'reference_files'
    ref_dir.mkdir(exist_ok=True)
    for src in (args.receptor_file, args.ref_ligand_file):
        if src is not None:
            shutil.copy(src, ref_dir / src.name)
    order, scores = list(range(len(pharms))), None
    if args.score_samples is not None:
        # the scores describe the frames as pharms.xyz holds them (three decimals, argmax types): scoring that file again
        # (--score_pharmacophores) with the same seed and levels gives the same numbers
        frames = [ph.as_written() for ph in pharms]
        scores = score_frames(pfa, model, pocket, frames, args)
        if args.keep_best is not None:
            order = sorted(order, key=lambda i: (scores[i].per_center, i))[:args.keep_best]
    if args.consensus or args.keep_diverse is not None:
        # the set is what pharms.xyz would hold without --keep_diverse (the best N with --keep_best), as written: --consensus_of on
        # that file gives the same analysis.  clusters.tsv numbers the samples of that set
        sset = analyse_set(pfa, [pharms[i].as_written() for i in order], args, model.dynamics.engine())
        picks = None if args.keep_diverse is None else sset.pick_diverse(args.keep_diverse)
        if args.consensus:
            write_consensus(pocket_dir, sset, picks)
            print(f'{name}: {len(sset.clusters)} clusters, sizes ' + ' '.join(str(c.size) for c in sset.clusters))
        if picks is not None:
            order = [order[a] for a in picks]
            print(f'{name}: --keep_diverse kept samples ' + ' '.join(str(a) for a in picks))
    if scores is not None or args.keep_diverse is not None:
        pharms = [pharms[i] for i in order]
    if scores is not None:
        scores = [scores[i] for i in order]
        write_scores(pocket_dir / 'scores.tsv', range(len(scores)), scores, None if clashes is None else [clashes[i] for i in order],
                     None if type_energies is None else [type_energies[i] for i in order],
                     None if pair_energies is None else [pair_energies[i] for i in order])
    if args.visualize_trajectory:
        for i, ph in enumerate(pharms):
            ph.traj_to_xyz(pocket_dir / f'pharm_{i}_traj.xyz')
    else:
        (pocket_dir / 'pharms.xyz').write_text(''.join(ph.to_xyz_file() for ph in pharms))
    if args.screen_lib is not None:
        if args.consensus:                       # the consensus pharmacophores as consensus.xyz lists them
            keep = lambda c: [i for i in range(c.types.shape[0]) if float(c.support[i]) >= args.min_support]
            queries = [(c.positions[keep(c)], c.types[keep(c)]) for c in sset.clusters]
            labels = [f'cluster_{c.cluster}' for c in sset.clusters]
        else:                                    # the samples as pharms.xyz holds them
            queries, labels = [ph.as_written() for ph in pharms], list(range(len(pharms)))
        hits = screen_and_write(pfa, pocket_dir, queries, labels, args, model.dynamics.engine())
        print(f'{name}: {len(queries)} queries against {len(args.screen_lib)} library entries, {sum(len(h) for h in hits)} hits listed')
    if args.metrics:
        print(pfa.SampleAnalyzer().analyze(pharms))


if __name__ == "__main__":
    main()
