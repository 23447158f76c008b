#!/usr/bin/env python3
"""Training driver in the shape of the reference's train.py (:26-175) without Lightning / wandb: config yaml ->
PharmacophoreDiff + CrossdockedDataModule -> epochs of training_step / backward (HIP gradient kernels) / fused Adam,
validation loss, ReduceLROnPlateau on 'val total loss', Lightning-format checkpoints (<output_dir>/<run>/checkpoints/
last.ckpt + config.yaml next to them, which generate_pharmacophores.py reads).

Data parallel, one process per GPU (``torchrun --nproc-per-node N train.py ...``):
  * every rank builds the model, then rank 0's parameters are BROADCAST, so all replicas start from the same weights
    whatever their RNG state; only afterwards does the seed get its rank offset (data order, noise, dropout draws);
  * each rank draws its own batches (DistributedSampler); gradients are averaged with ONE all-reduce of the flat
    gradient vector per step, so the replicas stay bitwise identical (``--check_replicas`` verifies that every epoch);
  * the validation loss is summed over the ranks before the plateau logic, so every rank takes the same LR decision;
  * rank 0 writes the checkpoint, which carries the optimiser moments, step count, learning rate, epoch and plateau
    state next to the weights; ``--resume`` restores all of them (a Lightning checkpoint's 'optimizer_states' /
    'lr_schedulers' / 'epoch' / 'global_step' keys are used for that).

Optimiser settings (optim_options): ``training.trainer_args.gradient_clip_val`` / ``gradient_clip_algorithm`` ('norm' by
default, or 'value') and ``accumulate_grad_batches`` mean what they mean to Lightning's Trainer; ``training.clip_value`` /
``--clip_value`` clip by value; ``training.ema_decay`` / ``--ema_decay`` (``--ema_warmup``) keep an exponential moving average
of the weights, under which validation and the checkpoint's 'ema_state_dict' run.  Any of them puts the step on FlatAdam's guarded
entry, which also skips a step whose gradient is not finite; other trainer arguments are named once and ignored."""
import argparse
import contextlib
import os
from datetime import datetime
from pathlib import Path

import torch
import yaml


def _collective(fn, t, **kw):
    """all_reduce / broadcast on ``t``; the gloo fallback (more ranks than GPUs: dry runs on one card) goes through a host
    copy, RCCL works on the device tensor."""
    import torch.distributed as dist
    if t.is_cuda and dist.get_backend() != "nccl":
        c = t.cpu()
        fn(c, **kw)
        t.copy_(c)
    else:
        fn(t, **kw)
    return t


HANDLED_TRAINER_ARGS = ('max_epochs', 'gradient_clip_val', 'gradient_clip_algorithm', 'accumulate_grad_batches')


def optim_options(config, args=None):
    """What the config and the command line ask of the optimiser step, as a dict: clip_norm, clip_value (at most one is set),
    accumulate (micro-batches per step, >= 1), ema_decay (or None), ema_warmup, ignored (names of the trainer arguments this
    driver does not act on).  Needs no GPU.  ``args``: the parsed command line (clip_value, ema_decay, ema_warmup) or None."""
    training = config.get('training') or {}
    ta = dict(training.get('trainer_args') or {})
    clip_norm = clip_value = None
    gcv = ta.get('gradient_clip_val')
    algo = ta.get('gradient_clip_algorithm') or 'norm'
    if algo not in ('norm', 'value'):
        raise ValueError(f"trainer_args.gradient_clip_algorithm must be 'norm' or 'value', got {algo!r}")
    if gcv is not None and float(gcv) > 0:          # Lightning: None or 0 = no clipping
        if algo == 'norm':
            clip_norm = float(gcv)
        else:
            clip_value = float(gcv)
    cv = getattr(args, 'clip_value', None)
    if cv is None:
        cv = training.get('clip_value')
    if cv is not None:
        if clip_norm is not None or clip_value is not None:
            raise ValueError("both trainer_args.gradient_clip_val and clip_value (training.clip_value / --clip_value) are set: "
                             "choose one way of clipping")
        clip_value = float(cv)
    acc = ta.get('accumulate_grad_batches')
    acc = 1 if acc is None else int(acc)
    if acc < 1:
        raise ValueError(f"trainer_args.accumulate_grad_batches must be >= 1, got {acc}")
    ema = getattr(args, 'ema_decay', None)
    if ema is None:
        ema = training.get('ema_decay')
    if ema is not None and not 0.0 <= float(ema) < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1), got {ema!r}")
    return {'clip_norm': clip_norm, 'clip_value': clip_value, 'accumulate': acc,
            'ema_decay': None if ema is None else float(ema),
            'ema_warmup': bool(getattr(args, 'ema_warmup', False) or training.get('ema_warmup', False)),
            'ignored': sorted(k for k in ta if k not in HANDLED_TRAINER_ARGS)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--config', type=str, required=True)
    p.add_argument('--resume', type=Path, default=None, help='run directory or checkpoint to continue from')
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--max_steps', type=int, default=None, help='stop after this many optimiser steps (smoke runs)')
    p.add_argument('--check_replicas', action='store_true',
                   help='data parallel: verify after every epoch that all ranks hold bitwise identical parameters')
    p.add_argument('--bind_prefetch', action='store_true',
                   help="bind the next batch on the dynamics' twin handle from a worker thread while a step is enqueued: the host's time per "
                        "step drops by a third (for ranks that share a busy host); the device-bound step itself pays ~1.5 %% for it")
    p.add_argument('--train_precision', choices=['f32', 'bf16'], default='f32',
                   help="arithmetic of the dense Linears in the training step: f32 (the reference's) or the bf16 leg (bf16 matrix "
                        "instructions, fp32 accumulation, fp32 master weights and optimiser)")
    p.add_argument('--train_family', choices=['auto', 'tuned', 'wide'], default='auto',
                   help="gradient kernels: tuned (n_hidden_scalars 128 / vector_size 16 only), wide (the width-generic fp32 leg, every "
                        "supported width pair) or auto: wide iff the config's widths are not 128 / 16")
    p.add_argument('--clip_value', type=float, default=None, help='max gradient value for clipping')
    p.add_argument('--ema_decay', type=float, default=None,
                   help='keep an exponential moving average of the weights with this decay; validation, sampling and the '
                        "checkpoint's ema_state_dict use it")
    p.add_argument('--ema_warmup', action='store_true', help='EMA decay min(d, (1 + k) / (10 + k)) at optimiser call k')
    args = p.parse_args()
    with open(args.config) as f:
        _dyn = (yaml.load(f, Loader=yaml.FullLoader).get('dynamics') or {})
    widths = (int(_dyn.get('n_hidden_scalars', 128)), int(_dyn.get('vector_size', 16)))
    family = args.train_family if args.train_family != 'auto' else ('tuned' if widths == (128, 16) else 'wide')
    if family == 'wide' and args.train_precision == 'bf16':
        p.error('--train_precision bf16 is not available on the wide training leg (fp32 only)')
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd.dataset import data_module_from_config

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # the rank's slice of the host and its pool sizes, before anything touches the GPU (a step is as long on the host as on the device)
    from pharmacoforge_amd.sharding import pin_host_threads
    host = pin_host_threads(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    if world > 1:
        print(f"[rank {rank}] host share: {host}", flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("train.py needs an MI355X: the kernels have no CPU fallback")
    ndev = torch.cuda.device_count()
    torch.cuda.set_device(local % ndev)
    dev = torch.device("cuda", local % ndev)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29541")
        if world <= ndev:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:                                   # ranks share a card: RCCL needs one GPU per rank
            dist.init_process_group("gloo", rank=rank, world_size=world)
    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    model = pfa.model_from_config(config).to(dev)
    model.dynamics.set_train_precision(args.train_precision)
    model.dynamics.set_train_family(family)
    print(f"training leg: {family} ({'width-generic fp32 kernels' if family == 'wide' else 'kernels specialised to 128 / 16'}; "
          f"n_hidden_scalars {widths[0]}, vector_size {widths[1]})", flush=True)
    lr_cfg = config['lr_scheduler']
    oo = optim_options(config, args)
    if oo['ignored'] and rank == 0:
        print("trainer_args not acted on by this driver: " + ", ".join(oo['ignored']), flush=True)
    n_acc = oo['accumulate']
    opt = pfa.FlatAdam(model.dynamics, lr=lr_cfg['base_lr'], weight_decay=lr_cfg.get('weight_decay', 0.0), clip_norm=oo['clip_norm'],
                       clip_value=oo['clip_value'], ema_decay=oo['ema_decay'], ema_warmup=oo['ema_warmup'])
    if (opt.guarded or n_acc > 1) and rank == 0:
        print(f"guarded optimiser step: clip_norm {oo['clip_norm']} clip_value {oo['clip_value']} accumulate_grad_batches {n_acc} "
              f"ema_decay {oo['ema_decay']}" + (" (warm-up)" if oo['ema_warmup'] else ""), flush=True)
    plateau = dict(lr_cfg.get('reducelronplateau', {}))
    best, bad_epochs, step, first_epoch = float('inf'), 0, 0, 0
    if args.resume is not None:
        ck_path = args.resume / 'checkpoints' / 'last.ckpt' if args.resume.is_dir() else args.resume
        ck = torch.load(str(ck_path), map_location='cpu', weights_only=False)
        model.load_state_dict(ck['state_dict'], strict=True)
        model.dynamics.engine()                                  # flat parameter vector on the device
        if ck.get('optimizer_states'):
            opt.load_state_dict(ck['optimizer_states'][0])
        if ck.get('lr_schedulers'):
            best, bad_epochs = ck['lr_schedulers'][0].get('best', best), ck['lr_schedulers'][0].get('num_bad_epochs', 0)
        first_epoch, step = int(ck.get('epoch', -1)) + 1, int(ck.get('global_step', 0))
    model.dynamics.engine()
    if world > 1:
        # identical replicas: rank 0's weights (fresh or resumed) and optimiser state go to everyone
        _collective(dist.broadcast, model.dynamics._flat, src=0)
        model.dynamics._weights_stamp = None                     # the engine re-reads the flat vector
        meta = [opt.state_dict_meta(), best, bad_epochs, step, first_epoch] if rank == 0 else [None] * 5
        dist.broadcast_object_list(meta, src=0)
        opt.ensure_state(*meta[0])
        best, bad_epochs, step, first_epoch = meta[1:]
        _collective(dist.broadcast, opt.exp_avg, src=0)
        _collective(dist.broadcast, opt.exp_avg_sq, src=0)
        if opt.ema_decay is not None:                            # the EMA vector (rank 0's, or its parameters) and the call count
            guard = [opt._calls, opt.ema is not None] if rank == 0 else [None, None]
            dist.broadcast_object_list(guard, src=0)
            opt._calls = guard[0]
            if guard[1]:
                if opt.ema is None:
                    opt.ema = torch.empty_like(model.dynamics._flat)
                _collective(dist.broadcast, opt.ema, src=0)
            else:
                opt.ema = None
    if args.seed is not None:
        torch.manual_seed(args.seed + 1000003 * (rank + 1))      # from here on: per-rank data order, noise, dropout
    guarded = opt.guarded or n_acc > 1               # (a resumed state may carry guard options of its own)
    dm = data_module_from_config(config)
    dm.setup('fit')
    run_dir = Path(config['training']['output_dir']) / f"{config['wandb']['name'].replace(' ', '_')}_{datetime.now():%Y-%m-%d_%H-%M-%S}"
    if rank == 0:
        (run_dir / 'checkpoints').mkdir(parents=True, exist_ok=True)
        with open(run_dir / 'config.yaml', 'w') as f:
            yaml.dump(config, f)
    stop = False
    for epoch in range(first_epoch, config['training']['trainer_args']['max_epochs']):
        model.train()
        sampler = torch.utils.data.distributed.DistributedSampler(dm.train_dataset, world, rank, shuffle=True) if world > 1 else None
        if sampler is not None:
            sampler.set_epoch(epoch)
        loader = dm.train_dataloader(shuffle=sampler is None, sampler=sampler)
        model.attach_trainer(dm, loader, current_epoch=epoch, optimizer=opt)
        # one batch of look-ahead: while a step's backward and optimiser step are being enqueued, the NEXT batch is bound on the
        # dynamics' twin handle by a worker thread (the bind is half a step's host time; PharmRecDynamicsGVP.prefetch_graph)
        batches = iter(loader)
        nxt = next(batches, None)
        nxt = None if nxt is None else nxt.to(dev)
        i = -1
        while nxt is not None:
            i += 1
            g = nxt
            nxt = next(batches, None)
            nxt = None if nxt is None else nxt.to(dev)
            if i % n_acc == 0:                                   # first micro-batch of a group: the deferred clear; the rest accumulate
                opt.zero_grad(lazy=True)
            loss = model.training_step(g, i)
            if nxt is not None and args.bind_prefetch:
                model.dynamics.prefetch_graph(nxt)
            loss.backward()
            if (i + 1) % n_acc != 0 and nxt is not None:         # (a short last group of an epoch steps with what it has)
                continue
            if world > 1:
                model.dynamics.allreduce_gradients()
            if guarded:
                opt.step(grad_scale=1.0 / n_acc)
            else:
                opt.step()
            step += 1
            if rank == 0 and step % 50 == 0:
                extra = f" grad_norm={opt.last_grad_norm():.4f} skipped={opt.skipped_steps()}" if guarded else ""
                print(f"epoch {epoch} step {step} " + " ".join(f"{k}={float(v):.4f}" for k, v in model.last_metrics.items()) + extra,
                      flush=True)
            if args.max_steps and step >= args.max_steps:
                stop = True
                break
        model.eval()
        acc = torch.zeros(2, dtype=torch.float64)
        # validation (and whatever validation_step samples and analyses) on the EMA weights when there are any
        with (opt.ema_weights() if opt.ema_decay is not None else contextlib.nullcontext()), torch.no_grad():
            for i, g in enumerate(dm.val_dataloader()):
                if i % world != rank:                            # validation batches dealt over the ranks
                    continue
                acc[0] += float(model.validation_step(g.to(dev), i)) * g.batch_size
                acc[1] += g.batch_size
        if world > 1:                                            # every rank sees the same 'val total loss'
            acc = acc.to(dev) if dist.get_backend() == "nccl" else acc
            dist.all_reduce(acc)
            acc = acc.cpu()
        val = float(acc[0] / acc[1].clamp(min=1))
        if plateau:                                              # ReduceLROnPlateau(mode='min', factor, patience, min_lr)
            if val < best - 1e-12:
                best, bad_epochs = val, 0
            else:
                bad_epochs += 1
                if bad_epochs > plateau.get('patience', 10):
                    opt.param_groups[0]['lr'] = max(opt.param_groups[0]['lr'] * plateau.get('factor', 0.1), plateau.get('min_lr', 0.0))
                    bad_epochs = 0
        if args.check_replicas and world > 1:
            flat = model.dynamics._flat
            sig = torch.stack([flat.double().sum(), flat.double().abs().sum(), flat[::997].double().square().sum()])
            lo, hi = sig.clone(), sig.clone()
            _collective(dist.all_reduce, lo, op=dist.ReduceOp.MIN)
            _collective(dist.all_reduce, hi, op=dist.ReduceOp.MAX)
            if not torch.equal(lo, hi):
                raise RuntimeError(f"replicas diverged after epoch {epoch}: parameter checksums differ by {(hi - lo).tolist()}")
            if opt.ema is not None:
                e = opt.ema
                esig = torch.stack([e.double().sum(), e.double().abs().sum(), e[::997].double().square().sum()])
                lo, hi = esig.clone(), esig.clone()
                _collective(dist.all_reduce, lo, op=dist.ReduceOp.MIN)
                _collective(dist.all_reduce, hi, op=dist.ReduceOp.MAX)
                if not torch.equal(lo, hi):
                    raise RuntimeError(f"replicas diverged after epoch {epoch}: EMA checksums differ by {(hi - lo).tolist()}")
            if rank == 0:
                print(f"epoch {epoch}: replicas identical on {world} ranks (checksum {float(sig[0]):.9e})", flush=True)
        if rank == 0:
            print(f"epoch {epoch}: val total loss {val:.5f} lr {opt.param_groups[0]['lr']:.2e}"
                  + (f" grad_norm {opt.last_grad_norm():.4f} skipped {opt.skipped_steps()}" if guarded and opt.last_grad_norm() is not None
                     else ""), flush=True)
            model.save_checkpoint(run_dir / 'checkpoints' / 'last.ckpt', epoch=epoch, global_step=step,
                                  ema_state_dict=opt.ema_state_dict(),
                                  optimizer_states=[opt.state_dict()],
                                  lr_schedulers=[{'best': best, 'num_bad_epochs': bad_epochs}])
        if stop:
            break
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
