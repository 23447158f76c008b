#!/usr/bin/env python3
"""Times the optimiser step at the parameter count of BASELINE config 5 (the dev.yml model, 244 tensors) on seeded vectors:

    legacy          pf_adam_step (k_adam + the weight gather)
    guarded_norm    pf_adam_step_guarded, PF_CLIP_NONE (norm, finalising launch, guarded Adam, gather)
    guarded_clip    ... with PF_CLIP_NORM
    guarded_ema     ... with PF_CLIP_NORM and the EMA stream
    framework       torch.nn.utils.clip_grad_norm_ on the 244 gradient views + pf_adam_step + torch._foreach_lerp_ on 244
                    EMA tensors: what a training loop pays for the same thing outside the library

    python tools/optim_bench.py [--rounds 5] [--calls 200] [--out FILE]

Per leg: us per call from HIP events around a window of back-to-back calls (the longer of the host's enqueue and the
device's work), the host's own time per call, medians over alternating windows, all windows listed.  One JSON line.  The
device time per kernel comes from a separate run under `rocprofv3 --kernel-trace --stats` (profiles/optim/)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()

    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dyn_cfg = dict(vector_size=16, n_convs=2, n_hidden_scalars=128, message_norm='mean', dropout=0.1, ff_k=0, pf_k=5,
                   n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4)
    m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=100,
                              graph_config={'graph_cutoffs': {'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9}}, dynamics_config=dyn_cfg,
                              precision=1e-5)
    sd = dict(synthetic.make_state_dict(0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    dyn = m.dynamics
    eng = dyn.engine()
    n = eng.n_params
    gen = torch.Generator(device="cuda").manual_seed(3)
    grad = torch.randn(n, device=dev, generator=gen) * 1e-2
    norm = float(grad.double().norm())
    p0 = dyn._flat.clone()
    views = [(p, off, k) for p, off, k in dyn._flat_views if k > 0]
    lr, betas, eps, wd = 1e-4, (0.9, 0.999), 1e-8, 1e-12

    def fresh():
        dyn._flat.copy_(p0)
        return dict(m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev), ema=p0.clone(), state=eng.optim_state(), t=0)

    def legacy(s):
        s["t"] += 1
        eng.adam_step(dyn._flat, grad, s["m"], s["v"], s["t"], lr, betas, eps, wd)

    def guarded(clip, ema):
        def run(s):
            eng.adam_step_guarded(dyn._flat, grad, s["m"], s["v"], s["state"], lr, betas, eps, wd, clip_norm=clip,
                                  ema=s["ema"] if ema else None, ema_decay=0.999 if ema else 0.0)
        return run

    grads = [grad[off:off + k].view(p.shape) for p, off, k in views]
    params = [p for p, _, _ in views]

    def framework(s):
        if "ema_t" not in s:
            s["ema_t"] = [s["ema"][off:off + k].view(p.shape) for p, off, k in views]
            s["g"] = grad.clone()
            s["gv"] = [s["g"][off:off + k].view(p.shape) for p, off, k in views]
        s["g"].copy_(grad)                                       # (clip_grad_norm_ scales in place: a step's gradient is fresh)
        for p, g in zip(params, s["gv"]):
            p.grad = g
        torch.nn.utils.clip_grad_norm_(params, 0.25 * norm)
        s["t"] += 1
        eng.adam_step(dyn._flat, s["g"], s["m"], s["v"], s["t"], lr, betas, eps, wd)
        with torch.no_grad():
            torch._foreach_lerp_(s["ema_t"], [p.data for p in params], 1.0 - 0.999)

    legs = {"legacy": legacy, "guarded_norm": guarded(None, False), "guarded_clip": guarded(0.25 * norm, False),
            "guarded_ema": guarded(0.25 * norm, True), "framework": framework}
    states = {k: fresh() for k in legs}
    for k, fn in legs.items():
        for _ in range(args.warmup):
            fn(states[k])
    torch.cuda.synchronize()
    win = {k: [] for k in legs}
    host = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            s = states[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn(s)
            th = time.perf_counter() - t0
            e1.record()
            torch.cuda.synchronize()
            win[k].append(round(e0.elapsed_time(e1) * 1e3 / args.calls, 3))
            host[k].append(round(th * 1e6 / args.calls, 3))
    st = pfa.PfEngine.read_optim_state(states["guarded_ema"]["state"])
    out = {"leg": "optim_bench", "n_params": n, "tensors": len(views), "chunk": eng.optim_chunk(), "calls_per_window": args.calls,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "us_per_call": {k: statistics.median(v) for k, v in win.items()},
           "host_us_per_call": {k: statistics.median(v) for k, v in host.items()},
           "windows_us_per_call": win, "windows_host_us_per_call": host,
           "guarded_ema_state": st}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
