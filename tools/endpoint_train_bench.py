#!/usr/bin/env python3
"""Times one training step at BASELINE config 5's shape (batch 256, 256-atom pockets, 4-8 centers, dropout 0.1) for each
parameterisation of the loss: noise (the default), endpoint_param_coord, endpoint_param_feat, or both.

    python tools/endpoint_train_bench.py --endpoint both --steps 200
    python tools/endpoint_train_bench.py --endpoint both --unfused      # forward()'s framework-op restatement of the loss

A step is what bench.py --train times: FlatAdam.zero_grad(lazy) + PharmacophoreDiff.training_step + backward + FlatAdam.step,
on a batch object that changes every step (four distinct batches in rotation, each step pays the bind).  Prints one JSON line
per leg: ms_per_step from events around K steps after a rehearsal pass over the same K steps, host_ms_per_step the host's mean
time inside a step of that region.  Uses only API that exists without the fused endpoint loss too (PharmacophoreDiff,
FlatAdam, training_step, the fused_loss attribute), so the same file times a commit before it: there a model with an endpoint
flag takes the restatement whatever fused_loss says."""
import argparse
import itertools
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLAGS = {"none": (False, False), "coord": (True, False), "feat": (False, True), "both": (True, True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--endpoint", choices=list(FLAGS), action="append", help="repeat for several legs in one process (default: both)")
    ap.add_argument("--unfused", action="store_true", help="fused_loss = False: the framework-op restatement of the loss")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--train-batches", type=int, default=4)
    ap.add_argument("--prewarm-ms", type=float, default=150.0)
    args = ap.parse_args()

    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import synthetic
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, K, T = args.batch, args.steps, 100
    sizes = [4 + (i % 5) for i in range(B)]
    dyn = dict(vector_size=16, n_convs=2, n_hidden_scalars=128, message_norm='mean', dropout=0.1, ff_k=0, pf_k=5,
               n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4)
    m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=T,
                              graph_config={'graph_cutoffs': {'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9}}, dynamics_config=dyn,
                              precision=1e-5, lr_scheduler_config={'base_lr': 1e-4, 'weight_decay': 1e-12})
    sd = dict(synthetic.make_state_dict(0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    m.fused_loss = not args.unfused
    eng = m.dynamics.engine()
    pockets = [synthetic.synthetic_pocket(i, args.n_prot) for i in range(B)]
    gen = torch.Generator().manual_seed(7)
    graphs = []
    for r in range(args.train_batches):
        order = [(i + r * (B // max(args.train_batches, 1))) % B for i in range(B)]
        sz = [sizes[(i + r) % B] for i in range(B)]
        xs, hs = [pockets[i][0] for i in order], [pockets[i][1] for i in order]
        prot_x, prot_h = torch.cat(xs), torch.cat(hs)
        prot_ptr = torch.arange(B + 1, dtype=torch.int64) * args.n_prot
        pharm_ptr = torch.tensor([0] + list(itertools.accumulate(sz)), dtype=torch.int64)
        pp_src, pp_dst = eng.build_pp_edges(prot_x.to(dev), prot_ptr)
        Nf = int(pharm_ptr[-1])
        x0 = torch.cat([xs[i].mean(0, keepdim=True) + 2.0 * torch.randn(sz[i], 3, generator=gen) for i in range(B)])
        h0 = torch.nn.functional.one_hot(torch.randint(0, 6, (Nf,), generator=gen), 6).float()
        graphs.append(pfa.PocketGraph(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst, pharm_x0=x0, pharm_h0=h0).to(dev))
    opt = pfa.FlatAdam(m.dynamics, lr=1e-4, weight_decay=1e-12)
    it = [0]

    def step():
        opt.zero_grad(lazy=True)
        g = graphs[it[0] % len(graphs)]
        it[0] += 1
        loss = m.training_step(g, 0)
        loss.backward()
        opt.step()
        return loss

    for leg in args.endpoint or ["both"]:
        m.endpoint_param_coord, m.endpoint_param_feat = FLAGS[leg]
        tp = time.perf_counter()
        while (time.perf_counter() - tp) * 1e3 < args.prewarm_ms:
            step()
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            step()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for e in ev:
            e.record()
        for rehearsal in (True, False):         # the region runs twice with everything in it; the second pass is the timed one
            torch.cuda.synchronize()
            ev[0].record()
            host = 0.0
            for _ in range(K):
                th = time.perf_counter()
                loss = step()
                host += time.perf_counter() - th
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / K
            if rehearsal:
                rehearsal_ms = ms
        print(json.dumps({"leg": "endpoint_train", "endpoint": leg, "endpoint_param_coord": FLAGS[leg][0],
                          "endpoint_param_feat": FLAGS[leg][1], "fused_loss_attr": bool(m.fused_loss),
                          "ms_per_step": round(ms, 5), "host_ms_per_step": round(host / K * 1e3, 5),
                          "rehearsal_ms_per_step": round(rehearsal_ms, 5), "steps": K, "warmup": args.warmup, "batch": B,
                          "n_prot": args.n_prot, "centers": "4-8", "dropout": 0.1, "distinct_batches": len(graphs),
                          "last_loss": float(loss.detach()), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
