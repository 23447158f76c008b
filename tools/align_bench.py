"""align_bench.py -- what screening a pharmacophore library costs (pf_pharm_align: k_align_self, k_align_pairs), one JSON line.
Recorded, not gated: there is no parent to compare against.

Shape: --queries queries (default 30) of 3..8 centers against --entries library entries (default 100000) of 3..10 centers, six
types, every center uniform in an 8 A box -- RANDOM entries, not ligand pharmacophores: with six types and few centers most pairs
have a handful of seeds or none, as a dataset-scale library has; what real entries change is the share of pairs with many seeds.
Legs:
  device    PfEngine.align with the library already on the device, the transforms not asked for and asked for: the median wall
            time of --rounds calls after a warm-up (the call packs two pointer arrays on the host, enqueues two launches and
            waits for the stream), the time between HIP events around the call, pairs per second from the wall time, and the
            seeds the call found
  host      analysis.align_pharmacophores (fp32) on the host of the same machine over the same queries and the first
            --host-entries entries (default 20): its own time and pairs per second, not an extrapolation

    python tools/align_bench.py --out profiles/align/align_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_pharmacophores(n, lo, hi, seed, types=6, box=8.0):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(lo, hi + 1, (n,), generator=g)
    N = int(sizes.sum())
    ptr = np.concatenate([[0], np.cumsum(sizes.numpy())]).astype(np.int32)
    return torch.rand(N, 3, generator=g) * box, torch.randint(0, types, (N,), generator=g).to(torch.int32), ptr


def device_leg(eng, q, lib, rounds, want_transform):
    (qx, qt, qp), (lx, lt, lp) = q, lib
    lx, lt = lx.to(eng.device), lt.to(eng.device)
    for _ in range(2):
        out = eng.align(qx, qt, qp, lx, lt, lp, want_transform=want_transform)
    torch.cuda.synchronize()
    wall, ev = [], []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = eng.align(qx, qt, qp, lx, lt, lp, want_transform=want_transform)
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    pairs = (len(qp) - 1) * (len(lp) - 1)
    w = statistics.median(wall)
    seeds = out["n_seeds"].long()
    return {"wall_ms": round(w, 3), "event_ms": round(statistics.median(ev), 3), "walls_ms": [round(v, 3) for v in wall], "pairs": pairs,
            "pairs_per_s": round(pairs / (w * 1e-3)), "seeds": int(seeds.sum()), "pairs_with_seeds": int((seeds > 0).sum()),
            "max_seeds_of_a_pair": int(seeds.max()), "mean_sim_of_pairs_with_seeds": round(float(out["sim"][seeds > 0].mean()), 4)}


def host_leg(analysis, q, lib, n_entries):
    (qx, qt, qp), (lx, lt, lp) = q, lib
    queries = [(qx[qp[k]:qp[k + 1]], qt[qp[k]:qp[k + 1]].long()) for k in range(len(qp) - 1)]
    entries = [(lx[lp[k]:lp[k + 1]], lt[lp[k]:lp[k + 1]].long()) for k in range(n_entries)]
    t0 = time.perf_counter()
    r = analysis.align_pharmacophores(queries, entries)
    dt = time.perf_counter() - t0
    pairs = len(queries) * len(entries)
    return {"pairs": pairs, "total_ms": round(dt * 1e3, 2), "pairs_per_s": round(pairs / dt, 1), "seeds": int(r["n_seeds"].sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=30)
    ap.add_argument("--entries", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-entries", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import analysis
    eng = pfa.PfEngine(device="cuda:0")
    q, lib = random_pharmacophores(args.queries, 3, 8, 0), random_pharmacophores(args.entries, 3, 10, 1)
    out = {"shape": {"queries": args.queries, "entries": args.entries, "query_centers": "3..8", "entry_centers": "3..10", "types": 6,
                     "box_A": 8.0, "entries_are": "random"},
           "device": device_leg(eng, q, lib, args.rounds, False), "device_with_transforms": device_leg(eng, q, lib, args.rounds, True)}
    if not args.no_host:
        out["host"] = host_leg(analysis, q, lib, min(args.host_entries, args.entries))
        out["device_over_host_pairs_per_s"] = round(out["device"]["pairs_per_s"] / out["host"]["pairs_per_s"], 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
