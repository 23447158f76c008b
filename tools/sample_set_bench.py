"""sample_set_bench.py -- what the analysis of sample sets (pf_sample_set_analyze: k_sset_overlap, k_sset_cluster,
k_sset_consensus) costs, one JSON line.  Recorded, not gated.

Shapes:
  config4   --sets sets (default 1000) x 30 samples x 3..8 centers -- the output of BASELINE config 4; each set is a few motifs plus
            jitter, so that clusters have members
  large     one set of 1024 samples x 64 centers, the caps
Legs per shape:
  device    PfEngine.sample_set on synthetic sets already on the device: the median wall time of --rounds calls after a warm-up
            (the call packs the pointer block on the host, enqueues three launches and waits for the stream), and the time
            between HIP events around the call
  host      analysis.analyze_sample_set on the host of the same machine, over --host-sets sets of the config4 shape (the figure
            is per set; the JSON says how many were timed) and over a subset of --host-large samples of the large shape (the
            host work grows with the square of the sample count; the subset's own time is listed, not an extrapolation)
  sampling  with --sample-slice P: bench.py --sample-slice P --samples 30 in a child process -- the time to SAMPLE P such sets,
            per set, next to the time to analyse one
--trace DIR: runs itself once more under `rocprofv3 --kernel-trace --stats` (a fresh child process; device legs only) and copies
the per-kernel statistics to DIR.

    python tools/sample_set_bench.py --out profiles/sample_set/sample_set_bench.json --trace profiles/sample_set"""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config4_sets(n_sets, samples=30, seed=0):
    """per set 3 motifs of 3..8 centers in a 12 A box; sample k of a set is motif k mod 3 plus jitter in +-0.3 A"""
    g = torch.Generator().manual_seed(seed)
    sets = []
    for _ in range(n_sets):
        motifs = []
        for _ in range(3):
            n = int(torch.randint(3, 9, (1,), generator=g))
            motifs.append((torch.rand(n, 3, generator=g) * 12.0, torch.randint(0, 6, (n,), generator=g)))
        sets.append([(motifs[k % 3][0] + (torch.rand(motifs[k % 3][0].shape, generator=g) - 0.5) * 0.6, motifs[k % 3][1])
                     for k in range(samples)])
    return sets


def large_set(samples=1024, centers=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    base, types = torch.rand(4, centers, 3, generator=g) * 16.0, torch.randint(0, 6, (4, centers), generator=g)
    return [(base[k % 4] + (torch.rand(centers, 3, generator=g) - 0.5) * 0.6, types[k % 4]) for k in range(samples)]


def packed(sets, dev):
    import numpy as np
    samples = [s for st in sets for s in st]
    set_ptr = np.concatenate([[0], np.cumsum([len(st) for st in sets])]).astype(np.int32)
    center_ptr = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in samples])]).astype(np.int32)
    return torch.cat([s[0] for s in samples]).to(dev), torch.cat([s[1] for s in samples]).to(dev, torch.int32), set_ptr, center_ptr


def device_leg(eng, sets, rounds):
    x, t, sp, cp = packed(sets, eng.device)
    for _ in range(2):
        out = eng.sample_set(x, t, sp, cp)
    torch.cuda.synchronize()
    wall, ev = [], []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = eng.sample_set(x, t, sp, cp)
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {"wall_ms": round(statistics.median(wall), 4), "event_ms": round(statistics.median(ev), 4), "walls_ms": [round(w, 4) for w in wall],
            "sets": len(sets), "samples": int(sp[-1]), "centers": int(cp[-1]), "clusters": int(out["n_clusters"].sum())}


def host_leg(analysis, sets):
    t0 = time.perf_counter()
    n_clusters = sum(len(analysis.analyze_sample_set(st).clusters) for st in sets)
    dt = time.perf_counter() - t0
    return {"sets_timed": len(sets), "samples_per_set": len(sets[0]), "total_ms": round(dt * 1e3, 3), "ms_per_set": round(dt * 1e3 / len(sets), 4),
            "clusters": n_clusters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--host-sets", type=int, default=50)
    ap.add_argument("--host-large", type=int, default=128)
    ap.add_argument("--sample-slice", type=int, default=0, metavar="P")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace", default=None, metavar="DIR")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds a child process (bench.py, the traced re-run) may take")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import analysis
    eng = pfa.PfEngine(device="cuda:0")
    c4, lg = config4_sets(args.sets), large_set()
    out = {"config4": {"device": device_leg(eng, c4, args.rounds)}, "large": {"device": device_leg(eng, [lg], args.rounds)}}
    if not args.no_host:
        out["config4"]["host"] = host_leg(analysis, c4[:args.host_sets])
        out["large"]["host_subset"] = host_leg(analysis, [lg[:args.host_large]])
        d = out["config4"]["device"]
        out["config4"]["host_over_device_per_set"] = round(out["config4"]["host"]["ms_per_set"] / (d["wall_ms"] / d["sets"]), 1)
    children_ok = True
    if args.sample_slice > 0:
        r = subprocess.run([sys.executable, os.path.join(HERE, "bench.py"), "--gpus", "1", "--sample-slice", str(args.sample_slice), "--samples", "30"],
                           capture_output=True, text=True, cwd=HERE, timeout=args.child_timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        children_ok = r.returncode == 0 and bool(line)
        if children_ok:
            cfg = json.loads(line[-1])["config"]
            d = out["config4"]["device"]
            out["sampling"] = {"pockets": cfg["pockets"], "wall_s": cfg["wall_s"], "ms_per_pocket": cfg["ms_per_pocket"],
                               "analysis_share_of_sampling": (d["wall_ms"] / d["sets"]) / cfg["ms_per_pocket"]}
        else:
            out["sampling"] = {"error": (r.stderr or r.stdout)[-400:]}
    if args.trace and children_ok:              # (after a failed child nothing more is started on the GPU)
        with tempfile.TemporaryDirectory() as tmp:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "sset", "--output-format", "csv", "--",
                   sys.executable, os.path.abspath(__file__), "--no-host", "--rounds", "3", "--sets", str(args.sets)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=HERE, timeout=args.child_timeout)
            stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
            os.makedirs(args.trace, exist_ok=True)
            if r.returncode == 0 and stats:
                shutil.copy(stats[0], os.path.join(args.trace, "sset_kernel_stats.csv"))
                out["trace"] = os.path.join(args.trace, "sset_kernel_stats.csv")
            else:
                out["trace"] = {"error": (r.stderr or r.stdout)[-400:]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
