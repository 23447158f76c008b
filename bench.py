#!/usr/bin/env python3
"""bench.py -- denoising sample-steps/s of the HIP path at BASELINE.json config 2
(256-atom pocket, 6 centers, T=500 schedule, batch=32 per GPU), one process per GPU.

A "step" is one pass of the hot path over one batch: one sample_p_zs_given_zt
(dynamics forward + p(z_s|z_t) update + COM removal) for the B graphs of this rank.  Inputs
(pockets, weights) are resident in HBM before the timed region; the per-step noise is drawn on
the device inside it.  Rank 0 prints ONE JSON line (see the task contract).  A plain run does
nothing beyond set-up, warm-up, the timed steps and the line.  --full adds "roofline" (dominant
kernel, HIP-event timed on the launch stream inside the timed region, topped up after it), the
legs that take runs of their own (rocprofv3 passes, secondary configurations, whole trajectory,
dense mode) and "cpu_baseline" (the CPU oracle timed on the host's cores on a bounded sample;
N=1 only).  --dump-outputs DIR writes what the last timed step computed."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
HOST_SHARE = {}


def pin_host_threads(local_rank, local_world):
    """sharding.pin_host_threads, loaded from its file: this runs first in a rank process, before the package (and with it the
    engine, the models, the HIP runtime) is imported."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_pf_sharding", os.path.join(ROOT, "pharmacophore-diffusion_amd", "sharding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.pin_host_threads(local_rank, local_world)


def step_time_stats(host_s, dev_ms):
    """Per-step times of a timed region: what the host spent enqueuing each step and what the device's timeline shows between the
    events recorded behind consecutive steps.  A stall shows up as ONE step far beyond the median, on one side or on both."""
    def stats(v, scale):
        if not v:
            return None
        srt = sorted(v)
        med = srt[len(srt) // 2]
        worst = max(range(len(v)), key=lambda i: v[i])
        return {"mean": sum(v) / len(v) * scale, "median": med * scale, "max": v[worst] * scale, "argmax": worst,
                "over_3x_median": [[i, round(x * scale, 4)] for i, x in enumerate(v) if x > 3 * med][:8]}
    return {"host_enqueue_ms": stats(host_s, 1e3), "device_timeline_ms": stats(dev_ms, 1.0)}

sys.path.insert(0, ROOT)

MAX_SHARED_GPU_RANKS = 4         # --gpus N with fewer than N GPUs visible: the gloo dry run of the N-rank plumbing, at most this many ranks
PEAK_F32_TFLOPS = 157.3          # MI355X dense fp32 matrix peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0
FLOP_PER_EDGE = 136742.0         # message chain, 2 FLOP / MAC
# roofline.traffic: bytes per launch of the dominant kernel from the hardware counters FETCH_SIZE / WRITE_SIZE, collected by two
# rocprofv3 --pmc child passes of this same script (pmc_passes) that the parent starts BEFORE it touches the GPU; corrected as
# MI355X_MICROARCH.md (HBM section) prescribes: both counters are in KB, FETCH_SIZE reports half of the bytes of wide (16 B per
# lane) reads on gfx950 -- every bulk read of these kernels -- and is doubled, WRITE_SIZE is exact.  null only when rocprofv3 is
# not available (the reason is given next to it).


def _child_json(cmd, env=None, timeout=600):
    """Run a child process and return the last JSON object line of its stdout (None, reason on failure)."""
    import subprocess
    try:
        pr = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    except Exception as e:
        return None, f"{type(e).__name__}: {e}"
    for line in reversed(pr.stdout.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            try:
                return json.loads(line), None
            except Exception:
                pass
    return None, f"exit code {pr.returncode}: {pr.stderr.strip().splitlines()[-1] if pr.stderr.strip() else 'no JSON line'}"


def pmc_passes(inner_args):
    """FETCH_SIZE and WRITE_SIZE per kernel (mean per launch, KB) from two separate rocprofv3 --pmc passes of a short inner run
    of this script (counters are never collected together with --stats or a trace domain; the profiled program is python3
    itself, directly after `--`).  Returns ({kernel name: {"fetch_kb", "write_kb", "launches"}}, None) or (None, reason)."""
    import csv
    import glob
    import shutil
    import tempfile
    from collections import defaultdict
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    env = dict(os.environ, TMPDIR="/tmp")
    res = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        out = tempfile.mkdtemp(prefix="pfbench_pmc_", dir="/tmp")
        try:
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out, "--",
                   "python3", os.path.abspath(__file__)] + inner_args
            _, err = _child_json(cmd, env=env, timeout=600)
            if err is not None:
                return None, f"{counter} pass failed: {err}"
            acc = defaultdict(lambda: [0.0, 0])
            for f in glob.glob(out + "/**/*counter_collection.csv", recursive=True):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        if row.get("Counter_Name") != counter:
                            continue
                        a = acc[row["Kernel_Name"]]
                        a[0] += float(row["Counter_Value"])
                        a[1] += 1
            if not acc:
                return None, f"{counter} pass wrote no counter rows"
            for k, (tot, n) in acc.items():
                d = res.setdefault(k, {"fetch_kb": 0.0, "write_kb": 0.0, "launches": n})
                d["fetch_kb" if counter == "FETCH_SIZE" else "write_kb"] = tot / n
        finally:
            shutil.rmtree(out, ignore_errors=True)
    # a third pass without counters: rocprofv3's own per-kernel durations (the counter passes serialise and stretch the kernels)
    out = tempfile.mkdtemp(prefix="pfbench_trace_", dir="/tmp")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
               "python3", os.path.abspath(__file__)] + inner_args
        _, err = _child_json(cmd, env=env, timeout=600)
        if err is None:
            for f in glob.glob(out + "/**/*kernel_stats.csv", recursive=True):
                with open(f) as fh:
                    for row in csv.DictReader(fh):
                        d = res.setdefault(row["Name"], {"fetch_kb": 0.0, "write_kb": 0.0, "launches": 0})
                        d["calls"] = int(row["Calls"])
                        d["avg_us"] = float(row["AverageNs"]) / 1e3
    finally:
        shutil.rmtree(out, ignore_errors=True)
    return res, None


# FLOPs of one GVP at 2 / MAC (the same formula as pf_debug_work)
def gvp_flops(vi, vo, si, so):
    hd = max(vi, vo)
    return 2.0 * (vi * hd * 3 + hd * vo * 3 + (hd + si) * so + so * vo)


G0, GG, GL = gvp_flops(17, 16, 144, 128), gvp_flops(16, 16, 128, 128), gvp_flops(16, 1, 128, 64)
PER_EDGE, PER_NODE = G0 + 2 * GG, 2 * GG                         # 136,742 / 88,064 at dev.yml depths
HEAD_FLOP = 3 * GG + GL + 2.0 * 64 * 6


def step_launches(pmc, cnt, arch_dev, hoist16):
    """roofline.launches: one entry per kernel a denoising step launches, from the rocprofv3 child passes (durations from the pass
    without counters, FETCH_SIZE / WRITE_SIZE from the counter passes), with the FLOPs each launch stands for (algorithmic:
    SURVEY 8(d) per-unit figures x the units the launch covers; executed: what its items really compute) computed from the
    step's row / edge counts `cnt` (pf_debug_counts).  FLOP models exist for the dev.yml network's small-batch launches; other
    kernels are listed with their time and traffic only."""
    if not pmc:
        return None
    step_k = {k: v for k, v in pmc.items() if "avg_us" in v and any(t in k for t in ("k_n16_", "k_rg_", "k_step_", "k_edge_msg", "k_node_", "k_noise_head"))}
    if not step_k:
        return None
    n_steps = max(v["calls"] for v in step_k.values())
    out = []
    l0 = cnt["ff"] + cnt["pf"] + cnt["fp"] + cnt["pa"]
    l1 = cnt["ff"] + cnt["pf"]
    for k, v in step_k.items():
        if v["calls"] < 0.5 * n_steps:
            continue                                     # set-up kernels (first edge build, tables): not part of a step
        alg = ex = None
        short = k[k.find("k_"):].split("(")[0]
        if arch_dev:
            hoisted = 2.0 * 128 * 128 + 2.0 * 16 * 17 * 3           # what a type-table / center-table row replaces of an edge's first GVP
            if "k_n16_edge<true>" in k or "k_n16_edge_u" in k:
                # (the launch's units are the edges it computes: the "pa" edges whose rows the previous step's last launch computed
                # ahead -- and this launch skipped -- are that launch's units, below)
                alg = PER_EDGE * (l0 - cnt.get("pa_skipped", 0))
                ex = PER_EDGE * l0 - ((cnt["pa"] + cnt["pf"]) * hoisted if hoist16 else 0.0)
                if cnt.get("center_hoist"):
                    ex -= (cnt["ff"] + cnt["fp"]) * hoisted         # ff / fp items start from the center hoist's tables too
                ex -= cnt.get("pa_skipped", 0) * (PER_EDGE - hoisted)     # "pa" regions computed ahead by the previous step's last launch
            elif "k_n16_fused" in k:
                alg = PER_EDGE * l1 + PER_NODE * (cnt["centers"] + cnt["active_atoms"])
                ex = (PER_EDGE + PER_NODE) * l1 + PER_NODE * cnt["centers"]
            elif ("k_rg_node<false, 1, true" in k) or "k_rg_node_hs" in k or "k_rg_tail" in k or "k_n16_tail" in k:
                alg = ex = (PER_NODE + HEAD_FLOP) * cnt["centers"]
                if "k_rg_node_hs_build" in k:                       # + the next call's "pa" items computed ahead, + the center hoist's encoders and products
                    alg = alg + PER_EDGE * cnt.get("pa_skipped", 0)  # (algorithmic: the rows computed ahead that the next call USED; executed: all of them)
                    ex = ex + cnt.get("pa_ahead", 0) * (PER_EDGE - hoisted) + (cnt["centers"] * (2.0 * 128 * 7 + 2 * 2.0 * 128 * 128) if cnt.get("center_hoist") else 0.0)
            elif "k_step_build" in k:
                alg = ex = 0.0
        lps = v["calls"] / n_steps
        e = {"kernel": short[:60], "launches_per_step": round(lps, 3), "avg_us": v["avg_us"],
             "algorithmic_flop": alg, "executed_flop": ex,
             "frac": (alg / (v["avg_us"] * 1e-6) / 1e12 / PEAK_F32_TFLOPS) if alg else None,
             "frac_executed": (ex / (v["avg_us"] * 1e-6) / 1e12 / PEAK_F32_TFLOPS) if ex else None,
             # FETCH_SIZE under-reports 16-B-per-lane reads by 2x on gfx950 (MI355X_MICROARCH.md): the conv kernels' bulk reads are
             # all of that shape (corrected figure), the build kernel's are 4..16-B rows (raw figure); both are given
             "fetch_bytes_raw": v["fetch_kb"] * 1024.0, "fetch_bytes": (1.0 if "k_step_" in k else 2.0) * v["fetch_kb"] * 1024.0,
             "write_bytes": v["write_kb"] * 1024.0}
        out.append(e)
    order = ["k_n16_edge", "k_rg_edge", "k_edge_msg", "k_n16_fused", "k_rg_node", "k_node_", "k_noise_head", "k_rg_tail", "k_n16_tail", "k_step_"]
    out.sort(key=lambda e: next((i for i, t in enumerate(order) if t in e["kernel"]), 99))
    return out


def secondary_legs(args):
    """The other BASELINE configurations as compact objects of the default line: children of this script, started before the
    parent touches the GPU.  config 3 (batch 128, ragged sizes 3-8), a config-4 slice (64 pockets x 30 pharmacophores end to end
    through PharmacophoreDiff.sample) and the training step of config 5 (batch 256, a new batch every step)."""
    me = [sys.executable, os.path.abspath(__file__)]
    # (--full with every leg switched off: the children run as they always have, roofline and its top-up steps included)
    light = ["--full", "--no-cpu-baseline", "--no-dense-leg", "--no-secondary", "--no-traffic", "--gpus", "1"]
    out = {}
    # the training legs first: measured behind the config-4 slice (the most power-hungry child) two of their short runs in three read
    # 10-60 % slow on some boxes, and never when run on their own; 100 steps each, so that a stall of tens of ms weighs less
    j, err = _child_json(me + light + ["--train", "--steps", "100", "--warmup", "10"])
    if j:
        r = j["roofline"]
        out["train_step"] = {"workload": j["config"]["workload"], "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"],
                             "dominant_kernel": r["kernel"], "kernel_avg_us": r["kernel_avg_us"], "frac_executed": r["frac"], "frac": r["frac"],
                             "per_step": j.get("per_step"),
                             "note": "a new batch every step (4 distinct batches rotate); the backward kernels execute exactly the algorithmic FLOPs"}
    else:
        out["train_step"] = {"error": err}
    # the labelled bf16 leg of the same step (never the headline: the reference trains in fp32)
    j, err = _child_json(me + light + ["--train", "--train-dtype", "bf16", "--steps", "100", "--warmup", "10"])
    if j:
        r = j["roofline"]
        out["train_step_bf16"] = {"workload": j["config"]["workload"], "dtype": "bf16", "value": j["value"], "unit": j["unit"],
                                  "ms_per_step": j["ms_per_step"], "dominant_kernel": r["kernel"], "kernel_avg_us": r["kernel_avg_us"],
                                  "per_step": j.get("per_step"),
                                  "note": "to_feats_out / gate products of the message chains' forward and of the gradient kernels on bf16 matrix "
                                          "instructions (operands rounded to nearest even, fp32 accumulation), fp32 master weights, LayerNorm, "
                                          "vector channel, scatter and Adam; contract: tests/test_gpu_train.py (per-tensor gradient cosine vs "
                                          "the fp32 path); no fraction of a roof is formed (mixed f32 / bf16 instructions)"}
    else:
        out["train_step_bf16"] = {"error": err}
    j, err = _child_json(me + light + ["--batch", "128", "--pharm-sizes", "3-8", "--steps", "50", "--warmup", "5", "--no-full-trajectory"])
    if j:
        r = j["roofline"]
        out["config3"] = {"workload": j["config"]["workload"], "value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"],
                          "dominant_kernel": r["kernel"], "kernel_avg_us": r["kernel_avg_us"], "frac_executed": r["frac_executed"], "frac": r["frac"]}
    else:
        out["config3"] = {"error": err}
    j, err = _child_json(me + light + ["--sample-slice", "64"])
    if j:
        out["config4_slice"] = {"workload": j["config"]["workload"], "value": j["value"], "unit": j["unit"], "wall_s": j["config"]["wall_s"],
                                "ms_per_pocket": j["config"]["ms_per_pocket"], "ms_per_step": j["ms_per_step"], **j.get("dominant", {})}
    else:
        out["config4_slice"] = {"error": err}
    return out


def settle_gc():
    """Before a timed region: collect what the set-up left behind and move the survivors out of the collector's sight
    (gc.freeze).  A full collection over the model, the engines and the set-up's tensors takes tens of milliseconds; when the
    collector's thresholds happened to trip inside a 50-130 ms timed region it showed as a run 10-25 % slower than its
    neighbours (about one training-leg run in ten).  The collector stays on; what it scans afterwards is what the region allocates."""
    import gc
    gc.collect()
    gc.freeze()


def gather_rank_times(dt, world, dev, backend, dist):
    """(max over ranks, [every rank's own time]) of a per-rank wall time: what makes a scaling run auditable."""
    where = dev if backend == "nccl" else "cpu"
    own = torch.tensor([dt], device=where, dtype=torch.float64)
    if world == 1:
        return dt, [dt]
    tl = [torch.zeros(1, device=where, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(tl, own)
    per = [float(t_.item()) for t_ in tl]
    return max(per), per


def rccl_world_of(world, backend, dist):
    return dist.get_world_size() if (world > 1 and backend == "nccl") else (1 if world == 1 else 0)


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N fresh processes, one per GPU, BEFORE this process touches
    the GPU (counting devices does not initialise HIP), with the torchrun environment contract; rank 0 prints the JSON
    line.  Never re-executes a process that has initialised the GPU."""
    import socket
    import subprocess
    ndev = torch.cuda.device_count()
    if ndev == 0:
        raise SystemExit("bench.py needs at least one MI355X (no CPU fallback)")
    if n > ndev and n > MAX_SHARED_GPU_RANKS:
        # ranks may share a card only in the plumbing dry run (gloo, no RCCL), and a card takes few processes at once
        raise SystemExit(f"bench.py --gpus {n}: only {ndev} GPU(s) visible here. One rank per GPU is the contract (RCCL); a dry run with "
                         f"ranks sharing a card is limited to {MAX_SHARED_GPU_RANKS} ranks (it uses gloo and reports rccl_world 0).")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for pr in procs:
        rc = max(rc, abs(pr.wait()))
    raise SystemExit(rc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--n-pharm", type=int, default=6)
    ap.add_argument("--timesteps", type=int, default=500)
    ap.add_argument("--pharm-sizes", type=str, default="", help="e.g. 3-8: ragged graphs, sizes cycling through the range (config 3)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-dense-leg", action="store_true", help="skip the extra dense-mode kernel measurement")
    ap.add_argument("--arch", choices=["dev", "class-default"], default="dev",
                    help="dev = configs/dev.yml dynamics block (the headline); class-default = the depth the reference's "
                         "class defaults give (SURVEY 8d secondary run): n_convs=4, n_noise_gvps=3, message_norm=1, radius pf edges")
    ap.add_argument("--prewarm-ms", type=float, default=150.0, help="untimed device activity before the W warm-up steps")
    ap.add_argument("--event-every", type=int, default=-1,
                    help="HIP events around the roofline kernel on every N-th timed step (0: never; default: every 10th, or every "
                         "(steps / 10)-th for long runs; the sample is topped up to 20 launches after the timed region)")
    ap.add_argument("--no-full-trajectory", action="store_true", help="skip the whole-schedule pf_sample leg")
    ap.add_argument("--breakdown", action="store_true", help="extra untimed pass: per-kernel device time to stderr")
    ap.add_argument("--sample-slice", type=int, default=0, metavar="P",
                    help="secondary benchmark (a slice of BASELINE config 4): P synthetic pockets per GPU x --samples pharmacophores "
                         "each (sizes 3..8), T=500, through PharmacophoreDiff.sample end to end (copies, batching, binds, the fused "
                         "reverse process, unbatching into SampledPharmacophore objects); pockets are dealt over the ranks by work")
    ap.add_argument("--samples", type=int, default=30, help="--sample-slice: pharmacophores per pocket")
    ap.add_argument("--max-batch-size", type=int, default=128, help="--sample-slice: graphs per batch")
    ap.add_argument("--lanes", type=int, default=2,
                    help="full-trajectory leg: also report the throughput with this many independent batches in flight (own handle "
                         "and HIP stream each; 1: skip)")
    ap.add_argument("--train-batches", type=int, default=4,
                    help="--train: number of distinct batches the steps rotate through (1: the same batch every step, no re-bind)")
    ap.add_argument("--prefetch", action="store_true",
                    help="--train: bind the NEXT batch on the dynamics' twin handle from a worker thread while a step is enqueued (host time of a "
                         "step 0.94-1.02 -> 0.70 ms; the device-bound step itself pays ~1.5 %% for the twin's weight refresh, so it is off by default)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the compact objects of the other configurations (config 3, config-4 slice, training step)")
    ap.add_argument("--no-traffic", action="store_true", help="skip the two rocprofv3 --pmc child passes behind roofline.traffic")
    ap.add_argument("--train-dtype", choices=["f32", "bf16"], default="f32",
                    help="--train: arithmetic of the dense Linears (f32: what the reference trains in and the line of record; bf16: the "
                         "labelled bf16 leg -- bf16 matrix instructions, fp32 accumulation, fp32 master weights)")
    ap.add_argument("--train", action="store_true",
                    help="secondary benchmark (BASELINE config 5): training steps (forward, backward kernels, Adam) at "
                         "batch 256 per GPU instead of the sampling metric")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline figure: the roofline object with its top-up steps after "
                         "the timed region, the rocprofv3 child passes behind roofline.traffic / roofline.launches, the secondary "
                         "configurations, the whole-trajectory leg, the dense-mode leg and the CPU baseline (the --no-* flags above "
                         "then skip single legs). A plain run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last of them computed (the samples' coordinates and features, as "
                         "the sampler hands them out) to DIR/<name>.npy in float32; the inputs are the same in every run with the "
                         "same arguments")
    args = ap.parse_args()
    if not args.full:
        args.no_traffic = args.no_secondary = args.no_full_trajectory = args.no_dense_leg = args.no_cpu_baseline = True
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args.gpus)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # one process per GPU shares the host with its peers: its CPU slice and pool sizes are fixed before anything touches the GPU
    # or starts a thread pool (one node: LOCAL_WORLD_SIZE = WORLD_SIZE unless the launcher says otherwise)
    global HOST_SHARE
    HOST_SHARE = pin_host_threads(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
    # children first: nothing in this process has touched the GPU yet (a process that has must not start other programs)
    headline = not args.train and args.sample_slice == 0
    pmc, pmc_err, secondary = None, "not collected (a run without --full, --no-traffic, or a multi-rank run)", None
    if rank == 0 and world == 1 and headline:
        if not args.no_traffic:
            inner = ["--full", "--no-cpu-baseline", "--no-dense-leg", "--no-full-trajectory", "--no-secondary", "--no-traffic", "--gpus", "1",
                     "--steps", "20", "--warmup", "2", "--batch", str(args.batch), "--n-prot", str(args.n_prot), "--n-pharm", str(args.n_pharm),
                     "--arch", args.arch] + (["--pharm-sizes", args.pharm_sizes] if args.pharm_sizes else [])
            pmc, pmc_err = pmc_passes(inner)
        default_cfg = (args.batch, args.n_prot, args.n_pharm, args.pharm_sizes, args.arch) == (32, 256, 6, "", "dev")
        if not args.no_secondary and default_cfg:
            secondary = secondary_legs(args)
    import torch.distributed as dist
    ndev = torch.cuda.device_count()
    if ndev == 0:
        raise SystemExit("bench.py needs at least one MI355X (no CPU fallback)")
    dev_index = local_rank % ndev                    # normally local_rank; ranks share a GPU only in the 1-GPU dry run
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    backend = "nccl" if world <= ndev else "gloo"    # RCCL needs one GPU per rank
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import synthetic, schedule

    if args.train:
        train_leg(args, pfa, synthetic, dev, rank, world, backend, dist)
        if world > 1:
            dist.destroy_process_group()
        return
    if args.sample_slice > 0:
        slice_leg(args, pfa, synthetic, dev, rank, world, backend, dist)
        if world > 1:
            dist.destroy_process_group()
        return
    B, T, K, W = args.batch, args.timesteps, args.steps, args.warmup
    if args.event_every < 0:
        # one instrumented step in twenty (five per run for long runs) inside the timed region (an event pair costs 3-6 us of stream
        # time: at every step it would take 7 % off `value`); the sample is topped up to 20 launches after the timed region
        args.event_every = max(20, K // 5)
    # ---- inputs: B distinct pockets per rank (weak scaling: per-GPU work fixed), resident in HBM
    arch_eng, arch_sd = {}, {}
    if args.arch == "class-default":
        arch_eng = dict(n_convs=4, n_noise_gvps=3, message_norm=1, pf_k=0)
        arch_sd = dict(n_convs=4, n_noise_gvps=3)
    eng = pfa.PfEngine(device=dev, **arch_eng)
    eng.load_state_dict(synthetic.make_state_dict(0, **arch_sd))
    xs, hs = zip(*[synthetic.synthetic_pocket(1000 * rank + i, args.n_prot) for i in range(B)])
    prot_x, prot_h = torch.cat(xs).to(dev), torch.cat(hs).to(dev)
    prot_ptr = torch.arange(B + 1, dtype=torch.int64) * args.n_prot
    if args.pharm_sizes:
        lo, hi = (int(v) for v in args.pharm_sizes.split("-"))
        sizes = [lo + (i % (hi - lo + 1)) for i in range(B)]
    else:
        sizes = [args.n_pharm] * B
    pharm_ptr = torch.tensor([0] + list(__import__("itertools").accumulate(sizes)), dtype=torch.int64)
    pp_src, pp_dst = eng.build_pp_edges(prot_x, prot_ptr)
    eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
    Nf = int(pharm_ptr[-1])
    sched = schedule.PredefinedNoiseSchedule('polynomial_2', T, 1e-5)
    coef = schedule.step_coefficients(sched.gamma, T)
    KK = max(K, 20)                                             # room for the roofline top-up pass
    order = [(W + KK - 1 - i) % T for i in range(W + KK)]        # the last W+K steps of the T-step schedule (s = W+K-1 ... 0):
    # with random-init weights the early, high-noise steps (1/alpha_t|s = 1.6) blow the coordinates up; the tail keeps
    # a realistic geometry (all ff edges present).  Work per step does not depend on s.
    carr = eng.coef_array(coef, order)
    # the trajectory's timesteps, as pf_sample announces them itself (layer-0 type tables: one launch per 64 timesteps
    # at set-up instead of one small launch in front of every step)
    eng.prepare_timesteps(carr, W + KK)
    gen = torch.Generator(device=dev).manual_seed(42 + rank)

    EV_MASK = (1 << 2) | (1 << 6) | (1 << 8) | (1 << 4)         # HIP events: edge launches of conv layer 0, of the last layer, node + head
    noise_buf = torch.empty(max(K, W, 20) + 1, Nf, 9, device=dev)

    def run(n, first, event_every=0):
        """n denoising steps.  event_every > 0: every event_every-th step has HIP events around its layer-0 edge-message
        launch (the roofline kernel): a pair of event records costs ~11 us of stream time on this stack, so bracketing
        every launch would inflate a 75 us step by 15 %; one step in event_every keeps the measurement live inside the
        timed region at ~1 us per step."""
        # x columns first, then h; drawn on the device inside the timed region, into a buffer allocated once outside it
        # (a fresh allocation in the timed region occasionally costs tens of milliseconds of host time)
        noise = noise_buf[:n + 1].normal_(generator=gen)
        if first:
            eng.sample_begin(noise[0])
        for i in range(n):
            if event_every:
                eng.profile_enable(EV_MASK if i % event_every == 0 else 0)
            eng.denoise_step(carr[(0 if first else W) + i], noise[i + 1])

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # GPU clocks: the first tens of milliseconds after an idle period run below the sustained clock (the first 100
    # steps after set-up measured 1.1-2.3x slower than the following ones at batch 128-256); the W warm-up steps
    # (0.8 ms at config 2) do not cover that, so the device is kept busy for --prewarm-ms first, on the same pockets
    # (the reverse process is restarted by the warm-up below)
    settle_gc()      # (in front of the pre-warm, not of the timed region: the device must not idle between the warm-up and the region)
    if args.prewarm_ms > 0:
        tp = time.perf_counter()
        while (time.perf_counter() - tp) * 1e3 < args.prewarm_ms:
            run(min(max(K, W), 50), True)
            torch.cuda.synchronize()
    # the pre-warm runs for a time, not a step count: the noise of the warm-up and the timed steps starts from the seed again,
    # so that every run with the same arguments feeds the timed steps the same inputs (--dump-outputs)
    gen.manual_seed(42 + rank)
    # the warm-up steps run with the events on: the library creates its event pairs on first use, and creating them
    # inside the timed region occasionally stalls the host for tens of milliseconds (observed at batch 128-256)
    run(W, True, event_every=1) if W > 0 else eng.sample_begin(torch.randn(Nf, 9, device=dev, generator=gen))
    wprof = eng.profile_read()
    eng.profile_enable(0)
    # the warm-up steps bracket all three matrix launches of a step; the one that takes longest is the roofline kernel, and only
    # that one is bracketed inside the timed region (an event pair costs ~3 us of stream time)
    CLS_BIT = {"edge_msg": 2, "edge_msg_coop": 6, "edge_msg_last": 8, "noise_head": 4}
    wavg = {k: (wprof[k][0] / wprof[k][1] if wprof[k][1] > 0 else 0.0) for k in CLS_BIT}
    dom_cls = max(wavg, key=lambda k: wavg[k]) if any(v > 0 for v in wavg.values()) else "edge_msg_coop"
    l0_cls = "edge_msg" if wprof["edge_msg"][1] > 0 else "edge_msg_coop"
    if pmc:
        # rocprofv3's own durations (child pass, no counters) decide when they are there: an event pair stretches what it brackets
        # by 3-6 us, more on the small node + head launch than on the edge launches
        def cls_of(name):
            if any(t in name for t in ("k_n16_edge<true>", "k_n16_edge_u", "k_rg_edge<true", "k_edge_msg<true", "k_edge_msg_coop<true", "k_edge_msg_coop2<true")):
                return l0_cls
            if any(t in name for t in ("k_n16_fused", "k_n16_edge<false>", "k_rg_edge<false", "k_edge_msg<false", "k_edge_msg_coop<false", "k_edge_msg_coop2<false")):
                return "edge_msg_last"
            if any(t in name for t in ("k_rg_node", "k_node_head", "k_noise_head")):
                return "noise_head"
            return None
        best = {}
        for name, v in pmc.items():
            c_ = cls_of(name)
            if c_ and "avg_us" in v and wavg.get(c_, 0.0) > 0:
                best[c_] = max(best.get(c_, 0.0), v["avg_us"])
        if best:
            dom_cls = max(best, key=lambda k: best[k])
    EV_MASK = 1 << CLS_BIT[dom_cls]
    barrier()
    t0 = time.perf_counter()
    run(K, False, event_every=args.event_every)
    barrier()
    dt = time.perf_counter() - t0
    prof = eng.profile_read()
    eng.profile_enable(0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, eng)
    in_region = prof[dom_cls][1]
    if args.full and 0 < in_region < 20:        # short timed regions: top the sample up to 20 launches, outside `value`
        eng.profile_enable(EV_MASK)
        run(20 - in_region, False)
        torch.cuda.synchronize()
        extra = eng.profile_read()
        eng.profile_enable(0)
        prof = {k: (prof[k][0] + extra[k][0], prof[k][1] + extra[k][1]) for k in prof}

    def max_over_ranks(x):
        t_ = torch.tensor([x], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        if world > 1:
            dist.all_reduce(t_, op=dist.ReduceOp.MAX)
        return float(t_.item())
    per_rank_ms = [dt / K * 1e3]
    if world > 1:                                   # every rank's own time, for auditing a scaling run
        tl = [torch.zeros(1, device=dev if backend == "nccl" else "cpu", dtype=torch.float64) for _ in range(world)]
        dist.all_gather(tl, torch.tensor([dt / K * 1e3], device=dev if backend == "nccl" else "cpu", dtype=torch.float64))
        per_rank_ms = [float(t_.item()) for t_ in tl]
    dt = max_over_ranks(dt)

    wk = eng.work_detail()                                      # work of the last call (actual edge counts)
    flops, bytes_, ne = wk["flops"], wk["bytes"], wk["edges"]
    prof = {k: v for k, v in prof.items()}
    # dominant kernel = the edge-message launch of conv layer 0; which kernel family runs it depends on the batch
    # (pf_debug_kernel_family): row-group kernel k_rg_edge (4 / 8 rows per wave), or the 32-row tile kernels;
    # FLOP = 136,742 per edge it actually processes
    dom = l0_cls
    cnt = eng.counts()
    try:                                                       # what the step's last launch does ahead for the next call (steady state of the region)
        cnt.update(eng.ahead())
    except Exception:
        cnt.update(pa_skipped=0, pa_ahead=0, center_hoist=0, centers=cnt.get("centers", 0))
    fam = eng.kernel_family(0)
    hoist_rows = eng.l0_hoist()
    # the template the launch really ran (pf_host.cpp: run_dynamics): the rocprofv3 kernel name starts with it
    if fam == 16:
        # (batches whose graphs all have the same number of centers run the arithmetic-tiling form k_n16_edge_u of the same items)
        dom_name, dom_match = "k_n16_edge<true> / k_n16_edge_u (conv layer 0: 16-row items on four waves, v_mfma_f32_16x16x4_f32)", "k_n16_edge"
    elif fam in (4, 8):
        rg_a, rg_p = fam // 4, hoist_rows // 4
        dom_name = (f"k_rg_edge<true, {rg_a}, ., {rg_p}> (conv layer 0: {fam} rows per wave" +
                    (f", hoisted pp items {hoist_rows}" if hoist_rows and hoist_rows != fam else "") + ", v_mfma_f32_4x4x1_16b_f32)")
        dom_match = f"k_rg_edge<true, {rg_a},"
    else:
        dom_name = {32: "k_edge_msg<true>", 128: "k_edge_msg_coop<true>"}[fam]
        dom_match = dom_name[:-6]
    edge_ms, edge_n = prof[dom] if dom == dom_cls else wprof[dom]      # (conv layer 0: inside the timed region only when it is the dominant launch)
    l0_edges = wk["executed_edges_per_layer"][0]
    edge_avg_s = edge_ms / max(edge_n, 1) * 1e-3
    edge_flops = FLOP_PER_EDGE * l0_edges
    achieved_tf = edge_flops / edge_avg_s / 1e12 if edge_avg_s > 0 else 0.0
    # static hoist of conv layer 0: its pp edges do not execute their first message GVP (48,678 FLOP of the
    # 136,742) except its gates (4,096); reported next to the algorithmic figure
    n_dyn = ne[0] + ne[1] + ne[2]
    hoisted_edges = (l0_edges - n_dyn if l0_edges < sum(ne) else ne[3]) if hoist_rows else 0
    edge_flops_exec = edge_flops - (48678.0 - 4096.0) * max(hoisted_edges, 0)
    if hoist_rows == 16:                        # n16 form: pp and pf edges start from a type-table row: the h_src block of the first
        hoisted_edges += ne[1]                  # scalar Linear (2 x 128 x 128) and the Vh matrix product (2 x 16 x 17 x 3) are not executed
        edge_flops_exec = edge_flops - (32768.0 + 1632.0) * max(hoisted_edges, 0)

    # ---- the time-dominant launch (dom_cls): name, FLOPs, HIP-event time inside the timed region
    dk_ms, dk_n = prof[dom_cls]
    dk_avg_s = dk_ms / max(dk_n, 1) * 1e-3
    l1_edges = wk["executed_edges_per_layer"][-1]
    fam_last = eng.kernel_family(len(wk["executed_edges_per_layer"]) - 1)
    if dom_cls == l0_cls:
        dk_name, dk_match, dk_alg, dk_exec = dom_name, dom_match, edge_flops, edge_flops_exec
    elif dom_cls == "edge_msg_last":
        if fam_last == 17:
            dk_name, dk_match = "k_n16_fused (last conv layer's edge messages with conv layer 0's node update of the source rows in front; 16-row items, v_mfma_f32_16x16x4_f32)", "k_n16_fused"
            dk_alg = PER_EDGE * l1_edges + PER_NODE * (cnt["centers"] + cnt["active_atoms"])
            dk_exec = (PER_EDGE + PER_NODE) * l1_edges + PER_NODE * cnt["centers"]
        else:
            dk_name = {16: "k_n16_edge<false>", 4: "k_rg_edge<false, 1, ...>", 8: "k_rg_edge<false, 2, ...>"}.get(fam_last, "k_edge_msg<false>") + " (last conv layer's edge messages)"
            dk_match = dk_name.split(" ")[0].split(",")[0]
            dk_alg = dk_exec = PER_EDGE * l1_edges
    else:
        merged = False
        try:
            merged = eng.kernel_family(len(wk["executed_edges_per_layer"])) == 2
        except Exception:
            pass
        if merged:
            dk_name = ("k_rg_node_hs_build (the step's last launch: the node + head items of the centers, every graph's sampler update + "
                       "edge build, and, computed ahead for the NEXT call, its conv-layer-0 'pa' messages -- algorithmic FLOPs: the centers' "
                       "node update + head and the 'pa' edges the next call takes from here instead of computing them -- and the centers' "
                       "encoder / h_src tables, all as workgroups of one grid; ~14 us of its duration is the six-block chain, the rest the "
                       "hand-over and the build)")
        else:
            dk_name = "k_rg_node<false, ., true, .> / k_rg_node_hs (last conv layer's node update of the centers + noise head)"
        dk_match = "k_rg_node"
        dk_alg = dk_exec = (PER_NODE + HEAD_FLOP) * cnt["centers"]
        if merged:      # + what the launch computes ahead for the next call: its "pa" items and the center hoist's encoders / products
            dk_alg += PER_EDGE * cnt.get("pa_skipped", 0)       # (its units: the "pa" edges whose rows the next call takes from it instead of computing them)
            dk_exec += cnt.get("pa_ahead", 0) * (PER_EDGE - (2.0 * 128 * 128 + 2.0 * 16 * 17 * 3)) + \
                (cnt["centers"] * (2.0 * 128 * 7 + 2 * 2.0 * 128 * 128) if cnt.get("center_hoist") else 0.0)
    dk_tf = dk_alg / dk_avg_s / 1e12 if dk_avg_s > 0 else 0.0

    out = {
        "metric": "denoising steps/sec (batch x T) at 256-atom pocket, 6 centers",
        "value": world * B * K / dt, "unit": "sample-steps/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": ("BASELINE config 2: 256-atom pocket, 6 centers, T=500 schedule, batch=32 per GPU, dev.yml network"
                                if (B, args.n_prot, args.n_pharm, args.pharm_sizes, args.arch) == (32, 256, 6, "", "dev") else
                                "BASELINE config 3: mixed pharm sizes 3-8 (ragged graphs), 256-atom pockets, batch=128 per GPU, dev.yml network"
                                if (B, args.n_prot, args.pharm_sizes, args.arch) == (128, 256, "3-8", "dev") else
                                f"custom: {args.n_prot}-atom pockets, centers {args.pharm_sizes or args.n_pharm}, batch={B} per GPU, "
                                + ("dev.yml network" if args.arch == "dev" else "class-default network (n_convs=4, n_noise_gvps=3, message_norm=1, radius pf)")),
                   "batch_per_gpu": B, "n_prot": args.n_prot, "n_pharm": args.pharm_sizes or args.n_pharm, "T": T,
                   "edges_per_step": {"ff": ne[0], "pf": ne[1], "fp": ne[2], "pp": ne[3]},
                   "edges_computed_per_layer": wk["executed_edges_per_layer"],
                   "parallelism": f"graphs sharded over {world} GPU(s), no data-path collective"},
        "roofline": {"bound": "mfma", "kernel": dk_name,
                     # the TIME-dominant launch of a step (chosen by the warm-up's HIP events).  What it EXECUTES over its duration
                     # comes first; `achieved` / `frac` are the contract's algorithmic figures (SURVEY 8d per-unit FLOPs x its units)
                     "frac_executed": (dk_exec / dk_avg_s / 1e12 / PEAK_F32_TFLOPS) if dk_avg_s > 0 else 0.0,
                     "achieved_executed": (dk_exec / dk_avg_s / 1e12) if dk_avg_s > 0 else 0.0,
                     "achieved": dk_tf, "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": dk_tf / PEAK_F32_TFLOPS,
                     "traffic": None, "traffic_unit": "bytes per launch", "traffic_detail": pmc_err,
                     "kernel_avg_us": dk_avg_s * 1e6, "launches_timed": dk_n, "flop_per_launch": dk_alg,
                     "executed_flop_per_launch": dk_exec,
                     "note": "the launch a step spends most time in, timed by HIP events on the launch stream inside the timed region (an event "
                             "pair adds ~3 us to what it brackets: the rocprofv3 durations in `launches` are that much shorter). Algorithmic "
                             "FLOP: 136,742 per edge message + 88,064 per updated node (+ 153,056 per center for the noise head), SURVEY 8d; "
                             "executed FLOP: what the launch's items really compute (the fused launch updates a source row once per edge item "
                             "that reads it; conv layer 0 skips what the static hoist's type tables provide). Outputs equal the dense "
                             "reference computation; rows / edges that cannot reach the output are not computed.",
                     "conv_layer0_launch": {"kernel": dom_name, "kernel_avg_us": edge_avg_s * 1e6, "launches_timed": edge_n,
                                            "timed": "inside the timed region" if dom == dom_cls else "warm-up steps",
                                            "flop_per_launch": edge_flops, "executed_flop_per_launch": edge_flops_exec,
                                            "hoisted_edges_per_launch": hoisted_edges, "frac": achieved_tf / PEAK_F32_TFLOPS,
                                            "frac_executed": (edge_flops_exec / edge_avg_s / 1e12 / PEAK_F32_TFLOPS) if edge_avg_s > 0 else 0.0},
                     "whole_step": {"executed_flop": wk["executed_flops"], "executed_tflops": wk["executed_flops"] / (dt / K) / 1e12,
                                    "frac_f32_peak_executed": wk["executed_flops"] / (dt / K) / 1e12 / PEAK_F32_TFLOPS,
                                    "dense_reference_flop": flops, "dense_reference_bytes": bytes_,
                                    "note": "dense_reference_* = what the reference's dense computation of this step would execute / move "
                                            "(SURVEY 8d formulas): information only -- the kernels do not execute or move it (dead-work "
                                            "elimination is exact), so no fraction is formed from it"}},
        "rccl_world": (dist.get_world_size() if (world > 1 and backend == "nccl") else (1 if world == 1 else 0)),
        "host": HOST_SHARE,
        "per_rank_ms_per_step": per_rank_ms,
    }
    if pmc is not None:
        launches = step_launches(pmc, cnt, args.arch == "dev", hoist_rows == 16)
        if launches:
            out["roofline"]["launches"] = launches
            out["roofline"]["launches_sum_us"] = sum(e["avg_us"] * e["launches_per_step"] for e in launches)
            out["roofline"]["launches_note"] = ("every kernel a denoising step launches: avg_us = rocprofv3 --kernel-trace --stats of a child pass of this "
                                                "script (no counters, --steps 20 --warmup 2); fetch / write bytes from two --pmc child passes; their sum "
                                                "stays below ms_per_step (the rest: gaps between launches and the per-step noise draw)")
        hits = {k: v for k, v in pmc.items() if dk_match in k and v.get("launches", 0) > 0}
        if hits:
            kname = max(hits, key=lambda k: hits[k]["launches"])
            d = hits[kname]
            fetch_b, write_b = 2.0 * d["fetch_kb"] * 1024.0, d["write_kb"] * 1024.0
            if dk_match == "k_n16_fused":        # gathers: the edges' end points + the source rows' partial message rows and type-table rows; stores: partial rows
                alg_b, alg_note = 736.0 * l1_edges + 5 * 704.0 * l1_edges + 704.0 * l1_edges / 3.0, \
                    "per edge: 736 B of end-point rows (SURVEY 8d) + ~5 partial / residual rows of 704 B for its source's node update; one 704-B partial row stored per (item, destination) run"
            else:
                alg_b, alg_note = 736.0 * l0_edges + 704.0 * l0_edges / 3.0, \
                    "gathers 736 B per edge (SURVEY 8d) + one 704-B partial message row per (item, destination) run (~1 in 3 edges)"
            out["roofline"]["traffic"] = fetch_b + write_b
            out["roofline"]["traffic_detail"] = {
                "kernel": kname[:120], "launches": d["launches"], "FETCH_SIZE_KB": d["fetch_kb"], "WRITE_SIZE_KB": d["write_kb"],
                "fetch_bytes_corrected": fetch_b, "fetch_bytes_raw": d["fetch_kb"] * 1024.0, "write_bytes": write_b,
                "correction": "FETCH_SIZE (KB) x 2: gfx950 tallies the 128-B requests of 16-B-per-lane reads at 64 B (MI355X_MICROARCH.md, "
                              "HBM section) -- the bulk reads of the conv kernels are all of that shape; WRITE_SIZE (KB) exact; memory-side "
                              "requests of the L2, Infinity-Cache hits included",
                "source": "two rocprofv3 --kernel-trace --pmc child passes of this script (--steps 20 --warmup 2), mean per launch",
                "algorithmic_bytes_per_launch": alg_b, "algorithmic_note": alg_note,
                "per_step_all_kernels_bytes": (sum((e["fetch_bytes"] + e["write_bytes"]) * e["launches_per_step"] for e in launches)
                                               if launches else None),
                "per_step_note": "sum over `launches` (corrected fetch for the conv kernels, raw for the build kernel), launches of one step only"}
        else:
            out["roofline"]["traffic_detail"] = f"no kernel matching {dk_match!r} in the counter output"
    if secondary is not None:
        out["secondary"] = secondary

    out["roofline"]["launches_timed_in_region"] = in_region
    if not args.no_full_trajectory:
        def eng2_factory(k):                        # lane k: its own handle, the same weights, other pockets of the same shape
            e2 = pfa.PfEngine(device=dev, **arch_eng)
            e2.load_state_dict(synthetic.make_state_dict(0, **arch_sd))
            xs2, hs2 = zip(*[synthetic.synthetic_pocket(5000 + 1000 * rank + 100 * k + i, args.n_prot) for i in range(B)])
            px2, ph2 = torch.cat(xs2).to(dev), torch.cat(hs2).to(dev)
            s2, d2 = e2.build_pp_edges(px2, prot_ptr)
            e2.set_batch(px2, ph2, prot_ptr, pharm_ptr, s2, d2)
            return e2
        coef_bounded = schedule.step_coefficients(schedule.PredefinedNoiseSchedule('polynomial_2', T, 0.25).gamma, T)
        out["full_trajectory"] = full_trajectory(args, eng, coef, dev, rank, world, B, T, Nf, barrier, max_over_ranks, eng2_factory,
                                                 coef_bounded)

    if args.breakdown and rank == 0:
        eng.profile_enable(0x1ff)
        run(min(K, 20), False)
        torch.cuda.synchronize()
        for k, (ms, n) in eng.profile_read().items():
            print(f"[breakdown] {k:12s} {ms / max(n, 1) * 1e3:9.1f} us/launch  x{n}", file=sys.stderr)
        eng.profile_enable(0)

    if rank == 0 and world == 1 and not args.no_dense_leg:
        out["roofline"]["dense_kernel"] = dense_leg(pfa, synthetic, dev, prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst,
                                                    carr, W, min(K, 50), Nf)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, prot_x.cpu(), prot_h.cpu(), prot_ptr, pharm_ptr, pp_src, pp_dst, T)
    if not args.full:
        # the roofline figures are read after the top-up steps (--full): a plain line carries the headline only.  The timed steps
        # keep their HIP events, so that they are the same steps with and without --full
        del out["roofline"]
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def dump_outputs(out_dir, eng):
    """--dump-outputs: what the timed steps computed, read after the last of them -- the batch's current sample as the sampler
    hands it to its caller (pf_sample_frame: pharm_x = coordinates in the pockets' frame [Nf, 3], pharm_h = features [Nf, 6],
    unscaled), float32.  Reading it leaves the sampling state as it is."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    x, h = eng.sample_frame()
    for name, t in (("pharm_x", x), ("pharm_h", h)):
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().to(torch.float32).cpu().numpy())


def full_trajectory(args, eng, coef, dev, rank, world, B, T, Nf, barrier, max_over_ranks, eng2_factory=None, coef_bounded=None):
    """SURVEY.md 8(d) row 1 as written: wall time of the WHOLE T-step reverse loop (pharmacodiff.py:466-472 equivalent)
    for the rank's batch -- pf_sample: begin, T steps, final frame, enqueued without a host sync; x_T, h_T ~ N(0, I) at
    the pocket COM, seed-0 weights, noise drawn on the device inside the timed region -- reported as B*T / wall.  With
    untrained weights the centers drift outwards over the schedule (1/alpha_T ~ 300 x the initial spread), so late steps
    see different neighbour sets than a trained model's would; the edge counts of the last step are reported.  Three
    repetitions, median; max over ranks."""
    arr = eng.coef_array(coef, reversed(range(T)))
    gen = torch.Generator(device=dev).manual_seed(4242 + rank)
    buf = torch.empty(T + 1, Nf, 9, device=dev)
    times = []
    settle_gc()
    for rep in range(4):
        barrier()
        t0 = time.perf_counter()
        noise = buf.normal_(generator=gen)
        x0, h0 = eng.sample(arr, T, noise)
        barrier()
        if rep:                                    # repetition 0 warms up (type tables for all T timesteps, allocations)
            times.append(max_over_ranks(time.perf_counter() - t0))
    times.sort()
    dt = times[len(times) // 2]
    wk = eng.work_detail()
    bounded = None
    if coef_bounded is not None:
        # the same reverse process in the regime a trained model lives in: schedule precision 0.25 bounds 1 / alpha_T by 2, the
        # centers stay inside the pocket at every step and every ff / pf / fp edge exists throughout (the configuration of
        # tests/golden/traj_c1_T500_bounded.npz, which pins it frame by frame against the reference)
        arr_b = eng.coef_array(coef_bounded, reversed(range(T)))
        tb = []
        for rep in range(3):
            barrier()
            t0 = time.perf_counter()
            xb, hb = eng.sample(arr_b, T, buf.normal_(generator=gen))
            barrier()
            if rep:
                tb.append(max_over_ranks(time.perf_counter() - t0))
        wkb = eng.work_detail()
        dtb = min(tb)
        bounded = {"value": world * B * T / dtb, "unit": "sample-steps/s", "wall_ms": dtb * 1e3, "schedule_precision": 0.25,
                   "max_abs_coordinate": float(xb.abs().max()), "finite": bool(torch.isfinite(xb).all() and torch.isfinite(hb).all()),
                   "edges_last_step": dict(zip(("ff", "pf", "fp", "pp"), wkb["edges"])),
                   "note": "schedule precision 0.25 instead of 1e-5: random-init weights cannot cancel the sampler's 1 / alpha factors, so "
                           "the bound on the coordinates comes from the schedule; same kernels, same launch policy"}
    lanes = None
    if args.lanes > 1 and world == 1 and eng2_factory is not None:      # informational leg, single-rank runs only; never costs the line
        try:
            lanes = batches_in_flight(args, eng2_factory, coef, dev, rank, world, B, T, Nf, barrier, max_over_ranks, arr)
        except Exception as e:                                          # (e.g. no memory for the extra handles)
            lanes = {"error": f"{type(e).__name__}: {e}"}
    drifted = {"value": world * B * T / dt, "unit": "sample-steps/s", "wall_ms": dt * 1e3, "ms_per_step": dt / T * 1e3,
               "repetitions_ms": [round(t * 1e3, 3) for t in times], "finite": bool(torch.isfinite(x0).all() and torch.isfinite(h0).all()),
               "max_abs_coordinate": float(x0.abs().max()),
               "edges_last_step": dict(zip(("ff", "pf", "fp", "pp"), wk["edges"])),
               "edges_computed_per_layer_last_step": wk["executed_edges_per_layer"],
               "note": "schedule precision 1e-5 with random-init weights: the centers drift out of the pockets (no ff edges at the end, "
                       "fewer conv-layer-0 edges) -- a lighter workload than a trained model's, reported for continuity with rounds 1-3"}
    # the figure of record is the bounded regime (what a trained model's trajectory looks like); the drifted one rides along
    lead = bounded if bounded is not None else drifted
    return {"lanes": lanes, "value": lead["value"], "unit": "sample-steps/s", "T": T, "wall_ms": lead["wall_ms"],
            "ms_per_step": lead["wall_ms"] / T, "regime": "bounded (schedule precision 0.25)" if bounded is not None else "drifted (schedule precision 1e-5)",
            "bounded": bounded, "drifted": drifted, "finite": lead["finite"], "max_abs_coordinate": lead["max_abs_coordinate"],
            "edges_last_step": lead["edges_last_step"],
            "note": "whole T-step reverse process of the rank's batch through pf_sample, noise generation included; `value` is the bounded "
                    "regime's, where every center stays inside its pocket and the ff / pf / fp edges exist at every step"}


def batches_in_flight(args, factory, coef, dev, rank, world, B, T, Nf, barrier, max_over_ranks, arr):
    """Throughput with args.lanes independent batches of the SAME configuration in flight at once, each on its own handle
    and HIP stream (what PharmacophoreDiff.sample does when a job has more than one batch: four of the five launches of a
    batched step leave part of the chip idle, so independent batches overlap).  Reported beside the single-batch numbers,
    never as `value`: the unit of work is L batches of B graphs, T steps each."""
    L = args.lanes
    engs = [factory(k) for k in range(L)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(L)]
    gens = [torch.Generator(device=dev).manual_seed(777 + 13 * rank + k) for k in range(L)]
    bufs = [torch.empty(T + 1, Nf, 9, device=dev) for _ in range(L)]
    times = []
    for rep in range(4):
        barrier()
        t0 = time.perf_counter()
        for k in range(L):
            with torch.cuda.stream(streams[k]):
                engs[k].sample(arr, T, bufs[k].normal_(generator=gens[k]))
        barrier()
        if rep:
            times.append(max_over_ranks(time.perf_counter() - t0))
    times.sort()
    dt = times[len(times) // 2]
    return {"batches_in_flight": L, "value": world * L * B * T / dt, "unit": "sample-steps/s", "wall_ms": dt * 1e3,
            "repetitions_ms": [round(t * 1e3, 3) for t in times],
            "note": f"{L} independent batches of {B} graphs (other pockets, same shape), each through pf_sample on its own handle and stream"}


def slice_leg(args, pfa, synthetic, dev, rank, world, backend, dist):
    """A slice of BASELINE config 4 (dataset-scale sampling: every pocket x 30 pharmacophores, T = 500): wall time of
    PharmacophoreDiff.sample over P x world synthetic pockets -- what test.py / generate_pharmacophores.py spend their time in.
    One JSON line; value = pharmacophores x T / wall, max over ranks."""
    P, S, T = args.sample_slice, args.samples, args.timesteps
    dyn = dict(vector_size=16, n_convs=2, n_hidden_scalars=128, message_norm='mean', dropout=0.1, ff_k=0, pf_k=5,
               n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4)
    cut = {'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9}
    m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=T, graph_config={'graph_cutoffs': cut},
                              dynamics_config=dyn, precision=1e-5)
    sd = dict(synthetic.make_state_dict(0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    pockets = []
    for i in range(P * world):                                   # every rank builds the whole list; sample() deals the batches
        x, h = synthetic.synthetic_pocket(i, args.n_prot)
        pockets.append(pfa.build_initial_complex_graph(x, h, cutoffs=cut, pharm_atom_positions=torch.zeros(1, 3),
                                                       pharm_atom_features=torch.zeros(1, 6)))
    sizes = (([3] * 5 + [4, 5, 6, 7, 8]) * (S // 10 + 1))[:S]
    n_pharms = [sizes for _ in pockets]

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    with torch.no_grad():
        torch.manual_seed(0)
        m.sample(pockets[:min(len(pockets), 8)], n_pharms[:min(len(pockets), 8)], max_batch_size=args.max_batch_size)   # handles, tables
        settle_gc()
        barrier()
        torch.manual_seed(0)
        t0 = time.perf_counter()
        out = m.sample(pockets, n_pharms, max_batch_size=args.max_batch_size, rank=rank, world_size=world)
        barrier()
        dt = time.perf_counter() - t0
    n = sum(len(o) for o in out)
    dominant = {}
    if rank == 0:
        # the dominant kernel of such a job: conv layer 0's edge-message launch of one full batch (copies of a few pockets, pocket
        # sharing on), timed by HIP events over 20 steps at the end of the schedule on a batch bound like sample() binds it
        try:
            from pharmacoforge_amd import schedule
            eng = m.dynamics.engine()
            per = max(args.max_batch_size // S, 1)
            copies = [c for k in range(per) for c in pfa.copy_graph(pockets[k], S, pharm_feats_per_copy=torch.tensor(sizes))][:args.max_batch_size]
            gb = pfa.batch(copies)
            eng.set_batch(gb.prot_x, gb.prot_h, gb.prot_ptr, gb.pharm_ptr, gb.pp_src, gb.pp_dst, pocket_uid=gb.pocket_uid)
            coef = schedule.step_coefficients(schedule.PredefinedNoiseSchedule('polynomial_2', T, 1e-5).gamma, T)
            nst = 25
            carr = eng.coef_array(coef, list(range(nst - 1, -1, -1)))
            eng.prepare_timesteps(carr, nst)
            Nfb = int(gb.pharm_ptr[-1])
            nz = torch.randn(nst + 1, Nfb, 9, device=dev)
            eng.sample_begin(nz[0])
            for i in range(nst):
                eng.profile_enable(((1 << 2) | (1 << 6)) if i >= 5 else 0)
                eng.denoise_step(carr[i], nz[i + 1])
            torch.cuda.synchronize()
            prof = eng.profile_read()
            eng.profile_enable(0)
            key = "edge_msg" if prof["edge_msg"][1] > 0 else "edge_msg_coop"
            ms, cnt = prof[key]
            wk = eng.work_detail()
            l0 = wk["executed_edges_per_layer"][0]
            ne = wk["edges"]
            fam, hoist = eng.kernel_family(0), eng.l0_hoist()
            avg = ms / max(cnt, 1) * 1e-3
            hoisted = max(l0 - (ne[0] + ne[1] + ne[2]), 0) if hoist else 0
            fl = FLOP_PER_EDGE * l0
            fl_ex = fl - ((32768.0 + 1632.0) * (hoisted + ne[1]) if hoist == 16 else (48678.0 - 4096.0) * hoisted)
            dominant = {"dominant_kernel": ("k_n16_edge<true>" if fam == 16 else f"k_rg_edge<true, {fam // 4}, ., {hoist // 4}>") + " (conv layer 0, pocket sharing)",
                        "kernel_avg_us": avg * 1e6, "batch_graphs": gb.batch_size, "edges_computed": l0,
                        "frac_executed": fl_ex / avg / 1e12 / PEAK_F32_TFLOPS if avg > 0 else 0.0,
                        "frac": fl / avg / 1e12 / PEAK_F32_TFLOPS if avg > 0 else 0.0}
        except Exception as e:                       # informational: never costs the line
            dominant = {"dominant_kernel": None, "error": f"{type(e).__name__}: {e}"}
    dt, per_rank_s = gather_rank_times(dt, world, dev, backend, dist)
    if world > 1:
        sm = torch.tensor([float(n)], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        n = int(sm[0])
    if rank == 0:
        print(json.dumps({
            "metric": "denoising steps/sec end to end through PharmacophoreDiff.sample (config-4 slice)", "value": n * T / dt,
            "unit": "sample-steps/s", "n_gpus": world, "steps": T, "warmup": 0, "ms_per_step": dt / T * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "rccl_world": rccl_world_of(world, backend, dist), "per_rank_ms_per_step": [v / T * 1e3 for v in per_rank_s],
            "host": HOST_SHARE,
            "config": {"workload": f"BASELINE config 4 slice: {P} pockets per GPU x {S} pharmacophores (sizes 3-8), {args.n_prot}-atom "
                                   f"pockets, T={T}, max_batch_size {args.max_batch_size}, dev.yml network",
                       "pockets": P * world, "pharmacophores": n, "wall_s": dt, "ms_per_pocket": dt / max(P, 1) * 1e3,
                       "batches_in_flight": "auto (2; 4 for batches of <= 32 graphs)" if m.sample_lanes is None else m.sample_lanes,
                       "parallelism": f"batches dealt over {world} GPU(s) by work, no data-path collective"},
            "dominant": dominant}))


def train_leg(args, pfa, synthetic, dev, rank, world, backend, dist):
    """BASELINE config 5: one training step = PharmacophoreDiff.training_step (noising, dynamics forward with dropout,
    loss) + backward (HIP gradient kernels) + gradient all-reduce over the ranks + Adam.  B graphs per GPU (weak)."""
    B = args.batch if args.batch != 32 else 256
    K, W = args.steps, args.warmup
    lo, hi = (int(v) for v in (args.pharm_sizes or "4-8").split("-"))
    sizes = [lo + (i % (hi - lo + 1)) for i in range(B)]
    T = 100                                                     # dev.yml diffusion.n_timesteps
    dyn = dict(vector_size=16, n_convs=2, n_hidden_scalars=128, message_norm='mean', dropout=0.1, ff_k=0, pf_k=5,
               n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4)
    m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=T,
                              graph_config={'graph_cutoffs': {'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9}}, dynamics_config=dyn,
                              precision=1e-5, lr_scheduler_config={'base_lr': 1e-4, 'weight_decay': 1e-12})
    sd = dict(synthetic.make_state_dict(0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).train()
    pockets = [synthetic.synthetic_pocket(1000 * rank + i, args.n_prot) for i in range(B)]
    m.dynamics.set_train_precision(args.train_dtype)
    eng = m.dynamics.engine()
    gen = torch.Generator().manual_seed(7 + rank)
    # a rotating set of DISTINCT batches (other pocket order, other center counts: other ptr arrays and coordinates), as a
    # data loader delivers them: every step pays the per-batch bind (pf_set_pocket_batch) like train.py does.  (The int32 host
    # form of the index arrays is made once per graph object -- PocketGraph.index_arrays_i32, which graph.batch() calls at
    # collate time, i.e. in the data loader's workers -- so it is not part of the timed steps here either.)
    graphs = []
    for r in range(args.train_batches):
        order = [(i + r * (B // max(args.train_batches, 1))) % B for i in range(B)]
        sz = [sizes[(i + r) % B] for i in range(B)]
        xs, hs = [pockets[i][0] for i in order], [pockets[i][1] for i in order]
        prot_x, prot_h = torch.cat(xs), torch.cat(hs)
        prot_ptr = torch.arange(B + 1, dtype=torch.int64) * args.n_prot
        pharm_ptr = torch.tensor([0] + list(__import__("itertools").accumulate(sz)), dtype=torch.int64)
        pp_src, pp_dst = eng.build_pp_edges(prot_x.to(dev), prot_ptr)
        Nf = int(pharm_ptr[-1])
        x0 = torch.cat([xs[i].mean(0, keepdim=True) + 2.0 * torch.randn(sz[i], 3, generator=gen) for i in range(B)])
        h0 = torch.nn.functional.one_hot(torch.randint(0, 6, (Nf,), generator=gen), 6).float()
        graphs.append(pfa.PocketGraph(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst, pharm_x0=x0, pharm_h0=h0).to(dev))
    it = [0]
    # optim.Adam(lr, weight_decay) of pharmacodiff.py:253 as one fused kernel on the flat parameter vector
    opt = pfa.FlatAdam(m.dynamics, lr=1e-4, weight_decay=1e-12)

    def step():
        opt.zero_grad(lazy=True)
        g = graphs[it[0] % len(graphs)]
        it[0] += 1
        loss = m.training_step(g, 0)
        if len(graphs) > 1 and args.prefetch:
            # what a data loader's look-ahead allows: the NEXT batch is bound on the twin handle by a worker thread while this
            # thread enqueues the backward and the optimiser step (models.PharmRecDynamicsGVP.prefetch_graph)
            m.dynamics.prefetch_graph(graphs[it[0] % len(graphs)])
        loss.backward()
        if world > 1:
            m.dynamics.allreduce_gradients()
        opt.step()
        return loss

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # sustained clocks before the warm-up (see main).  Every step of this leg holds a collective (the gradient all-reduce), so the
    # ranks must leave the loop after the SAME number of steps: a clock read per rank let one rank start a step its peers never
    # joined (an intermittent hang of the two-rank run) -- rank 0's verdict is broadcast each round
    settle_gc()      # (in front of the pre-warm: the device must not idle between the warm-up and the timed region)
    tp = time.perf_counter()
    while True:
        go = (time.perf_counter() - tp) * 1e3 < args.prewarm_ms
        if world > 1:
            flag = torch.tensor([1 if go else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
            dist.broadcast(flag, src=0)
            go = bool(int(flag.item()))
        if not go:
            break
        step()
        torch.cuda.synchronize()
    # the warm-up steps run with the events on: the library creates its event pairs on first use, and creating them inside the
    # timed region occasionally stalls the host for tens of milliseconds (one run in five of this leg read 1.35-1.6 ms per step
    # for a 1.26 ms step until this was moved here, as in the headline leg)
    eng.profile_enable(1 << 11)
    for _ in range(W):
        step()
    eng.profile_enable(0)
    eng.profile_read_train()
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]
    for e in step_ev:
        e.record()                                 # (created AND first recorded out here: see above)
    ev_every = max(1, K // 8)                      # HIP events around the edge-message backward launches of every n-th step
    # The region is run TWICE with everything in it -- the instrumented / plain step pattern, the per-step event records, the clock
    # reads -- and the second pass is the timed one.  The first process on a fresh box showed ONE host stall of ~4 ms at the second
    # step of its first such region (per_step caught it: host 5.3 ms, device timeline 4.8 ms at step 1, `BENCH_r04`'s 1.336 ms bf16
    # leg was the same thing), never in a second region: something the loop's exact pattern touches for the first time.  A rehearsal
    # of the pattern is warm-up like any other.
    for rehearsal in (True, False):
        barrier()
        step_ev[0].record()
        t0 = time.perf_counter()
        host_s = []
        for i in range(K):
            th = time.perf_counter()
            eng.profile_enable((1 << 11) if i % ev_every == 0 else 0)
            loss = step()
            step_ev[i + 1].record()                # (one event record per step: the device's own timeline of the region)
            host_s.append(time.perf_counter() - th)
        eng.profile_enable(0)
        barrier()
        dt = time.perf_counter() - t0
        if rehearsal:
            rehearsal_ms = dt / K * 1e3
            eng.profile_read_train()
    prof = eng.profile_read_train()
    dev_ms = [step_ev[i].elapsed_time(step_ev[i + 1]) for i in range(K)]
    per_step = step_time_stats(host_s, dev_ms)
    per_step["rehearsal_ms_per_step"] = rehearsal_ms      # (the untimed first pass over the same K steps)
    # what a step costs the HOST when the queue is empty (inside the region the host runs ahead until the queue is full, and its
    # time per step then mirrors the device's): a few steps with a synchronisation behind each, outside every timed figure
    idle = []
    for i in range(12):
        torch.cuda.synchronize()
        th = time.perf_counter()
        step()
        idle.append(time.perf_counter() - th)
    barrier()
    per_step["host_enqueue_idle_queue_ms"] = sorted(idle[2:])[len(idle[2:]) // 2] * 1e3
    host_mean = sum(host_s) / max(len(host_s), 1)
    _, per_rank_host = gather_rank_times(host_mean, world, dev, backend, dist)
    dt, per_rank_s = gather_rank_times(dt, world, dev, backend, dist)
    # dominant kernel of the step: k_bwd_edge_level (one launch per message-GVP level and conv layer).  Algorithmic work
    # of the message chain's backward = 2 x its forward (one product for the input gradient, one for the weight
    # gradient, per Linear): 2 x 136,742 FLOP per edge the layer computes, over its n_message_gvps launches
    wk = eng.work_detail()
    lvl_ms, lvl_n = prof["bwd_edge_level"]
    edges_exec = sum(wk["executed_edges_per_layer"])
    launches_per_step = 3 * len(wk["executed_edges_per_layer"])
    steps_timed = lvl_n / max(launches_per_step, 1)
    bwd_flop_per_step = 2.0 * FLOP_PER_EDGE * edges_exec
    lvl_s_per_step = lvl_ms * 1e-3 / max(steps_timed, 1e-9)
    ach = bwd_flop_per_step / lvl_s_per_step / 1e12 if lvl_ms > 0 else 0.0
    if rank == 0:
        print(json.dumps({
            "metric": "training graphs/sec (forward + backward + Adam), 256-atom pockets, 4-8 centers", "value": world * B * K / dt,
            "unit": "graphs/s", "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": dt / K * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.train_dtype, "data": "synthetic",
            "rccl_world": rccl_world_of(world, backend, dist), "per_rank_ms_per_step": [v / K * 1e3 for v in per_rank_s],
            "per_rank_host_enqueue_ms": [v * 1e3 for v in per_rank_host], "per_step": per_step, "host": HOST_SHARE,
            "config": {"workload": f"BASELINE config 5: training step, batch={B} per GPU, {args.n_prot}-atom pockets, centers {lo}-{hi}, "
                                   "dropout 0.1, dev.yml network", "batch_per_gpu": B, "n_prot": args.n_prot,
                       "distinct_batches": len(graphs), "bind_prefetch": bool(len(graphs) > 1 and args.prefetch),
                       "parallelism": f"data parallel over {world} GPU(s): one all-reduce of the flat gradient per step"},
            "roofline": {"bound": "mfma", "kernel": "k_bwd_edge_level (all levels of a step)", "achieved": ach, "peak": PEAK_F32_TFLOPS,
                         "unit": "TFLOP/s", "frac": ach / PEAK_F32_TFLOPS, "traffic": None, "traffic_detail": "profiles/r03/train_pmc_hbm.csv (rocprofv3 --pmc passes of this command)",
                         "kernel_avg_us": lvl_ms / max(lvl_n, 1) * 1e3, "launches_timed": lvl_n, "launches_per_step": launches_per_step,
                         "edge_backward_ms_per_step": lvl_s_per_step * 1e3, "flop_per_step": bwd_flop_per_step,
                         "edges_computed_per_layer": wk["executed_edges_per_layer"],
                         "note": "HIP events around the edge-message backward launches of every n-th timed step; FLOP = 2 x 136,742 "
                                 "per edge a layer computes (backward of the message chain = two products per Linear)"},
            "final_loss": float(loss.detach())}))


def dense_leg(pfa, synthetic, dev, prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst, carr, W, K, Nf):
    """The same steps with dead-work elimination switched off (every conv layer computed densely, like the
    reference does): times k_edge_msg -- one wave per 32 edges over ALL edges of conv layer 0 -- the kernel that
    dominates whenever a layer cannot be pruned (deeper nets, radius pf edges).  Extra information, outside the
    timed region of `value`."""
    os.environ["PFDYN_NO_PRUNE"] = "1"
    os.environ["PFDYN_NO_PRE"] = "1"
    os.environ["PFDYN_RG_ROWS_MAX"] = "0"          # the 32-row tile kernels (what large dense launches and training use)
    try:
        eng = pfa.PfEngine(device=dev)
    finally:
        del os.environ["PFDYN_NO_PRUNE"], os.environ["PFDYN_NO_PRE"], os.environ["PFDYN_RG_ROWS_MAX"]
    eng.load_state_dict(synthetic.make_state_dict(0))
    eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
    gen = torch.Generator(device=dev).manual_seed(7)
    noise = torch.randn(K + 1, Nf, 9, device=dev, generator=gen)
    eng.sample_begin(noise[0])
    for i in range(5):
        eng.denoise_step(carr[W + i], noise[i + 1])
    torch.cuda.synchronize()
    eng.profile_enable(1 << 2)
    t0 = time.perf_counter()
    for i in range(K):
        eng.denoise_step(carr[W + i], noise[i + 1])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms, n = eng.profile_read()["edge_msg"]
    wk = eng.work_detail()
    fl = FLOP_PER_EDGE * wk["executed_edges_per_layer"][0]
    avg = ms / max(n, 1) * 1e-3
    B = int(prot_ptr.numel() - 1)
    return {"kernel": "k_edge_msg", "edges_per_launch": wk["executed_edges_per_layer"][0], "kernel_avg_us": avg * 1e6,
            "achieved": fl / avg / 1e12, "peak": PEAK_F32_TFLOPS, "unit": "TFLOP/s", "frac": fl / avg / 1e12 / PEAK_F32_TFLOPS,
            "dense_mode_sample_steps_per_s": B * K / dt}


def cpu_baseline(args, prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst, T):
    """The CPU oracle (a PyTorch fp32 restatement of the reference path, oracle/pf_oracle.py) on the same workload on
    this box's host cores.  torch's default thread count (every hardware thread) oversubscribes this workload, so the
    oracle is timed at 8 (the survey container's count), 16, 32 and 64 threads -- a bounded sample each, ~args.cpu_seconds
    in total -- and the BEST is reported with its thread count.  Reported baseline, not the target."""
    from oracle import pf_oracle as O
    cfg = O.DynamicsConfig()
    sd = O.make_state_dict(cfg, 0)
    batch = O.PocketBatch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
    coef = O.step_coefficients(O.gamma_table(T, 1e-5), T)
    Nf = int(pharm_ptr[-1])
    B = int(prot_ptr.numel() - 1)
    ncpu = os.cpu_count() or 1
    try:
        ncpu = len(os.sched_getaffinity(0))
    except Exception:
        pass
    default_threads = torch.get_num_threads()
    # every hardware thread of a 256-thread host oversubscribes these small GEMMs by two orders of magnitude (measured
    # on the GPU box: 0.4 sample-steps/s at 256 threads against 150-180 at 8-32), so the sweep stops at 64
    cands = sorted({n for n in (8, 16, 32, 64) if n <= ncpu} or {ncpu})
    budget = max(args.cpu_seconds / len(cands), 2.0)
    results = {}
    for nthr in cands:
        torch.set_num_threads(nthr)
        g = torch.Generator().manual_seed(42)
        x_t, h_t = torch.randn(Nf, 3, generator=g), torch.randn(Nf, 6, generator=g)
        px = prot_x - O.segment_mean(prot_x, prot_ptr)[batch.batch_idxs()["prot"]]
        with torch.no_grad():
            nz = torch.randn(Nf, 9, generator=g)
            px, x_t, h_t = O.sample_step(sd, cfg, batch, coef, T - 1, px, x_t, h_t, nz[:, :3], nz[:, 3:])   # warm-up
            n, t0 = 0, time.perf_counter()
            while n < 2 or time.perf_counter() - t0 < budget:
                nz = torch.randn(Nf, 9, generator=g)
                px, x_t, h_t = O.sample_step(sd, cfg, batch, coef, T - 2 - n, px, x_t, h_t, nz[:, :3], nz[:, 3:])
                n += 1
                if n >= 200:
                    break
            dt = time.perf_counter() - t0
        results[nthr] = (B * n / dt, n, dt)
    torch.set_num_threads(default_threads)
    best = max(results, key=lambda k: results[k][0])
    return {"value": results[best][0], "unit": "sample-steps/s", "cores": best, "kind": "port",
            "by_threads": {str(k): round(v[0], 2) for k, v in results.items()}, "host_cpus": ncpu,
            "sample": f"{results[best][1]} denoising steps of the same B={B} batch (after 1 warm-up step) in {results[best][2]:.1f} s "
                      f"at {best} threads -- the best of {cands} threads, each timed for ~{budget:.0f} s; CPU oracle "
                      "(PyTorch fp32 restatement of the reference path)"}


if __name__ == "__main__":
    main()
