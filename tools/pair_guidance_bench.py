"""pair_guidance_bench.py -- what pair guidance (pf_guide_pairs_next: one launch of k_guide_pairs behind the other guidance
launches of a step) adds to a guided step, one JSON line.  Recorded, not gated.

Shape: BASELINE.json config 2 (B = 32 pockets of 256 atoms, 6 centers each, the dev.yml architecture; tools/type_guidance_bench.py's
batch), no pins, per graph a repel sphere on all centers plus an attract on one; no pocket field.  Legs, each on its own handle in
this one process, per training family (`@tuned`, `@wide`):
  guided      the guided step without the arming: exactly the launches of the parent commit
  pairs_w0    armed with (*, *, 4, inf, 0) on every graph: the launch alone, contributing exact zeros, so the run stays the
              guided leg's bit for bit
  pairs       the same restraint with weight 1: a minimum separation of 4 angstroms between the centers of a sample
A guided step's time depends on where the centers are (the edge sets are rebuilt from them every step): pairs_w0 - guided is the
launch alone, pairs - guided also holds what the moved state costs or saves.
The timed windows of --steps steps (HIP events around the window, after --warmup steps) alternate between the legs --rounds times;
the figure of a leg is the median of its windows (all of them are listed: their spread is the tool's run-to-run spread).

--root DIR imports the package from another checkout of the project (the parent commit, built) and --legs guided@tuned,guided@wide
restricts the run to what that checkout has: run so before and after the run of this tree, the parent's guided step is timed in
the same session.  k_guide_pairs' own duration is not seen by events around a window: run one leg under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/pair_guidance_bench.py --legs pairs@tuned --rounds 1) and read its row.

    python tools/pair_guidance_bench.py [--out profiles/pair_guidance/pair_guidance_bench.json]
    python tools/pair_guidance_bench.py --root ../parent --legs guided@tuned,guided@wide"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Leg:
    def __init__(self, name, pfa, synthetic, schedule, args):
        self.name = name
        kind, family = name.split("@")
        dev = torch.device("cuda:0")
        eng = self.eng = pfa.PfEngine(device=dev)
        eng.load_state_dict(synthetic.make_state_dict(0))
        B, n_prot, n_pharm = args.batch, args.n_prot, args.n_pharm
        xs, hs = zip(*[synthetic.synthetic_pocket(i, n_prot) for i in range(B)])
        prot_x, prot_h = torch.cat(xs).to(dev), torch.cat(hs).to(dev)
        prot_ptr = torch.arange(B + 1, dtype=torch.int64) * n_prot
        pharm_ptr = torch.arange(B + 1, dtype=torch.int64) * n_pharm
        pp_src, pp_dst = eng.build_pp_edges(prot_x, prot_ptr)
        eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
        T = 500
        gamma = schedule.PredefinedNoiseSchedule('polynomial_2', T, 1e-5).gamma
        n_all = args.warmup + args.rounds * args.steps
        order = [(n_all - 1 - i) % T for i in range(n_all)]     # the tail of the schedule (bench.py's choice)
        self.carr = eng.coef_array(schedule.step_coefficients(gamma, T), order)
        self.parr = eng.pin_coef_array(schedule.pin_coefficients(gamma, T), order)
        self.garr = eng.guide_coef_array(schedule.guide_coefficients(gamma, T), order)
        gen = torch.Generator(device=dev).manual_seed(42)
        self.noise = torch.empty(n_all + 1, B * n_pharm, 9, device=dev).normal_(generator=gen)
        c = prot_x.reshape(B, n_prot, 3).mean(dim=1).cpu()
        restraints = [[("repel", None, c[g].tolist(), 3.0, 1.0), ("attract", n_pharm - 1, (c[g] + 3.0).tolist(), 1.5, 1.0)]
                      for g in range(B)]
        kw = {}
        if kind != "guided":
            kw["pairs"] = [[(None, None, args.separation, math.inf, 0.0 if kind == "pairs_w0" else 1.0)] for _ in range(B)]
        eng.sample_begin(self.noise[0], restraints=restraints, guide_scale=1.0, guide_clip=1.0, guide_family=family, **kw)
        self.pos = 0
        self.windows = []

    def run(self, n, timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(self.pos, self.pos + n):
            self.eng.guided_step(self.carr[i], self.parr[i], self.garr[i], self.noise[i + 1])
        b.record()
        b.synchronize()
        self.pos += n
        if timed:
            self.windows.append(1e3 * a.elapsed_time(b) / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--n-pharm", type=int, default=6)
    ap.add_argument("--separation", type=float, default=4.0)
    ap.add_argument("--legs", default="guided@tuned,pairs_w0@tuned,pairs@tuned,guided@wide,pairs_w0@wide,pairs@wide")
    ap.add_argument("--root", default=HERE, help="the checkout whose package and library are measured (default: this one)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import schedule, synthetic
    legs = [Leg(n, pfa, synthetic, schedule, args) for n in args.legs.split(",")]
    for lg in legs:
        lg.run(args.warmup, False)
    for _ in range(args.rounds):
        for lg in legs:
            lg.run(args.steps, True)
    out = {"checkout": os.path.relpath(os.path.abspath(args.root), HERE),      # "." is this tree
           "shape": {"batch": args.batch, "n_prot": args.n_prot, "n_pharm": args.n_pharm, "separation": args.separation,
                     "steps": args.steps, "rounds": args.rounds}}
    by_name = {lg.name: lg for lg in legs}
    for lg in legs:
        out[lg.name] = {"step_us": round(statistics.median(lg.windows), 2), "windows_us": [round(w, 2) for w in lg.windows],
                        "xchg_timeouts": lg.eng.xchg_timeouts()}
        if not lg.name.startswith("guided"):
            out[lg.name]["last_E_pair_max"] = round(float(lg.eng.last_pair_guidance()[1].max()), 4)
    for family in ("tuned", "wide"):
        for kind in ("pairs_w0", "pairs"):
            if f"guided@{family}" in out and f"{kind}@{family}" in out:
                out[f"{kind}_minus_guided_us@{family}"] = round(out[f"{kind}@{family}"]["step_us"] - out[f"guided@{family}"]["step_us"], 2)
        if f"guided@{family}" in by_name and f"pairs_w0@{family}" in by_name:
            a, b = by_name[f"guided@{family}"].eng, by_name[f"pairs_w0@{family}"].eng
            out[f"pairs_w0_state_equals_guided@{family}"] = all(bool(torch.equal(x, y)) for x, y in zip(a.sample_frame(), b.sample_frame()))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
