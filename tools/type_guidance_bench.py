"""type_guidance_bench.py -- what type guidance (pf_guide_types_next: k_guide_types, the TYPES form of k_guide_field, g_pharm_h
from the inputs-only backward, the feature-shift form of the step end) adds to a guided step, one JSON line.  Recorded, not gated.

Shape: BASELINE.json config 2 (B = 32 pockets of 256 atoms, 6 centers each, the dev.yml architecture; tools/pocket_field_bench.py's
batch), the tuned family, no pins, per graph a repel sphere on all centers plus an attract on one, and the pocket field of
pocket_field_bench.py (radius 2.0 on every atom, 40 receptor features per graph).  Legs, each on its own handle in this one
process:
  guided      the guided step with the field and without the arming: exactly the launches of the parent commit
  armed_w0    armed with one windowed and one windowless type restraint per graph of weight zero and feat_scale 0: the launches
              alone -- k_guide_types, the encoders' backward for g_pharm_h, the timestep fill in front of it, the third form of
              the step end -- contributing exact zeros, so the run stays the guided leg's bit for bit
  types       the same restraints with weights 1 and feat_scale 1
  types_comp  ... plus comp_types (the TYPES form of k_guide_field), unmatched 1.5
A guided step's time depends on where the centers are (the edge sets are rebuilt from them every step): armed_w0 - guided is the
launches alone, the other differences also hold what the moved state costs or saves.
The timed windows of --steps steps (HIP events around the window, after --warmup steps) alternate between the legs --rounds times;
the figure of a leg is the median of its windows (all of them are listed: their spread is the tool's run-to-run spread).

--root DIR imports the package from another checkout of the project (the parent commit, built) and --legs guided restricts the
run to what that checkout has: run so before and after the run of this tree, the parent's guided step is timed in the same session.

    python tools/type_guidance_bench.py [--out profiles/type_guidance/type_guidance_bench.json]
    python tools/type_guidance_bench.py --root ../parent --legs guided"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Leg:
    def __init__(self, name, pfa, synthetic, schedule, args):
        self.name = name
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
        from pharmacoforge_amd.analysis import complementarity_tables
        match, dist = complementarity_tables()
        hgen = torch.Generator().manual_seed(7)
        nq = args.n_features
        ph_x = (c[:, None] + 4.0 * torch.randn(B, nq, 3, generator=hgen)).reshape(-1, 3)
        ph_t = torch.randint(0, 6, (B * nq,), generator=hgen)
        kw = dict(field=dict(atom_r=2.0, w_clash=1.0, ph=([g * nq for g in range(B + 1)], ph_x, ph_t), match=match, dist=dist,
                             w_comp=0.25, kappa=4.0, type_sharpness=4.0))
        if name != "guided":
            w = 0.0 if name == "armed_w0" else 1.0
            tr = [[(1, None, c[g].tolist(), 8.0, w), (2, 0, (0.0, 0.0, 0.0), 0.0, w)] for g in range(B)]
            kw["types"] = dict(restraints=tr, scale=w, clip=1.0, sharpness=4.0, complementarity=name == "types_comp",
                               unmatched=1.5 if name == "types_comp" else 0.0)
        eng.sample_begin(self.noise[0], restraints=restraints, guide_scale=1.0, guide_clip=1.0, guide_family="tuned", **kw)
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
    ap.add_argument("--n-features", type=int, default=40)
    ap.add_argument("--legs", default="guided,armed_w0,types,types_comp")
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
           "shape": {"batch": args.batch, "n_prot": args.n_prot, "n_pharm": args.n_pharm, "n_features": args.n_features,
                     "steps": args.steps, "rounds": args.rounds}}
    for lg in legs:
        out[lg.name] = {"step_us": round(statistics.median(lg.windows), 2), "windows_us": [round(w, 2) for w in lg.windows],
                        "xchg_timeouts": lg.eng.xchg_timeouts()}
        if lg.name != "guided":
            out[lg.name]["last_E_type_max"] = round(float(lg.eng.last_type_guidance()[3].max()), 4)
    for name in ("armed_w0", "types", "types_comp"):
        if "guided" in out and name in out:
            out[f"{name}_minus_guided_us"] = round(out[name]["step_us"] - out["guided"]["step_us"], 2)
    if "guided" in out and "armed_w0" in out:
        a, b = legs[[lg.name for lg in legs].index("guided")].eng, legs[[lg.name for lg in legs].index("armed_w0")].eng
        out["armed_w0_state_equals_guided"] = all(bool(torch.equal(x, y)) for x, y in zip(a.sample_frame(), b.sample_frame()))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
