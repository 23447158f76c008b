"""seeded_bench.py -- what a seeded run (pf_sample_seed_next) costs against the default run, one JSON line.  Recorded, not gated.

Shape: BASELINE.json config 2 (B = 32 pockets of 256 atoms, 6 centers each, the dev.yml architecture; tools/guided_bench.py's
batch).  Two legs, each on its own handle in this one process:
  default   the unseeded plain run as shipped (tuned kernels, merged last launch)
  seeded    the same steps behind a seeded begin
Part 1, the step: a seeded run's steps are the default path's own launches, so the expectation is EQUAL time per step.  The timed
windows of --steps steps (HIP events around the window, after --warmup steps) alternate between the legs --rounds times; the
figure of a leg is the median of its windows (all of them are listed: their spread is the tool's run-to-run spread).
Part 2, the begin's own cost: windows of --begins begins (for the seeded leg: pf_sample_seed_next + the begin), alternating
between the legs in the same way.  The unseeded begin is a memset + 4 small launches + the snapshot copy; the seeded one replaces
the noise load and the snapshot copy by two device-to-device copies and the seed move's launch (which also builds the edges the
first step would otherwise build).

    python tools/seeded_bench.py [--out profiles/seeded/seeded_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LEGS = ("default", "seeded")


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
        assert n_all <= T
        order = list(reversed(range(n_all)))                # a seeded run from level n_all: s = n_all-1 .. 0
        self.carr = eng.coef_array(schedule.step_coefficients(gamma, T), order)
        self.n_all = n_all
        gen = torch.Generator(device=dev).manual_seed(42)
        self.noise = torch.empty(n_all + 1, B * n_pharm, 9, device=dev).normal_(generator=gen)
        com = prot_x.reshape(B, n_prot, 3).mean(dim=1)
        self.com = com
        self.seed = None
        if name == "seeded":
            seed_x = (com[:, None] + 1.5 * torch.randn(B, n_pharm, 3, device=dev, generator=gen)).reshape(-1, 3)
            seed_h = torch.nn.functional.one_hot(torch.randint(0, 6, (B * n_pharm,), device=dev, generator=gen), 6).float()
            self.seed = (seed_x, seed_h, eng.seed_coef_struct(schedule.seed_coefficients(gamma, T, n_all)))
        self.pos = 0
        self.windows, self.begin_windows = [], []

    def begin(self):
        self.eng.sample_begin(self.noise[0], init_pharm_com=self.com, seed=self.seed)

    def run_begins(self, n, timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            self.begin()
        b.record()
        b.synchronize()
        if timed:
            self.begin_windows.append(1e3 * a.elapsed_time(b) / n)

    def start(self):
        self.begin()
        self.eng.prepare_timesteps(self.carr, self.n_all)

    def run(self, n, timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(self.pos, self.pos + n):
            self.eng.denoise_step(self.carr[i], self.noise[i + 1])
        b.record()
        b.synchronize()
        self.pos += n
        if timed:
            self.windows.append(1e3 * a.elapsed_time(b) / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--begins", type=int, default=50)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--n-pharm", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import schedule, synthetic
    legs = [Leg(n, pfa, synthetic, schedule, args) for n in LEGS]
    for lg in legs:
        lg.run_begins(10, False)
    for _ in range(args.rounds):
        for lg in legs:
            lg.run_begins(args.begins, True)
    for lg in legs:
        lg.start()
        lg.run(args.warmup, False)
    for _ in range(args.rounds):
        for lg in legs:
            lg.run(args.steps, True)
    out = {"shape": {"batch": args.batch, "n_prot": args.n_prot, "n_pharm": args.n_pharm, "steps": args.steps, "rounds": args.rounds,
                     "begins": args.begins}}
    for lg in legs:
        out[lg.name] = {"step_us": round(statistics.median(lg.windows), 2), "windows_us": [round(w, 2) for w in lg.windows],
                        "begin_us": round(statistics.median(lg.begin_windows), 2), "begin_windows_us": [round(w, 2) for w in lg.begin_windows],
                        "step_end_form": lg.eng.kernel_family(2), "center_hoist": lg.eng.ahead()["center_hoist"],
                        "xchg_timeouts": lg.eng.xchg_timeouts()}
    out["seeded_over_default_step"] = round(out["seeded"]["step_us"] / out["default"]["step_us"], 4)
    out["seeded_minus_default_begin_us"] = round(out["seeded"]["begin_us"] - out["default"]["begin_us"], 2)
    for lg in legs:
        lg.eng.sample_end()
    torch.cuda.synchronize()
    for lg in legs:
        lg.eng.sample_status()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
