"""pinned_bench.py -- what a pinned run (pf_denoise_step_pinned) costs per denoising step, at the shape of BASELINE.json config 2
(B = 32 pockets of 256 atoms, 6 centers each, the dev.yml architecture), one JSON line.

Legs: `default` -- the unpinned step as shipped (merged last launch); `separate` -- the unpinned step under PFDYN_HS_BUILD=0
(node + head launch, then the update + build launch: the launches a pinned step makes, on the unpinned code -- the yardstick);
`separate_generic` -- the same with PFDYN_NO_FAST_BUILD=1 as well, i.e. the generic move + build bodies (k_step_build<MovePlain>) a pinned step is built
from (what the latency-optimised k_step_build_fast saves); `pinned` -- 2 of every graph's 6 centers pinned (position and type).
Every leg has its own handle; the timed windows of --steps steps (HIP events around the window, after --warmup steps) alternate
between the legs --rounds times, and the figure of a leg is the median of its windows (all of them are listed).  Behind the timed
windows, --steps // 5 more steps per leg run with HIP events around every launch (pf_profile_*): device us per step of each kernel
class, which says where a leg's extra time sits (not for `default`: timing the update + build apart takes the merged launch apart).

--resamples R --jump J add the `resampled` leg: the pinned leg's batch driven through the head of schedule.resample_plan(500, J, R)
(pf_renoise_step between the stretches).  It reports the whole run's time per op (HIP events around --rounds windows of --steps
ops, median) and, from a pass with HIP events around every launch read back op by op, the median duration of the re-noise launch
next to that of k_step_build<MovePinned> from the same run."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LEGS = ("default", "separate", "separate_generic", "pinned")


class Leg:
    def __init__(self, name, pfa, synthetic, schedule, args):
        self.name, self.pinned = name, name in ("pinned", "resampled")
        dev = torch.device("cuda:0")
        env = {"separate": {"PFDYN_HS_BUILD": "0"}, "separate_generic": {"PFDYN_HS_BUILD": "0", "PFDYN_NO_FAST_BUILD": "1"}}.get(name, {})
        os.environ.update(env)                              # read at handle creation
        eng = self.eng = pfa.PfEngine(device=dev)
        for k in env:
            os.environ.pop(k)
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
        self.n_all = n_all = args.warmup + args.rounds * args.steps + args.steps // 5
        order = [(n_all - 1 - i) % T for i in range(n_all)]     # the tail of the schedule (bench.py's choice)
        self.carr = eng.coef_array(schedule.step_coefficients(gamma, T), order)
        self.parr = eng.pin_coef_array(schedule.pin_coefficients(gamma, T), order)
        self.ops = None
        if name == "resampled":                             # the head of the resampled plan, op by op (a kind-1 op is a re-noise)
            self.n_all = n_all = n_all + args.steps         # (the per-launch pass behind the windows is --steps ops long)
            plan = schedule.resample_plan(T, args.jump, args.resamples)
            plan = (plan * (n_all // len(plan) + 1))[:n_all]
            pairs = [(op[1], op[2]) for op in plan if op[0] == "renoise"]
            self.carr, self.parr, self.ops, self.rarr = eng.plan_arrays(plan, schedule.step_coefficients(gamma, T),
                                                                        schedule.pin_coefficients(gamma, T),
                                                                        schedule.renoise_coefficients(gamma, T, pairs))
            tv = [self.carr[i] for i in range(n_all) if self.ops[i] == 0]
            eng.prepare_timesteps(tv, len(tv))
        else:
            eng.prepare_timesteps(self.carr, n_all)
        gen = torch.Generator(device=dev).manual_seed(42)
        self.noise = torch.empty(n_all + 1, B * n_pharm, 9, device=dev).normal_(generator=gen)
        pins = None
        if self.pinned:
            flags = torch.zeros(B, n_pharm, dtype=torch.int32)
            flags[:, :args.n_pinned] = 3
            com = prot_x.reshape(B, n_prot, 3).mean(dim=1, keepdim=True)
            pin_x = (com + 1.5 * torch.randn(B, n_pharm, 3, device=dev, generator=gen)).reshape(-1, 3)
            pin_h = torch.nn.functional.one_hot(torch.randint(0, 6, (B * n_pharm,), device=dev, generator=gen), 6).float()
            pins = (flags.reshape(-1), pin_x, pin_h)
        eng.sample_begin(self.noise[0], pins=pins)
        self.pos = 0
        self.windows = []

    def run(self, n, timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(self.pos, self.pos + n):
            self.op(i)
        b.record()
        b.synchronize()
        self.pos += n
        if timed:
            self.windows.append(1e3 * a.elapsed_time(b) / n)

    def op(self, i):
        if self.ops is not None and self.ops[i] == 1:
            self.eng.renoise_step(self.rarr[i], self.noise[i + 1])
        else:
            self.eng.denoise_step(self.carr[i], self.noise[i + 1], pin_coef=self.parr[i] if self.pinned else None)

    def profile_launches(self, n):
        """HIP events around every launch, read back after every op: {op kind: durations in us of its step-end launch}"""
        self.eng.profile_enable(0x1FF)
        out = {"renoise": [], "step_build_pinned": []}
        for i in range(self.pos, self.pos + n):
            self.op(i)
            ms, cnt = self.eng.profile_read()["step_update"]
            assert cnt == 1
            out["renoise" if self.ops[i] == 1 else "step_build_pinned"].append(1e3 * ms)
        self.pos += n
        self.eng.profile_enable(0)
        return out

    def profile(self, n):
        self.eng.profile_enable(0x1FF)
        self.run(n, False)
        prof = self.eng.profile_read()
        self.eng.profile_enable(0)
        return {k: round(1e3 * ms / n, 2) for k, (ms, cnt) in prof.items() if cnt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--n-pharm", type=int, default=6)
    ap.add_argument("--n-pinned", type=int, default=2)
    ap.add_argument("--resamples", type=int, default=1, help="above 1: add the `resampled` leg")
    ap.add_argument("--jump", type=int, default=10)
    args = ap.parse_args()
    if args.resamples < 1 or args.jump < 1:
        ap.error("--resamples and --jump must be at least 1")
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import schedule, synthetic
    legs = [Leg(n, pfa, synthetic, schedule, args) for n in LEGS + (("resampled",) if args.resamples > 1 else ())]
    for lg in legs:
        lg.run(args.warmup, False)
    for _ in range(args.rounds):
        for lg in legs:
            lg.run(args.steps, True)
    out = {"shape": {"batch": args.batch, "n_prot": args.n_prot, "n_pharm": args.n_pharm, "n_pinned": args.n_pinned,
                     "steps": args.steps, "rounds": args.rounds}}
    for lg in legs:
        out[lg.name] = {"step_us": round(statistics.median(lg.windows), 2), "windows_us": [round(w, 2) for w in lg.windows],
                        "step_end_form": lg.eng.kernel_family(2), "xchg_timeouts": lg.eng.xchg_timeouts()}
        if lg.name != "default":
            out[lg.name]["kernel_us_per_step"] = lg.profile(args.steps // 5)
    if args.resamples > 1:
        lg = legs[-1]
        per = lg.profile_launches(args.steps)
        r = out["resampled"]
        r["op_us"] = r.pop("step_us")
        r.update({"resamples": args.resamples, "jump": args.jump,
                  "renoise_launch_us": round(statistics.median(per["renoise"]), 2), "renoise_launches": len(per["renoise"]),
                  "step_build_pinned_launch_us": round(statistics.median(per["step_build_pinned"]), 2),
                  "step_build_pinned_launches": len(per["step_build_pinned"])})
    out["pinned_over_separate"] = round(out["pinned"]["step_us"] / out["separate"]["step_us"], 4)
    out["pinned_over_separate_generic"] = round(out["pinned"]["step_us"] / out["separate_generic"]["step_us"], 4)
    out["pinned_over_default"] = round(out["pinned"]["step_us"] / out["default"]["step_us"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
