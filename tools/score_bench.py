"""score_bench.py -- what scoring (pf_score) costs per noise level and per candidate, next to the default sampling step of the same
build and shape, one JSON line.  Recorded, not gated.

Shape: BASELINE.json config 2's pocket and centers (256 atoms, 6 centers, the dev.yml architecture) as 32 candidates of ONE pocket,
bound with the pocket-group claim -- the shape PharmacophoreDiff.score builds for the samples of a pocket.  Legs, each on its own
handle in this one process, seeded random weights as everywhere in this repository:
  score16   one pf_score call of L = 16 levels stratified over 1..T (T = 500)
  scoreT    one pf_score call of L = T levels
  default   the unseeded plain sampling run as shipped on the same batch (tuned kernels, merged last launch): time per step
Timed windows (HIP events around a window, after warm-up calls) alternate between the legs --rounds times; a leg's figure is the
median of its windows, all of them are listed.  Part 2, the share of the two new kernels: one more scoreT call with the library's
per-class event timers on (pf_profile_enable; class 5 counts k_score_prepare and k_score_eval in a scoring call): device time of
the two kernels over the device time of all launches of the call.

    python tools/score_bench.py [--out profiles/score/score_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

T = 500


def bound_engine(pfa, synthetic, args):
    dev = torch.device("cuda:0")
    eng = pfa.PfEngine(device=dev)
    eng.load_state_dict(synthetic.make_state_dict(0))
    B, n_prot, n_pharm = args.batch, args.n_prot, args.n_pharm
    x, h = synthetic.synthetic_pocket(0, n_prot)
    prot_x, prot_h = x.repeat(B, 1), h.repeat(B, 1)                   # host tensors: the bind verifies the claim on the host
    prot_ptr = torch.arange(B + 1, dtype=torch.int64) * n_prot
    pharm_ptr = torch.arange(B + 1, dtype=torch.int64) * n_pharm
    src1, dst1 = eng.build_pp_edges(x.to(dev), prot_ptr[:2])
    off = (torch.arange(B) * n_prot)[:, None]
    pp_src, pp_dst = (src1[None] + off).reshape(-1), (dst1[None] + off).reshape(-1)
    eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst, pocket_uid=torch.zeros(B, dtype=torch.int64))
    return eng, dev, x.mean(dim=0)


class ScoreLeg:
    def __init__(self, name, L, pfa, synthetic, schedule, args):
        self.name, self.L = name, L
        self.eng, dev, com = bound_engine(pfa, synthetic, args)
        Nf = args.batch * args.n_pharm
        gen = torch.Generator(device=dev).manual_seed(7)
        self.x0 = com.to(dev) + 1.5 * torch.randn(Nf, 3, device=dev, generator=gen)
        self.h0 = torch.nn.functional.one_hot(torch.randint(0, 6, (Nf,), device=dev, generator=gen), 6).float()
        self.noise = torch.empty(L, Nf, 9, device=dev).normal_(generator=gen)
        gamma = schedule.PredefinedNoiseSchedule('polynomial_2', T, 1e-5).gamma
        self.levels = schedule.score_levels(T, L)
        self.w = schedule.score_weights(gamma, T, self.levels, "uniform")
        self.tabs = (schedule.alpha(gamma).float().to(dev), schedule.sigma(gamma).float().to(dev))
        self.windows = []

    def call(self):
        return self.eng.score(self.x0, self.h0, self.levels, self.noise, self.w[0], self.w[1], self.tabs[0], self.tabs[1], T)

    def run(self, n, timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            self.call()
        b.record()
        b.synchronize()
        if timed:
            self.windows.append(1e3 * a.elapsed_time(b) / (n * self.L))           # us per level


class StepLeg:
    name = "default"

    def __init__(self, pfa, synthetic, schedule, args):
        self.eng, dev, _ = bound_engine(pfa, synthetic, args)
        gamma = schedule.PredefinedNoiseSchedule('polynomial_2', T, 1e-5).gamma
        self.n_all = args.warmup + args.rounds * args.steps
        assert self.n_all <= T
        self.carr = self.eng.coef_array(schedule.step_coefficients(gamma, T), reversed(range(T)))
        gen = torch.Generator(device=dev).manual_seed(42)
        self.noise = torch.empty(self.n_all + 1, args.batch * args.n_pharm, 9, device=dev).normal_(generator=gen)
        self.pos, self.windows = 0, []
        self.eng.sample_begin(self.noise[0])
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
    ap.add_argument("--steps", type=int, default=80, help="sampling steps per timed window of the default leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls16", type=int, default=10, help="pf_score calls per timed window of the L = 16 leg")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--n-pharm", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import schedule, synthetic
    s16 = ScoreLeg("score16", 16, pfa, synthetic, schedule, args)
    sT = ScoreLeg("scoreT", T, pfa, synthetic, schedule, args)
    st = StepLeg(pfa, synthetic, schedule, args)
    s16.run(3, False)
    sT.run(1, False)
    st.run(args.warmup, False)
    for _ in range(args.rounds):
        s16.run(args.calls16, True)
        sT.run(1, True)
        st.run(args.steps, True)
    out = {"shape": {"batch": args.batch, "n_prot": args.n_prot, "n_pharm": args.n_pharm, "T": T, "one_pocket_claimed": True,
                     "rounds": args.rounds, "weights": "seeded random (synthetic.make_state_dict(0))"}}
    for lg in (s16, sT):
        us = statistics.median(lg.windows)
        out[lg.name] = {"levels": lg.L, "level_us": round(us, 2), "candidate_level_us": round(us / args.batch, 3),
                        "call_ms": round(us * lg.L / 1e3, 3), "candidate_ms": round(us * lg.L / 1e3 / args.batch, 4),
                        "windows_level_us": [round(w, 2) for w in lg.windows],
                        "kernel_family": [lg.eng.kernel_family(l) for l in range(2)], "l0_hoist": lg.eng.l0_hoist()}
    out["default"] = {"step_us": round(statistics.median(st.windows), 2), "windows_us": [round(w, 2) for w in st.windows],
                      "step_end_form": st.eng.kernel_family(2)}
    out["level_over_default_step"] = round(out["scoreT"]["level_us"] / out["default"]["step_us"], 3)
    # part 2: device time per kernel class of one scoreT call (event pairs around every launch)
    sT.eng.profile_enable(0x1FF)
    sT.eng.profile_read()
    sT.call()
    prof = sT.eng.profile_read()
    sT.eng.profile_enable(0)
    total = sum(ms for ms, _ in prof.values())
    own_ms, own_n = prof["step_update"]
    out["kernel_classes"] = {k: {"device_us_per_level": round(1e3 * ms / T, 3), "launches_per_level": round(n / T, 3)} for k, (ms, n) in prof.items() if n}
    out["score_kernels_share_of_device_time"] = round(own_ms / total, 4)
    out["score_kernels_us_per_level"] = round(1e3 * own_ms / T, 3)
    out["launches_per_level"] = round(sum(n for _, n in prof.values()) / T, 3)
    st.eng.sample_end()
    torch.cuda.synchronize()
    st.eng.sample_status()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
