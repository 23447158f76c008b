"""guided_bench.py -- what a guided step (pf_denoise_step_guided) costs, and what the inputs-only backward (pf_dynamics_input_vjp)
saves against the full pass, one JSON line.  Recorded, not gated.

Part 1, the step, at the shape of BASELINE.json config 2 (B = 32 pockets of 256 atoms, 6 centers each, the dev.yml architecture;
tools/pinned_bench.py's batch).  Legs, each on its own handle in this one process:
  default   the unguided step as shipped (tuned kernels, merged last launch)
  pinned    the pinned step, 2 of every graph's 6 centers pinned
  wide      an unguided step of a handle created under PFDYN_WIDE=1: the width-generic INFERENCE forward + k_step_update<MovePlain>.  The
            fair yardstick: a guided step's forward is the width-generic training forward
  guided    2 centers pinned, and per graph a repel sphere on all centers plus an attract on one
  guided_tuned  the same run with guide_family="tuned": the tuned training forward and the tuned inputs-only backward
The timed windows of --steps steps (HIP events around the window, after --warmup steps) alternate between the legs --rounds
times; the figure of a leg is the median of its windows (all of them are listed: their spread is the tool's run-to-run spread).

Part 2, the backward alone, at that shape and at the config-5 shape of tools/input_grad_bench.py (B = 256 pockets of 256 atoms,
4..8 centers, dropout 0.1): after one training forward on the wide family, the calls alternate between
  full        pf_train_backward_inputs, g_x requested (parameter gradient + g_x)
  vjp         pf_dynamics_input_vjp, g_x alone: no clear, no reduce, kernels without their weight-gradient products
  vjp_host    the same entry on a handle created under PFDYN_VJP_FULL_KERNELS=1: no clear, no reduce, but the full pass's kernels
              (what the host-level skip alone would give)
  tuned_plain / tuned_full / tuned_vjp   a handle on the tuned family with pf_train_set_input_grads: pf_train_backward,
              pf_train_backward_inputs with g_x, pf_dynamics_input_vjp with g_x (the full kernels without the reduces)
HIP events around every call; per leg the median over all calls and the [smallest .. largest] median of consecutive chunks of 20.

    python tools/guided_bench.py [--out profiles/guided/guided_bench.json]"""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LEGS = ("default", "pinned", "wide", "guided", "guided_tuned")


class Leg:
    def __init__(self, name, pfa, synthetic, schedule, args):
        self.name = name
        dev = torch.device("cuda:0")
        env = {"wide": {"PFDYN_WIDE": "1"}}.get(name, {})
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
        n_all = args.warmup + args.rounds * args.steps
        order = [(n_all - 1 - i) % T for i in range(n_all)]     # the tail of the schedule (bench.py's choice)
        self.carr = eng.coef_array(schedule.step_coefficients(gamma, T), order)
        self.parr = eng.pin_coef_array(schedule.pin_coefficients(gamma, T), order)
        self.garr = eng.guide_coef_array(schedule.guide_coefficients(gamma, T), order)
        eng.prepare_timesteps(self.carr, n_all)
        gen = torch.Generator(device=dev).manual_seed(42)
        self.noise = torch.empty(n_all + 1, B * n_pharm, 9, device=dev).normal_(generator=gen)
        pins = restraints = None
        com = prot_x.reshape(B, n_prot, 3).mean(dim=1)
        guided = self.guided = name.startswith("guided")
        if name == "pinned" or guided:
            flags = torch.zeros(B, n_pharm, dtype=torch.int32)
            flags[:, :args.n_pinned] = 3
            pin_x = (com[:, None] + 1.5 * torch.randn(B, n_pharm, 3, device=dev, generator=gen)).reshape(-1, 3)
            pin_h = torch.nn.functional.one_hot(torch.randint(0, 6, (B * n_pharm,), device=dev, generator=gen), 6).float()
            pins = (flags.reshape(-1), pin_x, pin_h)
        if guided:
            c = com.cpu()
            restraints = [[("repel", None, c[g].tolist(), 3.0, 1.0), ("attract", n_pharm - 1, (c[g] + 3.0).tolist(), 1.5, 1.0)]
                          for g in range(B)]
        eng.sample_begin(self.noise[0], pins=pins, restraints=restraints, guide_scale=1.0, guide_clip=1.0,
                         guide_family={"guided": "wide", "guided_tuned": "tuned"}.get(name))
        self.pos = 0
        self.windows = []

    def run(self, n, timed):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(self.pos, self.pos + n):
            if self.guided:
                self.eng.guided_step(self.carr[i], self.parr[i], self.garr[i], self.noise[i + 1])
            else:
                self.eng.denoise_step(self.carr[i], self.noise[i + 1], pin_coef=self.parr[i] if self.name == "pinned" else None)
        b.record()
        b.synchronize()
        self.pos += n
        if timed:
            self.windows.append(1e3 * a.elapsed_time(b) / n)


def chunks(ms):
    c = [statistics.median(ms[i:i + 20]) for i in range(0, len(ms) - 19, 20)]
    return {"median_ms": round(statistics.median(ms), 4), "chunk_medians_ms": [round(min(c), 4), round(max(c), 4)], "calls": len(ms)}


def backward_legs(pfa, synthetic, batch, n_prot, sizes, dropout, calls, warmup):
    """one training forward per handle, then the three calls alternating"""
    dev = torch.device("cuda:0")
    B = batch
    pockets = [synthetic.synthetic_pocket(50 + i, n_prot) for i in range(B)]
    gen = torch.Generator().manual_seed(11)
    prot_x, prot_h = torch.cat([p[0] for p in pockets]), torch.cat([p[1] for p in pockets])
    prot_ptr = torch.arange(B + 1, dtype=torch.int64) * n_prot
    pharm_ptr = torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int64)
    Nf = int(pharm_ptr[-1])
    x_t = torch.cat([pockets[i][0].mean(0, keepdim=True) + 2.0 * torch.randn(sizes[i], 3, generator=gen) for i in range(B)]).to(dev)
    h_t, t = torch.randn(Nf, 6, generator=gen).to(dev), torch.rand(B, generator=gen).to(dev)
    w_h, w_x = torch.zeros(Nf, 6, device=dev), torch.randn(Nf, 3, generator=gen).to(dev)      # (a guided step's upstream: g_eps_h = 0)
    engs = {}
    for name, env in (("this", {}), ("host_skip", {"PFDYN_VJP_FULL_KERNELS": "1"})):
        os.environ.update(env)
        eng = engs[name] = pfa.PfEngine(device=dev)
        for k in env:
            os.environ.pop(k)
        eng.load_state_dict(synthetic.make_state_dict(0))
        eng.set_train_family("wide")
        pp_src, pp_dst = eng.build_pp_edges(prot_x.to(dev), prot_ptr)
        eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
        eng.train_forward(x_t, h_t, t, dropout=dropout, seed=7)
    tuned = engs["tuned"] = pfa.PfEngine(device=dev)
    tuned.load_state_dict(synthetic.make_state_dict(0))
    tuned.set_train_input_grads(True)
    pp_src, pp_dst = tuned.build_pp_edges(prot_x.to(dev), prot_ptr)
    tuned.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
    tuned.train_forward(x_t, h_t, t, dropout=dropout, seed=7)
    calls_of = {"full": lambda: engs["this"].train_backward(w_h, w_x, input_grads=(True, False)),
                "vjp": lambda: engs["this"].input_vjp(w_h, w_x, want=(True, False)),
                "vjp_host": lambda: engs["host_skip"].input_vjp(w_h, w_x, want=(True, False)),
                "tuned_plain": lambda: tuned.train_backward(w_h, w_x),
                "tuned_full": lambda: tuned.train_backward(w_h, w_x, input_grads=(True, False)),
                "tuned_vjp": lambda: tuned.input_vjp(w_h, w_x, want=(True, False))}
    times = {k: [] for k in calls_of}
    for i in range(warmup + calls):
        for name, fn in calls_of.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    same = torch.equal(calls_of["full"]()[1], calls_of["vjp"]()[0]) and torch.equal(calls_of["vjp"]()[0], calls_of["vjp_host"]()[0])
    same_tuned = torch.equal(calls_of["tuned_full"]()[1], calls_of["tuned_vjp"]()[0])
    out = {"shape": {"batch": B, "n_prot": n_prot, "centers": Nf, "dropout": dropout}, "g_x_bitwise_equal": bool(same),
           "tuned_g_x_bitwise_equal": bool(same_tuned)}
    out.update({k: chunks(v) for k, v in times.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--n-pharm", type=int, default=6)
    ap.add_argument("--n-pinned", type=int, default=2)
    ap.add_argument("--calls", type=int, default=60, help="timed backward calls per leg (a multiple of 20)")
    ap.add_argument("--big-batch", type=int, default=256, help="pockets of the config-5 shape (0: skip it)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert args.calls >= 20
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import schedule, synthetic
    legs = [Leg(n, pfa, synthetic, schedule, args) for n in LEGS]
    for lg in legs:
        lg.run(args.warmup, False)
    for _ in range(args.rounds):
        for lg in legs:
            lg.run(args.steps, True)
    out = {"step": {"shape": {"batch": args.batch, "n_prot": args.n_prot, "n_pharm": args.n_pharm, "n_pinned": args.n_pinned,
                              "steps": args.steps, "rounds": args.rounds}}}
    for lg in legs:
        out["step"][lg.name] = {"step_us": round(statistics.median(lg.windows), 2), "windows_us": [round(w, 2) for w in lg.windows],
                                "step_end_form": lg.eng.kernel_family(2), "xchg_timeouts": lg.eng.xchg_timeouts()}
    s = out["step"]
    for k in ("default", "pinned", "wide"):
        s[f"guided_over_{k}"] = round(s["guided"]["step_us"] / s[k]["step_us"], 3)
    for k in ("default", "pinned", "guided"):
        s[f"guided_tuned_over_{k}"] = round(s["guided_tuned"]["step_us"] / s[k]["step_us"], 3)
    del legs
    torch.cuda.empty_cache()
    out["backward_config2"] = backward_legs(pfa, synthetic, args.batch, args.n_prot, [args.n_pharm] * args.batch, 0.0, args.calls, 10)
    if args.big_batch:
        out["backward_config5"] = backward_legs(pfa, synthetic, args.big_batch, 256, [4 + (i % 5) for i in range(args.big_batch)], 0.1,
                                                args.calls, 10)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
