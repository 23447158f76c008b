"""wide_bench.py -- denoising sample-steps/s of the width-generic family (pf_wide.hip) against the specialised kernels, at the
shape of BASELINE.json config 2 (B = 32 pockets of 256 atoms, 6 centers each, the dev.yml architecture), one JSON line.

Legs: (128, 16) specialised; (128, 16) with PFDYN_WIDE=1; (64, 16), (256, 16), (128, 32) on the width-generic family.  Per leg:
sample-steps/s over --steps timed denoising steps (after --warmup), the step time in us, and the device ms per step of each
kernel class (pf_profile_*, HIP events around every launch: a separate pass of --steps // 5 steps, not the timed one)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LEGS = [("spec_128_16", 128, 16, False), ("wide_128_16", 128, 16, True), ("wide_64_16", 64, 16, True),
        ("wide_256_16", 256, 16, True), ("wide_128_32", 128, 32, True)]


def leg(pfa, synthetic, schedule, S, V, wide, args):
    if wide:
        os.environ["PFDYN_WIDE"] = "1"                  # read at handle creation
    else:
        os.environ.pop("PFDYN_WIDE", None)
    dev = torch.device("cuda:0")
    eng = pfa.PfEngine(device=dev, n_hidden_scalars=S, vector_size=V)
    os.environ.pop("PFDYN_WIDE", None)
    eng.load_state_dict(synthetic.make_state_dict(0, n_hidden_scalars=S, vector_size=V))
    B = args.batch
    xs, hs = zip(*[synthetic.synthetic_pocket(i, args.n_prot) for i in range(B)])
    prot_x, prot_h = torch.cat(xs).to(dev), torch.cat(hs).to(dev)
    prot_ptr = torch.arange(B + 1, dtype=torch.int64) * args.n_prot
    pharm_ptr = torch.arange(B + 1, dtype=torch.int64) * args.n_pharm
    pp_src, pp_dst = eng.build_pp_edges(prot_x, prot_ptr)
    eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
    T, K, W = 500, args.steps, args.warmup
    coef = schedule.step_coefficients(schedule.PredefinedNoiseSchedule('polynomial_2', T, 1e-5).gamma, T)
    n_all = W + K + K // 5
    carr = eng.coef_array(coef, [(n_all - 1 - i) % T for i in range(n_all)])   # the tail of the schedule (bench.py's choice)
    eng.prepare_timesteps(carr, n_all)
    gen = torch.Generator(device=dev).manual_seed(42)
    noise = torch.empty(n_all + 1, B * args.n_pharm, 9, device=dev).normal_(generator=gen)
    eng.sample_begin(noise[0])
    for i in range(W):
        eng.denoise_step(carr[i], noise[i + 1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(W, W + K):
        eng.denoise_step(carr[i], noise[i + 1])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.profile_enable(0x1FF)
    for i in range(W + K, n_all):
        eng.denoise_step(carr[i], noise[i + 1])
    prof = eng.profile_read()
    eng.profile_enable(0)
    n_prof = n_all - W - K
    return {"sample_steps_per_s": B * K / dt, "step_us": 1e6 * dt / K,
            "kernel_ms_per_step": {k: round(ms / n_prof, 5) for k, (ms, n) in prof.items() if n},
            "family_layer0": eng.kernel_family(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--n-pharm", type=int, default=6)
    ap.add_argument("--legs", default=",".join(n for n, *_ in LEGS))
    args = ap.parse_args()
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import schedule, synthetic
    want = args.legs.split(",")
    out = {"shape": {"batch": args.batch, "n_prot": args.n_prot, "n_pharm": args.n_pharm, "steps": args.steps}}
    for name, S, V, wide in LEGS:
        if name in want:
            out[name] = leg(pfa, synthetic, schedule, S, V, wide, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
