"""wide_train_bench.py -- training step time of the width-generic training leg (pf_train_set_family('wide'): pf_wide.hip's
training form, pf_wide_train.hip) against the specialised gradient kernels, at the shape of BASELINE.json config 5 (B = 256
pockets of 256 atoms, dropout 0.1, the dev.yml architecture); writes profiles/wide/train_bench.json and prints it as one line.

Legs: (128, 16) tuned family (the yardstick); (128, 16) wide family; (64, 16), (256, 16), (128, 32) wide family.  A step is
FlatAdam.zero_grad(lazy) + training_step + backward + FlatAdam.step on one bound batch with a new noise draw every step.  Every
leg's model stays alive; the timed windows of --steps steps alternate between the legs (--windows rounds, leg order kept) and a
leg's figure is the median over its windows, HIP events around each window.  Peak device memory per leg is what the process
holds beyond the previous legs (torch.cuda.mem_get_info: the engine allocates through hipMalloc, outside torch's allocator),
read after the leg's warm-up.  Per-launch device times come from pf_profile_* in a pass of their own.  There is no pass mark."""
import argparse
import itertools
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LEGS = [("tuned_128_16", 128, 16, "tuned"), ("wide_128_16", 128, 16, "wide"), ("wide_64_16", 64, 16, "wide"),
        ("wide_256_16", 256, 16, "wide"), ("wide_128_32", 128, 32, "wide")]


def used_bytes():
    free, total = torch.cuda.mem_get_info()
    return total - free


class Leg:
    def __init__(self, pfa, synthetic, S, V, family, args):
        dyn = dict(vector_size=V, n_convs=2, n_hidden_scalars=S, message_norm='mean', dropout=0.1, ff_k=0, pf_k=5,
                   n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4)
        B, T = args.batch, 100
        m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=T,
                                  graph_config={'graph_cutoffs': {'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9}}, dynamics_config=dyn,
                                  precision=1e-5)
        sd = dict(synthetic.make_state_dict(0, n_hidden_scalars=S, vector_size=V))
        sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
        m.load_state_dict(sd, strict=True)
        self.m = m.to("cuda").train()
        self.m.dynamics.set_train_family(family)
        self.eng = self.m.dynamics.engine()
        pockets = [synthetic.synthetic_pocket(50 + i, args.n_prot) for i in range(B)]
        sizes = [4 + (i % 5) for i in range(B)]
        gen = torch.Generator().manual_seed(11)
        prot_x, prot_h = torch.cat([p[0] for p in pockets]), torch.cat([p[1] for p in pockets])
        prot_ptr = torch.arange(B + 1, dtype=torch.int64) * args.n_prot
        pharm_ptr = torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int64)
        pp_src, pp_dst = self.eng.build_pp_edges(prot_x.to("cuda"), prot_ptr)
        Nf = int(pharm_ptr[-1])
        x0 = torch.cat([pockets[i][0].mean(0, keepdim=True) + 2.0 * torch.randn(sizes[i], 3, generator=gen) for i in range(B)])
        h0 = torch.nn.functional.one_hot(torch.randint(0, 6, (Nf,), generator=gen), 6).float()
        self.g = pfa.PocketGraph(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst, pharm_x0=x0, pharm_h0=h0).to("cuda")
        self.opt = pfa.FlatAdam(self.m.dynamics, lr=1e-4)
        self.windows = []
        self.loss = None

    def steps(self, n):
        for _ in range(n):
            self.opt.zero_grad(lazy=True)
            loss = self.m.training_step(self.g, 0)
            loss.backward()
            self.opt.step()
        self.loss = float(loss.detach())

    def window(self, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.steps(n)
        b.record()
        torch.cuda.synchronize()
        self.windows.append(a.elapsed_time(b) / n)

    def profile(self, n):
        self.eng.profile_enable(0x1FFF)
        self.steps(n)
        torch.cuda.synchronize()
        prof = {**self.eng.profile_read(), **self.eng.profile_read_train()}      # forward classes, gradient-kernel classes
        self.eng.profile_enable(0)
        return {k: {"ms_per_step": round(ms / n, 5), "launches_per_step": cnt / n, "ms_per_launch": round(ms / cnt, 5)}
                for k, (ms, cnt) in prof.items() if cnt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--legs", default=",".join(n for n, *_ in LEGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide", "train_bench.json"))
    args = ap.parse_args()
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import synthetic
    torch.manual_seed(1234)
    torch.zeros(1, device="cuda")
    want = args.legs.split(",")
    legs, out = {}, {"shape": {"batch": args.batch, "n_prot": args.n_prot, "centers": "4..8", "dropout": 0.1,
                               "steps_per_window": args.steps, "windows": args.windows}}
    for name, S, V, family in LEGS:
        if name not in want:
            continue
        torch.cuda.synchronize()
        base = used_bytes()
        legs[name] = Leg(pfa, synthetic, S, V, family, args)
        legs[name].steps(args.warmup)
        torch.cuda.synchronize()
        out[name] = {"family": legs[name].eng.train_family(), "device_memory_MiB": round((used_bytes() - base) / 2 ** 20, 1)}
        print(name, out[name], flush=True)
    for w in range(args.windows):
        for name, lg in legs.items():
            lg.window(args.steps)
        print("window", w, {n: round(lg.windows[-1], 3) for n, lg in legs.items()}, flush=True)
    for name, lg in legs.items():
        out[name].update({"step_ms_median": round(statistics.median(lg.windows), 4), "step_ms_windows": [round(x, 4) for x in lg.windows],
                          "last_loss": lg.loss, "launches": lg.profile(max(1, args.steps // 2))})
    if "tuned_128_16" in out and "wide_128_16" in out:
        out["wide_over_tuned_128_16"] = round(out["wide_128_16"]["step_ms_median"] / out["tuned_128_16"]["step_ms_median"], 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
