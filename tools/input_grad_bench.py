"""input_grad_bench.py -- what the input gradients cost the wide family's backward pass (pf_train_backward_inputs), at the shape
of BASELINE.json config 5 as tools/wide_train_bench.py builds it (B = 256 pockets of 256 atoms, 4..8 centers, dropout 0.1, the
dev.yml architecture at 128 / 16 on the wide training family).  Recorded, not gated.

Legs, each in a fresh process (the library is chosen when the package is imported):
  parent     --parent-lib's libpfdyn.so through PFDYN_LIB (a build of the parent commit), pf_train_backward; run twice, first
             and last, so that the spread the tool reports for it is a run-to-run one
  this       this tree's library: pf_train_backward ("none") and pf_train_backward_inputs with both outputs ("both"), the
             calls alternating
  this, tuned  (--tuned) the same batch on the tuned family with pf_train_set_input_grads, in the "this" process: pf_train_backward
             ("tuned none"), pf_train_backward_inputs with both outputs ("tuned both") and pf_dynamics_input_vjp ("tuned vjp": the
             inputs-only mode -- the full kernels without the reduces)
One training forward, then --warmup backward calls, then --calls timed ones per leg, HIP events around every call.  Per leg the
median over all calls and the medians of consecutive chunks of 20 calls.  Writes profiles/input_grads/backward_cost.txt."""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW_ENTRY = "pf_train_backward_inputs"


def child(args):
    import torch
    import pharmacoforge_amd as pfa
    from pharmacoforge_amd import synthetic
    has_entry = hasattr(ctypes.CDLL(pfa._lib.LIB_PATH), NEW_ENTRY)
    if not has_entry:                                           # the parent commit's library: bind what it exports
        pfa._lib.SYMBOLS.pop(NEW_ENTRY, None)
    torch.manual_seed(1234)
    S, V, B = 128, 16, args.batch
    eng = pfa.PfEngine(device="cuda:0", pharm_nf=6, rec_nf=11, vector_size=V, n_convs=2, n_hidden_scalars=S, message_norm='mean',
                       ff_k=0, pf_k=5, n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4,
                       graph_cutoffs={'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9})
    eng.load_state_dict({k: v for k, v in synthetic.make_state_dict(0, n_hidden_scalars=S, vector_size=V).items()
                         if k.startswith("dynamics.")})
    eng.set_train_family("wide")
    pockets = [synthetic.synthetic_pocket(50 + i, args.n_prot) for i in range(B)]
    sizes = [4 + (i % 5) for i in range(B)]
    gen = torch.Generator().manual_seed(11)
    prot_x, prot_h = torch.cat([p[0] for p in pockets]), torch.cat([p[1] for p in pockets])
    prot_ptr = torch.arange(B + 1, dtype=torch.int64) * args.n_prot
    pharm_ptr = torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int64)
    pp_src, pp_dst = eng.build_pp_edges(prot_x.to("cuda"), prot_ptr)
    eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
    Nf = int(pharm_ptr[-1])
    x_t = torch.cat([pockets[i][0].mean(0, keepdim=True) + 2.0 * torch.randn(sizes[i], 3, generator=gen) for i in range(B)]).cuda()
    h_t, t = torch.randn(Nf, 6, generator=gen).cuda(), torch.rand(B, generator=gen).cuda()
    w_h, w_x = torch.randn(Nf, 6, generator=gen).cuda(), torch.randn(Nf, 3, generator=gen).cuda()
    eng.train_forward(x_t, h_t, t, dropout=0.1, seed=7)
    legs = {"none": False, "both": True} if (args.child == "this" and has_entry) else {"none": False}
    calls = {name: ((lambda: eng.train_backward(w_h, w_x, input_grads=True)) if flag else (lambda: eng.train_backward(w_h, w_x)))
             for name, flag in legs.items()}
    if args.tuned and args.child == "this":
        tuned = pfa.PfEngine(device="cuda:0", pharm_nf=6, rec_nf=11, vector_size=V, n_convs=2, n_hidden_scalars=S, message_norm='mean',
                             ff_k=0, pf_k=5, n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4,
                             graph_cutoffs={'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9})
        tuned.load_state_dict({k: v for k, v in synthetic.make_state_dict(0, n_hidden_scalars=S, vector_size=V).items()
                               if k.startswith("dynamics.")})
        tuned.set_train_input_grads(True)
        tuned.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
        tuned.train_forward(x_t, h_t, t, dropout=0.1, seed=7)
        calls.update({"tuned none": lambda: tuned.train_backward(w_h, w_x),
                      "tuned both": lambda: tuned.train_backward(w_h, w_x, input_grads=True),
                      "tuned vjp": lambda: tuned.input_vjp(w_h, w_x)})
    times = {k: [] for k in calls}
    for i in range(args.warmup + args.calls):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(a.elapsed_time(b))
    print("RESULT " + json.dumps({"lib": pfa._lib.LIB_PATH, "has_entry": has_entry, "Nf": Nf, "times": times}), flush=True)


def summary(ms):
    chunks = [statistics.median(ms[i:i + 20]) for i in range(0, len(ms) - 19, 20)]
    return statistics.median(ms), min(chunks), max(chunks), len(ms)


def run_child(args, which, lib):
    env = dict(os.environ)
    env.pop("PFDYN_LIB", None)
    if lib:
        env["PFDYN_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--calls", str(args.calls), "--warmup", str(args.warmup),
           "--batch", str(args.batch), "--n-prot", str(args.n_prot)] + (["--tuned"] if args.tuned else [])
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=args.child_timeout).stdout
    return json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libpfdyn.so built from the parent commit")
    ap.add_argument("--calls", type=int, default=100, help="timed backward calls per leg (a multiple of 20)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-prot", type=int, default=256)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--tuned", action="store_true", help="also the tuned family's legs (pf_train_set_input_grads)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_grads", "backward_cost.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    assert args.calls >= 20
    lines = [f"Wide-family backward pass at batch {args.batch} x {args.n_prot} atoms, 4..8 centers, 128 / 16, dropout 0.1 (tools/input_grad_bench.py):",
             f"ms per call, HIP events around every call, {args.warmup} warm-up calls, then {args.calls} timed calls per leg; median over all",
             "calls and [smallest .. largest] median of the consecutive chunks of 20 calls.", ""]
    parent = []
    if args.parent_lib:
        parent.append(run_child(args, "parent", os.path.abspath(args.parent_lib)))
    this = run_child(args, "this", None)
    if args.parent_lib:
        parent.append(run_child(args, "parent", os.path.abspath(args.parent_lib)))
    rows = {}
    for i, p in enumerate(parent):
        assert not p["has_entry"], "--parent-lib exports pf_train_backward_inputs: it is not the parent commit's library"
        rows[f"parent, run {i + 1} (pf_train_backward)"] = summary(p["times"]["none"])
    rows["this commit, no input gradients (pf_train_backward)"] = summary(this["times"]["none"])
    rows["this commit, both input gradients (pf_train_backward_inputs)"] = summary(this["times"]["both"])
    for k, label in (("tuned none", "this commit, tuned family, no input gradients (pf_train_backward)"),
                     ("tuned both", "this commit, tuned family, both (pf_train_backward_inputs)"),
                     ("tuned vjp", "this commit, tuned family, inputs only (pf_dynamics_input_vjp)")):
        if k in this["times"]:
            rows[label] = summary(this["times"][k])
    for name, (med, lo, hi, n) in rows.items():
        lines.append(f"  {name:62s} {med:8.3f}   [{lo:.3f} .. {hi:.3f}]   {n} calls")
    none, both = rows["this commit, no input gradients (pf_train_backward)"][0], rows["this commit, both input gradients (pf_train_backward_inputs)"][0]
    lines.append("")
    if parent:
        meds = [summary(p["times"]["none"]) for p in parent]
        lo, hi = min(m[1] for m in meds), max(m[2] for m in meds)
        base = statistics.median(m[0] for m in meds)
        lines.append(f"  parent's run-to-run spread (chunk medians of both runs): [{lo:.3f} .. {hi:.3f}]; this commit without input "
                     f"gradients: {none:.3f} ({'inside' if lo <= none <= hi else ('below it: faster' if none < lo else 'above it: slower')})")
        lines.append(f"  overhead of both input gradients: {both - none:+.3f} ms = {100 * (both - none) / base:+.1f} % of the parent's backward "
                     f"({this['Nf']} centers)")
    else:
        lines.append(f"  overhead of both input gradients: {both - none:+.3f} ms = {100 * (both - none) / none:+.1f} % ({this['Nf']} centers)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
