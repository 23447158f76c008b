"""train_host_equality.py -- what the gradient path computes, as one sha256 per case: run it once per build of the library
(PFDYN_LIB selects the build, one process each) and compare the two outputs line for line.  A refactor of the host code that
sequences the training launches must leave every line unchanged; the suite's repeatability tests are what make the comparison
meaningful (per-block gradient copies summed in block order, the level-0 scatter on fixed-point accumulators).

Cases: n_convs 1 / 2 / 3  x  dropout 0 / 0.1 (fixed seed)  x  entry (pf_train_loss_forward + pf_train_loss_backward,
pf_train_loss_forward_ep + pf_train_loss_backward_out with both endpoint flags, pf_train_forward + pf_train_backward)  x
f32 / bf16  x  the specialised / the width-generic leg (forced onto 128 / 16)  x  default / PFDYN_NO_PRUNE=1 (read when the
handle is created).  The hash covers the gradient, eps_h, eps_x and, for the loss entries, the nine loss outputs.  The
width-generic leg is fp32 only: its bf16 cases print the refusal.

    python tools/train_host_equality.py [--out FILE]"""
import argparse
import ctypes
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

T = 100


def digest(tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


def run_case(pfa, n_convs, p_drop, entry, dtype, leg, no_prune):
    from pharmacoforge_amd import schedule, synthetic
    from pharmacoforge_amd.engine import _dptr, _f32, _stream_ptr
    if no_prune:
        os.environ["PFDYN_NO_PRUNE"] = "1"
    else:
        os.environ.pop("PFDYN_NO_PRUNE", None)
    eng = pfa.PfEngine(n_convs=n_convs)
    eng.load_state_dict(synthetic.make_state_dict(3, n_convs=n_convs))
    if leg == "wide":
        eng.set_train_family("wide")
    try:
        eng.set_train_precision(dtype)
    except Exception as e:
        return "refused: " + str(e).splitlines()[0]
    # two graphs: 12 and 20 atoms, 2 and 3 centers
    pockets = [synthetic.synthetic_pocket(21, 12), synthetic.synthetic_pocket(22, 20)]
    prot_x, prot_h = torch.cat([p[0] for p in pockets]), torch.cat([p[1] for p in pockets])
    prot_ptr, pharm_ptr = torch.tensor([0, 12, 32]), torch.tensor([0, 2, 5])
    pp_src, pp_dst = eng.build_pp_edges(prot_x, prot_ptr)
    eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, pp_src, pp_dst)
    gen = torch.Generator().manual_seed(7)
    Nf, B, nf = 5, 2, eng.pharm_nf
    com = torch.cat([pockets[g][0].mean(0, keepdim=True).expand(n, 3) for g, n in ((0, 2), (1, 3))])      # per center: its pocket's
    seed = 4321
    if entry == "plain":
        x_t = com + 2.5 * torch.randn(Nf, 3, generator=gen)
        h_t = torch.randn(Nf, nf, generator=gen)
        t = torch.rand(B, generator=gen)
        w_h, w_x = torch.randn(Nf, nf, generator=gen), torch.randn(Nf, 3, generator=gen)
        eps_h, eps_x = eng.train_forward(x_t, h_t, t, dropout=p_drop, seed=seed)
        grad = eng.train_backward(w_h, w_x)
        return digest([grad, eps_h, eps_x])
    x0 = com + 2.0 * torch.randn(Nf, 3, generator=gen)
    h0 = torch.nn.functional.one_hot(torch.randint(0, nf, (Nf,), generator=gen), nf).float()
    t_int = torch.randint(0, T, (B,), generator=gen)
    e_x, e_h = torch.randn(Nf, 3, generator=gen), torch.randn(Nf, nf, generator=gen)
    gamma = schedule.PredefinedNoiseSchedule("polynomial_2", T, 1e-5).gamma.detach()
    a_tab, s_tab = schedule.alpha(gamma).float().contiguous(), schedule.sigma(gamma).float().contiguous()
    if entry == "loss_ep":
        out = eng.train_loss_forward(x0, h0, t_int, e_x, e_h, a_tab, s_tab, T, 1.0, True, True, dropout=p_drop, seed=seed,
                                     ep_coord=True, ep_feat=True)
        eps_h, eps_x = eng.last_eps()
        g_out = torch.zeros(9)
        g_out[0], g_out[1], g_out[6] = 0.5, 0.25, 1.0
        grad = eng.train_loss_backward_out(g_out)
    else:       # the entry without the endpoint flags, which the engine class never calls
        dev = eng.device
        args = [_f32(x0, dev), _f32(h0, dev), t_int.to(dev, torch.int32).contiguous(), _f32(e_x, dev), _f32(e_h, dev), _f32(a_tab, dev),
                _f32(s_tab, dev)]
        out = torch.empty(9, device=dev)
        with torch.cuda.device(dev):
            eng._ck(eng.lib.pf_train_loss_forward(eng._h, *[_dptr(a) for a in args], T, ctypes.c_float(1.0), 1, 0, ctypes.c_float(p_drop),
                                                  seed, _dptr(out), _stream_ptr()), "pf_train_loss_forward")
        eps_h, eps_x = eng.last_eps()
        grad = eng.train_loss_backward(torch.tensor(1.0), torch.tensor(0.5))
    return digest([grad, eps_h, eps_x, out])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import pharmacoforge_amd as pfa
    torch.zeros(1, device="cuda")
    lines = ["library " + pfa._lib.load().pf_version().decode()]
    for n_convs, p_drop, entry, dtype, leg, no_prune in itertools.product((1, 2, 3), (0.0, 0.1), ("loss", "loss_ep", "plain"), ("f32", "bf16"),
                                                                           ("spec", "wide"), (0, 1)):
        name = f"convs{n_convs} drop{p_drop} {entry} {dtype} {leg} {'no_prune' if no_prune else 'default'}"
        lines.append(f"{name}: {run_case(pfa, n_convs, p_drop, entry, dtype, leg, no_prune)}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
