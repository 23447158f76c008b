#!/usr/bin/env python3
"""Golden vectors of the reference's training forward with the endpoint parameterisations (endpoint_param_coord /
endpoint_param_feat, pharmacodiff.py:204-215): tests/golden/train_endpoint.npz.

Same recipe as make_golden.py's golden_train_forward, whose helpers it imports: the reference's own PharmacophoreDiff.forward
on top of ref_shim in eval() mode (dropout is the identity), weights from oracle.pf_oracle.make_state_dict(cfg, wseed), clean
centers from Generator().manual_seed(3), the reference's draws (t_int, eps_h, eps_x) reproduced under torch.manual_seed(5).
Three cases share the batch and the draws and differ in the model's flags; their arrays carry the case's prefix:

    both_   endpoint_param_coord + endpoint_param_feat, remove_com, unweighted: losses, metrics and d(total loss)/d(parameter)
            of every dynamics parameter (backward() through the reference, grad enabled, eval mode)
    feat_   endpoint_param_feat only, remove_com, weighted_loss: losses and metrics
    coord_  endpoint_param_coord only, remove_com off, unweighted: losses and metrics

The gradients are fp32 noise to a compressor (about 2.2 MB): they go to train_endpoint_grads_<i>.npz, each below the size
limit of a committed file; train_endpoint.npz lists the parts in `grad_parts`.

Every case runs in a fresh process (state left behind by one reference model must not reach the next), writes a part file
next to this script, and the parent merges the parts.  For every case the generator asserts that the two largest entries of
the row whose argmax feeds the accuracy are at least 1e-2 apart at every center: the accuracy cannot flip within fp32 error.

    python tests/golden/make_golden_endpoint.py             # all three cases, one process each, then the merge
    python tests/golden/make_golden_endpoint.py both_       # one case, in this process (writes its part file only)
"""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

NAME = "train_endpoint.npz"
GRAD_PART_BYTES = 900 * 1024                 # uncompressed payload of one gradient file (limit of a committed file: 1 MiB)
CASES = {
    #          endpoint_param_coord, endpoint_param_feat, remove_com, weighted_loss, gradients
    "both_": (True, True, True, False, True),
    "feat_": (False, True, True, True, False),
    "coord_": (True, False, False, False, False),
}
MIN_GAP = 1e-2


def run_case(prefix):
    import make_golden as G
    O = G.O
    ep_coord, ep_feat, remove_com, weighted, with_grads = CASES[prefix]
    cfg, T, wseed, rseed = O.DynamicsConfig(), 100, 0, 5
    m, _ = G.ref_model(cfg, T, 1e-5, seed=wseed)        # eval(): dropout is the identity
    m.endpoint_param_coord, m.endpoint_param_feat = ep_coord, ep_feat
    m.remove_com, m.weighted_loss = remove_com, weighted
    batch = O.synthetic_batch([11, 12, 13], [40, 52, 33], [4, 6, 3], cfg)
    Nf, B = int(batch.pharm_ptr[-1]), batch.batch_size
    gen = torch.Generator().manual_seed(3)
    x0 = 3.0 * torch.randn(Nf, 3, generator=gen)
    types = torch.randint(0, cfg.pharm_nf, (Nf,), generator=gen)
    h0 = torch.nn.functional.one_hot(types, cfg.pharm_nf).float()
    g = G.ref_graph(batch, x0, h0, cfg.pharm_nf)
    torch.manual_seed(rseed)
    t_int = torch.randint(0, T, size=(B,))
    eps_h = torch.randn(Nf, cfg.pharm_nf)
    eps_x = torch.randn(Nf, 3)

    seen = {}

    def hook(mod, inputs, output):          # the dynamics' input state and outputs: what the accuracy's argmax is taken of
        seen["h_t"] = inputs[0].nodes['pharm'].data['h_t'].detach().clone()
        seen["t"] = inputs[1].detach().clone()
        seen["h_dyn"] = output[0].detach().clone()

    handle = m.dynamics.register_forward_hook(hook)
    torch.manual_seed(rseed)
    with torch.set_grad_enabled(with_grads):
        losses, metrics = m.forward(g, 'train')
        if with_grads:
            torch.sum(torch.stack(list(losses.values()), dim=0)).backward()      # pharmacodiff.py:276
    handle.remove()

    with torch.no_grad():
        if ep_feat:
            rows = seen["h_dyn"]
        else:
            bp = batch.batch_idxs()["pharm"]
            gamma_t = m.gamma(seen["t"])
            rows = (seen["h_t"] - m.sigma(gamma_t)[bp][:, None] * seen["h_dyn"]) / m.alpha(gamma_t)[bp][:, None]
        top = rows.topk(2, dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min())
    assert gap >= MIN_GAP, f"{prefix}: the two largest entries of an accuracy row are {gap} apart (< {MIN_GAP}); choose other inputs"
    print(f"{prefix} smallest argmax gap {gap:.4f}")

    out = dict(G.batch_arrays(batch), x0=x0, h0=h0, t_int=t_int, eps_h=eps_h, eps_x=eps_x, T=T, wseed=wseed)
    out[prefix + "endpoint_param_coord"], out[prefix + "endpoint_param_feat"] = int(ep_coord), int(ep_feat)
    out[prefix + "remove_com"], out[prefix + "weighted_loss"] = int(remove_com), int(weighted)
    out[prefix + "argmax_gap"] = gap
    for k, v in {**losses, **metrics}.items():
        out[prefix + "out_" + k.replace(" ", "_")] = v.detach()
    if with_grads:
        for k, prm in m.named_parameters():
            if k.startswith("dynamics.") and prm.numel() > 0:
                out[prefix + "grad_" + k] = torch.zeros_like(prm) if prm.grad is None else prm.grad.detach()
    G.npz(part_name(prefix), **out)


def part_name(prefix):
    return f"_train_endpoint_part_{prefix}.npz"


def merge():
    shared, grads = {}, {}
    for prefix in CASES:
        path = os.path.join(HERE, part_name(prefix))
        with np.load(path) as z:
            for k in z.files:
                if k.startswith(prefix + "grad_"):
                    grads[k] = z[k]
                    continue
                if k in shared:                 # the batch and the draws: identical in every case
                    assert np.array_equal(shared[k], z[k]), k
                shared[k] = z[k]
        os.remove(path)
    parts, cur, size = [], {}, 0
    for k, v in grads.items():
        if cur and size + v.nbytes > GRAD_PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes
    if cur:
        parts.append(cur)
    names = [f"train_endpoint_grads_{i}.npz" for i in range(len(parts))]
    shared["grad_parts"] = np.array(names)
    for n, p in zip(names, parts):
        np.savez_compressed(os.path.join(HERE, n), **p)
    np.savez_compressed(os.path.join(HERE, NAME), **shared)
    for n in [NAME] + names:
        kib = os.path.getsize(os.path.join(HERE, n)) / 1024
        assert kib < 1024, (n, kib)
        print(f"wrote {n}: {kib:.1f} KiB")


def main():
    want = sys.argv[1:]
    if not want:
        for prefix in CASES:
            subprocess.run([sys.executable, os.path.abspath(__file__), prefix], check=True)
        merge()
        return
    torch.set_num_threads(1)
    for prefix in want:
        run_case(prefix)


if __name__ == "__main__":
    main()
