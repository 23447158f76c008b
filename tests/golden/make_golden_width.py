#!/usr/bin/env python3
"""Golden vectors of the reference model at hidden widths other than 128 / 16 (the width-generic kernels, pf_wide.hip).

Same recipe as make_golden.py, whose generator helpers it imports: the reference's own modules on top of ref_shim, weights
from oracle.pf_oracle.make_state_dict(cfg, wseed) (no weight file is committed).  Every job runs in a fresh process of its
own: state left behind by one reference model (the shim's caches, torch's global generator) must not reach the next.

    python tests/golden/make_golden_width.py                        # every fixture below, one process each
    python tests/golden/make_golden_width.py dynamics_w256.npz      # one fixture, in this process
"""
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def jobs():
    import make_golden as G
    O = G.O
    return {
        # S = 256, V = 16: kNN pf edges, message_norm 'mean', two conv layers
        "dynamics_w256.npz": lambda n: G.golden_conv_and_dynamics(
            O.DynamicsConfig(n_hidden_scalars=256, vector_size=16), n, seeds=[40, 41], n_prot=36, n_pharm=[4, 5], wseed=4),
        # S = 64, V = 32: radius pf edges, message_norm 0 (per-graph normalisers), three conv layers, ragged batch
        "dynamics_w64v32.npz": lambda n: G.golden_conv_and_dynamics(
            O.DynamicsConfig(n_hidden_scalars=64, vector_size=32, n_convs=3, message_norm=0, pf_k=0), n,
            seeds=[42, 43, 44], n_prot=[30, 44, 36], n_pharm=[4, 6, 3], wseed=5),
        # S = 192, V = 32: a T = 50 trajectory, every frame
        "traj_w192v32_T50.npz": lambda n: G.golden_trajectory(
            O.DynamicsConfig(n_hidden_scalars=192, vector_size=32), n, seeds=[45], n_prot=48, n_pharm=4, T=50, wseed=6),
    }


NAMES = ["dynamics_w256.npz", "dynamics_w64v32.npz", "traj_w192v32_T50.npz"]


def main():
    want = sys.argv[1:]
    if not want:
        for name in NAMES:
            subprocess.run([sys.executable, os.path.abspath(__file__), name], check=True)
        return
    torch.set_num_threads(1)
    table = jobs()
    for name in want:
        table[name](name)


if __name__ == "__main__":
    main()
