#!/usr/bin/env python3
"""Training goldens of the reference model at hidden widths other than 128 / 16 (the width-generic training leg:
pf_train_set_family, pf_wide_train.hip).

Same recipe as make_golden_width.py: make_golden.golden_train_grads -- the reference's own training_step in train() mode, its
GVPDropout draws recorded -- on weights from oracle.pf_oracle.make_state_dict(cfg, wseed), one fresh process per fixture.  A
full gradient set is larger than a committed file may be, so each fixture is written as parts of at most PART_BYTES of array
data: NAME.npz holds the batch, the draws, the masks, the losses and as many gradient tensors as fit, NAME.p1.npz, NAME.p2.npz,
... the rest (tests/test_oracle_width_train.py: load_parts puts them together again).

    python tests/golden/make_golden_width_train.py                              # both fixtures, one process each
    python tests/golden/make_golden_width_train.py train_grads_w96v16.npz       # one fixture, in this process
"""
import glob
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

PART_BYTES = 900 * 1024


def jobs():
    import make_golden as G
    O = G.O
    return {
        # S = 64, V = 32: radius pf edges, message_norm 0 (per-graph normalisers), three conv layers, ragged batch
        "train_grads_w64v32.npz": lambda n: G.golden_train_grads(
            O.DynamicsConfig(n_hidden_scalars=64, vector_size=32, n_convs=3, message_norm=0, pf_k=0), n,
            seeds=[46, 47, 48], n_prot=[30, 44, 36], n_pharm=[4, 6, 3], wseed=7),
        # S = 96, V = 16: kNN pf edges, message_norm 'mean', two conv layers
        "train_grads_w96v16.npz": lambda n: G.golden_train_grads(
            O.DynamicsConfig(n_hidden_scalars=96, vector_size=16), n, seeds=[49, 50], n_prot=36, n_pharm=[5, 3], wseed=8),
    }


NAMES = ["train_grads_w64v32.npz", "train_grads_w96v16.npz"]


def split(name):
    """NAME.npz as written by make_golden.npz -> NAME.npz, NAME.p1.npz, ... of at most PART_BYTES of array data each"""
    path = os.path.join(HERE, name)
    with np.load(path, allow_pickle=False) as z:
        arrs = {k: z[k] for k in z.files}
    for old in glob.glob(path[:-4] + ".p*.npz"):
        os.remove(old)
    parts, size = [{}], 0
    for k in sorted(arrs, key=lambda k: k.startswith("grad_")):          # everything but the gradients first, in one part
        if parts[-1] and size + arrs[k].nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = arrs[k]
        size += arrs[k].nbytes
    parts[0]["n_parts"] = np.asarray(len(parts))
    for i, part in enumerate(parts):
        out = path if i == 0 else f"{path[:-4]}.p{i}.npz"
        np.savez_compressed(out, **part)
        print(f"wrote {os.path.basename(out)}: {os.path.getsize(out) / 1024:.1f} KiB, {len(part)} arrays")


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
        split(name)


if __name__ == "__main__":
    main()
