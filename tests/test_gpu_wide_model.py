"""The width-generic kernels through the user-facing Python layer: PharmacophoreDiff.sample over several pockets with
pocket sharing, a checkpoint round trip at another width, training refused with the library's message, and
generate_pharmacophores.py on a (256, 16) checkpoint."""
import os
import subprocess
import sys

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O
from test_gpu_api import DEV_GRAPH, _write_pocket_files, graph_from

pytestmark = pytest.mark.gpu


def make_model(S, V, T, wseed=0):
    dyn = dict(vector_size=V, n_convs=2, n_hidden_scalars=S, message_norm='mean', dropout=0.1, ff_k=0, pf_k=5,
               n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4)
    m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=T, graph_config=DEV_GRAPH,
                              dynamics_config=dyn, precision=1e-5)
    sd = dict(O.make_state_dict(O.DynamicsConfig(n_hidden_scalars=S, vector_size=V), wseed))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    return m.to("cuda").eval()


def test_sample_three_pockets_with_sharing_vs_oracle():
    S, V, T = 256, 16, 15
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
    m = make_model(S, V, T, wseed=2)
    batches = [O.synthetic_batch([s], n, 1, cfg) for s, n in ((50, 40), (51, 52), (52, 33))]
    pockets = [graph_from(b) for b in batches]
    n_pharms = [[3, 4], [5], [8, 3, 6]]
    mb = 4
    sizes = [n for p in n_pharms for n in p]
    gen = torch.Generator().manual_seed(3)
    noises = [torch.randn(T + 1, sum(sizes[i:i + mb]), 9, generator=gen) for i in range(0, len(sizes), mb)]
    com = torch.stack([b.prot_x.mean(dim=0) for b in batches]) + 0.5
    out = m.sample(pockets, n_pharms, max_batch_size=mb, init_pharm_com=com, noise=noises)
    ref = O.sample(O.make_state_dict(cfg, 2), cfg, batches, n_pharms, mb, T, 1e-5, noises, init_pharm_com=com)
    assert [[p.n_ph_centers for p in o] for o in out] == n_pharms
    for o, r in zip(out, ref):
        for p, (x0, h0) in zip(o, r):
            torch.testing.assert_close(p.ph_coords.cpu(), x0, rtol=0, atol=2e-2)
            torch.testing.assert_close(p.g.pharm_h0.cpu(), h0, rtol=0, atol=2e-2)


def test_checkpoint_round_trip_and_training_refused(tmp_path):
    S, V, T = 256, 32, 10
    cfg = O.DynamicsConfig(n_hidden_scalars=S, vector_size=V)
    m = make_model(S, V, T, wseed=1)
    pockets = [graph_from(O.synthetic_batch([s], 48, 1, cfg)) for s in (53, 54)]
    n_pharms = [[3, 5], [4]]
    torch.manual_seed(0)
    out = m.sample(pockets, n_pharms, max_batch_size=4)
    ck = tmp_path / "w256v32.ckpt"
    m.save_checkpoint(ck)
    m2 = pfa.PharmacophoreDiff.load_from_checkpoint(ck).to("cuda").eval()
    torch.manual_seed(0)
    out2 = m2.sample(pockets, n_pharms, max_batch_size=4)
    for a, b in zip(out, out2):
        for pa, pb in zip(a, b):
            assert torch.isfinite(pa.ph_coords).all()
            assert torch.equal(pa.ph_coords, pb.ph_coords)
    # training is specialised to 128 / 16: the library refuses, naming the widths
    g = pfa.batch(pfa.copy_graph(pockets[0], 2, pharm_feats_per_copy=[3, 4])).to("cuda")
    m2.train()
    with pytest.raises(pfa.PfError, match="n_hidden_scalars 128 / vector_size 16"):
        m2.training_step(g, 0)
    with pytest.raises(pfa.PfError, match="n_hidden_scalars 128 / vector_size 16"):
        m2.forward(g, phase='train')


def test_generate_pharmacophores_at_width_256(tmp_path):
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_pocket_files(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(root, "tests", "golden", "dev_config_subset.yml")))
    cfg['diffusion']['n_timesteps'] = 12
    cfg['dataset']['pocket_cutoff'] = 8
    cfg['dynamics']['n_hidden_scalars'] = 256
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True)
    yaml.dump(cfg, open(run / "config.yaml", "w"))
    m = pfa.model_from_config(cfg)
    sd = dict(O.make_state_dict(O.DynamicsConfig(n_hidden_scalars=256), 0))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m.save_checkpoint(run / "checkpoints" / "last.ckpt")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "generate_pharmacophores.py"), str(tmp_path / "rec.pdb"), "--ref_ligand_file",
           str(tmp_path / "lig.sdf"), "--model_dir", str(run), "--samples_per_pocket", "4", "--pharm_sizes", "3", "4", "5", "6",
           "--max_batch_size", "2", "--output_dir", str(out), "--seed", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    xyz = (out / "rec" / "pharms.xyz").read_text().splitlines()
    counts, i = [], 0
    while i < len(xyz):
        n = int(xyz[i]); counts.append(n)
        for l in xyz[i + 1:i + 1 + n]:
            el, x, y, z = l.split()
            assert el in "PSFNOC" and all(abs(float(v)) < 1e4 for v in (x, y, z))
        i += n + 1
    # copy_graph indexes pharm_sizes from 0 in every chunk (the reference's quirk, as test_gpu_api): chunks of 2 samples
    assert counts == [3, 4, 3, 4]
