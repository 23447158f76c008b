"""Host side of pinned centers: the noise-level table of a pinned run, the pin fields of PocketGraph through the batch
helpers, the pinned-centers file and the command line's size rules.  No GPU."""
import dataclasses
import os
import sys

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import generate_pharmacophores as cli  # noqa: E402


@pytest.mark.parametrize("T", [50, 500])
def test_pin_coefficients_equal_the_oracle(T):
    for prec in (1e-5, 0.25):
        gamma = O.gamma_table(T, prec)
        pc = pfa.schedule.pin_coefficients(gamma, T)
        s = torch.arange(T).float() / T
        g_s = O.gamma_lookup(gamma, s, T)
        assert pc["alpha_s"].dtype == torch.float32 and pc["alpha_s"].shape == (T,)
        assert torch.equal(pc["alpha_s"], O.alpha(g_s)) and torch.equal(pc["sigma_s"], O.sigma(g_s))
    arr = pfa.PfEngine.pin_coef_array(pc, reversed(range(T)))
    assert len(arr) == T and arr[0].alpha_s == float(pc["alpha_s"][T - 1]) and arr[T - 1].sigma_s == float(pc["sigma_s"][0])


def pocket(seed, n_prot, n_pharm):
    b = O.synthetic_batch([seed], n_prot, n_pharm, O.DynamicsConfig())
    return pfa.PocketGraph(b.prot_x, b.prot_h, b.prot_ptr, b.pharm_ptr, b.pp_src, b.pp_dst,
                           torch.zeros(n_pharm, 3), torch.zeros(n_pharm, 6))


def test_pin_fields_survive_copy_batch_unbatch_to():
    g = pocket(1, 20, 2)
    flags = torch.tensor([3, 1], dtype=torch.int32)
    px = torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    ph = torch.nn.functional.one_hot(torch.tensor([2, 5]), 6).float()
    gp = dataclasses.replace(g, pharm_pin=flags, pharm_pin_x=px, pharm_pin_h=ph)
    copies = pfa.copy_graph(gp, 2, pharm_feats_per_copy=[4, 2])
    assert copies[0].pharm_pin.tolist() == [3, 1, 0, 0] and copies[1].pharm_pin.tolist() == [3, 1]
    assert torch.equal(copies[0].pharm_pin_x[:2], px) and copies[0].pharm_pin_x.shape == (4, 3)
    assert torch.equal(copies[0].pharm_pin_h[:2], ph) and copies[0].pharm_pin_h.shape == (4, 6)
    with pytest.raises(ValueError):
        pfa.copy_graph(gp, 1, pharm_feats_per_copy=[1])
    plain = pfa.copy_graph(gp, 1)[0]                    # no resize: cloned as they are
    assert torch.equal(plain.pharm_pin, flags) and plain.pharm_pin is not flags
    free = pfa.copy_graph(pocket(2, 16, 3), 1, pharm_feats_per_copy=[3])[0]
    assert free.pharm_pin is None
    b = pfa.batch([copies[0], free, copies[1]])         # a graph without pins contributes free centers
    assert b.pharm_pin.tolist() == [3, 1, 0, 0] + [0, 0, 0] + [3, 1]
    assert b.pharm_pin_x.shape == (9, 3) and b.pharm_pin_h.shape == (9, 6)
    assert torch.equal(b.pharm_pin_x[7:], px) and torch.equal(b.pharm_pin_h[7:], ph)
    assert pfa.batch([free, free]).pharm_pin is None
    parts = pfa.unbatch(b)
    assert [p.pharm_pin.tolist() for p in parts] == [[3, 1, 0, 0], [0, 0, 0], [3, 1]]
    assert torch.equal(parts[2].pharm_pin_x, px) and torch.equal(parts[2].pharm_pin_h, ph)
    moved = b.to("cpu")
    assert torch.equal(moved.pharm_pin, b.pharm_pin) and torch.equal(moved.pharm_pin_x, b.pharm_pin_x)
    assert torch.equal(moved.pharm_pin_h, b.pharm_pin_h)
    sp = pfa.SampledPharmacophore(dataclasses.replace(parts[0], pharm_x0=torch.zeros(4, 3), pharm_h0=torch.eye(6)[:4]),
                                  pfa.analysis.ph_idx_to_type)
    assert sp.pinned.tolist() == [3, 1, 0, 0]
    assert pfa.SampledPharmacophore(g, pfa.analysis.ph_idx_to_type).pinned.tolist() == [0, 0]


def test_pinned_file_round_trips_the_output_format(tmp_path):
    text = pfa.write_pharmacophore_file([[[1.5, -2.25, 3.125], [0.001, 10.0, -7.5]]], [[2, 5]], pfa.analysis.ph_idx_to_type)
    f = tmp_path / "pins.xyz"
    f.write_text(text)
    x, types = pfa.analysis.read_pinned_centers(f)
    assert types.tolist() == [2, 5] and x.dtype == torch.float32
    assert torch.equal(x, torch.tensor([[1.5, -2.25, 3.125], [0.001, 10.0, -7.5]]))
    assert pfa.write_pharmacophore_file([x], [types], pfa.analysis.ph_idx_to_type) == text
    for bad in ("2\nF 1 2 3\nX 1 2 3\n", "2\nF 1 2 3\n", "F 1 2 3\n", "1\nF 1 2\n", "1\nF a b c\n", ""):
        f.write_text(bad)
        with pytest.raises(ValueError):
            pfa.analysis.read_pinned_centers(f)


def test_cli_size_rules(tmp_path, capsys):
    f = tmp_path / "pins.xyz"
    f.write_text("3\nP 0.000 1.000 2.000\nC 1.000 1.000 1.000\nN -1.000 0.500 2.500\n")
    base = ["rec.pdb", "--residue_list", "A:1", "--model_dir", "run", "--pinned_centers", str(f)]
    a = cli.parse_arguments(base + ["--samples_per_pocket", "2", "--pharm_sizes", "3", "6"])
    assert a.pin_what == "both" and a.pinned[1].tolist() == [0, 5, 3] and a.pinned[0].shape == (3, 3)
    assert cli.parse_arguments(base + ["--pin_what", "type"]).pin_what == "type"
    with pytest.raises(ValueError, match="below the 3 centers"):
        cli.parse_arguments(base + ["--samples_per_pocket", "2", "--pharm_sizes", "2", "6"])
    f.write_text("1\nQ 0 0 0\n")
    with pytest.raises(ValueError, match="bad center line"):
        cli.parse_arguments(base)
    assert cli.parse_arguments(["rec.pdb", "--residue_list", "A:1", "--model_dir", "run"]).pinned is None
    # sizes drawn uniformly: raised to k, with a note on stderr
    assert cli.pinned_sizes(torch.tensor([3, 8, 4, 5]), 5) == [5, 8, 5, 5]
    assert "2 drawn size(s) below the 5 pinned centers raised to 5" in capsys.readouterr().err
    assert cli.pinned_sizes([6, 7], 5) == [6, 7]
    assert capsys.readouterr().err == ""
