"""The inputs of tests/test_gpu_feature_counts.py, checked on the CPU oracle alone: at every (pharm_nf, rec_nf) the GPU tests run,
every encoder input column counts.  Zeroing ONE column of an encoder's first Linear -- what a kernel does that never reads that
column, reads a zero for it, or reads the wrong type-table row for that type -- moves eps_h or eps_x by at least ten times the
error budget the GPU tests allow (helpers.within_budget's bound for that tensor).  Also: every type occurs, and the edge sets
are decided by no exact tie and no neighbour cap, so any correct implementation builds the same sets (the statement of
grad_budget.permuted_case).

With O.synthetic_pocket's types (columns 0..3 only) columns 4.. of the protein encoder see nothing but zeros; with random
types over all columns the least-used type's column moved the output by 0.0-1.6 budgets.  nf_cases.ranked_types puts the types
on the sources of the call's pf edges in turn."""
import pytest
import torch

from oracle import pf_oracle as O
from helpers import BUDGET_FACTOR, BUDGET_FLOOR
from nf_cases import NF_DESIGNS, SCORE_SEEDS, edge_margins, nf_case, score_case, score_reference

KNOCK_OUT = 10.0            # budgets an output has to move by when a column is zeroed
# (pharm_nf, rec_nf, features): every case of tests/test_gpu_feature_counts.py
CASES = [(1, 1, "onehot"), (7, 5, "onehot"), (8, 16, "onehot"), (8, 16, "dense"), (15, 17, "onehot"), (16, 40, "onehot"),
         (6, 127, "onehot"), (6, 130, "onehot"), (9, 11, "onehot"), (7, 33, "onehot")]
ENCODERS = (("prot", "dynamics.prot_encoder.0.weight"), ("pharm", "dynamics.pharm_encoder.0.weight"))


def budget(ref32, ref64):
    """within_budget's bound as an absolute error"""
    m = float(ref64.abs().max())
    e32 = float((ref32.double() - ref64).abs().max()) / m
    return BUDGET_FACTOR * max(e32, BUDGET_FLOOR) * m


def knock_out_ratios(c):
    """{(encoder, column): budgets the worse-hit output moves by with that column zeroed} on the live weights, fp32 oracle"""
    bh, bx = budget(c.live.oh, c.live.h64), budget(c.live.ox, c.live.x64)
    out = {}
    for name, key in ENCODERS:
        for col in range(c.live.sd[key].shape[1]):
            sd = dict(c.live.sd)
            w = sd[key].clone()
            w[:, col] = 0.0
            sd[key] = w
            oh, ox = O.dynamics_forward(sd, c.cfg, c.batch, c.prot_x, c.x_t, c.h_t, c.t)
            out[(name, col)] = max(float((oh - c.live.oh).abs().max()) / bh, float((ox - c.live.ox).abs().max()) / bx)
    return out


@pytest.mark.parametrize("pharm_nf,rec_nf,features", CASES)
def test_every_encoder_column_counts(pharm_nf, rec_nf, features):
    c = nf_case(pharm_nf, rec_nf, features=features)
    assert c.cfg.pharm_nf == pharm_nf and c.cfg.rec_nf == rec_nf
    assert c.batch.prot_h.shape == (int(c.batch.prot_ptr[-1]), rec_nf) and c.h_t.shape[1] == pharm_nf
    assert c.live.sd["dynamics.prot_encoder.0.weight"].shape[1] == rec_nf + 1
    assert c.live.sd["dynamics.pharm_encoder.0.weight"].shape[1] == pharm_nf + 1
    assert 0.5 <= float(c.live.ox.abs().max()) < 1.0                      # the live head: eps_x counts
    ratios = knock_out_ratios(c)
    assert len(ratios) == rec_nf + 1 + pharm_nf + 1
    (enc, col), least = min(ratios.items(), key=lambda kv: kv[1])
    print(f"feature counts ({pharm_nf}, {rec_nf}) {features}: least knock-out ratio {least:.1f} budgets ({enc} encoder column {col}), "
          f"{c.n_sources} distinct pf sources")
    assert least >= KNOCK_OUT, (enc, col, least)


@pytest.mark.parametrize("pharm_nf,rec_nf,features", [k for k in CASES if k[2] == "onehot"])
def test_every_type_occurs_on_a_pf_source(pharm_nf, rec_nf, features):
    c = nf_case(pharm_nf, rec_nf, features=features)
    h = c.batch.prot_h
    assert bool(((h == 0) | (h == 1)).all()) and bool((h.sum(dim=1) == 1).all())
    assert torch.equal(h.argmax(dim=1), c.types)
    src = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)["pf"][0]
    assert sorted(set(c.types[src].tolist())) == list(range(rec_nf))
    assert c.n_sources >= rec_nf


@pytest.mark.parametrize("pharm_nf,rec_nf,features", CASES)
def test_edge_sets_have_no_ties_and_reach_no_cap(pharm_nf, rec_nf, features):
    c = nf_case(pharm_nf, rec_nf, features=features)
    m = edge_margins(c.cfg, c.batch, c.prot_x, c.x_t)
    assert m == {"ties": 0, "cap_reached": 0}, m
    edges = O.build_dynamic_edges(c.cfg, c.batch, c.prot_x, c.x_t)
    for et in ("ff", "pf", "fp"):
        pairs = list(zip(edges[et][0].tolist(), edges[et][1].tolist()))
        assert len(pairs) == len(set(pairs)) > 0, et


def test_training_case_has_every_type_in_every_graph():
    """(8, 16): the last rec_nf of the per-(graph, element) sums of the encoder's backward -- every one of the 16 sums of every
    graph must be a sum over at least one atom"""
    c = nf_case(8, 16)
    for g in range(c.batch.batch_size):
        p0, p1 = int(c.batch.prot_ptr[g]), int(c.batch.prot_ptr[g + 1])
        assert sorted(set(c.types[p0:p1].tolist())) == list(range(16)), g


@pytest.mark.parametrize("pharm_nf,rec_nf", sorted(SCORE_SEEDS))
def test_score_cases_have_clear_margins(pharm_nf, rec_nf):
    """test_score_host.py's conditions at the counts the GPU score test runs: the predicted type of every center is clear of its
    runner-up (so `hits` compares exactly) and the fp32 and fp64 compositions count the same hits"""
    import score_ref as R
    r32, r64 = score_reference(pharm_nf, rec_nf, False), score_reference(pharm_nf, rec_nf, True)
    for p in R.PARAMS:
        assert torch.equal(r32[p][0][:, :, 3].double(), r64[p][0][:, :, 3])
        assert float(r64[p][1].min()) > 1e-3 and float(r32[p][1].min()) > 1e-3, (p, float(r64[p][1].min()))
        assert bool(torch.isfinite(r64[p][0]).all())
    if pharm_nf == 1:                                       # one class: every center is a hit, the cross-entropy is exactly zero
        sizes = (score_case(1, rec_nf).batch.pharm_ptr[1:] - score_case(1, rec_nf).batch.pharm_ptr[:-1]).double()
        for p in R.PARAMS:
            assert torch.equal(r64[p][0][:, :, 3], sizes.expand(len(R.LEVELS), -1))
        assert float(r64[(False, True)][0][:, :, 1].abs().max()) == 0.0


def test_designs_stay_small():
    """at most 150 atoms per pocket and three graphs: a GPU test on them takes a few seconds"""
    for (nf, rf), (n_prot, n_pharm, fields) in NF_DESIGNS.items():
        assert len(n_prot) == len(n_pharm) <= 3 and max(n_prot) <= 150, (nf, rf)


def test_nf_case_is_cached_and_seeded():
    a, b = nf_case(7, 5), nf_case(7, 5)
    assert a is b
    d = nf_case(7, 5, iseed=1)
    assert d is not a and not torch.equal(d.x_t, a.x_t) and torch.equal(d.batch.prot_x, a.batch.prot_x)
