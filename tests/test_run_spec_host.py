"""The run spec of the sampling front (models.RunSpec): the whole keyword grid once, through the way sample and the
way sample_given_receptor build the spec -- every cell is either the ValueError of the composition rule it breaks or the batch's
answer (run kind, n_ops, noise rows), and the two entry points agree in every cell.  No device work is reached."""
import dataclasses
import itertools

import pytest
import torch

import pharmacoforge_amd as pfa
from pharmacoforge_amd import schedule as S
from test_host_logic import make_model
from test_seeded_host import pocket

T, LEVEL, N, JUMP = 12, 4, 3, 3


class _Resolved(Exception):
    pass


def expected(pins, resamples, guide, seed, few):
    """The README's / DESIGN's rules, written out: a message fragment, or (kind, n_ops, noise rows) of a batch that holds what the
    cell asks for"""
    has_pins, guided = pins or seed == "keep", guide is not None
    if few is not None and resamples > 1:
        return "pin_resamples > 1"                          # no resampling jumps over a strided plan
    if few == "multistep" and (has_pins or guided):
        return "composes with seeds only"
    if guided and resamples > 1:
        return "resampling"                                 # guidance with resampling jumps is not supported
    if seed is not None and pins:
        return "use seed_keep"
    top = LEVEL if seed is not None else T
    if few == "multistep":
        return "multistep", N, 1                            # the initial draw only
    kind = "guided" if guided else "pinned" if has_pins else "plain"
    if few is not None:
        return kind, N, N + 1
    if has_pins and resamples > 1:
        n_ops = len(S.resample_plan(top, JUMP, resamples))
        return "resampled", n_ops, n_ops + 1
    return kind, top, top + 1                               # T + 1 rows, a + 1 from a seed level a


def test_keyword_grid():
    m = make_model(T)
    g = pocket(3, 1)
    g_pinned = dataclasses.replace(g, pharm_pin=torch.tensor([3, 0, 0], dtype=torch.int32), pharm_pin_x=torch.zeros(3, 3),
                                   pharm_pin_h=torch.eye(6)[:3])
    restr = [[("repel", None, [0.0, 0.0, 0.0], 3.0, 1.0)]]
    specs = []
    resolve = m._run_spec

    def capture(*a, **k):
        specs.append(resolve(*a, **k))
        raise _Resolved
    m._run_spec = capture
    kinds = set()
    for pins, resamples, guide, seed, few in itertools.product((False, True), (1, 2), (None, "restraints", "field"),
                                                               (None, "seeded", "keep"), (None, "ancestral", "ddim", "multistep")):
        kw = dict(pin_resamples=resamples, pin_jump=JUMP)
        if guide is not None:
            kw.update(restraints=restr) if guide == "restraints" else kw.update(pocket_field=pfa.PocketField())
        if seed is not None:
            kw.update(seeds=[(torch.zeros(3, 3), torch.tensor([0, 1, 2]))], seed_level=LEVEL)
        if seed == "keep":
            kw.update(seed_keep=[[0]])
        if few is not None:
            kw.update(sample_steps=N, sampler=few)
        entries = (lambda: m.sample([g], [[3]], pinned=[(torch.zeros(1, 3), torch.tensor([0]), None)] if pins else None, **kw),
                   lambda: m.sample_given_receptor(g_pinned if pins else g, **kw))
        want = expected(pins, resamples, guide, seed, few)
        cell = (pins, resamples, guide, seed, few)
        del specs[:]
        for call in entries:
            with pytest.raises(ValueError if isinstance(want, str) else _Resolved, match=want if isinstance(want, str) else None):
                call()
        if isinstance(want, str):
            assert not specs, cell
            continue
        assert len(specs) == 2 and specs[0] == specs[1], cell
        spec = specs[0]
        assert (spec.top, spec.seeded, spec.guided) == (LEVEL if seed else T, seed is not None, guide is not None), cell
        got = spec.batch(m, pins or seed == "keep", guide is not None)
        assert got[:3] == want, (cell, got[:3])
        kinds.add(got[0])
        # a batch of the same call without a flag or a restraint in it runs the default path of that spec
        if few is None:
            top = LEVEL if seed else T
            assert spec.batch(m, False, guide == "field")[:3] == ("guided" if guide == "field" else "plain", top, top + 1), cell
    assert kinds == {"plain", "pinned", "resampled", "guided", "multistep"}
