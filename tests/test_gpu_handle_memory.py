"""What a handle owns comes back (csrc/pf_mem.h, pf_debug_live_memory): the library counts its own live allocations and their bytes,
device and pinned memory together, so the checks hold on a device that other processes allocate on too.

Small shapes only: two graphs of 24 and 40 atoms with 3 and 5 centers, n_convs 2, T = 8; the larger batch has four graphs of 60
atoms.  No result is compared with a reference here -- the parity tests do that -- except where a switch released a buffer: the next
pass of that kind must give the bits it gave before."""
import gc
import math

import pytest
import torch

import pharmacoforge_amd as pfa
from oracle import pf_oracle as O
from test_gpu_pinned import bound, engine_for, pins_for

pytestmark = pytest.mark.gpu

S = pfa.schedule
T, PREC = 8, 1e-4
live = pfa.PfEngine.live_memory


def config(width):
    return O.DynamicsConfig(n_hidden_scalars=width[0], vector_size=width[1], n_convs=2)


def small_batch(cfg):
    return O.synthetic_batch([0, 1], [24, 40], [3, 5], cfg)


def large_batch(cfg):
    return O.synthetic_batch([2, 3, 4, 5], 60, [4, 6, 5, 3], cfg)


def step_arrays(eng):
    gamma, order = O.gamma_table(T, PREC), list(reversed(range(T)))
    return (gamma, eng.coef_array(O.step_coefficients(gamma, T), order), eng.pin_coef_array(S.pin_coefficients(gamma, T), order),
            eng.guide_coef_array(S.guide_coefficients(gamma, T), order))


def inputs(cfg, batch, seed=7):
    gen = torch.Generator().manual_seed(seed)
    Nf = int(batch.pharm_ptr[-1])
    noise = torch.randn(T + 1, Nf, 3 + cfg.pharm_nf, generator=gen)
    pins = pins_for(batch, cfg, [1 if i == 1 else 0 for i in range(Nf)])         # the second center of the batch keeps its position
    return noise, pins


def guided_run(eng, cfg, batch, family):
    """a guided run armed with a pocket field (clash term), type guidance and pair restraints, next to one spatial restraint per graph"""
    _, arr, parr, garr = step_arrays(eng)
    noise, pins = inputs(cfg, batch)
    pcom = O.segment_mean(batch.prot_x, batch.prot_ptr)
    B = batch.batch_size
    restraints = [[("attract", 0, (pcom[g] + 1.0).tolist(), 1.0, 1.0)] for g in range(B)]
    types = dict(restraints=[[(2, None, pcom[g].tolist(), 0.0, 1.0)] for g in range(B)], scale=0.5)
    pairs = [[(None, None, 4.0, math.inf, 0.5)] for _ in range(B)]
    return eng.sample(arr, T, noise, pins=pins, pin_coef_arr=parr, restraints=restraints, guide_coef_arr=garr, guide_scale=2.0,
                      guide_family=family, field=dict(atom_r=1.5, w_clash=1.0), types=types, pairs=pairs, energies=True)


def train_pass(eng, cfg, batch, input_grads, seed=11):
    gen = torch.Generator().manual_seed(seed)
    Nf, B = int(batch.pharm_ptr[-1]), batch.batch_size
    x_t, h_t, t = torch.randn(Nf, 3, generator=gen), torch.randn(Nf, cfg.pharm_nf, generator=gen), torch.rand(B, generator=gen)
    w_h, w_x = torch.randn(Nf, cfg.pharm_nf, generator=gen), torch.randn(Nf, 3, generator=gen)
    eng.train_forward(x_t, h_t, t, prot_x=batch.prot_x, dropout=0.0)
    out = eng.train_backward(w_h, w_x, input_grads=input_grads)
    return tuple(o.cpu() for o in out) if input_grads else (out.cpu(),)


def everything(cfg, tuned):
    """every entry point that allocates, one after another on one engine"""
    batch = small_batch(cfg)
    eng = bound(engine_for(cfg, O.make_state_dict(cfg, 0)), batch)
    gamma, arr, parr, _ = step_arrays(eng)
    noise, pins = inputs(cfg, batch)
    eng.sample(arr, T, noise)                                                     # plain
    eng.sample(arr, T, noise, pins=pins, pin_coef_arr=parr)                       # pinned
    a = 6                                                                         # seeded multistep: from level 6 in three steps
    lv = S.level_plan(T, 3, top=a)
    eng.sample(None, len(lv) - 1, noise[:1], ms_coef_arr=eng.ms_coef_array(S.multistep_coefficients(gamma, T, lv)),
               seed=(pins[1], pins[2], S.seed_coefficients(gamma, T, a)))
    guided_run(eng, cfg, batch, "tuned" if tuned else "wide")
    bound(eng, batch)                                                             # (scoring is refused while a run holds the engine)
    levels = [2, 5]
    eng.score(pins[1], pins[2], levels, noise[:2], [0.5, 0.5], [0.5, 0.5], O.alpha(gamma), O.sigma(gamma), T)
    eng.sample_set(pins[1], pins[2].argmax(1), [0, 2], batch.pharm_ptr.tolist())  # the two graphs' centers as two samples of one set
    if tuned:
        eng.set_train_input_grads(True)
        train_pass(eng, cfg, batch, True)
    eng.set_train_family("wide")
    grad = train_pass(eng, cfg, batch, True)[0]
    params = eng.get_flat_params().clone()
    m, v = torch.zeros_like(params), torch.zeros_like(params)
    eng.adam_step_guarded(params, grad.to(params.device), m, v, eng.optim_state(), lr=1e-3, clip_norm=1.0)
    eng.build_pp_edges(batch.prot_x, batch.prot_ptr)
    torch.cuda.synchronize()
    assert eng.xchg_timeouts() == 0
    return eng


@pytest.mark.parametrize("width", [(128, 16), (64, 32)])
def test_destroy_gives_everything_back(width):
    gc.collect()                                       # (engines that earlier tests dropped into cycles go now, not between the readings)
    before = live()
    eng = everything(config(width), tuned=width == (128, 16))
    during = live()
    print(f"{width}: live before {before}, with the engine {during}")
    assert during[0] > before[0] and during[1] > before[1]
    del eng
    gc.collect()
    assert live() == before


def test_steady_state_allocates_nothing():
    cfg = config((128, 16))
    small, large = small_batch(cfg), large_batch(cfg)
    eng = bound(engine_for(cfg, O.make_state_dict(cfg, 0)), small)
    guided_run(eng, cfg, small, "tuned")
    first = live()
    guided_run(eng, cfg, small, "tuned")
    assert live() == first                             # the same shapes again: not one allocation, not one release
    bound(eng, large)
    guided_run(eng, cfg, large, "tuned")
    grown = live()
    print(f"live after the small batch {first}, after the large one {grown}")
    assert grown[0] >= first[0] and grown[1] >= first[1]
    bound(eng, small)
    guided_run(eng, cfg, small, "tuned")
    assert live() == grown                             # buffers are kept, not shrunk
    torch.cuda.synchronize()


def test_switches_give_back():
    cfg = config((128, 16))
    batch = small_batch(cfg)
    eng = bound(engine_for(cfg, O.make_state_dict(cfg, 0)), batch)
    # the family switch releases the workspace of the leg that is left
    tuned = train_pass(eng, cfg, batch, False)
    with_tuned = live()
    eng.set_train_family("wide")
    assert live()[1] < with_tuned[1] and live()[0] < with_tuned[0]
    wide = train_pass(eng, cfg, batch, False)
    with_wide = live()
    eng.set_train_family("tuned")
    assert live()[1] < with_wide[1]
    assert torch.equal(train_pass(eng, cfg, batch, False)[0], tuned[0])
    eng.set_train_family("wide")
    assert torch.equal(train_pass(eng, cfg, batch, False)[0], wide[0])
    eng.set_train_family("tuned")
    # the input-gradient switch releases the rows it owns
    eng.set_train_input_grads(True)
    first = train_pass(eng, cfg, batch, True)
    with_rows = live()
    eng.set_train_input_grads(False)
    assert live()[1] < with_rows[1] and live()[0] == with_rows[0] - 1
    eng.set_train_input_grads(True)
    again = train_pass(eng, cfg, batch, True)
    assert live() == with_rows
    for a, b in zip(first, again):
        assert torch.equal(a, b)
