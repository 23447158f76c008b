"""sampler_host_equality.py -- what the sampler's host code enqueues, as one line per case: run it once per build of the library
(PFDYN_LIB selects the build, one process each) and compare the two outputs line for line.  A refactor of the host code that
sequences the sampling launches must leave every line unchanged; the sampler is bitwise repeatable (the suite asserts it), so a
line that differs is a bug, not a tolerance question.  The tool uses the public surface only, so the same file also runs on a checkout of another
commit: a refactor of the Python front is checked by running it from both trees.

Cases: run kind (plain, pinned, pinned with all flags zero, resampled with jump 3 and 2 resamples, guided, guided with pins)  x
entry (the whole-loop C call, the step API driven op by op)  x  batch (two graphs of 12 and 20 atoms with 2 and 3 centers; 32
copies of one 20-atom pocket with 3..8 centers, the size at which the default plain step takes its merged launch with a center
hoist; at n_convs 2 only, `edge`: four graphs of 300 / 70 / 33 / 48 atoms with 64 / 1 / 17 / 2 centers, which reach what the small
batches cannot -- the stride-64 loop of the frame offset, the stride-256 loop over the protein rows, lanes 8..63 of the move's
center mapping, a graph with a single center)  x  n_convs 1 / 2 / 3  x  environment (read when the handle is created: every case
creates its own).  T = 12; the noise is seeded.  Five further kinds -- seeded (seed level 5), multistep and seeded_multistep (4 steps; the step entry makes them with
ms_step), guided_field (a pocket field with a clash radius, no restraints), guided_tuned (guide_family="tuned"), guided_types (type
restraints only, one graph in two without any, feat_scale 1) and guided_field_types (a pocket field with receptor features and
w_comp > 0 plus type guidance with complementarity=True and unmatched 1.5: the TYPES form of the field launch) -- run with the
default environment and PFDYN_WIDE=1 only.

--model adds one line per model-level case (MODEL_CASES), a sha256 over every returned pharmacophore's x_0, h_0 and score, through
PharmacophoreDiff.sample and through sample_given_receptor on the batch of the same graphs, each with drawn noise
(torch.manual_seed, noise=None) and with given noise: the "two" batch, T = 12, n_convs 2, default environment.

A line holds: a sha256 over x_0, h_0, both trajectory arrays, last_eps() and, for guided runs, the energies and last_guidance(), with a pocket field last_field_energies(), with type guidance
last_type_guidance();
ahead() after the step in the middle of the run (step API) or after the run (whole loop); kernel_family(0) and l0_hoist(); and the
launch counts per kernel class of a second pass of the same case on the same handle, through the step API with every kernel class
profiled (profiling the step class switches the merged launch off, hence a second pass; only the counts are printed, times are not
reproducible).

    python tools/sampler_host_equality.py [--out FILE] [--only SUBSTRING] [--model]"""
import argparse
import dataclasses
import hashlib
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

T, JUMP, RESAMPLES, PREC = 12, 3, 2, 0.25
SEED_LEVEL, MS_STEPS = 5, 4
KINDS = ("plain", "pinned", "pinned0", "resampled", "guided", "guided_pins")
FRONT_KINDS = ("seeded", "multistep", "seeded_multistep", "guided_field", "guided_tuned", "guided_types", "guided_field_types")     # (default environment and PFDYN_WIDE=1)
FIELD = dict(atom_r=1.5, w_clash=1.0)
ENVS = ("default", "PFDYN_NO_ENC_FLY=1", "PFDYN_NO_CENTER_HOIST=1", "PFDYN_NO_PA_SPEC=1", "PFDYN_NO_FAST_BUILD=1", "PFDYN_TAIL_FORM=16",
        "PFDYN_WIDE=1")
_cache = {}


def digest(tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().cpu().contiguous().numpy().tobytes())
    return m.hexdigest()[:32]


def batch_of(name):
    """(pockets' tensors, prot_ptr, pharm_ptr, COM per graph, COM per center) -- 'two': 12 and 20 atoms, 2 and 3 centers; 'copies': 32 x 20 atoms"""
    from pharmacoforge_amd import synthetic
    if name not in _cache:
        if name == "two":
            pockets, nfs = [synthetic.synthetic_pocket(21, 12), synthetic.synthetic_pocket(22, 20)], [2, 3]
        elif name == "edge":
            pockets, nfs = [synthetic.synthetic_pocket(23 + g, n) for g, n in enumerate((300, 70, 33, 48))], [64, 1, 17, 2]
        else:
            pockets, nfs = [synthetic.synthetic_pocket(22, 20)] * 32, [3 + g % 6 for g in range(32)]
        ptr = lambda ns: torch.tensor([0] + list(itertools.accumulate(ns)))
        com = torch.stack([p[0].mean(0) for p in pockets])
        _cache[name] = (torch.cat([p[0] for p in pockets]), torch.cat([p[1] for p in pockets]), ptr([p[0].shape[0] for p in pockets]), ptr(nfs),
                        com + 0.5, com.repeat_interleave(torch.tensor(nfs), 0))
    return _cache[name]


def schedule_arrays(eng, kind):
    """(n_ops, op kinds or None, coef_arr, pin_arr, renoise_arr, guide_arr), one entry per op"""
    from pharmacoforge_amd import schedule
    gamma = schedule.PredefinedNoiseSchedule("polynomial_2", T, PREC).gamma.detach()
    coef, pin = schedule.step_coefficients(gamma, T), schedule.pin_coefficients(gamma, T)
    top = SEED_LEVEL if kind.startswith("seeded") else T
    if kind.endswith("multistep"):
        lv = schedule.level_plan(T, MS_STEPS, "uniform", top, gamma_table=gamma)
        return MS_STEPS, None, eng.ms_coef_array(schedule.multistep_coefficients(gamma, T, lv)), None, None, None
    if kind == "resampled":
        plan = schedule.resample_plan(T, JUMP, RESAMPLES)
        pairs = [(op[1], op[2]) for op in plan if op[0] == "renoise"]
        arr, parr, op_arr, re_arr = eng.plan_arrays(plan, coef, pin, schedule.renoise_coefficients(gamma, T, pairs))
        return len(plan), op_arr, arr, parr, re_arr, None
    order = list(reversed(range(top)))
    return top, None, eng.coef_array(coef, order), eng.pin_coef_array(pin, order), None, eng.guide_coef_array(schedule.guide_coefficients(gamma, T), order)


def step_api(eng, kind, sched, noise, com, pins, restraints, mid_ahead, seed=None, field=None, types=None):
    """the run op by op: (x_0, h_0, frames x, frames h) and, in mid_ahead, ahead() after the middle op"""
    n_ops, op_arr, arr, parr, re_arr, garr = sched
    guided = restraints is not None or field is not None or types is not None
    family, grads = eng.train_family(), eng.train_input_grads()
    kw = {k: v for k, v in (("seed", seed), ("field", field), ("types", types)) if v is not None}
    if kind == "guided_tuned":
        kw["guide_family"] = "tuned"
    elif guided:
        eng.set_train_family("wide")
    try:
        eng.sample_begin(noise[0], init_pharm_com=com, pins=pins, restraints=restraints, guide_scale=1.5, guide_clip=0.5, **kw)
        fx, fh = ([t] for t in eng.sample_frame())
        if not guided:
            eng.prepare_timesteps([arr[i] for i in range(n_ops) if op_arr is None or op_arr[i] == 0])
        for i in range(n_ops):
            if kind.endswith("multistep"):
                eng.ms_step(arr[i])
            elif op_arr is not None and op_arr[i] == 1:
                eng.renoise_step(re_arr[i], noise[i + 1])
            elif guided:
                eng.guided_step(arr[i], parr[i], garr[i], noise[i + 1])
            else:
                eng.denoise_step(arr[i], noise[i + 1], pin_coef=parr[i] if pins is not None else None)
            if i == n_ops // 2:
                mid_ahead.update(eng.ahead())
            x, h = eng.sample_frame()
            fx.append(x); fh.append(h)
        x0, h0 = eng.sample_end()
    finally:
        if guided:
            if eng.train_input_grads() != grads:
                eng.set_train_input_grads(grads)
            eng.set_train_family(family)
    return x0, h0, torch.stack(fx), torch.stack(fh)


def run_case(pfa, kind, entry, batch, n_convs, env):
    from pharmacoforge_amd import synthetic
    key, _, val = env.partition("=")
    if val:
        os.environ[key] = val
    try:
        eng = pfa.PfEngine(n_convs=n_convs)
    finally:
        os.environ.pop(key, None)
    if ("sd", n_convs) not in _cache:
        _cache["sd", n_convs] = synthetic.make_state_dict(3, n_convs=n_convs)
    eng.load_state_dict(_cache["sd", n_convs])
    prot_x, prot_h, prot_ptr, pharm_ptr, com, com_f = batch_of(batch)
    if ("pp", batch) not in _cache:
        _cache["pp", batch] = eng.build_pp_edges(prot_x, prot_ptr)
    eng.set_batch(prot_x, prot_h, prot_ptr, pharm_ptr, *_cache["pp", batch])
    B, Nf, nf = int(pharm_ptr.numel() - 1), int(pharm_ptr[-1]), eng.pharm_nf
    sched = schedule_arrays(eng, kind)
    n_ops = sched[0]
    gen = torch.Generator().manual_seed(7)
    noise = torch.randn(n_ops + 1, Nf, 3 + nf, generator=gen).to(eng.device)
    pins = restraints = seed = field = types = None
    if kind.startswith("seeded"):
        from pharmacoforge_amd import schedule
        gamma = schedule.PredefinedNoiseSchedule("polynomial_2", T, PREC).gamma.detach()
        seed = (com_f + 1.5 * torch.randn(Nf, 3, generator=gen), torch.nn.functional.one_hot(torch.randint(0, nf, (Nf,), generator=gen), nf).float(),
                schedule.seed_coefficients(gamma, T, SEED_LEVEL))
    if kind == "guided_field":
        field = FIELD
    if kind == "guided_types":
        types = dict(restraints=[[(1, None, (com[g] + torch.tensor([0.5, 0.5, -1.0])).tolist(), 6.0, 1.0), (2, 0, (0.0, 0.0, 0.0), 0.0, 0.5)]
                                 if g % 2 == 0 else None for g in range(B)], scale=1.0, clip=1.0, sharpness=4.0)
    if kind == "guided_field_types":
        from pharmacoforge_amd.analysis import complementarity_tables
        match, dist = complementarity_tables()
        ph = ([3 * g for g in range(B + 1)], com.repeat_interleave(3, 0) + 3.0 * torch.randn(3 * B, 3, generator=gen), torch.randint(0, nf, (3 * B,), generator=gen))
        field = dict(FIELD, ph=ph, match=match, dist=dist, w_comp=0.25, kappa=4.0, type_sharpness=4.0)
        types = dict(scale=1.0, clip=1.0, sharpness=4.0, complementarity=True, unmatched=1.5)
    if kind in ("pinned", "pinned0", "resampled", "guided_pins"):
        flags = torch.zeros(Nf, dtype=torch.int32)
        if kind != "pinned0":
            flags[pharm_ptr[:-1]] = 3                   # the first center of every graph: position and type; the second: position
            flags[pharm_ptr[:-1][pharm_ptr[1:] - pharm_ptr[:-1] >= 2] + 1] = 1
        pins = (flags, com_f + 1.5 * torch.randn(Nf, 3, generator=gen),
                torch.nn.functional.one_hot(torch.randint(0, nf, (Nf,), generator=gen), nf).float())
    guided = kind.startswith("guided")
    if guided and field is None and types is None:
        restraints = [[("attract", 0, (com[g] + torch.tensor([1.5, -0.5, -0.5])).tolist(), 1.0, 1.0),
                       ("repel", None, (com[g] - torch.tensor([0.5, 1.5, 0.5])).tolist(), 2.0, 0.5)] if g % 2 == 0 else None for g in range(B)]
    mid, steps_sched = {}, sched
    try:
        if entry == "loop":
            kw = {k: v for k, v in (("seed", seed), ("field", field), ("types", types)) if v is not None}
            if kind == "guided_tuned":
                kw["guide_family"] = "tuned"
            if kind.endswith("multistep"):
                kw["ms_coef_arr"], sched = sched[2], (n_ops, None, None) + sched[3:]
            if pins is not None or guided:
                kw.update(pins=pins, pin_coef_arr=sched[3])
            if kind == "resampled":
                kw.update(plan=(sched[1], sched[4]))
            if guided:
                kw.update(restraints=restraints, guide_coef_arr=sched[5], guide_scale=1.5, guide_clip=0.5, energies=True)
            out = eng.sample(sched[2], n_ops, noise, init_pharm_com=com, trajectory=True, **kw)
            mid = eng.ahead()
        else:
            out = step_api(eng, kind, sched, noise, com, pins, restraints, mid, seed, field, types)
        out = tuple(out) + tuple(eng.last_eps()) + (tuple(eng.last_guidance()) if guided else ()) + ((eng.last_field_energies(),) if field else ())
        out += tuple(eng.last_type_guidance()) if types else ()
        line = f"{digest(out)} ahead {[int(v) for v in mid.values()]} family {eng.kernel_family(0)} l0_hoist {eng.l0_hoist()}"
        eng.profile_enable((1 << len(eng.KERNEL_CLASSES)) - 1)
        step_api(eng, kind, steps_sched, noise, com, pins, restraints, {}, seed, field, types)
        line += f" launches {[int(n) for _, n in eng.profile_read().values()]}"
        torch.cuda.synchronize()
        eng.sample_status()
        return line
    except pfa.PfError as e:
        return "refused: " + str(e).splitlines()[0]


def model_cases(pfa, only=None):
    """(name, line) per MODEL_CASES entry x entry point (sample; sample_given_receptor on the batch of the same graphs) x noise
    (drawn under torch.manual_seed; given)"""
    from pharmacoforge_amd import schedule, synthetic
    cut = {'pp': 3.5, 'pf': 8, 'fp': 8, 'ff': 9}
    m = pfa.PharmacophoreDiff(6, 11, pfa.analysis.ph_idx_to_type, None, n_timesteps=T, graph_config={'graph_cutoffs': cut}, precision=PREC,
                              dynamics_config=dict(vector_size=16, n_convs=2, n_hidden_scalars=128, message_norm='mean', dropout=0.1, ff_k=0,
                                                   pf_k=5, n_message_gvps=3, n_update_gvps=2, n_noise_gvps=4))
    sd = dict(synthetic.make_state_dict(3))
    sd["gamma.gamma"] = m.state_dict()["gamma.gamma"]
    m.load_state_dict(sd, strict=True)
    m = m.to("cuda").eval()
    pockets = [pfa.build_initial_complex_graph(*synthetic.synthetic_pocket(s, n), cutoffs=cut, pharm_atom_positions=torch.zeros(1, 3),
                                               pharm_atom_features=torch.zeros(1, 6)) for s, n in ((21, 12), (22, 20))]
    sizes, nf = [2, 3], 6
    gen = torch.Generator().manual_seed(11)
    coms = [p.prot_x.mean(0) for p in pockets]
    pinned = [(c[None] + torch.randn(1, 3, generator=gen), torch.tensor([r]), None) for r, c in enumerate(coms)]
    restraints = [[("attract", 0, (coms[0] + torch.tensor([1.5, -0.5, -0.5])).tolist(), 1.0, 1.0)], None]
    seeds = [(c + 1.5 * torch.randn(n, 3, generator=gen), torch.randint(0, nf, (n,), generator=gen)) for c, n in zip(coms, sizes)]
    seeded = dict(seeds=seeds, seed_level=SEED_LEVEL)
    rows = lambda top, kw: (1 if kw.get("sampler") == "multistep" else kw["sample_steps"] + 1 if "sample_steps" in kw
                            else len(schedule.resample_plan(top, JUMP, RESAMPLES)) + 1 if kw.get("pin_resamples", 1) > 1 else top + 1)
    MODEL_CASES = {
        "plain": {}, "pinned": dict(pinned=pinned), "resampled": dict(pinned=pinned, pin_resamples=RESAMPLES, pin_jump=JUMP),
        "restraints": dict(restraints=restraints, guide_scale=1.5, guide_clip=0.5),
        "restraints_pins": dict(restraints=restraints, pinned=pinned, guide_scale=1.5),
        "pocket_field": dict(pocket_field=pfa.PocketField(clash_radius=1.5)),
        "seeded": seeded, "seeded_keep": dict(seeded, seed_keep=[[0], [1, 2]]),
        "seeded_resampled": dict(seeded, seed_keep=[[0], [1, 2]], pin_resamples=RESAMPLES, pin_jump=JUMP),
        "ancestral": dict(sample_steps=MS_STEPS), "ddim": dict(sample_steps=MS_STEPS, sampler="ddim", eta=0.5),
        "multistep": dict(sample_steps=MS_STEPS, sampler="multistep"), "seeded_multistep": dict(seeded, sample_steps=MS_STEPS, sampler="multistep"),
        "guide_tuned": dict(restraints=restraints, guide_family="tuned"), "score_levels": dict(score_levels=2),
        "lanes1": dict(lanes=1, max_batch_size=1), "lanes2": dict(lanes=2, max_batch_size=1)}
    for (case, kw), entry, given in itertools.product(MODEL_CASES.items(), ("sample", "given_receptor"), (False, True)):
        name = f"model {case} {entry} {'given' if given else 'drawn'} noise"
        if (only and only not in name) or (entry == "given_receptor" and case in ("score_levels", "lanes1", "lanes2")):
            continue
        n_rows = rows(SEED_LEVEL if "seeds" in kw else T, kw)
        per_batch = [[0], [1]] if "max_batch_size" in kw else [[0, 1]]
        noise = [torch.randn(n_rows, sum(sizes[r] for r in b), 3 + nf, generator=torch.Generator().manual_seed(13 + i)) for i, b in enumerate(per_batch)]
        torch.manual_seed(3)
        try:
            if entry == "sample":
                out = [p for ps in m.sample(pockets, [[n] for n in sizes], noise=noise if given else None, **kw) for p in ps]
            else:
                kw, gs = dict(kw), list(pockets)
                for r, (x, types, _) in enumerate(kw.pop("pinned", ())):    # the pins ride on the graphs, as generate_pharmacophores.py builds them
                    gs[r] = dataclasses.replace(gs[r], pharm_pin=torch.tensor([3], dtype=torch.int32), pharm_pin_x=x,
                                                pharm_pin_h=torch.nn.functional.one_hot(types, nf).float())
                g = pfa.batch([c for p, n in zip(gs, sizes) for c in pfa.copy_graph(p, 1, pharm_feats_per_copy=torch.tensor([n]))])
                out = m.sample_given_receptor(g, init_pharm_com=torch.stack(coms), noise=noise[0] if given else None, **kw)
            score = [torch.tensor([p.score.pos, p.score.feat]) for p in out if p.score is not None]
            yield name, digest([t for p in out for t in (p.ph_coords, p.g.pharm_h0)] + score)
        except (pfa.PfError, ValueError) as e:
            yield name, "refused: " + str(e).splitlines()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--only", default=None, help="run the cases whose name contains this")
    ap.add_argument("--model", action="store_true", help="also the model-level cases, through PharmacophoreDiff.sample and sample_given_receptor")
    args = ap.parse_args()
    import pharmacoforge_amd as pfa
    torch.zeros(1, device="cuda")
    lines = ["library " + pfa._lib.load().pf_version().decode()]
    for n_convs, env, batch, kind, entry in itertools.product((1, 2, 3), ENVS, ("two", "copies", "edge"), KINDS + FRONT_KINDS, ("loop", "steps")):
        name = f"convs{n_convs} {env} {batch} {kind} {entry}"
        if (args.only and args.only not in name) or (kind in FRONT_KINDS and env not in ("default", "PFDYN_WIDE=1")) or (batch == "edge" and n_convs != 2):
            continue
        lines.append(f"{name}: {run_case(pfa, kind, entry, batch, n_convs, env)}")
        print(lines[-1], flush=True)
    for name, line in (model_cases(pfa, args.only) if args.model else ()):
        lines.append(f"{name}: {line}")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
