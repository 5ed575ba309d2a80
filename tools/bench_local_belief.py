#!/usr/bin/env python3
"""The density filter under a communication range on the device (profiles/local_belief.json): what the kernel costs and what the
range costs where shared knowledge should matter.

  kernel  cs_local_belief_actions beside cs_belief_actions and cs_local_coverage_actions in the same process, on the same state: B =
          4096, side 50, teams of 3 and 5, walk and evade models (speed 1.0, sense 10), moved 0 and 1, comm_range 0, 10 and
          unlimited; the state is 30 steps into an episode against evaders flown by LocalBeliefAgents at comm_range 10 (the private
          grids differ as they do in use).  The kernel is compared with its definition on the first 64 envs before anything is timed.
          `expected_ms` is the sum the issue wrote down before the first run: cs_local_coverage_actions' time, plus, with moved = 1,
          n times the prediction step, taken here as cs_belief_actions(moved 1) - cs_belief_actions(moved 0) on the same state.
  range   targets found of 15 by steps 60 / 120 / 200 on flight_easy, B = 1024, teams of 3 and 5: evaders (sense 10, every 1) at
          speeds 0.5 and 1.0 and one static row; LocalBeliefAgents and LocalCoverageAgents at comm_range {0, 5, 10, 20, 35,
          unlimited}, beside BeliefAgents, CoverageAgents and random_policy; four seeds per row (a fresh env of the same seeds for every
          policy: every policy meets the same episodes), mean and spread between seeds.  The unlimited row of LocalBeliefAgents
          must equal BeliefAgents' row exactly, seed by seed: asserted before anything is written.
HIP events, windows of `--calls` calls, median and minimum of `--reps` windows after a warm-up window; one run, no profiler.
usage: python tools/bench_local_belief.py [--out FILE] [--envs B] [--batch B] [--reps N] [--calls N] [--seeds N] [--skip kernel|range]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cooperative_search_amd as cs  # noqa: E402
from cooperative_search_amd import local_belief as lb  # noqa: E402
from bench_imitate import found, ms  # noqa: E402
from bench_plan import event_ms  # noqa: E402

DEV = "cuda"
RANGES = (0, 5, 10, 20, 35, None)
KEYS = ("found_by_step_60", "found_by_step_120", "found_by_step_200")


def name_of(comm):
    return "unlimited" if comm is None else str(comm)


def make_env(n, B, motion, seed0):
    seeds = np.arange(B, dtype=np.uint32) + seed0
    return cs.MovingTargetEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=seeds, target_motion=motion), seeds


def kernel_case(n, B, a):
    flight = cs.TargetMotion(mode="evade", speed=1.0, sense=10.0, seed=1)
    env, _ = make_env(n, B, flight, 1)
    flown, shared, cover = cs.LocalBeliefAgents(env, 10), cs.BeliefAgents(env), cs.LocalCoverageAgents(env, 10)
    pols = [x.policy() for x in (flown, shared, cover)]
    env.reset(init=True)
    for t in range(30):
        state = env.get_state()
        acts = [p(None, state, None, t) for p in pols]
        env.step(acts[0])
    state = env.get_state().clone()
    grids0, prev0, heard0 = flown.grids.clone(), flown.prev.clone(), flown.heard.clone()
    grid0, sprev0, cgrids0 = shared.grid.clone(), shared.prev.clone(), cover.grids.clone()
    cells = flown.side * flown.side
    row = dict(n_agents=n, B=B, side=flown.side, view_range=flown.view_range, grid_bytes_local=B * n * 8 * cells, cases=[])

    def restore_shared():
        shared.grid.copy_(grid0)
        shared.prev.copy_(sprev0)
    for comm in (0, 10, None):
        cov = cs.LocalCoverageAgents(env, comm)
        row[f"local_coverage_actions_comm_{name_of(comm)}"] = ms(event_ms(lambda: cov.choose_action(state), a.reps, a.calls,
                                                                         before=lambda: cov.grids.copy_(cgrids0)))
    for mode in ("walk", "evade"):
        motion = cs.TargetMotion(mode=mode, speed=1.0, sense=10.0, seed=1)
        bel = cs.BeliefAgents(env, motion=motion)
        bel.grid, bel.prev = shared.grid, shared.prev
        belief = {moved: ms(event_ms(lambda: bel.choose_action(state, moved), a.reps, a.calls, before=restore_shared)) for moved in (0, 1)}
        predict_ms = belief[1]["ms_median"] - belief[0]["ms_median"]
        row[f"belief_actions_{mode}"] = dict(moved_0=belief[0], moved_1=belief[1], predict_ms=predict_ms)
        for comm in (0, 10, None):
            ag = cs.LocalBeliefAgents(env, comm, motion=motion)

            def restore():
                ag.grids.copy_(grids0)
                ag.prev.copy_(prev0)
                ag.heard.copy_(heard0)
            for moved in (0, 1):
                restore()
                want = [x[:64].clone() for x in (grids0, prev0, heard0)]
                want_a = lb.local_belief_actions_torch(state[:64], *want, n, ag.side, ag.view_range, ag.keep, ag.model, moved, ag.comm_range,
                                                       ag.lookahead)
                got_a = ag.choose_action(state, moved)
                if not (torch.equal(got_a[:64], want_a) and torch.equal(ag.grids[:64], want[0]) and torch.equal(ag.prev[:64], want[1])
                        and torch.equal(ag.heard[:64], want[2])):
                    raise SystemExit(f"bench_local_belief: {n} agents, {mode}, moved {moved}, comm_range {comm}: cs_local_belief_actions "
                                     "differs from its definition")
                r = ms(event_ms(lambda: ag.choose_action(state, moved), a.reps, a.calls, before=restore))
                base = row[f"local_coverage_actions_comm_{name_of(comm)}"]["ms_median"]
                r.update(mode=mode, moved=moved, comm_range=name_of(comm), expected_ms=base + moved * n * predict_ms)
                r["measured_over_expected"] = r["ms_median"] / r["expected_ms"]
                r["over_local_coverage_actions"] = r["ms_median"] / base
                row["cases"].append(r)
    return row


def spread(rows):
    """Per-seed dicts of KEYS -> per key the mean, the lowest and the highest seed and the sample deviation, and the seeds' values."""
    out = {}
    for k in KEYS:
        v = [r[k] for r in rows]
        out[k] = dict(mean=statistics.fmean(v), min=min(v), max=max(v), stdev=statistics.stdev(v) if len(v) > 1 else 0.0, seeds=v)
    return out


def range_case(n, B, label, motion_of, seeds_n):
    per = {}   # policy name -> [per-seed dict]

    def add(name, res):
        per.setdefault(name, []).append(res)
    for k in range(seeds_n):
        def fly(policy_of):   # a FRESH env per policy: the walk headings are keyed by the env's episode counter, which re-seeding keeps
            env, seeds = make_env(n, B, motion_of(k + 1), 300 + 1000 * k)
            env.seed(seeds)
            return found(env, policy_of(env))
        add("belief_agents", fly(lambda env: cs.BeliefAgents(env).policy()))
        add("coverage_agents", fly(lambda env: cs.CoverageAgents(env).policy()))
        add("random_policy", fly(lambda env: cs.random_policy(torch.Generator(DEV).manual_seed(3 + k))))
        for comm in RANGES:
            add(f"local_belief_{name_of(comm)}", fly(lambda env: cs.LocalBeliefAgents(env, comm).policy()))
            add(f"local_coverage_{name_of(comm)}", fly(lambda env: cs.LocalCoverageAgents(env, comm).policy()))
        if per["local_belief_unlimited"][k] != per["belief_agents"][k]:
            raise SystemExit(f"bench_local_belief: {label}, {n} agents, seed {k}: the unlimited row {per['local_belief_unlimited'][k]} is not "
                             f"BeliefAgents' row {per['belief_agents'][k]}")
    row = dict(targets=label, n_agents=n, B=B, seeds=seeds_n)
    for name in ("belief_agents", "coverage_agents", "random_policy"):
        row[name] = spread(per[name])
    for kind in ("local_belief", "local_coverage"):
        row[kind] = [dict(comm_range="unlimited" if c is None else c, **spread(per[f"{kind}_{name_of(c)}"])) for c in RANGES]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_belief.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernel, range")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_local_belief.py needs the GPU: a CPU run says nothing about the kernel")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_local_belief.py: the density filter under a communication range (csrc/local_belief.h, local_belief.py) on "
                    f"flight_easy; HIP events, windows of {a.calls} calls, median / minimum of {a.reps} windows after a warm-up window; "
                    "everything in one run, no profiler attached; nothing was tuned after the first run",
               device=torch.cuda.get_device_name(0))
    if "range" not in skip:   # first: its assertion must hold before anything is written
        settings = [("evade_speed_0.5", lambda s: cs.TargetMotion(mode="evade", speed=0.5, sense=10.0, every=1, seed=s)),
                    ("evade_speed_1.0", lambda s: cs.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=1, seed=s)),
                    ("static", lambda s: cs.TargetMotion(mode="walk", speed=0.0, seed=s))]
        out["range"] = [range_case(n, a.batch, label, motion_of, a.seeds) for label, motion_of in settings for n in (3, 5)]
    if "kernel" not in skip:
        out["kernel"] = [kernel_case(n, a.envs, a) for n in (3, 5)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
