#!/usr/bin/env python3
"""The target-density filter policy on the device (profiles/belief.json): time per decision, and what it finds.

  per_call   HIP-event time of one `BeliefAgents.choose_action` (the kernel of csrc/belief.h) at B envs of flight_easy: teams of 3
             and 5, walk and evade models, moved 0 and 1; per-call time over windows of `--calls` back-to-back calls, median and
             minimum of `--reps` windows after a warm-up window.  Beside it, timed in the same run: `CoverageAgents.choose_action`
             (the kernel of csrc/coverage.h, the thing to compare against) and the torch definition on the same device (`--def-reps`
             single calls); the kernel's outputs are compared with the definition's on the timed state.  The timed grid is the
             one a 30-step episode leaves behind, restored before every window so that every window does the same work.
  policies   one batch of B episodes on a `MovingTargetEnv`, every = 1: evade with sense 10 at speeds 0.25, 0.5 and 1.0 and walk
             at 0.5; targets found by steps 60 and 200, mean episode length and `collect_sweep_data`'s swept share for
             `BeliefAgents`, `CoverageAgents` and `random_policy`.
usage: python tools/bench_belief.py [--out FILE] [--batch B] [--reps N] [--calls N] [--def-reps N] [--skip per_call|policies]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cooperative_search_amd as cs  # noqa: E402


def event_ms(fn, reps, calls=1, before=None):
    def window():
        if before is not None:
            before()
        for _ in range(calls):
            fn()
    window()
    times = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return statistics.median(times), min(times)


def make_env(n, B, motion, seed0=1):
    return cs.MovingTargetEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=np.arange(B, dtype=np.uint32) + seed0,
                              target_motion=motion)


def per_call_cases(n, B, a):
    """The timed state: 30 steps into an episode flown by the policy itself, so that the grid holds swept ground, piled-up mass
    and zeros as it does in use."""
    rows = []
    for mode in ("walk", "evade"):
        motion = cs.TargetMotion(mode=mode, speed=1.0, sense=10.0 if mode == "evade" else 0.0, seed=1)
        env = make_env(n, B, motion)
        hip, ref, cov = cs.BeliefAgents(env), cs.BeliefAgents(env, impl="torch"), cs.CoverageAgents(env)
        pol, cpol = hip.policy(), cov.policy()
        env.reset(init=True)
        for t in range(30):
            cpol(None, env.get_state(), None, t)
            env.step(pol(None, env.get_state(), None, t))
        state = env.get_state().clone()
        grid0, prev0, cgrid0 = hip.grid.clone(), hip.prev.clone(), cov.grid.clone()

        def restore(ag):
            def f():
                ag.grid.copy_(grid0)
                ag.prev.copy_(prev0)
            return f
        c_med, c_min = event_ms(lambda: cov.choose_action(state), a.reps, a.calls, before=lambda: cov.grid.copy_(cgrid0))
        for moved in (0, 1):
            restore(hip)()
            restore(ref)()
            equal = bool(torch.equal(hip.choose_action(state, moved), ref.choose_action(state, moved)) and torch.equal(hip.grid, ref.grid)
                         and torch.equal(hip.prev, ref.prev))
            k_med, k_min = event_ms(lambda: hip.choose_action(state, moved), a.reps, a.calls, before=restore(hip))
            d_med, d_min = event_ms(lambda: ref.choose_action(state, moved), a.def_reps, before=restore(ref))
            rows.append(dict(n_agents=n, B=B, mode=mode, speed=motion.speed, sense=motion.sense, moved=moved,
                             nonzero_cells_share=float((grid0 != 0).float().mean()), kernel_equals_definition=equal,
                             belief_kernel=dict(ms_median=k_med, ms_min=k_min), coverage_kernel=dict(ms_median=c_med, ms_min=c_min),
                             definition=dict(ms_median=d_med, ms_min=d_min), over_coverage=k_med / c_med, speedup_over_definition=d_med / k_med,
                             grid_GBps=2 * 4 * hip.side * hip.side * B / (k_med * 1e-3) / 1e9))
    return rows


def policy_cases(B, n=3):
    rows = []
    for mode, speed in (("evade", 0.25), ("evade", 0.5), ("evade", 1.0), ("walk", 0.5)):
        motion = cs.TargetMotion(mode=mode, speed=speed, sense=10.0 if mode == "evade" else 0.0, seed=1)
        env = make_env(n, B, motion, seed0=300)
        col = cs.EpisodeCollector(env)
        row = dict(mode=mode, speed=speed, every=1, sense=motion.sense, B=B, n_agents=n, n_targets=int(env.target_num))
        for name, make in (("belief", lambda: cs.BeliefAgents(env).policy()), ("coverage", lambda: cs.CoverageAgents(env).policy()),
                           ("random", lambda: cs.random_policy(torch.Generator(device="cuda").manual_seed(3)))):
            curve, stats = cs.collect_experiment_data(env, make(), batches=1, return_stats=True)
            sw = cs.collect_sweep_data(col, make(), batches=1)
            m = env.target_num / 100
            row[name] = dict(found_by_step_60=float(curve[59]) * m, found_by_step_120=float(curve[119]) * m,
                             found_by_step_200=float(curve[-1]) * m, steps=stats["steps"], swept_percent_by_row_200=float(sw["curve"][-1]),
                             sweep_efficiency=sw["efficiency"])
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "belief.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--def-reps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: per_call, policies")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_belief.py needs the GPU: a CPU run says nothing about the kernel")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_belief.py: the density-filter policy (csrc/belief.h) on flight_easy; per_call: HIP events, kernels over "
                    f"windows of {a.calls} calls (median / minimum of {a.reps} windows after a warm-up window, the grid restored before "
                    f"each), the torch definition over {a.def_reps} single calls, same device; policies: one batch each, every = 1",
               device=torch.cuda.get_device_name(0))
    if "per_call" not in skip:
        out["per_call"] = [r for n in (3, 5) for r in per_call_cases(n, a.batch, a)]
    if "policies" not in skip:
        out["policies"] = policy_cases(a.batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
