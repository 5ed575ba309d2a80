#!/usr/bin/env python3
"""The receding-horizon planner on the device (profiles/plan.json): time per decision, and what it finds.

  per_call   HIP-event time of one cs_plan_actions launch (the kernel of csrc/plan.h, through its op) at B envs of flight_easy:
             teams of 3 and 5, (depth, stride) = (1, 7), (4, 3) and (5, 2), discount 230, on the grid and the state that 30 steps
             of the coverage baseline leave behind; per-call time over windows of `--calls` back-to-back calls, median and
             minimum of `--reps` windows after a warm-up window.  Beside it, timed in the same run on the same state:
             `CoverageAgents.choose_action` and `BeliefAgents.choose_action` (the kernels of csrc/coverage.h and csrc/belief.h, what
             a `PlanAgents` decision runs BEFORE the planner) and the planner's torch definition on the same device over the first
             `--def-envs` envs (`--def-reps` single calls); the kernel's outputs are compared with the definition's on those envs.
  policies   one batch of B episodes on a `MovingTargetEnv`, every = 1: static targets, walkers at speeds 0.25 and 1.0, evaders
             with sense 10 at speeds 0.25 and 1.0; targets found by steps 60, 120 and 200 and the mean episode length for
             `PlanAgents` over each base, for each base alone and for `random_policy`.
usage: python tools/bench_plan.py [--out FILE] [--batch B] [--reps N] [--calls N] [--def-reps N] [--def-envs N] [--skip per_call|policies]"""
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
from cooperative_search_amd import _lib  # noqa: E402

SHAPES = ((1, 7), (4, 3), (5, 2))
DISCOUNT = 230


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
    motion = cs.TargetMotion(mode="evade", speed=1.0, sense=10.0, seed=1)
    env = make_env(n, B, motion)
    cov, bel = cs.CoverageAgents(env), cs.BeliefAgents(env)
    cpol, bpol = cov.policy(), bel.policy()
    env.reset(init=True)
    for t in range(30):
        bpol(None, env.get_state(), None, t)
        env.step(cpol(None, env.get_state(), None, t))
    state = env.get_state().clone()
    cgrid0, bgrid0, prev0 = cov.grid.clone(), bel.grid.clone(), bel.prev.clone()

    def restore_belief():
        bel.grid.copy_(bgrid0)
        bel.prev.copy_(prev0)
    c_med, c_min = event_ms(lambda: cov.choose_action(state), a.reps, a.calls, before=lambda: cov.grid.copy_(cgrid0))
    b_med, b_min = event_ms(lambda: bel.choose_action(state, 1), a.reps, a.calls, before=restore_belief)
    ops = _lib.torch_ops()
    outs = [torch.empty(B, n, dtype=torch.int64, device="cuda") for _ in range(3)]
    rows, E = [], min(a.def_envs, B)
    for depth, stride in SHAPES:
        def kernel():
            ops.plan_actions(state, cgrid0, *outs, n, cov.side, cov.view_range, depth, stride, DISCOUNT)

        def definition():
            return cs.plan_actions_torch(state[:E], cgrid0[:E], n, cov.side, cov.view_range, depth, stride, DISCOUNT, return_plans=True)
        kernel()
        equal = all(bool(torch.equal(g[:E], w)) for g, w in zip(outs, definition()))
        k_med, k_min = event_ms(kernel, a.reps, a.calls)
        d_med, d_min = event_ms(definition, a.def_reps)
        rows.append(dict(n_agents=n, B=B, depth=depth, stride=stride, discount=DISCOUNT, sequences=3 ** depth,
                         nonzero_cells_share=float((cgrid0 != 0).float().mean()), kernel_equals_definition=equal,
                         plan_kernel=dict(ms_median=k_med, ms_min=k_min), coverage_kernel=dict(ms_median=c_med, ms_min=c_min),
                         belief_kernel=dict(ms_median=b_med, ms_min=b_min), over_coverage=k_med / c_med, over_belief=k_med / b_med,
                         definition=dict(envs=E, ms_median=d_med, ms_min=d_min),
                         speedup_over_definition_per_env=(d_med / E) / (k_med / B)))
    return rows


def policy_cases(B, n=3):
    rows = []
    for mode, speed in (("walk", 0.0), ("walk", 0.25), ("walk", 1.0), ("evade", 0.25), ("evade", 1.0)):
        motion = cs.TargetMotion(mode=mode, speed=speed, sense=10.0 if mode == "evade" else 0.0, seed=1)
        env = make_env(n, B, motion, seed0=300)
        row = dict(targets="static" if speed == 0 else mode, speed=speed, every=1, sense=motion.sense, B=B, n_agents=n,
                   n_targets=int(env.target_num), depth=4, stride=3, discount=DISCOUNT)
        for name, make in (("plan_over_coverage", lambda: cs.PlanAgents(env, base="coverage").policy()),
                           ("plan_over_belief", lambda: cs.PlanAgents(env, base="belief").policy()),
                           ("coverage", lambda: cs.CoverageAgents(env).policy()), ("belief", lambda: cs.BeliefAgents(env).policy()),
                           ("random", lambda: cs.random_policy(torch.Generator(device="cuda").manual_seed(3)))):
            curve, stats = cs.collect_experiment_data(env, make(), batches=1, return_stats=True)
            m = env.target_num / 100
            row[name] = dict(found_by_step_60=float(curve[59]) * m, found_by_step_120=float(curve[119]) * m,
                             found_by_step_200=float(curve[-1]) * m, steps=stats["steps"])
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--def-reps", type=int, default=3)
    ap.add_argument("--def-envs", type=int, default=64)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: per_call, policies")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan.py needs the GPU: a CPU run says nothing about the kernel")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_plan.py: the receding-horizon planner (csrc/plan.h) on flight_easy; per_call: HIP events, kernels over "
                    f"windows of {a.calls} calls (median / minimum of {a.reps} windows after a warm-up window; the bases' grids restored "
                    f"before each), the planner's torch definition over {a.def_reps} single calls on {a.def_envs} envs, same device; "
                    "policies: one batch each, every = 1, depth 4, stride 3",
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
