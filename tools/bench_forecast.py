#!/usr/bin/env python3
"""The forecast planner on the device (profiles/forecast.json): time per decision, and what it finds.

  per_call   HIP-event times of one cs_belief_forecast launch and one cs_plan_forecast_actions launch (the kernels of
             csrc/forecast.h, through their ops) at B envs of flight_easy: teams of 3 and 5, (depth, stride) = (1, 7), (4, 3) and
             (5, 2), discount 230, every = 1 (so level d is `stride` moves beyond level d - 1), on the density and the state that 30
             steps of the coverage baseline leave behind; per-call time over windows of `--calls` back-to-back calls, median and
             minimum of `--reps` windows after a warm-up window.  Beside them, timed in the same run on the same state:
             cs_plan_actions on the same density, `BeliefAgents.choose_action` and `CoverageAgents.choose_action`, and the forecast
             launch with every move count 0 (the copies alone: what is left is the depth * stride scatter passes).  The kernels'
             outputs are compared with the definitions' on the first `--def-envs` envs.
  policies   bench_plan.py's table -- one batch of B episodes on a `MovingTargetEnv`, every = 1: static targets, walkers at speeds
             0.25 and 1.0, evaders with sense 10 at speeds 0.25 and 1.0; targets found by steps 60, 120 and 200 -- with
             `ForecastAgents` (depth 4, stride 3, discount 230) added to every row.
usage: python tools/bench_forecast.py [--out FILE] [--batch B] [--reps N] [--calls N] [--def-envs N] [--skip per_call|policies]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cooperative_search_amd as cs  # noqa: E402
from cooperative_search_amd import _lib  # noqa: E402
from cooperative_search_amd import forecast as fc  # noqa: E402
from bench_plan import DISCOUNT, SHAPES, event_ms, make_env  # noqa: E402


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
    ops, m = _lib.torch_ops(), bel.model
    outs = [torch.empty(B, n, dtype=torch.int64, device="cuda") for _ in range(3)]
    plain = [torch.empty(B, n, dtype=torch.int64, device="cuda") for _ in range(3)]
    rows, E = [], min(a.def_envs, B)
    for depth, stride in SHAPES:
        moves = fc.segment_moves(30, depth, stride, 1, motion.speed)
        stack = torch.empty(B, depth, bel.side * bel.side, dtype=torch.int32, device="cuda")

        def forecast(moves=moves):
            ops.belief_forecast(bgrid0, prev0, stack, n, bel.side, m.mode, m.sense16, list(m.dx), list(m.dy), list(moves))

        def plan_forecast():
            ops.plan_forecast_actions(state, stack, *outs, n, bel.side, bel.view_range, depth, stride, DISCOUNT)

        def plan():
            ops.plan_actions(state, bgrid0, *plain, n, bel.side, bel.view_range, depth, stride, DISCOUNT)
        z_med, z_min = event_ms(lambda: forecast((0,) * depth), a.reps, a.calls)
        f_med, f_min = event_ms(forecast, a.reps, a.calls)   # (last: `stack` holds the forecast from here on)
        pf_med, pf_min = event_ms(plan_forecast, a.reps, a.calls)
        p_med, p_min = event_ms(plan, a.reps, a.calls)
        want_stack = fc.forecast_torch(bgrid0[:E], prev0[:E], n, bel.side, m, moves)
        want = fc.plan_forecast_actions_torch(state[:E], want_stack, n, bel.side, bel.view_range, depth, stride, DISCOUNT, return_plans=True)
        equal = bool(torch.equal(stack[:E], want_stack)) and all(bool(torch.equal(g[:E], w)) for g, w in zip(outs, want))
        rows.append(dict(n_agents=n, B=B, depth=depth, stride=stride, discount=DISCOUNT, moves=list(moves),
                         kernels_equal_definitions=equal, envs_compared=E,
                         forecast_kernel=dict(ms_median=f_med, ms_min=f_min), forecast_copies_only=dict(ms_median=z_med, ms_min=z_min),
                         ms_per_move=(f_med - z_med) / sum(moves), plan_forecast_kernel=dict(ms_median=pf_med, ms_min=pf_min),
                         plan_kernel=dict(ms_median=p_med, ms_min=p_min), belief_kernel=dict(ms_median=b_med, ms_min=b_min),
                         coverage_kernel=dict(ms_median=c_med, ms_min=c_min), forecast_over_plan=f_med / p_med,
                         plan_forecast_over_plan=pf_med / p_med, both_over_plan=(f_med + pf_med) / p_med,
                         decision_ms=b_med + f_med + pf_med, plain_decision_ms=b_med + p_med))
    return rows


def policy_cases(B, n=3):
    rows = []
    for mode, speed in (("walk", 0.0), ("walk", 0.25), ("walk", 1.0), ("evade", 0.25), ("evade", 1.0)):
        motion = cs.TargetMotion(mode=mode, speed=speed, sense=10.0 if mode == "evade" else 0.0, seed=1)
        env = make_env(n, B, motion, seed0=300)
        row = dict(targets="static" if speed == 0 else mode, speed=speed, every=1, sense=motion.sense, B=B, n_agents=n,
                   n_targets=int(env.target_num), depth=4, stride=3, discount=DISCOUNT)
        for name, make in (("forecast", lambda: cs.ForecastAgents(env).policy()),
                           ("plan_over_coverage", lambda: cs.PlanAgents(env, base="coverage").policy()),
                           ("plan_over_belief", lambda: cs.PlanAgents(env, base="belief").policy()),
                           ("coverage", lambda: cs.CoverageAgents(env).policy()), ("belief", lambda: cs.BeliefAgents(env).policy()),
                           ("random", lambda: cs.random_policy(torch.Generator(device="cuda").manual_seed(3)))):
            curve, stats = cs.collect_experiment_data(env, make(), batches=1, return_stats=True)
            scale = env.target_num / 100
            row[name] = dict(found_by_step_60=float(curve[59]) * scale, found_by_step_120=float(curve[119]) * scale,
                             found_by_step_200=float(curve[-1]) * scale, steps=stats["steps"])
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forecast.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--def-envs", type=int, default=64)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: per_call, policies")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_forecast.py needs the GPU: a CPU run says nothing about the kernels")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_forecast.py: the forecast planner (csrc/forecast.h) on flight_easy; per_call: HIP events, kernels over "
                    f"windows of {a.calls} calls (median / minimum of {a.reps} windows after a warm-up window; the bases' grids restored "
                    f"before each), outputs compared with the torch definitions on {a.def_envs} envs; policies: one batch each, "
                    "every = 1, depth 4, stride 3",
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
