#!/usr/bin/env python3
"""The coverage baseline on the device (profiles/coverage.json): time per decision, closed-loop rate, found curves.

flight_easy, B = 4096 envs, teams of 3 and 5:
  per_call      HIP-event time of one `CoverageAgents.choose_action` (the kernel of csrc/coverage.h: per-call time over windows of
                `--calls` back-to-back calls, median and minimum of `--reps` windows after a warm-up window) beside the torch
                definition on the same device (`--def-reps` single calls); grid_GBps = 2 * 4 * side^2 * B bytes (the belief grid
                read once and written once) / median time -- the figure to hold against the write stream of
                profiles/r06_write_bw.log;
  closed_loop   env-steps per second of `EpisodeCollector.generate_episodes(policy=...)` (B * time_limit steps per call, wall
                clock around a synchronised call, best of `--loop-reps`) with the coverage policy and with `random_policy`;
  curves        `collect_experiment_data`, one batch: percent of targets found by step t, coverage beside random.
usage: python tools/bench_coverage.py [--out FILE] [--batch B] [--reps N] [--calls N] [--def-reps N] [--loop-reps N]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cooperative_search_amd as cs  # noqa: E402


def event_ms(fn, reps, calls=1):
    for _ in range(calls):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / calls)
    return statistics.median(times), min(times)


def loop_rate(env, policy, reps):
    col = cs.EpisodeCollector(env)
    best = None
    for _ in range(reps + 1):   # the first call warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col.generate_episodes(policy=policy, init=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return env.batch * env.time_limit / best, best


def case(n, B, a):
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=np.arange(B, dtype=np.uint32) + 1)
    env.reset(init=True)
    state = env.get_state().clone()
    hip, ref = cs.CoverageAgents(env), cs.CoverageAgents(env, impl="torch")
    equal = bool(torch.equal(hip.choose_action(state), ref.choose_action(state)) and torch.equal(hip.grid, ref.grid))
    k_med, k_min = event_ms(lambda: hip.choose_action(state), a.reps, a.calls)
    d_med, d_min = event_ms(lambda: ref.choose_action(state), a.def_reps)
    grid_bytes = 2 * 4 * hip.side * hip.side * B
    rnd = cs.random_policy(torch.Generator(device="cuda").manual_seed(7))
    cov_rate, cov_s = loop_rate(env, hip.policy(), a.loop_reps)
    rnd_rate, rnd_s = loop_rate(env, rnd, a.loop_reps)
    cov_curve, cov_stats = cs.collect_experiment_data(env, hip.policy(), batches=1, return_stats=True)
    rnd_curve, rnd_stats = cs.collect_experiment_data(env, rnd, batches=1, return_stats=True)
    m = env.target_num
    return dict(n_agents=n, B=B, side=hip.side, view_range=hip.view_range, keep=hip.keep, regrow=hip.regrow, lookahead=hip.lookahead,
                kernel_equals_definition=equal, grid_bytes_per_call=grid_bytes,
                per_call=dict(kernel=dict(ms_median=k_med, ms_min=k_min, grid_GBps=grid_bytes / (k_med * 1e-3) / 1e9),
                              definition=dict(ms_median=d_med, ms_min=d_min), speedup=d_med / k_med),
                closed_loop=dict(steps_per_call=B * env.time_limit,
                                 coverage=dict(env_steps_per_s=cov_rate, seconds=cov_s), random=dict(env_steps_per_s=rnd_rate, seconds=rnd_s)),
                curves=dict(unit="percent of the targets found by step t + 1", n_targets=m,
                            coverage=[round(float(v), 3) for v in cov_curve], random=[round(float(v), 3) for v in rnd_curve],
                            found_by_step_60=dict(coverage=float(cov_curve[59]) * m / 100, random=float(rnd_curve[59]) * m / 100),
                            found_by_step_200=dict(coverage=float(cov_curve[-1]) * m / 100, random=float(rnd_curve[-1]) * m / 100),
                            stats=dict(coverage=cov_stats, random=rnd_stats)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--def-reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coverage.py needs the GPU: a CPU run says nothing about the kernel")
    out = dict(_doc="tools/bench_coverage.py: the coverage baseline (csrc/coverage.h) on flight_easy; per_call: HIP events, kernel over "
                    f"windows of {a.calls} calls (median / minimum of {a.reps} windows), the torch definition over {a.def_reps} single "
                    "calls, same device; closed_loop: wall clock of a synchronised generate_episodes call, best of "
                    f"{a.loop_reps}; curves: collect_experiment_data, one batch",
               device=torch.cuda.get_device_name(0), cases=[case(n, a.batch, a) for n in (3, 5)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    brief = [{k: c[k] for k in ("n_agents", "per_call", "closed_loop")} | {"found": {k: c["curves"][k] for k in ("found_by_step_60", "found_by_step_200")}}
             for c in out["cases"]]
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
