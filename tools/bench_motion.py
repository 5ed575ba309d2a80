#!/usr/bin/env python3
"""Moving targets on the device (profiles/motion.json): the move kernel's time, what the moves cost an open-loop rollout, and
what they do to the coverage and random policies.

flight_easy, 3 agents:
  kernel    (a) HIP-event time of one `motion.move_targets` call (the kernel of csrc/motion.h: per-call time over windows of
            `--calls` back-to-back calls, median and minimum of `--reps` windows after a warm-up window) beside the torch
            definition on the same device (`--def-reps` single calls), B = 4096 and 65536 envs after a reset, walk and evade;
            the kernel is checked against the definition on the same state first.  bytes = what the kernel reads and writes,
            counted from the shapes (64 + 32 n + 256 read and up to 256 written per env).
  rollout   (b) open-loop `rollout` (reset + T = 200 steps, outputs into buffers allocated once) at B = 4096: env-steps/s of
            a `MovingTargetEnv` with `every` in {1, 2, 5, 10} beside the plain env of the parent path, in the same process, the
            plain env timed before and after.
  policies  (c) `collect_experiment_data` and `collect_sweep_data`, one batch of `--batch` envs each: targets found by step 60
            and 200, swept share and sweep efficiency of `CoverageAgents` and `random_policy` at speed 0, 0.25, 0.5 and 1
            (walk) and at 0.25, 0.5 and 1 with evade, sense = 10.
usage: python tools/bench_motion.py [--out FILE] [--batch B] [--reps N] [--calls N] [--def-reps N] [--skip kernel,rollout,policies]"""
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
from cooperative_search_amd import motion as mo  # noqa: E402

N = 3


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


def make_env(B, motion=None, seed0=1):
    args = cs.make_env_args("flight_easy", n_agents=N)
    seeds = np.arange(B, dtype=np.uint32) + seed0
    if motion is None:
        return cs.BatchedFlightEnv(args, batch=B, seeds=seeds)
    return cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion)


def kernel_case(B, mode, a):
    motion = cs.TargetMotion(mode=mode, speed=0.5, persist=4, sense=10.0, seed=1)
    env = make_env(B)
    raw = env.raw()
    want = cs.move_targets_torch(raw["tgt"], raw["agent"], raw["hdr"], motion, env)
    mo.move_targets(env, motion)
    equal = bool(torch.equal(raw["tgt"].view(torch.int64), want.view(torch.int64)))
    k_med, k_min = event_ms(lambda: mo.move_targets(env, motion), a.reps, a.calls)
    d_med, d_min = event_ms(lambda: cs.move_targets_torch(raw["tgt"], raw["agent"], raw["hdr"], motion, env), a.def_reps)
    nbytes = B * (64 + 32 * N + 256 + 16 * int(env.target_num))
    return dict(B=B, mode=mode, n_agents=N, n_targets=int(env.target_num), kernel_equals_definition=equal, bytes_counted=nbytes,
                kernel=dict(ms_median=k_med, ms_min=k_min, counted_gb_per_s=nbytes / (k_med * 1e-3) / 1e9),
                definition=dict(ms_median=d_med, ms_min=d_min), speedup=d_med / k_med)


def rollout_cases(B, T, a):
    actions = torch.randint(0, 3, (T, B, N), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))

    def timed(env):
        out = env.rollout(actions)

        def call():
            env.reset()
            env.rollout(actions, out=out, update_views=False)
        med, low = event_ms(call, a.reps, max(1, a.calls // 4))
        return dict(ms_median=med, ms_min=low, env_steps_per_s=B * T / (med * 1e-3))
    rows = [dict(env="plain", **timed(make_env(B)))]
    for every in (1, 2, 5, 10):
        motion = cs.TargetMotion(mode="walk", speed=0.5, every=every, persist=4, seed=1)
        rows.append(dict(env="moving", every=every, launches_per_call=len(mo.split_runs(0, T, every)) * 2, **timed(make_env(B, motion))))
    rows.append(dict(env="plain, again", **timed(make_env(B))))
    return dict(B=B, T=T, n_agents=N, note="reset + rollout per call; a moving env makes one move launch and one rollout launch per run",
                rows=rows)


def policy_cases(B):
    specs = [("walk", s) for s in (0.0, 0.25, 0.5, 1.0)] + [("evade", s) for s in (0.25, 0.5, 1.0)]
    rows = []
    for mode, speed in specs:
        motion = cs.TargetMotion(mode=mode, speed=speed, sense=10.0 if mode == "evade" else 0.0, seed=1)
        env = make_env(B, motion, seed0=300)
        col = cs.EpisodeCollector(env)
        row = dict(mode=mode, speed=speed, every=1, sense=motion.sense, B=B)
        for name, make in (("coverage", lambda: cs.CoverageAgents(env).policy()),
                           ("random", lambda: cs.random_policy(torch.Generator(device="cuda").manual_seed(3)))):
            curve, stats = cs.collect_experiment_data(env, make(), batches=1, return_stats=True)
            sw = cs.collect_sweep_data(col, make(), batches=1)
            row[name] = dict(found_percent_by_step_60=float(curve[59]), found_percent_by_step_200=float(curve[-1]),
                             targets_find=stats["targets_find"], steps=stats["steps"], swept_percent_by_row_200=float(sw["curve"][-1]),
                             sweep_efficiency=sw["efficiency"], targets_find_swept_run=sw["targets_find"])
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--def-reps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out: kernel, rollout, policies")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion.py needs the GPU: a CPU run says nothing about the kernel")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_motion.py: moving targets (csrc/motion.h) on flight_easy, 3 agents; kernel / rollout: HIP events over "
                    f"windows of back-to-back calls (median / minimum of {a.reps} windows after a warm-up window), the torch definition "
                    f"over {a.def_reps} single calls, same device; policies: one batch each",
               device=torch.cuda.get_device_name(0))
    if "kernel" not in skip:
        out["kernel"] = [kernel_case(B, mode, a) for B in (4096, 65536) for mode in ("walk", "evade")]
    if "rollout" not in skip:
        out["rollout"] = rollout_cases(4096, 200, a)
    if "policies" not in skip:
        out["policies"] = policy_cases(a.batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
