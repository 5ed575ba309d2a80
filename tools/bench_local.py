#!/usr/bin/env python3
"""Coverage under a communication range on the device (profiles/local.json): what the kernel costs and what the range costs.

  kernel  cs_local_coverage_actions beside cs_coverage_actions in the same process, on the same state: B = 4096, teams of 3 and 5, 30
          steps into an episode flown by LocalCoverageAgents at comm_range 10 (the private grids differ as they do in use), at
          comm_range 0, 10 and unlimited.  Grid bytes = 2 * 4 * side^2 per grid (read once, written once), n grids against one.
          The kernel is compared with its definition on the first 64 envs before anything is timed.
  range   targets found of 15 by steps 60 / 120 / 200 on flight_easy with static targets, B = 1024, teams of 3 and 5, comm_range in
          {0, 5, 10, 20, 35, unlimited}, beside CoverageAgents and random_policy, one seed (the env is re-seeded before every policy:
          every policy meets the same episodes).  The unlimited row must equal CoverageAgents' row exactly: asserted before anything is
          written.
HIP events, windows of `--calls` calls, median and minimum of `--reps` windows after a warm-up window; one run, no profiler.
usage: python tools/bench_local.py [--out FILE] [--envs B] [--batch B] [--reps N] [--calls N] [--skip kernel|range]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import cooperative_search_amd as cs  # noqa: E402
from cooperative_search_amd import local as lc  # noqa: E402
from bench_imitate import found, ms  # noqa: E402
from bench_plan import event_ms  # noqa: E402

DEV = "cuda"
RANGES = (0, 5, 10, 20, 35, None)


def make_env(n, B, seed0=1):
    seeds = np.arange(B, dtype=np.uint32) + seed0
    return cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=seeds), seeds


def kernel_case(n, B, a):
    env, _ = make_env(n, B)
    cov, flown = cs.CoverageAgents(env), cs.LocalCoverageAgents(env, 10)
    cpol, lpol = cov.policy(), flown.policy()
    env.reset(init=True)
    for t in range(30):
        cpol(None, env.get_state(), None, t)
        env.step(lpol(None, env.get_state(), None, t))
    state = env.get_state().clone()
    cgrid0, grids0 = cov.grid.clone(), flown.grids.clone()
    cells = cov.side * cov.side
    row = dict(n_agents=n, B=B, side=cov.side, view_range=cov.view_range, grid_bytes_coverage=B * 8 * cells, grid_bytes_local=B * n * 8 * cells,
               coverage_actions=ms(event_ms(lambda: cov.choose_action(state), a.reps, a.calls, before=lambda: cov.grid.copy_(cgrid0))))
    for comm in (0, 10, None):
        ag = cs.LocalCoverageAgents(env, comm)
        ag.grids.copy_(grids0)
        want_g = grids0[:64].clone()
        want_a = lc.local_coverage_actions_torch(state[:64], want_g, n, ag.side, ag.view_range, ag.keep, ag.comm_range)
        got_a = ag.choose_action(state)
        if not (torch.equal(got_a[:64], want_a) and torch.equal(ag.grids[:64], want_g)):
            raise SystemExit(f"bench_local: {n} agents, comm_range {comm}: cs_local_coverage_actions differs from its definition")
        key = "unlimited" if comm is None else str(comm)
        r = ms(event_ms(lambda: ag.choose_action(state), a.reps, a.calls, before=lambda: ag.grids.copy_(grids0)))
        r["over_coverage_actions"] = r["ms_median"] / row["coverage_actions"]["ms_median"]
        r["over_n_times_coverage_actions"] = r["over_coverage_actions"] / n
        r["grid_gb_per_s"] = row["grid_bytes_local"] / (r["ms_median"] * 1e-3) / 1e9
        row[f"local_coverage_actions_comm_{key}"] = r
    row["coverage_grid_gb_per_s"] = row["grid_bytes_coverage"] / (row["coverage_actions"]["ms_median"] * 1e-3) / 1e9
    return row


def range_case(n, B):
    env, seeds = make_env(n, B, seed0=300)

    def fly(policy):
        env.seed(seeds)
        return found(env, policy)
    row = dict(n_agents=n, B=B, n_targets=int(env.target_num), coverage_agents=fly(cs.CoverageAgents(env).policy()),
               random_policy=fly(cs.random_policy(torch.Generator(DEV).manual_seed(3))), local=[])
    for comm in RANGES:
        row["local"].append(dict(comm_range="unlimited" if comm is None else comm, **fly(cs.LocalCoverageAgents(env, comm).policy())))
    if row["local"][-1] != dict(comm_range="unlimited", **row["coverage_agents"]):
        raise SystemExit(f"bench_local: {n} agents: the unlimited row {row['local'][-1]} is not CoverageAgents' row {row['coverage_agents']}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernel, range")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_local.py needs the GPU: a CPU run says nothing about the kernel")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_local.py: coverage under a communication range (csrc/local.h, local.py) on flight_easy; HIP events, "
                    f"windows of {a.calls} calls, median / minimum of {a.reps} windows after a warm-up window; everything in one run, no "
                    "profiler attached; nothing was tuned after the first run",
               device=torch.cuda.get_device_name(0))
    if "range" not in skip:   # first: its assertion must hold before anything is written
        out["range"] = [range_case(n, a.batch) for n in (3, 5)]
    if "kernel" not in skip:
        out["kernel"] = [kernel_case(n, a.envs, a) for n in (3, 5)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
