#!/usr/bin/env python3
"""The planner on private grids under a communication range on the device (profiles/local_plan.json): what the kernel costs, what
the range costs a planner, and what a student cloned from it keeps.

  kernel   cs_local_plan_actions beside cs_plan_actions in the same process: B = 4096, side 50, view range 7, depth 4, stride 3,
           discount 230, teams of 3 and 5, comm_range 0, 10 and unlimited, on the state and the grids 30 steps into a flight against
           evaders flown by LocalBeliefAgents at comm_range 10 (the private grids differ as they do in use); cs_plan_actions reads the
           grid of a BeliefAgents shown the same flight.  The kernel is compared with its definition on the first 64 envs before
           anything is timed.  `expected_ms` is what was written down before the first run (EXPECTED).
  range    targets found of 15 by steps 60 / 120 / 200 on flight_easy, B = 1024, 3 agents: static targets and evaders (sense 10,
           every 1) at speeds 0.25 and 1.0; LocalPlanAgents(base="belief") and LocalBeliefAgents at comm_range {0, 10, 20, 35,
           unlimited}, beside PlanAgents(base="belief"); a fresh env of the same seeds for every policy.  All envs of a row fly ONE
           flight path: each figure is one path on 1024 target layouts, not a cost curve.  The unlimited row of
           LocalPlanAgents must equal PlanAgents' row exactly: asserted before anything is written.
  distil   one distil_local_grid run per range (0 and 35) with LocalPlanAgents(base="belief") as expert and LocalBeliefAgents at the
           same range as filter, section 27's schedule (evaders at speed 1.0, B = 1024, 3 agents, `--iterations` x `--updates`, sample
           32), the plain student (imitate.distil, no features) beside the private-grid student.
HIP events, windows of `--calls` calls, median and minimum of `--reps` windows after a warm-up window; one run, no profiler.
usage: python tools/bench_local_plan.py [--out FILE] [--envs B] [--batch B] [--reps N] [--calls N] [--iterations N] [--updates N]
                                        [--skip kernel|range|distil]"""
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
from cooperative_search_amd import _lib  # noqa: E402
from cooperative_search_amd import gridobs as go  # noqa: E402
from cooperative_search_amd import imitate as im  # noqa: E402
from cooperative_search_amd import local_plan as lp  # noqa: E402
from cooperative_search_amd import localobs as lo  # noqa: E402
from bench_imitate import found, learner_setup, ms, student_policy  # noqa: E402
from bench_plan import event_ms, make_env  # noqa: E402

DEV = "cuda"
DEPTH, STRIDE, DISCOUNT = 4, 3, 230
RANGES = (0, 10, 20, 35, None)
EVADE = dict(mode="evade", speed=1.0, sense=10.0)

# Written before the first run; nobody has measured this kernel.  The search -- 120 nodes, their gains, 81 scores per agent -- is
# cs_plan_actions' own, stage for stage, and runs at its occupancy (eight workgroups per CU, 63 VGPRs); so the expectation is
# cs_plan_actions' time MEASURED IN THE SAME RUN (section 21 has the only prior figure, 0.54 ms at 3 agents) plus what is new: n
# clamped grid loads per env where cs_plan_actions does one.  A load is 4 B cells bytes (41 MB at B = 4096, side 50); the n grids
# of a batch (123 and 205 MB) do not fit the 32 MB of L2, so the rate taken is the 6 TB/s the chip streams at: 6.8 us per grid,
# 20 us with 3 agents and 34 us with 5.  The claim passes cost what cs_plan_actions' stage d costs at an unlimited range with 3
# agents (3 D discs either way), less at a finite range, 5 D more with 5 agents (a disc is one pass of 256 threads): taken as zero.
# The tree is walked once per agent in both kernels: zero.  A quarter either way is the allowance (section 26).
EXPECTED = dict(formula="plan_actions_ms (this run) + n_agents * 4 * B * cells / load_bytes_per_s", load_bytes_per_s=6.0e12,
                extra_tree_or_claim_ms=0.0, prior_plan_actions_ms_3_agents=0.54, allowance=0.25)


def name_of(comm):
    return "unlimited" if comm is None else str(comm)


def kernel_case(n, B, a):
    env = make_env(n, B, cs.TargetMotion(seed=1, **EVADE))
    flown, shared = cs.LocalBeliefAgents(env, 10), cs.BeliefAgents(env)
    fpol, spol = flown.policy(), shared.policy()
    env.reset(init=True)
    for t in range(30):
        spol(None, env.get_state(), None, t)
        env.step(fpol(None, env.get_state(), None, t))
    state, grids, grid = env.get_state().clone(), flown.grids.clone(), shared.grid.clone()
    side, vr, cells = flown.side, flown.view_range, flown.side * flown.side
    ops = _lib.torch_ops()
    outs = [torch.empty(B, n, dtype=torch.int64, device=DEV) for _ in range(3)]
    plan = ms(event_ms(lambda: ops.plan_actions(state, grid, *outs, n, side, vr, DEPTH, STRIDE, DISCOUNT), a.reps, a.calls))
    load_ms = 1e3 * n * 4 * B * cells / EXPECTED["load_bytes_per_s"]
    row = dict(n_agents=n, B=B, side=side, view_range=vr, depth=DEPTH, stride=STRIDE, discount=DISCOUNT, grid_bytes_local=4 * B * n * cells,
               grid_bytes_shared=4 * B * cells, envs_whose_agents_hold_different_grids=int((grids[:, 0] != grids[:, 1]).any(1).sum()),
               plan_actions=plan, expected_ms=plan["ms_median"] + load_ms, expected_load_ms=load_ms, cases=[])
    for comm in (0, 10, None):
        c = -1 if comm is None else comm

        def kernel():
            ops.local_plan_actions(state, grids, *outs, n, side, vr, DEPTH, STRIDE, DISCOUNT, c)
        kernel()
        want = lp.local_plan_actions_torch(state[:64], grids[:64], n, side, vr, DEPTH, STRIDE, DISCOUNT, c, return_plans=True)
        if not all(torch.equal(g[:64], w) for g, w in zip(outs, want)) or not torch.equal(grids, flown.grids):
            raise SystemExit(f"bench_local_plan: {n} agents, comm_range {comm}: cs_local_plan_actions differs from its definition")
        r = ms(event_ms(kernel, a.reps, a.calls))
        r.update(comm_range=name_of(comm), measured_over_expected=r["ms_median"] / row["expected_ms"],
                 over_plan_actions=r["ms_median"] / plan["ms_median"])
        row["cases"].append(r)
    return row


def range_case(B, label, motion, n=3):
    seeds = np.arange(B, dtype=np.uint32) + 300

    def fly(policy_of):   # a fresh env of the same seeds for every policy: every policy meets the same episodes
        env = cs.MovingTargetEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=seeds, target_motion=motion)
        env.seed(seeds)
        return found(env, policy_of(env))
    row = dict(targets=label, n_agents=n, B=B, depth=DEPTH, stride=STRIDE, discount=DISCOUNT,
               plan_agents=fly(lambda env: cs.PlanAgents(env, base="belief").policy()),
               belief_agents=fly(lambda env: cs.BeliefAgents(env).policy()), local_plan=[], local_belief=[])
    for comm in RANGES:
        row["local_plan"].append(dict(comm_range=name_of(comm), **fly(lambda env: cs.LocalPlanAgents(env, comm, base="belief").policy())))
        row["local_belief"].append(dict(comm_range=name_of(comm), **fly(lambda env: cs.LocalBeliefAgents(env, comm).policy())))
    unlimited = {k: v for k, v in row["local_plan"][-1].items() if k != "comm_range"}
    if unlimited != row["plan_agents"]:
        raise SystemExit(f"bench_local_plan: {label}: the unlimited row {unlimited} is not PlanAgents' row {row['plan_agents']}")
    return row


def distil_cases(a, n=3):
    for comm in (0, 35):
        motion = cs.TargetMotion(seed=1, **EVADE)
        seeds = np.arange(a.batch, dtype=np.uint32) + 900

        def score(policy):   # a fresh env of the same seeds for every scored policy
            fresh = cs.MovingTargetEnv(cs.make_env_args("flight_easy", n_agents=n), batch=a.batch, seeds=seeds, target_motion=motion)
            fresh.seed(seeds)
            return found(fresh, policy)
        args, env = learner_setup(a.batch, n, 3, motion)
        row = dict(comm_range=comm, expert="LocalPlanAgents(base='belief')", filter="LocalBeliefAgents", n_agents=n, B=a.batch,
                   n_targets=int(env.target_num), iterations=a.iterations, updates=a.updates, sample=32, lr=args.lr_actor,
                   expert_found=score(cs.LocalPlanAgents(env, comm, base="belief").policy()),
                   filter_found=score(cs.LocalBeliefAgents(env, comm).policy()),
                   random_found=score(cs.random_policy(torch.Generator(DEV).manual_seed(3))))
        # the plain student: imitate.distil (no features; the labels of the planner come through impl="rows")
        learner = im.ImitationLearner(args, device=DEV)
        agents = cs.FusedAgents(args, a.batch, net=learner.eval_rnn, seed=1)
        history = im.distil(env, cs.LocalPlanAgents(env, comm, base="belief"), learner, agents,
                            im.LabelledRing(args, a.batch * a.iterations, device=DEV), a.iterations, a.updates, 32, torch.Generator(DEV).manual_seed(2))
        row["plain_student"] = dict(history=history, **score(student_policy(agents)))
        del learner, agents
        # the private-grid student: features from one launch per recorded batch, the planner's labels through the rows path
        args, env = learner_setup(a.batch, n, 3, motion)
        filt = cs.LocalBeliefAgents(env, comm)
        learner = go.GridImitationLearner(args, device=DEV)
        agents = lo.LocalGridAgents(args, filt, net=learner.eval_rnn, seed=1)
        history = lo.distil_local_grid(env, cs.LocalPlanAgents(env, comm, base="belief"), filt, learner, agents,
                                       go.FeatureRing(args, a.batch * a.iterations, device=DEV), a.iterations, a.updates, 32,
                                       torch.Generator(DEV).manual_seed(2))
        row["private_grid_student"] = dict(history=history, **score(agents.policy()))
        del learner, agents
        yield row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_plan.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernel, range, distil")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_local_plan.py needs the GPU: a CPU run says nothing about the kernel")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_local_plan.py: the planner on private grids under a communication range (csrc/local_plan.h, local_plan.py) "
                    f"on flight_easy; HIP events, windows of {a.calls} calls, median / minimum of {a.reps} windows after a warm-up window; "
                    "everything in one run, no profiler attached; nothing was tuned after the first run",
               device=torch.cuda.get_device_name(0), expected_before_the_first_run=EXPECTED)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if "kernel" not in skip:
        out["kernel"] = [kernel_case(n, a.envs, a) for n in (3, 5)]
        write()
    if "range" not in skip:
        out["range"] = []
        for label, motion in (("static", cs.TargetMotion(mode="walk", speed=0.0, seed=1)),
                              ("evade_speed_0.25", cs.TargetMotion(mode="evade", speed=0.25, sense=10.0, every=1, seed=1)),
                              ("evade_speed_1.0", cs.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=1, seed=1))):
            out["range"].append(range_case(a.batch, label, motion))
            write()
    if "distil" not in skip:
        out["distil"] = []
        for row in distil_cases(a):
            out["distil"].append(row)
            write()
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
