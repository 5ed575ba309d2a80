#!/usr/bin/env python3
"""The forecast planner on private grids under a communication range on the device (profiles/local_forecast.json): what the two
kernels cost, what the range costs a forecasting planner, and what a student cloned from it keeps.

  kernel   B = 4096, side 50, view range 7, depth 4, stride 3, discount 230, teams of 3 and 5, on the state, the grids, prev and heard
           30 steps into a flight against evaders flown by LocalBeliefAgents at comm_range 10 (the private grids and the masks differ
           as they do in use).  cs_local_belief_forecast (moves 3, 3, 3, 3: every 1) beside cs_belief_forecast on the grid of a
           BeliefAgents shown the same flight, with the flight's own masks and with all-heard masks;
           cs_local_plan_forecast_actions at comm_range 0, 10 and unlimited beside cs_plan_forecast_actions and cs_local_plan_actions;
           the whole decision of LocalForecastAgents (three launches) beside ForecastAgents' and LocalPlanAgents(base="belief")'s.  Both kernels are compared with their definitions on the first 64
           envs before anything is timed.  `expected` is what was written down before the first run (EXPECTED).
  range    targets found of 15 by steps 60 / 120 / 200 on flight_easy, B = 1024, 3 agents, section 28's seeds: evaders (sense 10,
           every 1) at speeds 1.0 and 0.25; LocalForecastAgents, LocalPlanAgents(base="belief") and LocalBeliefAgents at comm_range
           {0, 10, 20, 35, unlimited}, beside ForecastAgents; a fresh env of the same seeds for every policy.  The unlimited row of
           LocalForecastAgents must equal ForecastAgents' row exactly: asserted before anything is written.
  distil   one distil_local_grid run per range (0 and 35) with LocalForecastAgents as expert and LocalBeliefAgents at the same range
           as filter, section 27's schedule (evaders at speed 1.0, B = 1024, 3 agents, `--iterations` x `--updates`, sample 32), the
           plain student (imitate.distil, no features) beside the private-grid student.
HIP events, windows of `--calls` calls, median and minimum of `--reps` windows after a warm-up window; one run, no profiler.
usage: python tools/bench_local_forecast.py [--out FILE] [--envs B] [--batch B] [--reps N] [--calls N] [--iterations N] [--updates N]
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
from cooperative_search_amd import local_forecast as lf  # noqa: E402
from cooperative_search_amd import localobs as lo  # noqa: E402
from bench_imitate import found, learner_setup, ms, student_policy  # noqa: E402
from bench_plan import event_ms, make_env  # noqa: E402

DEV = "cuda"
DEPTH, STRIDE, DISCOUNT = 4, 3, 230
MOVES = [3, 3, 3, 3]   # every 1: a target move before every step of every segment
RANGES = (0, 10, 20, 35, None)
EVADE = dict(mode="evade", speed=1.0, sense=10.0)

# Written before the first run; nobody has measured these kernels.
#   forecast   n times the workgroups of cs_belief_forecast, each with the same two 16 KB LDS arrays, the same 12 moves and the same
#              four level stores; an agent's list is at most the team's, so a workgroup does no more than the centralised one.  4096
#              workgroups are already many waves of the 256 CUs x 4 resident workgroups (LDS: 160 / 33 KB), so the time is taken as
#              linear in the workgroups: n x cs_belief_forecast's time MEASURED IN THE SAME RUN (section 22 has the only prior figure,
#              2.73 ms at 3 agents).  Shorter lists at a short range can only help: the allowance of a quarter covers it.
#   search     cs_plan_forecast_actions' time measured in the same run plus what is new: n stack loads of depth * cells * 4 bytes
#              per env where it does one.  The n stacks of a batch (491 MB at 3 agents) do not fit the L2 or the 256 MB of
#              MALL, so the rate taken is the 6 TB/s of section 28: 27 us per agent.  The claim replay zeroes what stage d zeroes: zero.
EXPECTED = dict(forecast_formula="n_agents * belief_forecast_ms (this run)",
                search_formula="plan_forecast_actions_ms (this run) + n_agents * 4 * B * depth * cells / load_bytes_per_s",
                load_bytes_per_s=6.0e12, prior_belief_forecast_ms_3_agents=2.73, allowance=0.25)


def name_of(comm):
    return "unlimited" if comm is None else str(comm)


def kernel_case(n, B, a):
    motion = cs.TargetMotion(seed=1, **EVADE)
    env = make_env(n, B, motion)
    flown, shared = cs.LocalBeliefAgents(env, 10), cs.BeliefAgents(env)
    fpol, spol = flown.policy(), shared.policy()
    env.reset(init=True)
    for t in range(30):
        spol(None, env.get_state(), None, t)
        env.step(fpol(None, env.get_state(), None, t))
    state = env.get_state().clone()
    side, vr, cells, m = flown.side, flown.view_range, flown.side * flown.side, flown.model
    ops = _lib.torch_ops()
    model = (m.mode, m.sense16, list(m.dx), list(m.dy), MOVES)
    stack = torch.empty(B, DEPTH, cells, dtype=torch.int32, device=DEV)
    stacks = torch.empty(B, n, DEPTH, cells, dtype=torch.int32, device=DEV)
    outs = [torch.empty(B, n, dtype=torch.int64, device=DEV) for _ in range(3)]
    # the forecast
    ops.local_belief_forecast(flown.grids, flown.prev, flown.heard, stacks, n, side, *model)
    want = lf.local_forecast_torch(flown.grids[:64], flown.prev[:64], flown.heard[:64], n, side, m, MOVES)
    if not torch.equal(stacks[:64], want):
        raise SystemExit(f"bench_local_forecast: {n} agents: cs_local_belief_forecast differs from its definition")
    central = ms(event_ms(lambda: ops.belief_forecast(shared.grid, shared.prev, stack, n, side, *model), a.reps, a.calls))
    local = ms(event_ms(lambda: ops.local_belief_forecast(flown.grids, flown.prev, flown.heard, stacks, n, side, *model), a.reps, a.calls))
    heard = int(sum(bin(int(w) & ((1 << n) - 1)).count("1") for w in flown.heard[:, :n].flatten().tolist()))
    local.update(expected_ms=n * central["ms_median"], measured_over_expected=local["ms_median"] / (n * central["ms_median"]),
                 over_belief_forecast=local["ms_median"] / central["ms_median"], mean_agents_heard=heard / (B * n))
    everyone = torch.full_like(flown.heard, -1)   # all-heard masks: every list is the whole team, what an unlimited range meets
    whole = ms(event_ms(lambda: ops.local_belief_forecast(flown.grids, flown.prev, everyone, stacks, n, side, *model), a.reps, a.calls))
    whole.update(expected_ms=n * central["ms_median"], measured_over_expected=whole["ms_median"] / (n * central["ms_median"]),
                 over_belief_forecast=whole["ms_median"] / central["ms_median"], mean_agents_heard=float(n))
    ops.local_belief_forecast(flown.grids, flown.prev, flown.heard, stacks, n, side, *model)   # the stacks the search is timed on
    # the search
    plan_fc = ms(event_ms(lambda: ops.plan_forecast_actions(state, stack, *outs, n, side, vr, DEPTH, STRIDE, DISCOUNT), a.reps, a.calls))
    load_ms = 1e3 * n * 4 * B * DEPTH * cells / EXPECTED["load_bytes_per_s"]
    expected = plan_fc["ms_median"] + load_ms
    row = dict(n_agents=n, B=B, side=side, view_range=vr, depth=DEPTH, stride=STRIDE, discount=DISCOUNT, moves=MOVES, stacks_bytes=4 * B * n * DEPTH * cells,
               belief_forecast=central, local_belief_forecast=local, local_belief_forecast_all_heard=whole, plan_forecast_actions=plan_fc, search_expected_ms=expected,
               search_expected_load_ms=load_ms, search=[])
    for comm in (0, 10, None):
        c = -1 if comm is None else comm

        def search():
            ops.local_plan_forecast_actions(state, stacks, *outs, n, side, vr, DEPTH, STRIDE, DISCOUNT, c)
        search()
        want = lf.local_plan_forecast_actions_torch(state[:64], stacks[:64], n, side, vr, DEPTH, STRIDE, DISCOUNT, c, return_plans=True)
        if not all(torch.equal(g[:64], w) for g, w in zip(outs, want)):
            raise SystemExit(f"bench_local_forecast: {n} agents, comm_range {comm}: cs_local_plan_forecast_actions differs from its definition")
        r = ms(event_ms(search, a.reps, a.calls))
        plain = ms(event_ms(lambda: ops.local_plan_actions(state, flown.grids, *outs, n, side, vr, DEPTH, STRIDE, DISCOUNT, c), a.reps, a.calls))
        r.update(comm_range=name_of(comm), measured_over_expected=r["ms_median"] / expected, over_plan_forecast_actions=r["ms_median"] / plan_fc["ms_median"],
                 local_plan_actions=plain, over_local_plan_actions=r["ms_median"] / plain["ms_median"])
        row["search"].append(r)
    # the whole decision: the base's launch, the forecast, the search (t = 30: all four segments hold three moves)
    del stack, stacks
    agents = dict(local_forecast_agents=cs.LocalForecastAgents(env, 10), forecast_agents=cs.ForecastAgents(env),
                  local_plan_agents=cs.LocalPlanAgents(env, 10, base="belief"))
    row["decision"] = {}
    for name, ag in agents.items():
        call = (lambda ag=ag: ag.choose_action(state, 1, 30)) if "forecast" in name else (lambda ag=ag: ag.choose_action(state, 1))
        row["decision"][name] = ms(event_ms(call, a.reps, a.calls, before=ag.reset))
    return row


def range_case(B, label, motion, n=3):
    seeds = np.arange(B, dtype=np.uint32) + 300

    def fly(policy_of):   # a fresh env of the same seeds for every policy: every policy meets the same episodes
        env = cs.MovingTargetEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=seeds, target_motion=motion)
        env.seed(seeds)
        return found(env, policy_of(env))
    row = dict(targets=label, n_agents=n, B=B, depth=DEPTH, stride=STRIDE, discount=DISCOUNT,
               forecast_agents=fly(lambda env: cs.ForecastAgents(env).policy()), local_forecast=[], local_plan=[], local_belief=[])
    for comm in RANGES:
        row["local_forecast"].append(dict(comm_range=name_of(comm), **fly(lambda env: cs.LocalForecastAgents(env, comm).policy())))
        row["local_plan"].append(dict(comm_range=name_of(comm), **fly(lambda env: cs.LocalPlanAgents(env, comm, base="belief").policy())))
        row["local_belief"].append(dict(comm_range=name_of(comm), **fly(lambda env: cs.LocalBeliefAgents(env, comm).policy())))
    unlimited = {k: v for k, v in row["local_forecast"][-1].items() if k != "comm_range"}
    if unlimited != row["forecast_agents"]:
        raise SystemExit(f"bench_local_forecast: {label}: the unlimited row {unlimited} is not ForecastAgents' row {row['forecast_agents']}")
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
        row = dict(comm_range=comm, expert="LocalForecastAgents", filter="LocalBeliefAgents", n_agents=n, B=a.batch,
                   n_targets=int(env.target_num), iterations=a.iterations, updates=a.updates, sample=32, lr=args.lr_actor,
                   expert_found=score(cs.LocalForecastAgents(env, comm).policy()), filter_found=score(cs.LocalBeliefAgents(env, comm).policy()),
                   random_found=score(cs.random_policy(torch.Generator(DEV).manual_seed(3))))
        # the plain student: imitate.distil (no features; the labels of the planner come through impl="rows")
        learner = im.ImitationLearner(args, device=DEV)
        agents = cs.FusedAgents(args, a.batch, net=learner.eval_rnn, seed=1)
        history = im.distil(env, cs.LocalForecastAgents(env, comm), learner, agents, im.LabelledRing(args, a.batch * a.iterations, device=DEV),
                            a.iterations, a.updates, 32, torch.Generator(DEV).manual_seed(2))
        row["plain_student"] = dict(history=history, **score(student_policy(agents)))
        del learner, agents
        # the private-grid student: features from one launch per recorded batch, the planner's labels through the rows path
        args, env = learner_setup(a.batch, n, 3, motion)
        filt = cs.LocalBeliefAgents(env, comm)
        learner = go.GridImitationLearner(args, device=DEV)
        agents = lo.LocalGridAgents(args, filt, net=learner.eval_rnn, seed=1)
        history = lo.distil_local_grid(env, cs.LocalForecastAgents(env, comm), filt, learner, agents,
                                       go.FeatureRing(args, a.batch * a.iterations, device=DEV), a.iterations, a.updates, 32,
                                       torch.Generator(DEV).manual_seed(2))
        row["private_grid_student"] = dict(history=history, **score(agents.policy()))
        del learner, agents
        yield row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_forecast.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: kernel, range, distil")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_local_forecast.py needs the GPU: a CPU run says nothing about the kernels")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_local_forecast.py: the forecast planner on private grids under a communication range (csrc/local_forecast.h, "
                    f"local_forecast.py) on flight_easy; HIP events, windows of {a.calls} calls, median / minimum of {a.reps} windows after a "
                    "warm-up window; everything in one run, no profiler attached; nothing was tuned after the first run",
               device=torch.cuda.get_device_name(0), expected_before_the_first_run=EXPECTED)
    if os.path.exists(a.out) and skip:   # a part left out keeps what an earlier run of it wrote
        with open(a.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k in skip})

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if "kernel" not in skip:
        out["kernel"] = [kernel_case(n, a.envs, a) for n in (3, 5)]
        write()
    if "range" not in skip:
        out["range"] = []
        for label, motion in (("evade_speed_1.0", cs.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=1, seed=1)),
                              ("evade_speed_0.25", cs.TargetMotion(mode="evade", speed=0.25, sense=10.0, every=1, seed=1))):
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
