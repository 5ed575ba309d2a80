#!/usr/bin/env python3
"""Private-grid observations on the device (profiles/localobs.json): what the two kernels cost and what a student that reads its own
grid keeps under a communication range.

  per_decision  cs_local_grid_features beside cs_grid_features, B = 4096, teams of 3 and 5, on the state and the grids 30 steps into an
                episode against evaders flown by LocalBeliefAgents at comm_range 10 (the private grids differ as they do in use);
                cs_grid_features reads a BeliefAgents grid of the same flight.
  episodes      cs_local_feature_episodes with and without labels on bench_gridobs' recorded batches (E episodes of T = 200 flown by
                CoverageAgents, teams of 3 and 5: they end early; and flown at random, 3 agents: nearly full length), filters
                LocalCoverageAgents and LocalBeliefAgents (evade, speed 1.0, sense 10) at comm_range 10, beside (a) the parent's way,
                imitate.label_episodes(expert, batch, impl="rows"), and (b) T launches of the step kernel plus T launches of
                cs_local_grid_features.
  quality       flight_easy, evaders at speed 1.0, sense 10, B = 1024, 3 agents, LocalBeliefAgents at comm_range 0, 10 and 35 as expert
                AND filter: targets found of 15 by steps 60 / 120 / 200 for the expert, random_policy, the plain student
                (imitate.distil, no features) and the private-grid student (distil_local_grid); section 24's schedule; a fresh env of the
                same seeds for every scored policy, as bench_local_belief does.  All envs of a row fly ONE path:
                these are single flight paths, not a cost curve.
EXPECTED holds what was written down BEFORE the first run: the per-decision times outright, the per-batch
times as a formula over components measured in the same run.  Every kernel is compared with its definition on 64 envs / episodes
before it is timed.  HIP events, windows of `--calls` calls (2 for the T-launch paths), median and minimum of `--reps` windows after a
warm-up window; one run, no profiler.
usage: python tools/bench_localobs.py [--out FILE] [--envs B] [--episodes E] [--batch B] [--reps N] [--calls N] [--iterations N]
                                      [--updates N] [--skip per_decision|episodes|quality]"""
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
from cooperative_search_amd import gridobs as go  # noqa: E402
from cooperative_search_amd import imitate as im  # noqa: E402
from cooperative_search_amd import localobs as lo  # noqa: E402
from bench_imitate import found, learner_setup, ms, student_policy  # noqa: E402
from bench_plan import event_ms, make_env  # noqa: E402

DEV = "cuda"
EVADE = dict(mode="evade", speed=1.0, sense=10.0)
COMM = 10

# Written before the first run.  per_decision_us: cs_grid_features took 65.8 / 96.0 us (section 24); the probe work is identical, the
# grids are n times the bytes but a probe reads its footprint only, so 1.0 to 1.3 times that, the point in the middle.  per_batch: the
# walk does per live row what the step kernel and cs_local_grid_features do per call, so mean_len * (step_ms + feature_ms), both
# measured in this run at the same E; without labels the choose stage (about a third of the coverage step, a twentieth of a moved belief
# step) is saved, which the formula ignores.  The one launch should beat (a) and (b) by about T / mean_len on a batch that ends early
# and roughly tie on a full-length one (section 23's pattern).  A quarter either way is the allowance (section 26).
EXPECTED = dict(per_decision_us={3: 78.0, 5: 115.0}, per_decision_over_grid_features=(1.0, 1.3),
                per_batch_ms="mean_len * (step_kernel_ms + local_grid_features_ms)", allowance=0.25)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def per_decision_cases(n, B, a):
    env = make_env(n, B, cs.TargetMotion(seed=1, **EVADE))
    flown, shared = cs.LocalBeliefAgents(env, COMM), cs.BeliefAgents(env)
    fpol, spol = flown.policy(), shared.policy()
    env.reset(init=True)
    for t in range(30):
        spol(None, env.get_state(), None, t)
        env.step(fpol(None, env.get_state(), None, t))
    state, grids, grid = env.get_state().clone(), flown.grids.clone(), shared.grid.clone()
    side, vr = flown.side, flown.view_range
    out = torch.empty(B, n, 16, device=DEV)
    want = lo.local_grid_features_torch(state[:64], grids[:64], n, side, vr)
    if not bits_equal(lo.local_grid_features_hip(state, grids, n, side, vr)[:64], want):
        raise SystemExit(f"bench_localobs: {n} agents: cs_local_grid_features differs from its definition")
    row = dict(n_agents=n, B=B, side=side, view_range=vr, grid_bytes_local=4 * B * n * side * side, grid_bytes_shared=4 * B * side * side,
               envs_whose_agents_hold_different_grids=int((grids[:, 0] != grids[:, 1]).any(1).sum()),
               local_grid_features=ms(event_ms(lambda: lo.local_grid_features_hip(state, grids, n, side, vr, out=out), a.reps, a.calls)),
               grid_features=ms(event_ms(lambda: go.grid_features_hip(state, grid, n, side, vr, out=out), a.reps, a.calls)),
               expected_us=EXPECTED["per_decision_us"][n])
    row["over_grid_features"] = row["local_grid_features"]["ms_median"] / row["grid_features"]["ms_median"]
    row["measured_over_expected"] = 1e3 * row["local_grid_features"]["ms_median"] / row["expected_us"]
    return row


def episode_cases(n, E, a, flown):
    env = make_env(n, E, cs.TargetMotion(mode="walk", speed=0.0), seed0=11)
    flying = cs.CoverageAgents(env).policy() if flown == "coverage" else cs.random_policy(torch.Generator(DEV).manual_seed(1))
    episode = cs.EpisodeCollector(env).generate_episodes(policy=flying, init=True)[0]
    batch = {"s": episode["s"].contiguous(), "padded": episode["padded"]}
    del episode
    T, lens = int(batch["s"].shape[1]), im.episode_lens(batch)
    st = batch["s"].transpose(0, 1).contiguous()   # the rows step-major, laid out once outside the timing
    few = max(1, a.calls // 10)
    rows = []
    for name in ("local_coverage", "local_belief_evade"):
        filt = cs.LocalCoverageAgents(env, COMM) if name == "local_coverage" else cs.LocalBeliefAgents(env, COMM, motion=cs.TargetMotion(**EVADE))
        p = lo.local_expert_params(filt)
        feat, labels = lo.local_feature_episodes(filt, batch, labels=True)
        want = lo.local_feature_episodes_torch(batch["s"][:64], lens[:64], p)
        equal = (bits_equal(feat[:64], want[0]) and torch.equal(labels[:64], want[1]) and bits_equal(lo.local_feature_episodes(filt, batch), feat)
                 and torch.equal(labels, im.label_episodes(filt, batch, impl="rows")))
        del feat, labels, want
        if not equal:
            raise SystemExit(f"bench_localobs: {name}, {n} agents: cs_local_feature_episodes differs from its definition or from the rows path")
        policy, out = filt.policy(), torch.empty(E, n, 16, device=DEV)

        def steps_only():
            for t in range(T):
                policy(None, st[t], None, t)

        def steps_and_features():
            for t in range(T):
                policy(None, st[t], None, t)
                lo.local_grid_features_hip(st[t], filt.grids, n, filt.side, filt.view_range, out=out)
        step = event_ms(steps_only, a.reps, few)
        both = event_ms(steps_and_features, a.reps, few)
        row = dict(filter=name, comm_range=COMM, n_agents=n, flown_by=flown, E=E, T=T, equal_to_definition_and_rows_path=equal,
                   mean_len=float(lens.float().mean()), episodes_ended_early=int((lens < T).sum()),
                   one_launch_with_labels=ms(event_ms(lambda: lo.local_feature_episodes(filt, batch, labels=True), a.reps, a.calls)),
                   one_launch_without_labels=ms(event_ms(lambda: lo.local_feature_episodes(filt, batch), a.reps, a.calls)),
                   a_rows_path_labels_only=ms(event_ms(lambda: im.label_episodes(filt, batch, impl="rows"), a.reps, few)),
                   b_step_and_feature_launches=ms(both), step_launches_only=ms(step))
        row["step_kernel_ms"] = step[0] / T
        row["local_grid_features_ms"] = (both[0] - step[0]) / T
        row["expected_ms"] = row["mean_len"] * (row["step_kernel_ms"] + row["local_grid_features_ms"])
        one = row["one_launch_with_labels"]["ms_median"]
        row["measured_over_expected"] = one / row["expected_ms"]
        row["a_over_one_launch"] = row["a_rows_path_labels_only"]["ms_median"] / one
        row["b_over_one_launch"] = row["b_step_and_feature_launches"]["ms_median"] / one
        row["without_labels_over_with"] = row["one_launch_without_labels"]["ms_median"] / one
        row["one_launch_us_per_live_row"] = 1e3 * one / row["mean_len"]
        rows.append(row)
    return rows


def quality_cases(a, n=3):
    for comm in (0, 10, 35):
        motion = cs.TargetMotion(seed=1, **EVADE)
        args, env = learner_setup(a.batch, n, 3, motion)
        seeds = np.arange(a.batch, dtype=np.uint32) + 900

        def score(policy):   # a fresh env of the same seeds for every scored policy
            fresh = cs.MovingTargetEnv(cs.make_env_args("flight_easy", n_agents=n), batch=a.batch, seeds=seeds, target_motion=motion)
            fresh.seed(seeds)
            return found(fresh, policy)
        expert = filt = cs.LocalBeliefAgents(env, comm)
        row = dict(comm_range=comm, expert="LocalBeliefAgents", n_agents=n, B=a.batch, n_targets=int(env.target_num), iterations=a.iterations,
                   updates=a.updates, sample=32, lr=args.lr_actor, expert_found=score(cs.LocalBeliefAgents(env, comm).policy()),
                   random_found=score(cs.random_policy(torch.Generator(DEV).manual_seed(3))))
        # the plain student: imitate.distil (no features; the labels of a local expert come through impl="rows")
        learner = im.ImitationLearner(args, device=DEV)
        agents = cs.FusedAgents(args, a.batch, net=learner.eval_rnn, seed=1)
        history = im.distil(env, expert, learner, agents, im.LabelledRing(args, a.batch * a.iterations, device=DEV), a.iterations, a.updates, 32,
                            torch.Generator(DEV).manual_seed(2))
        row["plain_student"] = dict(history=history, **score(student_policy(agents)))
        del learner, agents
        # the private-grid student: distil_local_grid, features and labels from one launch per recorded batch
        args, env = learner_setup(a.batch, n, 3, motion)
        expert = filt = cs.LocalBeliefAgents(env, comm)
        learner = go.GridImitationLearner(args, device=DEV)
        agents = lo.LocalGridAgents(args, filt, net=learner.eval_rnn, seed=1)
        history = lo.distil_local_grid(env, expert, filt, learner, agents, go.FeatureRing(args, a.batch * a.iterations, device=DEV), a.iterations,
                                       a.updates, 32, torch.Generator(DEV).manual_seed(2))
        row["private_grid_student"] = dict(history=history, **score(agents.policy()))
        del learner, agents
        yield row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localobs.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: per_decision, episodes, quality")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_localobs.py needs the GPU: a CPU run says nothing about the kernels")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_localobs.py: private-grid observations (csrc/localobs.h, localobs.py) on flight_easy; HIP events, "
                    f"windows of {a.calls} calls ({max(1, a.calls // 10)} for the T-launch paths), median / minimum of {a.reps} windows after a "
                    "warm-up window; everything in one run, no profiler attached; nothing was tuned after the first run",
               device=torch.cuda.get_device_name(0), expected_before_the_first_run=EXPECTED)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if "per_decision" not in skip:
        out["per_decision"] = [per_decision_cases(n, a.envs, a) for n in (3, 5)]
        write()
    if "episodes" not in skip:
        out["episodes"] = []
        for n, flown in ((3, "coverage"), (5, "coverage"), (3, "random")):
            out["episodes"] += episode_cases(n, a.episodes, a, flown)
            write()
    if "quality" not in skip:
        out["quality"] = []
        for row in quality_cases(a):
            out["quality"].append(row)
            write()
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
