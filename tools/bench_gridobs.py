#!/usr/bin/env python3
"""Grid observations on the device (profiles/gridobs.json): what the features cost and what a student that reads them keeps.

  per_decision  cs_grid_features beside cs_belief_actions and cs_coverage_actions on the same state and grids (30 steps into an
                episode against evaders), B = 4096, teams of 3 and 5.
  episodes      cs_feature_episodes with and without labels beside cs_label_episodes, on bench_imitate's recorded batches (E
                episodes of T = 200 flown by CoverageAgents, teams of 3 and 5, and flown at random, 3 agents); filters coverage
                and belief-evade (speed 1.0, sense 10).  Features and labels are compared with the definition's on a few episodes first.
  acting        one decision at B = 1024: GridAgents over a belief filter (three launches) beside FusedAgents (one) and
                ForecastAgents.
  quality       bench_imitate's quality table (static targets cloned from CoverageAgents; evaders at speed 1.0 cloned from
                ForecastAgents; same seeds, same schedule) for the plain student and, in the same run, for the grid student:
                filter CoverageAgents / BeliefAgents, GridImitationLearner, distil_grid's steps one iteration at a time.
HIP events, windows of `--calls` calls, median and minimum of `--reps` windows after a warm-up window; one run, no profiler.
usage: python tools/bench_gridobs.py [--out FILE] [--episodes E] [--batch B] [--reps N] [--calls N] [--iterations N] [--updates N]
                                     [--skip per_decision|episodes|acting|quality]"""
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
from bench_imitate import found, learner_setup, ms, quality_cases  # noqa: E402
from bench_plan import event_ms, make_env  # noqa: E402

DEV = "cuda"
EVADE = dict(mode="evade", speed=1.0, sense=10.0)


def per_decision_cases(n, B, a):
    env = make_env(n, B, cs.TargetMotion(seed=1, **EVADE))
    cov, bel = cs.CoverageAgents(env), cs.BeliefAgents(env)
    cpol, bpol = cov.policy(), bel.policy()
    env.reset(init=True)
    for t in range(30):
        bpol(None, env.get_state(), None, t)
        env.step(cpol(None, env.get_state(), None, t))
    state = env.get_state().clone()
    cgrid0, bgrid0, prev0 = cov.grid.clone(), bel.grid.clone(), bel.prev.clone()
    out = torch.empty(B, n, 16, device=DEV)

    def restore_belief():
        bel.grid.copy_(bgrid0)
        bel.prev.copy_(prev0)
    want = go.grid_features_torch(state[:64], bgrid0[:64], n, bel.side, bel.view_range)
    if not torch.equal(go.grid_features_hip(state, bgrid0, n, bel.side, bel.view_range)[:64].view(torch.int32), want.view(torch.int32)):
        raise SystemExit(f"bench_gridobs: {n} agents: cs_grid_features differs from its definition")
    return dict(n_agents=n, B=B, side=bel.side, view_range=bel.view_range,
                grid_features_on_belief_grid=ms(event_ms(lambda: go.grid_features_hip(state, bgrid0, n, bel.side, bel.view_range, out=out), a.reps, a.calls)),
                grid_features_on_coverage_grid=ms(event_ms(lambda: go.grid_features_hip(state, cgrid0, n, cov.side, cov.view_range, out=out), a.reps, a.calls)),
                belief_actions_moved=ms(event_ms(lambda: bel.choose_action(state, 1), a.reps, a.calls, before=restore_belief)),
                coverage_actions=ms(event_ms(lambda: cov.choose_action(state), a.reps, a.calls, before=lambda: cov.grid.copy_(cgrid0))))


def episode_cases(n, E, a, flown):
    env = make_env(n, E, cs.TargetMotion(mode="walk", speed=0.0), seed0=11)
    flying = cs.CoverageAgents(env).policy() if flown == "coverage" else cs.random_policy(torch.Generator(DEV).manual_seed(1))
    episode = cs.EpisodeCollector(env).generate_episodes(policy=flying, init=True)[0]
    batch = {"s": episode["s"].contiguous(), "padded": episode["padded"]}
    del episode
    T, lens = int(batch["s"].shape[1]), im.episode_lens(batch)
    rows = []
    for name, motion in (("coverage", None), ("belief_evade", cs.TargetMotion(**EVADE))):
        filt = cs.CoverageAgents(env) if motion is None else cs.BeliefAgents(env, motion=motion)
        p = im.expert_params(filt)
        feat, labels = go.feature_episodes(filt, batch, labels=True)
        want = go.feature_episodes_torch(batch["s"][:8], lens[:8], p)
        equal = (torch.equal(feat[:8].view(torch.int32), want[0].view(torch.int32)) and torch.equal(labels[:8], want[1])
                 and torch.equal(labels, im.label_episodes(filt, batch)) and torch.equal(go.feature_episodes(filt, batch).view(torch.int32), feat.view(torch.int32)))
        del feat, labels, want
        if not equal:
            raise SystemExit(f"bench_gridobs: {name}, {n} agents: cs_feature_episodes differs from its definition or from cs_label_episodes")
        row = dict(filter=name, n_agents=n, flown_by=flown, E=E, T=T, equal_to_definition_and_labeller=equal, mean_len=float(lens.float().mean()),
                   label_episodes=ms(event_ms(lambda: im.label_episodes(filt, batch), a.reps, a.calls)),
                   feature_episodes_with_labels=ms(event_ms(lambda: go.feature_episodes(filt, batch, labels=True), a.reps, a.calls)),
                   feature_episodes_without_labels=ms(event_ms(lambda: go.feature_episodes(filt, batch), a.reps, a.calls)))
        row["with_labels_over_label_episodes"] = row["feature_episodes_with_labels"]["ms_median"] / row["label_episodes"]["ms_median"]
        row["without_labels_over_label_episodes"] = row["feature_episodes_without_labels"]["ms_median"] / row["label_episodes"]["ms_median"]
        rows.append(row)
    return rows


def acting_case(a, n=3):
    args, env = learner_setup(a.batch, n, 3, cs.TargetMotion(seed=1, **EVADE))
    grid_agents = go.GridAgents(args, cs.BeliefAgents(env), seed=1)
    plain, planner = cs.FusedAgents(args, a.batch, seed=1), cs.ForecastAgents(env)
    pol = planner.policy()
    env.reset(init=True)
    for t in range(30):
        env.step(pol(None, env.get_state(), None, t))
    state, obs = env.get_state().clone(), env.get_obs().clone()
    grid_agents.filter.grid.copy_(planner.base.grid)
    return dict(n_agents=n, B=a.batch,
                grid_agents_three_launches=ms(event_ms(lambda: grid_agents.choose_action(obs, state, True, 0.0, True), a.reps, a.calls)),
                fused_agents_one_launch=ms(event_ms(lambda: plain.choose_action(obs, 0.0, True), a.reps, a.calls)),
                forecast_agents=ms(event_ms(lambda: planner.choose_action(state, 1, 30), a.reps, a.calls)))


def grid_quality_cases(a, n=3):
    """bench_imitate.quality_cases for the grid student: the same envs, seeds, schedule and scoring."""
    rows = []
    for name, motion, make, make_filter in (
            ("static", None, lambda env: cs.CoverageAgents(env), lambda env: cs.CoverageAgents(env)),
            ("evade_speed_1", cs.TargetMotion(seed=1, **EVADE), lambda env: cs.ForecastAgents(env), lambda env: cs.BeliefAgents(env))):
        args, env = learner_setup(a.batch, n, 3, motion)
        expert, filt = make(env), make_filter(env)
        own = type(expert) is type(filt)
        learner = go.GridImitationLearner(args, device=DEV)
        agents = go.GridAgents(args, filt, net=learner.eval_rnn, seed=1)
        ring = go.FeatureRing(args, a.batch * a.iterations, device=DEV)
        g = torch.Generator(DEV).manual_seed(2)
        row = dict(targets=name, expert=type(expert).__name__, filter=type(filt).__name__, n_agents=n, B=a.batch, n_targets=int(env.target_num),
                   iterations=a.iterations, updates=a.updates, sample=32, lr=args.lr_actor, expert_found=found(env, expert.policy()),
                   untrained_student_found=found(env, agents.policy()), student=[])
        for it in range(a.iterations):   # distil_grid one iteration at a time, so the student can be scored between them
            if it == 0:
                h = go.distil_grid(env, expert, filt, learner, agents, ring, 1, a.updates, 32, g)[0]
            else:
                episode, _, _, tf = cs.EpisodeCollector(env).generate_episodes(policy=agents.policy(), init=False)
                if own:
                    episode["f"], labels = go.feature_episodes(filt, episode, labels=True)
                else:
                    episode["f"], labels = go.feature_episodes(filt, episode), im.label_episodes(expert, episode)
                episode["u_expert"] = labels.unsqueeze(3).to(episode["u"].dtype)
                ring.store_episode(episode)
                del episode
                for _ in range(a.updates):
                    learner.learn(ring.sample(32, g))
                agents.sync_weights()
                h = dict(iteration=it, flown_by="student", loss=float(learner.last_stats[0]), agreement=float(learner.last_stats[1]),
                         targets_find=float(tf.double().mean()))
            row["student"].append(dict(h, **found(env, agents.policy())))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridobs.json"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: per_decision, episodes, acting, quality")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gridobs.py needs the GPU: a CPU run says nothing about the kernels")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_gridobs.py: grid observations (csrc/gridobs.h, gridobs.py) on flight_easy; HIP events, "
                    f"windows of {a.calls} calls, median / minimum of {a.reps} windows after a warm-up window; everything in one run, no "
                    "profiler attached; nothing was tuned after the first run",
               device=torch.cuda.get_device_name(0))

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
    if "acting" not in skip:
        out["acting"] = acting_case(a)
        write()
    if "quality" not in skip:
        out["quality_plain_student"] = quality_cases(a)
        write()
        out["quality_grid_student"] = grid_quality_cases(a)
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
