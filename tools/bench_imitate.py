#!/usr/bin/env python3
"""Imitation learning on the device (profiles/imitate.json): what relabelling costs, what the loss costs, what a student keeps.

  labelling  one cs_label_episodes launch (csrc/label.h) against the `rows` path of imitate.label_episodes (T launches of the
             per-step kernel, with the torch glue that path needs) and against those T launches alone, on the same recorded batch:
             E episodes of T = 200 flown by CoverageAgents on flight_easy, teams of 3 and 5 (most end early), and flown at random,
             3 agents (nearly all run to T); experts coverage, belief-walk
             (speed 1.0) and belief-evade (speed 1.0, sense 10).  Labels and final grids of the two paths are compared first.
             HIP events, windows of `--calls` calls, median and minimum of `--reps` windows after a warm-up window.
  loss       cs_bc_loss (forward, through BCLoss) against bc_loss_torch (forward), and a whole ImitationLearner.learn call fused
             against torch, at E = 32, T = 200, 3 agents, same protocol.
  quality    imitate.distil on static targets (expert CoverageAgents) and on evaders at speed 1.0, sense 10 (expert ForecastAgents),
             3 agents: targets found by steps 60, 120 and 200 (collect_experiment_data, one batch) for the student after every
             iteration, for its expert and for random_policy; loss and agreement per iteration; each side's time per decision.
usage: python tools/bench_imitate.py [--out FILE] [--episodes E] [--batch B] [--reps N] [--calls N] [--iterations N] [--updates N]
                                     [--skip labelling|loss|quality]"""
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
from cooperative_search_amd import imitate as im  # noqa: E402
from bench_plan import event_ms, make_env  # noqa: E402

DEV = "cuda"


def ms(pair):
    return dict(ms_median=pair[0], ms_min=pair[1])


def labelling_cases(n, E, a, flown="coverage"):
    env = make_env(n, E, cs.TargetMotion(mode="walk", speed=0.0), seed0=11)
    flying = cs.CoverageAgents(env).policy() if flown == "coverage" else cs.random_policy(torch.Generator(DEV).manual_seed(1))
    episode = cs.EpisodeCollector(env).generate_episodes(policy=flying, init=True)[0]
    batch = {"s": episode["s"].contiguous(), "padded": episode["padded"]}
    del episode
    T, lens = int(batch["s"].shape[1]), im.episode_lens(batch)
    st = batch["s"].transpose(0, 1).contiguous()
    rows = []
    for name, motion in (("coverage", None), ("belief_walk", cs.TargetMotion(mode="walk", speed=1.0)),
                         ("belief_evade", cs.TargetMotion(mode="evade", speed=1.0, sense=10.0))):
        expert = cs.CoverageAgents(env) if motion is None else cs.BeliefAgents(env, motion=motion)
        one = im.label_episodes(expert, batch, return_state=True)
        per_row = im.label_episodes(expert, batch, impl="rows", return_state=True)
        equal = all(bool(torch.equal(x, y)) for x, y in zip(one, per_row))
        del one, per_row
        if not equal:
            raise SystemExit(f"bench_imitate: {name}, {n} agents: the one-launch labels or grids differ from the rows path's")
        policy = expert.policy()

        def launches_only():   # (st: the rows step-major, laid out once outside the timing -- the launches and nothing else)
            for t in range(T):
                policy(None, st[t], None, t)
        row = dict(expert=name, n_agents=n, flown_by=flown, E=E, T=T, side=int(env.map_size), labels_and_grids_equal=equal,
                   episodes_ended_early=int((lens < T).sum()), mean_len=float(lens.float().mean()),
                   one_launch=ms(event_ms(lambda: im.label_episodes(expert, batch), a.reps, a.calls)),
                   rows_path=ms(event_ms(lambda: im.label_episodes(expert, batch, impl="rows"), a.reps, max(1, a.calls // 10))),
                   per_step_launches_only=ms(event_ms(launches_only, a.reps, max(1, a.calls // 10))))
        row["rows_path_over_one_launch"] = row["rows_path"]["ms_median"] / row["one_launch"]["ms_median"]
        row["launches_only_over_one_launch"] = row["per_step_launches_only"]["ms_median"] / row["one_launch"]["ms_median"]
        row["one_launch_us_per_row"] = 1e3 * row["one_launch"]["ms_median"] / T
        rows.append(row)
    return rows


def learner_setup(B, n, seed, motion=None, time_limit=None):
    args = cs.make_env_args("flight_easy", n_agents=n)
    if time_limit:
        args.time_limit = time_limit
    seeds = np.arange(B, dtype=np.uint32) + 900
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds) if motion is None else cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion)
    cs.apply_env_info(args, env)
    im.get_bc_args(args, seed=seed)
    return args, env


def loss_cases(a, E=32, n=3):
    args, env = learner_setup(E, n, 7)
    episode = cs.EpisodeCollector(env).generate_episodes(policy=cs.random_policy(torch.Generator(DEV).manual_seed(1)), init=True)[0]
    episode["u_expert"] = im.label_episodes(cs.CoverageAgents(env), episode).unsqueeze(3).float()
    T, A = int(episode["u"].shape[1]), args.n_actions
    logits = torch.randn(E, T, n, A, device=DEV)
    avail, labels, mask = episode["avail_u"], episode["u_expert"].squeeze(3).long(), (1 - episode["padded"]).reshape(E, T)
    inv = 1 / (n * mask.sum())
    out = dict(E=E, T=T, n_agents=n, n_actions=A, rows=E * T * n,
               bc_loss_kernel=ms(event_ms(lambda: im.BCLoss.apply(logits, avail, labels, mask, inv), a.reps, a.calls)),
               bc_loss_torch=ms(event_ms(lambda: im.bc_loss_torch(logits, avail, labels, mask), a.reps, a.calls)))
    for unroll in ("fused", "torch"):
        learner = im.ImitationLearner(args, device=DEV, unroll=unroll)
        out["learn_" + unroll] = ms(event_ms(lambda: learner.learn(episode), a.reps if unroll == "fused" else max(3, a.reps // 4),
                                             a.calls if unroll == "fused" else max(1, a.calls // 10)))
    out["loss_torch_over_kernel"] = out["bc_loss_torch"]["ms_median"] / out["bc_loss_kernel"]["ms_median"]
    out["learn_torch_over_fused"] = out["learn_torch"]["ms_median"] / out["learn_fused"]["ms_median"]
    return out


def student_policy(agents):
    def policy(obs, state, last, t):
        if t == 0:
            agents.init_hidden()
        return agents.choose_action(obs.contiguous(), 0.0, True).clone()
    return policy


def found(env, policy):
    curve = cs.collect_experiment_data(env, policy, batches=1)
    scale = env.target_num / 100
    return dict(found_by_step_60=float(curve[59]) * scale, found_by_step_120=float(curve[119]) * scale, found_by_step_200=float(curve[-1]) * scale)


def quality_cases(a, n=3):
    rows = []
    for name, motion, make in (("static", None, lambda env: cs.CoverageAgents(env)),
                               ("evade_speed_1", cs.TargetMotion(mode="evade", speed=1.0, sense=10.0, seed=1), lambda env: cs.ForecastAgents(env))):
        args, env = learner_setup(a.batch, n, 3, motion)
        expert = make(env)
        learner = im.ImitationLearner(args, device=DEV)
        agents = cs.FusedAgents(args, a.batch, net=learner.eval_rnn, seed=1)
        ring = im.LabelledRing(args, a.batch * a.iterations, device=DEV)
        g = torch.Generator(DEV).manual_seed(2)
        row = dict(targets=name, expert=type(expert).__name__, n_agents=n, B=a.batch, n_targets=int(env.target_num), iterations=a.iterations,
                   updates=a.updates, sample=32, lr=args.lr_actor, expert_found=found(env, expert.policy()),
                   random_found=found(env, cs.random_policy(torch.Generator(DEV).manual_seed(3))),
                   untrained_student_found=found(env, student_policy(agents)), student=[])
        for it in range(a.iterations):   # distil one iteration at a time, so the student can be scored between them
            if it == 0:
                h = im.distil(env, expert, learner, agents, ring, 1, a.updates, 32, g)[0]
            else:
                episode, _, _, tf = cs.EpisodeCollector(env).generate_episodes(agents=agents, evaluate=True)
                episode["u_expert"] = im.label_episodes(expert, episode).unsqueeze(3).to(episode["u"].dtype)
                ring.store_episode(episode)
                del episode
                for _ in range(a.updates):
                    learner.learn(ring.sample(32, g))
                agents.sync_weights()
                h = dict(iteration=it, flown_by="student", loss=float(learner.last_stats[0]), agreement=float(learner.last_stats[1]),
                         targets_find=float(tf.double().mean()))
            row["student"].append(dict(h, **found(env, student_policy(agents))))
        state, obs = env.get_state().clone(), env.get_obs().clone()
        if isinstance(expert, cs.ForecastAgents):
            call = lambda: expert.choose_action(state, 1, 30)
        else:
            call = lambda: expert.choose_action(state)
        row["expert_ms_per_decision"] = ms(event_ms(call, a.reps, a.calls))
        row["student_ms_per_decision_one_launch_per_step"] = ms(event_ms(lambda: agents.choose_action(obs, 0.0, True), a.reps, a.calls))
        col = cs.EpisodeCollector(env)
        per_episode = event_ms(lambda: col.generate_episodes(agents=agents, evaluate=True), max(3, a.reps // 4), 1)
        row["student_ms_per_step_closed_loop_with_env_and_assembly"] = dict(ms_median=per_episode[0] / env.time_limit, ms_min=per_episode[1] / env.time_limit)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imitate.json"))
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=6)
    ap.add_argument("--updates", type=int, default=100)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: labelling, loss, quality")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_imitate.py needs the GPU: a CPU run says nothing about the kernels")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_imitate.py: imitation learning (csrc/label.h, csrc/bc_loss.h, imitate.py) on flight_easy; HIP events, "
                    f"windows of {a.calls} calls (a tenth of that for the T-launch paths and the torch learner), median / minimum of {a.reps} "
                    "windows after a warm-up window; everything in one run, no profiler attached",
               device=torch.cuda.get_device_name(0))

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if "labelling" not in skip:
        out["labelling"] = [r for n, flown in ((3, "coverage"), (5, "coverage"), (3, "random")) for r in labelling_cases(n, a.episodes, a, flown)]
        write()
    if "loss" not in skip:
        out["loss"] = loss_cases(a)
        write()
    if "quality" not in skip:
        out["quality"] = quality_cases(a)
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
