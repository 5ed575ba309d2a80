#!/usr/bin/env python3
"""Swept-area accounting on the device (profiles/sweep.json): kernel time, its cost inside a learn call, swept curves, and
PPO's found curve with the exploration bonus.

flight_easy:
  kernel    (a) HIP-event time of one `sweep_episodes` call (the kernel of csrc/sweep.h: per-call time over windows of `--calls`
            back-to-back calls, median and minimum of `--reps` windows after a warm-up window) beside the torch definition on
            the same device (`--def-reps` single calls), on the rows of a random-policy batch: E = 32 and 4096 episodes of
            T1 = 201 rows, teams of 3 and 5;  tests_per_s = cells * n * valid rows / median time (the kernel is bound by its
            integer sweep tests, not by memory).
  learn     (b) one `Runner.train` call of PPO (the learn call and the repack) on one batch of E = 32 episodes of T = 200 steps
            with args.sweep_bonus on against off (off: the batch goes to the learner as it is), the same windows.
  curves    (c) `collect_sweep_data`, one batch of `--batch` envs: percent of the map swept by row t and the efficiency
            sum(new_cells) / sum(seen_cells), `CoverageAgents` beside `random_policy`, teams of 3 and 5.
  training  (d) PPO on flight_easy, 3 agents, B = 256, `--epochs` epochs, evaluated every `--evaluate-cycle`: targets_find of
            every evaluation with args.sweep_bonus = 0 and the values of `--bonus` (evaluation never sees the bonus).
usage: python tools/bench_sweep.py [--out FILE] [--batch B] [--reps N] [--calls N] [--def-reps N] [--epochs N] [--bonus a,b]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

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


def make_env(n, B, seed0=1):
    return cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=np.arange(B, dtype=np.uint32) + seed0)


def kernel_case(n, E, a):
    env = make_env(n, E)
    episode, *_ = cs.EpisodeCollector(env).generate_episodes(policy=cs.random_policy(torch.Generator(device="cuda").manual_seed(7)), init=True)
    states, _maps, counts = cs.episode_tables(episode, env)
    del episode
    side, vr = int(env.map_size), int(env.view_range)
    hip = cs.sweep_episodes(states, counts, n, side, vr)
    ref = cs.sweep_episodes_torch(states, counts, n, side, vr)
    equal = all(bool(torch.equal(x, y)) for x, y in zip(hip, ref))
    k_med, k_min = event_ms(lambda: cs.sweep_episodes(states, counts, n, side, vr), a.reps, a.calls)
    d_med, d_min = event_ms(lambda: cs.sweep_episodes_torch(states, counts, n, side, vr), a.def_reps)
    tests = side * side * n * int(counts.to(torch.int64).sum())
    T1, S = int(states.shape[1]), int(states.shape[2])
    return dict(n_agents=n, E=E, T1=T1, side=side, view_range=vr, state_width=S, mean_valid_rows=float(counts.float().mean()),
                kernel_equals_definition=equal, bytes_read=16 * n * int(counts.to(torch.int64).sum()), bytes_written=E * (8 * T1 + 4 * side * side),
                sweep_tests=tests,
                kernel=dict(ms_median=k_med, ms_min=k_min, tests_per_s=tests / (k_med * 1e-3)),
                definition=dict(ms_median=d_med, ms_min=d_min), speedup=d_med / k_med)


def make_runner(B, root, seed=1, **over):
    args = cs.make_env_args("flight_easy", n_agents=3)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 11)
    cs.apply_env_info(args, env)
    args.alg = "ppo"
    cs.get_ppo_args(args, seed=seed)
    args.model_dir, args.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
    args.save_cycle = 10 ** 9   # no checkpoints inside the timed calls
    for k, v in over.items():
        setattr(args, k, v)
    return cs.Runner(env, args), env


def learn_case(a, E=32, beta=0.02):
    with tempfile.TemporaryDirectory() as root:
        r, env = make_runner(E, root)
        batch, *_ = r.collector.generate_episodes(agents=r.agents, evaluate=False, episode_num=0)
        step = [1]

        def call():
            r.train(batch, step[0])
            step[0] += 1
        out = dict(alg="ppo", E=E, T=int(env.time_limit), n_agents=3, sweep_bonus=beta)
        r.args.sweep_bonus = 0.0
        out["off_ms_median"], out["off_ms_min"] = event_ms(call, a.reps, a.calls)
        r.args.sweep_bonus = beta
        out["on_ms_median"], out["on_ms_min"] = event_ms(call, a.reps, a.calls)
        r.args.sweep_bonus = 0.0
        out["off_again_ms_median"], out["off_again_ms_min"] = event_ms(call, a.reps, a.calls)   # (the order of the two is not what is seen)
        out["with_sweep_bonus_alone_ms_median"], out["with_sweep_bonus_alone_ms_min"] = event_ms(
            lambda: cs.with_sweep_bonus(batch, r.args, beta), a.reps, a.calls)
        out["overhead_ms"] = out["on_ms_median"] - min(out["off_ms_median"], out["off_again_ms_median"])
        out["overhead_percent"] = 100.0 * out["overhead_ms"] / min(out["off_ms_median"], out["off_again_ms_median"])
    return out


def curve_case(n, B):
    env = make_env(n, B, seed0=300)
    col = cs.EpisodeCollector(env)
    out = dict(n_agents=n, B=B, unit="percent of the map swept by row t (row 0: the reset pose)")
    for name, policy in (("coverage", cs.CoverageAgents(env).policy()), ("random", cs.random_policy(torch.Generator(device="cuda").manual_seed(3)))):
        d = cs.collect_sweep_data(col, policy, batches=1)
        out[name] = dict(curve=[round(float(v), 3) for v in d["curve"]], swept_by_row_60=float(d["curve"][60]),
                         swept_by_row_200=float(d["curve"][-1]), efficiency=d["efficiency"], targets_find=d["targets_find"], steps=d["steps"])
    return out


def training_case(a, beta):
    with tempfile.TemporaryDirectory() as root:
        over = dict(evaluate_cycle=a.evaluate_cycle)
        if beta:
            over["sweep_bonus"] = beta
        r, env = make_runner(256, root, **over)
        r.run(0, n_epoch=a.epochs)
        return dict(sweep_bonus=beta, targets_find=[round(v, 4) for v in r.targets_find], episode_reward=[round(v, 3) for v in r.episode_rewards],
                    win_rate=[round(v, 4) for v in r.win_rates])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep.json"))
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--def-reps", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--evaluate-cycle", type=int, default=10)
    ap.add_argument("--bonus", type=lambda s: [float(x) for x in s.split(",")], default=[0.02, 0.1])
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out: kernel, learn, curves, training")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweep.py needs the GPU: a CPU run says nothing about the kernel")
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(_doc="tools/bench_sweep.py: swept-area accounting (csrc/sweep.h) on flight_easy; kernel / learn: HIP events over windows of "
                    f"{a.calls} calls (median / minimum of {a.reps} windows), the torch definition over {a.def_reps} single calls, same "
                    "device; curves: collect_sweep_data, one batch; training: Runner.run of PPO, B = 256, targets_find of every evaluation",
               device=torch.cuda.get_device_name(0))
    if "kernel" not in skip:
        out["kernel"] = [kernel_case(n, E, a) for n in (3, 5) for E in (32, a.batch)]
    if "learn" not in skip:
        out["learn"] = learn_case(a)
    if "curves" not in skip:
        out["curves"] = [curve_case(n, a.batch) for n in (3, 5)]
    if "training" not in skip:
        out["training"] = dict(alg="ppo", env="flight_easy", n_agents=3, B=256, epochs=a.epochs, evaluate_cycle=a.evaluate_cycle,
                               runs=[training_case(a, beta) for beta in [0.0] + list(a.bonus)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    brief = dict(kernel=[{k: c[k] for k in ("n_agents", "E", "kernel_equals_definition", "kernel", "speedup")} for c in out.get("kernel", [])],
                 learn=out.get("learn"),
                 curves=[{k: ({q: c[k][q] for q in ("swept_by_row_60", "swept_by_row_200", "efficiency")} if isinstance(c[k], dict) else c[k])
                          for k in ("n_agents", "coverage", "random")} for c in out.get("curves", [])],
                 training=[dict(sweep_bonus=r["sweep_bonus"], targets_find=r["targets_find"]) for r in out.get("training", {}).get("runs", [])])
    print(json.dumps(brief))


if __name__ == "__main__":
    main()
