#!/usr/bin/env python3
"""Time per training epoch on one GPU: `Runner`'s epoch body (collect -> store -> sample -> learn -> repack) with the acting
network repacked on the device (`FusedAgents.sync_weights`, the pack kernel) against the same loop repacked on the host
(`load_weights`: device-to-host copy of the parameters, host pack, host-to-device copy of the blob -- a host synchronisation per
learn call).  flight_easy with 3 agents at B = 32, 256, 4096 envs; n_episodes = train_steps = 1, batch_size 32 (the reference's
defaults); the ring holds max(buffer_size, B) episodes.  Epochs are timed in windows of --window back-to-back epochs between two
HIP events (what the host can enqueue ahead shows up there); ms/epoch = the median window / window.  Also times one repack
either way: the pack kernel under HIP events, the host pack with a wall clock (it blocks the host).  Prints ONE JSON line.

--curve: instead, one learning curve of --alg (flight_easy, 3 agents, B = 256): targets_find of every evaluation of Runner.run,
next to the random policy under the same evaluation.

    python tools/train_bench.py [--alg qmix|dop|reinforce|ppo] [--warmup 10] [--windows 5] [--window 5] [--batches 32,256,4096]
    python tools/train_bench.py --curve [--alg qmix] [--epochs 3000] [--evaluate-cycle 100]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARGS_FN = {"qmix": "get_mixer_args", "dop": "get_dop_args", "reinforce": "get_reinforce_args", "ppo": "get_ppo_args"}


def make_runner(alg, B, root, seed=1, **over):
    import numpy as np
    import cooperative_search_amd as cs
    args = cs.make_env_args("flight_easy", n_agents=3)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 11)
    cs.apply_env_info(args, env)
    args.alg = alg
    getattr(cs, ARGS_FN[alg])(args, seed=seed)
    if hasattr(args, "buffer_size"):   # (PPO keeps no ring)
        args.buffer_size = max(args.buffer_size, B)
    args.model_dir, args.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
    args.save_cycle = 10 ** 9   # no checkpoints inside the timed epochs
    for k, v in over.items():
        setattr(args, k, v)
    return cs.Runner(env, args), env


def time_epochs(r, warmup, windows, window):
    import torch
    steps = 0
    for _ in range(warmup):
        steps = r.train_epoch(steps)
    torch.cuda.synchronize()
    per = []
    for _ in range(windows):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(window):
            steps = r.train_epoch(steps)
        t1.record()
        t1.synchronize()
        per.append(t0.elapsed_time(t1) / window)
    per.sort()
    return round(per[len(per) // 2], 3), round(per[0], 3)


def time_pack(agents, reps=50):
    import torch
    dev = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        agents.sync_weights()
        t1.record()
        t1.synchronize()
        dev.append(t0.elapsed_time(t1))
    host = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        agents.load_weights()
        host.append((time.perf_counter() - t) * 1e3)
    dev.sort()
    host.sort()
    return round(dev[reps // 2], 4), round(host[reps // 2], 4)


def bench(a):
    import torch
    cases = []
    for B in a.batches:
        with tempfile.TemporaryDirectory() as root:
            case = dict(env="flight_easy", n_agents=3, B=B)
            for how in ("sync_weights", "load_weights"):
                r, env = make_runner(a.alg, B, root)
                if how == "load_weights":
                    r.agents.sync_weights = r.agents.load_weights   # the hand loop of INTEGRATION.md before this driver
                med, best = time_epochs(r, a.warmup, a.windows, a.window)
                case[f"{how}_ms_per_epoch"], case[f"{how}_min_ms_per_epoch"] = med, best
                if how == "sync_weights":
                    case["pack_kernel_ms"], case["host_pack_ms"] = time_pack(r.agents)
                del r, env
                torch.cuda.empty_cache()
            case["speedup"] = round(case["load_weights_ms_per_epoch"] / case["sync_weights_ms_per_epoch"], 3)
            cases.append(case)
    return dict(tool="train_bench", alg=a.alg, device=torch.cuda.get_device_name(0), warmup=a.warmup, windows=a.windows,
                window=a.window, timer="HIP events around windows of back-to-back epochs; median window / window",
                epoch="collect (1 launch) -> store -> sample(32) -> learn -> repack", cases=cases)


def curve(a):
    import torch
    import cooperative_search_amd as cs
    with tempfile.TemporaryDirectory() as root:
        r, env = make_runner(a.alg, a.curve_batch, root, seed=a.seed, evaluate_cycle=a.evaluate_cycle)
        ev = r.evaluate

        def evaluate():   # progress on stderr, one line per evaluation
            res = ev()
            print(f"evaluation {len(r.targets_find)}: targets_find {res[2]:.3f}", file=sys.stderr, flush=True)
            return res
        r.evaluate = evaluate
        t = time.time()
        r.run(0, n_epoch=a.epochs)
        wall = time.time() - t
        g = torch.Generator("cuda").manual_seed(5)
        batches = max(1, math.ceil(r.args.evaluate_epoch / env.batch))
        rand = [cs.evaluate(env, cs.random_policy(g), batches) for _ in range(5)]
    return dict(tool="train_bench --curve", alg=a.alg, env="flight_easy", n_agents=3, B=a.curve_batch, seed=a.seed,
                epochs=a.epochs, evaluate_cycle=a.evaluate_cycle, evaluate_episodes=batches * a.curve_batch,
                train_steps_per_epoch=r.args.train_steps, batch_size=getattr(r.args, "batch_size", a.curve_batch), wall_s=round(wall, 1),
                targets_find=[round(v, 4) for v in r.targets_find], episode_reward=[round(v, 3) for v in r.episode_rewards],
                win_rate=[round(v, 4) for v in r.win_rates],
                random_policy_targets_find=[round(x[2], 4) for x in rand],
                random_policy_shipped_mean_targets_found=_shipped_random())


def _shipped_random():
    with open(os.path.join(ROOT, "tests", "golden", "random_curves.json")) as f:
        d = json.load(f)
    return [c["mean_targets_found"] for c in d["curves"] if c["n_agents"] == 3 and c["agent_mode"] == 0][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alg", choices=tuple(ARGS_FN), default="qmix")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--batches", type=lambda s: [int(x) for x in s.split(",")], default=[32, 256, 4096])
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--curve-batch", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=3000)
    ap.add_argument("--evaluate-cycle", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    t0 = time.time()
    out = curve(a) if a.curve else bench(a)
    out["total_wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
