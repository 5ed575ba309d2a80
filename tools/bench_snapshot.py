#!/usr/bin/env python3
"""Times of env snapshot / restore and of Runner.save_state (profiles/snapshot.json).

One `snapshot` and one `restore` of a whole batch between HIP events (median of `--reps` calls after a warm-up call), with
the bytes each moves, at flight_easy B = 4096 and 65536 and flight B = 8192; then the size and the host-clock write time of a
state file of a QMIX run at B = 256 (flight_easy, one epoch in), with and without the ring.
usage: python tools/bench_snapshot.py [--out FILE] [--reps N]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cooperative_search_amd as cs  # noqa: E402
from cooperative_search_amd import runner as rn  # noqa: E402


def event_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def env_case(variant, B, reps):
    env = cs.BatchedFlightEnv(cs.make_env_args(variant, n_agents=3), batch=B)
    env.rollout(torch.randint(0, 3, (8, B, 3), dtype=torch.int32, device="cuda"))
    snap = env.snapshot()
    rec = snap.records.shape[1]
    cells = env.cells * 4 if env.flight else 0
    fixed = 64 + 256 + 256   # an env's header words, targets and agents in the state blob
    # snapshot: reads header, targets, agents, `ahead`, the 624-word row (and the map), writes the record
    snap_bytes = B * (fixed + 4 + 624 * 4 + cells + rec)
    # restore: reads the record, writes header, targets, agents, `ahead`, row + 32 mirror words, 56 bytes of tape (the map, and
    # 16 bytes of each job record); the emission that follows reads header, targets, agents (and the map) of every env and
    # writes get_obs() / get_state()
    rest_bytes = B * (rec + fixed + 4 + 656 * 4 + 56 + cells + (32 if env.flight else 0))
    emit_bytes = B * (fixed + cells) + (env.get_obs().numel() + env.get_state().numel()) * 4
    s_med, s_min = event_ms(lambda: env.snapshot(), reps)
    r_med, r_min = event_ms(lambda: env.restore(snap), reps)
    return dict(variant=variant, batch=B, n_agents=3, record_bytes=rec,
                snapshot=dict(ms_median=s_med, ms_min=s_min, bytes_moved=snap_bytes),
                restore=dict(ms_median=r_med, ms_min=r_min, bytes_moved=rest_bytes + emit_bytes, restore_kernel_bytes=rest_bytes,
                             emit_bytes=emit_bytes, note="timed with the re-emission of get_obs() / get_state() that "
                                                         "BatchedFlightEnv.restore always asks for"))


def state_file_case(B, with_buffer):
    with tempfile.TemporaryDirectory() as d:
        args = cs.make_env_args("flight_easy", n_agents=3)
        env = cs.BatchedFlightEnv(args, batch=B)
        cs.apply_env_info(args, env)
        args.alg = "qmix"
        cs.get_mixer_args(args, seed=1)
        args.buffer_size, args.batch_size, args.evaluate_cycle = 2 * B, 32, 1000
        args.model_dir, args.result_dir = os.path.join(d, "model") + "/", os.path.join(d, "result") + "/"
        r = rn.Runner(env, args)
        r.run(0, n_epoch=1)
        path = os.path.join(d, "state.pt")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.save_state(path, with_buffer=with_buffer)
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        r.load_state(path)
        torch.cuda.synchronize()
        dl = time.perf_counter() - t0
        return dict(alg="qmix", variant="flight_easy", batch=B, with_buffer=with_buffer, ring_episodes=int(r.buffer.current_size),
                    file_bytes=os.path.getsize(path), write_s=dt, load_s=dl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = dict(_doc="tools/bench_snapshot.py: one snapshot / restore of the whole batch between HIP events (median and minimum of "
                    f"{a.reps} calls); bytes_moved counts reads + writes of the kernels; state files: host clock around save_state / "
                    "load_state in a temporary directory", device=torch.cuda.get_device_name(0),
               envs=[env_case("flight_easy", 4096, a.reps), env_case("flight_easy", 65536, a.reps), env_case("flight", 8192, a.reps)],
               state_files=[state_file_case(256, True), state_file_case(256, False)])
    for e in out["envs"]:
        for k in ("snapshot", "restore"):
            e[k]["GBps"] = e[k]["bytes_moved"] / (e[k]["ms_median"] * 1e-3) / 1e9
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
