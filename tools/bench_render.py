#!/usr/bin/env python3
"""Time of the frame kernel (cs_render_episodes) and of its torch definition on the same device (profiles/render.json).

E = 16 episodes of R = 201 rows at W = 256, random-policy episodes of 3 agents: flight_easy (no map) and flight (with the
probability maps).  The kernel is timed between HIP events around `--calls` back-to-back calls (median and minimum of `--reps`
windows after a warm-up window); the definition around one call (`--def-reps` windows).  bytes_written = E * R * W * W * 3 is
what the kernel must write; it reads the state rows (and, through the cache, the maps).  The figure to hold the rate against is
the write stream of profiles/r06_write_bw.log.
usage: python tools/bench_render.py [--out FILE] [--reps N] [--calls N] [--def-reps N]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cooperative_search_amd as cs  # noqa: E402
from cooperative_search_amd import render as rd  # noqa: E402

E, W = 16, 256


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


def tables(variant):
    """Random-policy episodes of E envs: states [E, T + 1, S], maps [E, T + 1, cells] or None, counts."""
    args = cs.make_env_args(variant, n_agents=3)
    env = cs.BatchedFlightEnv(args, batch=E)
    env.reset(init=True)
    T = env.time_limit
    s0 = env.get_state().clone()
    m0 = env.get_obs()[:, 0, :env.cells].clone() if env.flight else None
    g = torch.Generator(device="cuda").manual_seed(1)
    out = env.rollout(torch.randint(0, 3, (T, E, 3), dtype=torch.int32, device="cuda", generator=g))
    states = torch.cat([s0[None], out["state"]], 0).transpose(0, 1).contiguous()
    maps = None
    if env.flight:
        maps = torch.cat([m0[None], out["obs"][:, :, 0, :env.cells]], 0).transpose(0, 1).contiguous()
    real = 1 + (~out["terminated"][:-1]).sum(0)   # a step is real if the env had not terminated before it
    return states, maps, (real + 1).to(torch.int32), rd.RenderSpec.for_env(env, W)


def case(variant, reps, calls, def_reps):
    states, maps, counts, spec = tables(variant)
    R = int(states.shape[1])
    out = torch.empty(E, R, W, W, 3, dtype=torch.uint8, device="cuda")
    k_med, k_min = event_ms(lambda: rd.render_episodes(states, maps, counts, spec, out=out), reps, calls)
    d_med, d_min = event_ms(lambda: rd.render_episodes_torch(states, maps, counts, spec), def_reps)
    equal = bool(torch.equal(out, rd.render_episodes_torch(states, maps, counts, spec)))
    written = E * R * W * W * 3
    read = states.numel() * 4 + (maps.numel() * 4 if maps is not None else 0)
    return dict(variant=variant, E=E, R=R, W=W, n_agents=3, with_maps=maps is not None, counts=counts.tolist(),
                bytes_written=written, input_bytes=read, kernel_equals_definition=equal,
                kernel=dict(ms_median=k_med, ms_min=k_min, write_GBps=written / (k_med * 1e-3) / 1e9),
                definition=dict(ms_median=d_med, ms_min=d_min, write_GBps=written / (d_med * 1e-3) / 1e9),
                speedup=d_med / k_med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--def-reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs the GPU: a CPU run says nothing about the kernel")
    out = dict(_doc="tools/bench_render.py: render_episodes (the HIP kernel) and render_episodes_torch (stock torch ops) on the same "
                    f"device, HIP events; kernel: per-call time over windows of {a.calls} calls, median and minimum of {a.reps} windows "
                    f"after a warm-up window; definition: {a.def_reps} single calls after a warm-up call; write_GBps = bytes_written / "
                    "median time (compare with the write stream of profiles/r06_write_bw.log)",
               device=torch.cuda.get_device_name(0), cases=[case(v, a.reps, a.calls, a.def_reps) for v in ("flight_easy", "flight")])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
