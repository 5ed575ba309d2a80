#!/usr/bin/env python3
"""Dense against map-once episode storage on the flight variant, one GPU.

Per team size (3 and 5 agents), T = 200, HIP events, `--repeats` timed repeats after `--warmup` untimed ones, the two formats
alternating inside one process:
  (a) one collection into the ring at B = 1024: generate_episodes(agents, into=ring) as it is (dense: the per-step branch and
      cs_store_episodes) against generate_episodes(compact=True) (cs_collect_flight and cs_store_episodes_compact);
  (b) one QMIX learn (fused unroll) at E = 32 and E = 256 on samples of the two rings -- the same episodes, the same indices.
Each figure is the median, with min, max and spread = max - min of the repeats; `ok` says whether the compact median is within
the dense median + the dense spread.  The first learn of every new conv shape pays MIOpen's first-use search (87 s for the dense
batch at E = 32, beyond 7 minutes at E = 256): the warm-up absorbs it; the E = 256 figures of profiles/compact_flight.json
come from a run under MIOPEN_FIND_MODE=FAST (recorded as `miopen_find_mode`), both formats alike.  `capacity` is the largest B whose collection tables + a ring of B episodes fit in 64e9
bytes, from the formulas, cross-checked by allocating exactly those tensors at that B (`--no-alloc-check` skips it).

    python tools/compact_bench.py [--repeats 5] [--warmup 2] [--batch 1024] [--out profiles/compact_flight.json]
    python tools/compact_bench.py --dense-only          # the dense half alone: runs on a checkout without the compact format
    python tools/compact_bench.py --trace-workload      # a few collections of each kind and nothing else, for
                                                        # rocprofv3 --kernel-trace --stats (in a run of its own)
    python tools/compact_bench.py --kernel-stats FILE --out JSON   # add the map kernels' achieved bytes/s from
                                                        # tools/prof_summary.py's table of that trace to the JSON
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, CELLS, TARGETS, A = 200, 2500, 15, 3
BUDGET = 64e9


# ---- bytes, from the shapes ----------------------------------------------------------------------------------------------------

def ring_bytes(n, compact):
    S = 4 * n + 3 * TARGETS
    if compact:   # map, s_full [T+1]; u [T, n]; r, padded, terminated [T]
        return 4 * ((T + 1) * (CELLS + S) + T * (n + 3))
    return 4 * T * (2 * n * (CELLS + 4) + n + 2 * S + 1 + 3 * n * A + 2)   # o, o_next, u, s, s_next, r, 3 x [n, A], padded, terminated


def table_bytes(n, compact):
    """Per env: the collector's step-major tables (obs or map, state, int64 actions, reward, terminated)."""
    S = 4 * n + 3 * TARGETS
    wide = CELLS if compact else n * (CELLS + 4)
    return 4 * (T + 1) * (wide + S) + T * n * 8 + T * 4 + T


def capacity(n, compact):
    return int(BUDGET // (ring_bytes(n, compact) + table_bytes(n, compact)))


def sweep_bytes(kernel, n, B):
    """HBM bytes one map sweep needs: the map read once plus the copies it writes (the in-place update rewrites only the
    cells in view and is not counted)."""
    copies = {"k_map": n, "k_map_snap": 1, "k_map_update": 0}[kernel]
    return B * CELLS * 4 * (1 + copies)


# ---- timing --------------------------------------------------------------------------------------------------------------------

def timed(fn, label=None):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1)
    if label:   # progress on stderr: a dense learn at E = 256 takes seconds, the run must not look hung
        print(f"{label}: {ms:.2f} ms", file=sys.stderr, flush=True)
    return ms


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
                spread_ms=round(max(ms) - min(ms), 3), all_ms=[round(v, 3) for v in ms])


def verdict(entry):
    if "dense" in entry and "compact" in entry:
        d, c = entry["dense"], entry["compact"]
        entry["speedup"] = round(d["median_ms"] / c["median_ms"], 2)
        entry["ok"] = c["median_ms"] <= d["median_ms"] + d["spread_ms"]
    return entry


class Side:
    """One format's env, agents, collector and ring; the two sides start from equal seeds and take equal steps."""

    def __init__(self, n, B, compact):
        import numpy as np
        import torch
        import cooperative_search_amd as cs
        self.compact = compact
        self.args = cs.make_env_args("flight", n_agents=n)
        self.env = cs.BatchedFlightEnv(self.args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 7)
        cs.apply_env_info(self.args, self.env)
        self.args.alg = "qmix"
        cs.get_mixer_args(self.args, seed=1)
        torch.manual_seed(2)
        self.agents = cs.FusedAgents(self.args, B, seed=3)
        self.col = cs.EpisodeCollector(self.env, cs.EpsilonSchedule(self.args, B))
        self.ring = (cs.CompactReplayBuffer if compact else cs.DeviceReplayBuffer)(self.args, B)
        self.kw = dict(compact=True) if compact else {}

    def collect(self):
        self.col.generate_episodes(agents=self.agents, evaluate=False, episode_num=0, into=self.ring, **self.kw)

    def learner(self):
        import cooperative_search_amd as cs
        return cs.QMixLearner(self.args, device="cuda", unroll="fused")


def run_team(n, B, warmup, repeats, formats, sizes):
    import torch
    sides = {f: Side(n, B, f == "compact") for f in formats}
    out = dict(n_agents=n, B=B, T=T, collect={}, learn={})
    ms = {f: [] for f in formats}
    for k in range(warmup + repeats):
        for f in formats:   # alternating: both formats see the same drift of the machine
            t = timed(sides[f].collect, f"{n} agents collect {f} #{k}")
            if k >= warmup:
                ms[f].append(t)
    out["collect"] = verdict({f: summary(ms[f]) for f in formats})
    for E in sizes:
        ms = {f: [] for f in formats}
        learners = {f: sides[f].learner() for f in formats}
        gens = {f: torch.Generator(device="cuda").manual_seed(E) for f in formats}
        for k in range(warmup + repeats):
            for f in formats:
                batch = sides[f].ring.sample(E, generator=gens[f])
                t = timed(lambda: learners[f].learn(batch), f"{n} agents learn E={E} {f} #{k}")
                if k >= warmup:
                    ms[f].append(t)
                del batch
        out["learn"][f"E{E}"] = verdict({f: summary(ms[f]) for f in formats})
        del learners
        torch.cuda.empty_cache()
    del sides
    torch.cuda.empty_cache()
    return out


def alloc_check(n, compact):
    """Allocate the collection tables and the ring of `capacity` episodes, nothing else: bytes torch hands out."""
    import torch
    B, S = capacity(n, compact), 4 * n + 3 * TARGETS
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    f32 = dict(dtype=torch.float32, device="cuda")
    wide = (T + 1, B, CELLS) if compact else (T + 1, B, n, CELLS + 4)
    held = [torch.empty(wide, **f32), torch.empty(T + 1, B, S, **f32), torch.empty(T, B, n, dtype=torch.int64, device="cuda"),
            torch.empty(T, B, **f32), torch.empty(T, B, dtype=torch.bool, device="cuda")]
    if compact:
        shapes = [(B, T + 1, CELLS), (B, T + 1, S), (B, T, n, 1)] + [(B, T, 1)] * 3
    else:
        shapes = ([(B, T, n, CELLS + 4)] * 2 + [(B, T, n, 1)] + [(B, T, S)] * 2 + [(B, T, 1)] + [(B, T, n, A)] * 3 + [(B, T, 1)] * 2)
    held += [torch.empty(s, **f32) for s in shapes]
    got = torch.cuda.memory_allocated() - before
    del held
    torch.cuda.empty_cache()
    return dict(B=B, formula_bytes=B * (ring_bytes(n, compact) + table_bytes(n, compact)), allocated_bytes=got)


def trace_workload(B):
    """What the kernel trace should see: k_map (dense collections), k_map_snap (compact collections) and k_map_update
    (the closed loop without observation rows), 3 and 5 agents."""
    import torch
    for n in (3, 5):
        for compact in (False, True):
            side = Side(n, B, compact)
            for _ in range(3):
                side.collect()
            if compact:
                side.agents.init_hidden()
                side.env.rollout_policy(side.agents, T, 0.3, False, emit=False)
            torch.cuda.synchronize()
            del side
            torch.cuda.empty_cache()


def add_kernel_stats(path, out_path, B):
    """tools/prof_summary.py's table -> achieved bytes/s of the three map sweeps, merged into the JSON at out_path."""
    rows = {}
    for line in open(path):
        m = re.search(r"\b(k_map_snap|k_map_update|k_map)<(\d)>", line)
        if not m:
            continue
        nums = line[70:].split()
        kernel, n, calls, avg_us = m.group(1), int(m.group(2)), int(nums[0]), float(nums[1])
        nbytes = sweep_bytes(kernel, n, B)
        rows[f"{kernel}<{n}>"] = dict(calls=calls, avg_us=avg_us, bytes=nbytes, gbytes_per_s=round(nbytes / avg_us / 1e3, 1))
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["map_sweeps"] = dict(B=B, source="rocprofv3 --kernel-trace of --trace-workload; bytes = map read + copies written",
                             kernels=rows)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc["map_sweeps"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sizes", type=int, nargs="*", default=[32, 256])
    ap.add_argument("--teams", type=int, nargs="*", default=[3, 5])
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--no-alloc-check", action="store_true")
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.kernel_stats:
        return add_kernel_stats(a.kernel_stats, a.out, a.batch)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("compact_bench needs the GPU: nothing here is measured without one")
    if a.trace_workload:
        return trace_workload(a.batch)
    t0 = time.time()
    formats = ("dense",) if a.dense_only else ("dense", "compact")
    doc = dict(tool="compact_bench", device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats,
               miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE", "default"),
               timer="HIP events around one call; median, min, max, spread = max - min of the repeats; formats alternate",
               teams=[run_team(n, a.batch, a.warmup, a.repeats, formats, a.sizes) for n in a.teams])
    doc["bytes"] = {f"{n}_agents": dict(ring_per_episode=dict(dense=ring_bytes(n, False), compact=ring_bytes(n, True)),
                                        tables_per_env=dict(dense=table_bytes(n, False), compact=table_bytes(n, True)),
                                        largest_B_in_64e9=dict(dense=capacity(n, False), compact=capacity(n, True)))
                    for n in a.teams}
    if not a.no_alloc_check and not a.dense_only:
        doc["alloc_check"] = {f"{n}_agents_{'compact' if c else 'dense'}": alloc_check(n, c) for n in a.teams for c in (False, True)}
    doc["wall_s"] = round(time.time() - t0, 1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
