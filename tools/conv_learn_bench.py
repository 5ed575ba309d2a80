#!/usr/bin/env python3
"""The flight conv front end in a learn step: `conv_impl="hip"` (k_conv_features / k_conv_features_bwd) against
`conv_impl="torch"` (the torch modules, i.e. MIOpen), one GPU.

HIP events, `--repeats` timed repeats after `--warmup` untimed ones, the two implementations alternating inside one process,
median / min / max / spread = max - min; `ok` says whether the "hip" median is within the "torch" median + the "torch" spread.
  (a) one QMIX learn (fused unroll) on flight, T = 200, 3 and 5 agents, a map-once sample and its dense expansion, E = 32 and 256:
      the same episodes and the same initial weights for both implementations;
  (b) the op alone at 6 400 and 51 200 maps: forward and backward of ConvFeatures against the torch modules on the same maps
      (uniform maps, every second dfeat row zero as in a padded batch; `--live-seed` weights, a live front end);
  (c) the wall time of the FIRST learn (E = 32, 3 agents, map-once) of a fresh process, one child process per implementation.
MIOpen's find mode is recorded (`miopen_find_mode`): in the default mode the first use of a conv shape searches for tens of
seconds to minutes, which the warm-up absorbs for (a) and (b) and which (c) is there to show; under
MIOPEN_FIND_MODE=FAST there is no search, but some shapes get a slow fallback solver.  `--out` APPENDS the run to the file's list
of runs, so one file holds the default-mode runs (E = 32, the op, the first learn) and the FAST-mode run (E = 256).

    python tools/conv_learn_bench.py [--repeats 5] [--warmup 2] [--out profiles/conv_learn.json]
    python tools/conv_learn_bench.py --torch-only      # the "torch" column alone: runs on a checkout without conv_impl
    python tools/conv_learn_bench.py --trace-workload  # a few conv_impl="hip" learns and nothing else, for
                                                       # rocprofv3 --kernel-trace --stats (in a run of its own)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, CELLS = 200, 2500


def timed(fn, label=None):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1)
    if label:
        print(f"{label}: {ms:.3f} ms", file=sys.stderr, flush=True)
    return ms


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                spread_ms=round(max(ms) - min(ms), 4), all_ms=[round(v, 4) for v in ms])


def verdict(entry):
    if "torch" in entry and "hip" in entry:
        t, h = entry["torch"], entry["hip"]
        entry["speedup"] = round(t["median_ms"] / h["median_ms"], 2)
        entry["ok"] = h["median_ms"] <= t["median_ms"] + t["spread_ms"]
    return entry


def alternate(fns, warmup, repeats, label):
    ms = {k: [] for k in fns}
    for r in range(warmup + repeats):
        for k, fn in fns.items():
            t = timed(fn, f"{label} {k} #{r}")
            if r >= warmup:
                ms[k].append(t)
    return verdict({k: summary(v) for k, v in ms.items()})


def ring_of(n, B, seed):
    """(args, a map-once ring of B collected flight episodes, T = 200)."""
    import numpy as np
    import torch
    import cooperative_search_amd as cs
    args = cs.make_env_args("flight", n_agents=n)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 7)
    cs.apply_env_info(args, env)
    args.alg = "qmix"
    cs.get_mixer_args(args, seed=seed)
    torch.manual_seed(2)
    agents = cs.FusedAgents(args, B, seed=3)
    ring = cs.CompactReplayBuffer(args, B)
    cs.EpisodeCollector(env, cs.EpsilonSchedule(args, B)).generate_episodes(agents=agents, evaluate=False, episode_num=0, into=ring,
                                                                            compact=True)
    return args, ring


def make_learner(args, impl):
    import cooperative_search_amd as cs
    kw = {} if impl == "torch" and "conv_impl" not in cs.QMixLearner.__init__.__code__.co_varnames else dict(conv_impl=impl)
    return cs.QMixLearner(args, device="cuda", unroll="fused", **kw)


def learn_points(n, impls, sizes, warmup, repeats, seed):
    import torch
    from cooperative_search_amd.replay import expand_compact
    args, ring = ring_of(n, max(sizes), seed)
    out = {}
    for E in sizes:
        c = ring.sample(E, generator=torch.Generator(device="cuda").manual_seed(E))
        for fmt in ("map_once", "dense"):
            batch = c if fmt == "map_once" else expand_compact(c, n, 3)
            learners = {impl: make_learner(args, impl) for impl in impls}
            fns = {impl: (lambda lr=learners[impl]: lr.learn(batch)) for impl in impls}
            out[f"{fmt}_E{E}"] = alternate(fns, warmup, repeats, f"{n} agents {fmt} E={E}")
            out[f"{fmt}_E{E}"]["real_step_share"] = round(float(1 - c["padded"].mean()), 4)
            del learners, fns, batch
            torch.cuda.empty_cache()
    return dict(n_agents=n, T=T, learn=out)


def op_points(impls, counts, warmup, repeats, seed):
    """Forward and backward alone: ConvFeatures against the torch modules, the same weights, maps and dfeat."""
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    conv = nn.Sequential(nn.Conv2d(1, 4, 4, 2), nn.ReLU(), nn.Conv2d(4, 1, 3, 1, 1), nn.ReLU()).cuda()
    linear = nn.Linear(576, 16).cuda()
    w = [conv[0].weight, conv[0].bias, conv[2].weight, conv[2].bias, linear.weight, linear.bias]
    out = {}
    for n_maps in counts:
        g = torch.Generator(device="cuda").manual_seed(n_maps)
        maps = torch.rand(n_maps, CELLS, device="cuda", generator=g)
        dfeat = torch.randn(n_maps, 16, device="cuda", generator=g)
        dfeat[1::2] = 0
        maps[1::2] = 0   # padded steps: zero map, zero gradient
        fwd, bwd = {}, {}
        if "torch" in impls:
            run = lambda: linear(conv(maps.view(-1, 1, 50, 50)).reshape(-1, 576))
            feat_t = run()
            fwd["torch"] = run
            bwd["torch"] = lambda: torch.autograd.grad(feat_t, w, dfeat, retain_graph=True)
        if "hip" in impls:
            from cooperative_search_amd.learner import ConvFeatures
            run_h = lambda: ConvFeatures.apply(maps, CELLS, n_maps, *w)
            feat_h = run_h()
            fwd["hip"] = run_h
            bwd["hip"] = lambda: torch.autograd.grad(feat_h, w, dfeat, retain_graph=True)
        out[f"maps_{n_maps}"] = dict(forward=alternate(fwd, warmup, repeats, f"op forward {n_maps}"),
                                     backward=alternate(bwd, warmup, repeats, f"op backward {n_maps}"))
    return out


def first_learn(impl, seed):
    """In a fresh process: the wall time of the first learn (host clock around learn + synchronize)."""
    import torch
    args, ring = ring_of(3, 32, seed)
    batch = ring.sample(32, generator=torch.Generator(device="cuda").manual_seed(32))
    lr = make_learner(args, impl)
    torch.cuda.synchronize()
    t0 = time.time()
    lr.learn(batch)
    torch.cuda.synchronize()
    first = time.time() - t0
    t0 = time.time()
    lr.learn(batch)
    torch.cuda.synchronize()
    print(json.dumps(dict(first_learn_s=round(first, 3), second_learn_s=round(time.time() - t0, 4))))


def trace_workload(seed):
    import torch
    args, ring = ring_of(3, 32, seed)
    for fmt in ("map_once", "dense"):
        from cooperative_search_amd.replay import expand_compact
        c = ring.sample(32, generator=torch.Generator(device="cuda").manual_seed(32))
        batch = c if fmt == "map_once" else expand_compact(c, 3, 3)
        lr = make_learner(args, "hip")
        for _ in range(5):
            lr.learn(batch)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=[32, 256])
    ap.add_argument("--teams", type=int, nargs="*", default=[3, 5])
    ap.add_argument("--counts", type=int, nargs="*", default=[6400, 51200])
    ap.add_argument("--live-seed", type=int, default=12, help="weights' seed: 12 gives a live front end (DESIGN.md section 13)")
    ap.add_argument("--torch-only", action="store_true")
    ap.add_argument("--no-first-learn", action="store_true")
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--first-learn", choices=["torch", "hip"], help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("conv_learn_bench needs the GPU: nothing here is measured without one")
    if a.first_learn:
        return first_learn(a.first_learn, a.live_seed)
    if a.trace_workload:
        return trace_workload(a.live_seed)
    t0 = time.time()
    impls = ("torch",) if a.torch_only else ("torch", "hip")
    doc = dict(tool="conv_learn_bench", device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats,
               miopen_find_mode=os.environ.get("MIOPEN_FIND_MODE", "default"), weights_seed=a.live_seed,
               timer="HIP events around one call; median, min, max, spread = max - min of the repeats; implementations alternate")
    if not a.no_first_learn:   # children first: this process has not touched the device's caches for them
        doc["first_learn"] = {}
        for impl in impls:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-learn", impl, "--live-seed", str(a.live_seed)],
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"first-learn child ({impl}) failed:\n{r.stderr[-2000:]}")
            doc["first_learn"][impl] = json.loads(r.stdout.strip().splitlines()[-1])
            print(f"first learn {impl}: {doc['first_learn'][impl]}", file=sys.stderr, flush=True)
    doc["op"] = op_points(impls, a.counts, a.warmup, a.repeats, a.live_seed)
    doc["teams"] = [learn_points(n, impls, a.sizes, a.warmup, a.repeats, a.live_seed) for n in a.teams]
    doc["wall_s"] = round(time.time() - t0, 1)
    if a.out:   # the file holds a list of runs: one per MIOpen find mode / set of sizes
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        runs = json.load(open(a.out))["runs"] if os.path.exists(a.out) else []
        json.dump(dict(tool="conv_learn_bench", runs=runs + [doc]), open(a.out, "w"), indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
