"""The N > 1 path on CPU: 2-rank gloo process group exercising the sharding helpers and the metric all-gather
(the path's only collective).  The env kernels themselves need a GPU and are covered by the shard-invariance test in
test_gpu_parity.py; here each rank fabricates the per-env counters of its shard deterministically from the global
env index, so the reduced result must not depend on the sharding."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cooperative_search_amd import dist as csd


def fake_counters(offset, count):
    g = np.arange(offset, offset + count, dtype=np.int64)
    total_reward = (g * 7919) % 400 - 300
    target_find = (g * 31) % 16
    win = (target_find == 15).astype(np.int64)
    return total_reward, win, target_find


def _worker(rank, world, port, B, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        off, cnt = csd.shard(B, rank, world)
        tr, win, tf = fake_counters(off, cnt)
        part = torch.tensor([tr.sum(), win.sum(), tf.sum(), cnt], dtype=torch.float64)
        m = csd.reduce_metrics(part)
        curve = csd.FoundCurve(200, 15, "cpu")
        for t in range(200):
            curve.add_step(t, torch.from_numpy(np.minimum(tf, t // 10)))
        curve.end_episodes(cnt)
        res = curve.result()
        seeds = csd.seeds_for(off, cnt)
        if rank == 0:
            torch.save({"metrics": m, "curve": res, "seeds0": seeds[:4].tolist()}, out)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("B", [4096, 1001])
def test_two_rank_gloo_metric_reduction_is_shard_invariant(tmp_path, B):
    out = str(tmp_path / "r0.pt")
    mp.spawn(_worker, args=(2, _free_port(), B, out), nprocs=2, join=True)
    got = torch.load(out, weights_only=False)
    tr, win, tf = fake_counters(0, B)
    assert got["metrics"]["episodes"] == B
    assert got["metrics"]["episode_reward"] == pytest.approx(tr.mean(), abs=1e-12)
    assert got["metrics"]["win_rate"] == pytest.approx(win.mean(), abs=1e-12)
    assert got["metrics"]["targets_find"] == pytest.approx(tf.mean(), abs=1e-12)
    want = np.array([np.minimum(tf, t // 10).mean() / 15 * 100 for t in range(200)])
    np.testing.assert_allclose(got["curve"], want, rtol=0, atol=1e-9)
    assert got["seeds0"] == [20240000, 20240001, 20240002, 20240003]


def test_shard_covers_batch_exactly():
    for B in (1, 7, 64, 4096, 65536, 1001):
        for world in (1, 2, 3, 8):
            spans = [csd.shard(B, r, world) for r in range(world)]
            assert spans[0][0] == 0 and sum(c for _, c in spans) == B
            for (o0, c0), (o1, _) in zip(spans, spans[1:]):
                assert o0 + c0 == o1
            assert max(c for _, c in spans) - min(c for _, c in spans) <= 1


def test_all_gather_sum_is_identity_without_process_group():
    x = torch.arange(5, dtype=torch.float64)
    assert torch.equal(csd.all_gather_sum(x), x)


def _run_bench(args, env_extra=None, timeout=300):
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None)


def test_bench_gpus_flag_spawns_that_many_ranks():
    """`bench.py --gpus 2` outside torchrun must start two rank processes itself: the dry-run ranks
    all-gather their shard's env count over gloo, so the line proves the process group had two members."""
    p, line = _run_bench(["--gpus", "2", "--dry-run", "--steps", "20", "--warmup", "5"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len([ln for ln in p.stdout.splitlines() if ln.startswith("{")]) == 1   # rank 0's line only
    assert line["n_gpus"] == 2 and line["eval"]["envs"] == 2 * 4096 and line["eval"]["world_size"] == 2
    assert line["steps"] == 20 and line["warmup"] == 5
    # a plain run measures the headline only: no all-gather timing, no secondary workloads (those are --full's)
    assert line["eval"]["allgather_us"] is None and "c5_strong_total" not in line and "also_at_this_n" not in line


def test_bench_line_is_compact_whatever_the_record_holds():
    """the stdout line never exceeds 6000 characters.  compact_line() on the 21.8 KB record of round 5 (17
    secondary workloads with a roofline object each, the CPU baseline's whole calibration) keeps every contract field, turns
    the secondary workloads into [value, fraction] pairs and cuts cpu_baseline to six fields; a record that is too big even
    then loses optional blocks, never the headline; the dry-run line goes through the same ceiling."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod4", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    full = json.load(open(os.path.join(root, "profiles", "r05_bench_driver_args.json")))
    assert len(json.dumps(full)) > 20000
    for i, ent in enumerate(full["also"]):
        ent["key"] = f"workload_{i:02d}"
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    text = json.dumps(line)
    assert len(text) < 4000 < bench.MAX_LINE <= 6000 and json.loads((" " * 9000 + text)[-8000:]) == line
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data"):
        assert line[key] == full[key], key
    assert line["config"]["workload"] == full["config"]["workload"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert line["roofline"][key] == full["roofline"][key], key
    cb = line["cpu_baseline"]
    assert set(cb) == {"value", "unit", "cores", "kind", "single_thread_value", "sample"} and len(cb["sample"]) <= 300
    assert cb["cores"] == 14 and cb["kind"] == "port" and cb["value"] == pytest.approx(full["cpu_baseline"]["value"], rel=1e-6)
    assert len(line["also_summary"]) == 18 and line["also_summary"]["workload_03"] == [pytest.approx(5.118e9, rel=1e-3),
                                                                                        pytest.approx(0.234, abs=1e-3)]
    assert line["detail"] == "gpurun_out/bench_detail.json" and "dropped_to_fit" not in line
    # a record with 400 secondary workloads: the summary goes, the contract fields stay, the ceiling holds
    full["also"] = [dict(full["also"][0], key=f"workload_{i:03d}") for i in range(400)]
    line = bench.compact_line(full, None)
    assert len(json.dumps(line)) <= bench.MAX_LINE and line["dropped_to_fit"][0] == "also_summary"
    assert line["value"] == full["value"] and line["roofline"]["frac"] == full["roofline"]["frac"] and "cpu_baseline" in line
    with pytest.raises(RuntimeError):
        bench._fits({"x": "y" * bench.MAX_LINE})
    # sig(): six significant digits, ints / None / strings untouched
    assert bench.sig(1234567.891) == 1234570.0 and bench.sig(None) is None and bench.sig(7) == 7 and bench.sig("a") == "a"
    assert bench.sig([0.123456789, {"a": 2.0000001}]) == [0.123457, {"a": 2.0}]


def test_bench_eight_rank_control_flow():
    """The driver's 8-GPU launch, as far as a GPU-less container can take it: eight rank processes over gloo, the all-gather
    sees all eight shards, and BASELINE config 5 shows up as fields of its own (65536 envs = 8 x 8192: the strong and the
    weak point coincide at N = 8)."""
    p, line = _run_bench(["--gpus", "8", "--dry-run", "--steps", "20", "--warmup", "5", "--full"], timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(p.stdout) < 6000 and json.loads(p.stdout[-8000:]) == line   # what a consumer of the last 8 KB reads
    assert line["n_gpus"] == 8 and line["eval"]["envs"] == 8 * 4096 and line["eval"]["world_size"] == 8
    # the metric all-gather has a number of its own, every rank's rate is reported (not only the slowest's),
    # and a scaling run measures the headline + the two c5 lines only
    ag = line["eval"]["allgather_us"]
    assert ag["floats"] == 204 and ag["reps"] == 20 and 0 < ag["min"] <= ag["median"] <= ag["max"]
    pr = line["per_rank_value"]
    assert (pr["min"], pr["max"], pr["slowest_rank"]) == (1.0e9, 1.0e9 + 7, 0) and pr["min"] < pr["median"] < pr["max"]
    assert line["also_at_this_n"] == "c5 weak + c5 strong only"
    assert line["c5_strong_total"]["envs_total"] == 65536 and line["c5_strong_total"]["envs_per_gpu"] == 8192
    assert line["c5_weak_total"]["envs_total"] == 65536 and line["c5_weak_total"]["n_gpus"] == 8


def test_rank_binding_reads_the_gpu_numa_node_from_sysfs(tmp_path):
    """bench.py binds each rank to the CPUs next to its GPU BEFORE any GPU call, from sysfs alone: KFD topology nodes with
    SIMDs, in node order, are the GPUs; unreadable nodes (another container's GPUs) are skipped; the node's render minor
    leads to the device's local_cpulist.  Layout below: what an 8-GPU MI355X node shows a one-GPU container (gpurun_out/a_topology.txt)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    nodes = tmp_path / "class/kfd/kfd/topology/nodes"
    for k, (simd, minor) in enumerate([(0, 0), (0, 0), (1024, 128), (1024, 136)]):
        (nodes / str(k)).mkdir(parents=True)
        (nodes / str(k) / "properties").write_text(f"cpu_cores_count {0 if simd else 128}\nsimd_count {simd}\ndrm_render_minor {minor}\n")
    (nodes / "4").mkdir()   # a node without readable properties
    for minor, (node, cpus) in {128: (0, "0-3,8-11"), 136: (1, "4-7,12-15")}.items():
        d = tmp_path / f"class/drm/renderD{minor}/device"
        d.mkdir(parents=True)
        (d / "numa_node").write_text(f"{node}\n")
        (d / "local_cpulist").write_text(cpus + "\n")
    for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"):
        os.environ.pop(k, None)
    assert bench.parse_cpulist("0-3,8-11") == {0, 1, 2, 3, 8, 9, 10, 11}
    assert bench.gpu_local_cpus(0, str(tmp_path)) == (0, {0, 1, 2, 3, 8, 9, 10, 11})
    assert bench.gpu_local_cpus(1, str(tmp_path)) == (1, {4, 5, 6, 7, 12, 13, 14, 15})
    assert bench.gpu_local_cpus(2, str(tmp_path)) is None          # fewer GPUs than ranks: no binding, no error
    assert bench.gpu_local_cpus(0, str(tmp_path / "nowhere")) is None
    # device filters renumber (a gpurun box exports ROCR_VISIBLE_DEVICES=0 and HIP_VISIBLE_DEVICES=0)
    try:
        os.environ["ROCR_VISIBLE_DEVICES"] = "0"
        os.environ["HIP_VISIBLE_DEVICES"] = "0"
        assert bench.gpu_local_cpus(0, str(tmp_path))[0] == 0 and bench.gpu_local_cpus(1, str(tmp_path)) is None
        os.environ["ROCR_VISIBLE_DEVICES"] = "1,0"
        assert bench.gpu_local_cpus(0, str(tmp_path))[0] == 1
        os.environ["HIP_VISIBLE_DEVICES"] = "1"
        assert bench.gpu_local_cpus(0, str(tmp_path))[0] == 0
        os.environ["HIP_VISIBLE_DEVICES"] = "GPU-1234abcd"
        assert bench.gpu_local_cpus(0, str(tmp_path)) is None      # not a list of indices: no guess
    finally:
        for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
            os.environ.pop(k, None)
    before = os.sched_getaffinity(0)
    try:
        got = bench.bind_rank_to_gpu_node(0, str(tmp_path))
        want = {0, 1, 2, 3, 8, 9, 10, 11} & before
        if want:
            assert got["numa_node"] == 0 and os.sched_getaffinity(0) == want
        else:
            assert got is None
    finally:
        os.sched_setaffinity(0, before)


def test_rank_binding_falls_back_to_the_pci_address_and_the_kfd_io_link(tmp_path):
    """What a gpurun box shows (gpurun_out/a_topology.txt): the container's GPU is KFD node 3 with render minor 136, but
    /sys/class/drm lists renderD128..135 only -- the lookup by minor finds nothing.  Second source: the PCI device by the
    node's domain / location_id; third: the GPU's io_link to a CPU node, whose number is the NUMA node's."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "GPU_DEVICE_ORDINAL"):
        os.environ.pop(k, None)

    def tree(base, with_pci, with_link):
        nodes = base / "class/kfd/kfd/topology/nodes"
        for k in (0, 1):
            (nodes / str(k)).mkdir(parents=True)
            (nodes / str(k) / "properties").write_text("cpu_cores_count 128\nsimd_count 0\ndrm_render_minor 0\n")
        (nodes / "2").mkdir()    # somebody else's GPU: unreadable
        (nodes / "3").mkdir()
        (nodes / "3" / "properties").write_text("cpu_cores_count 0\nsimd_count 1024\nlocation_id 3328\ndomain 0\ndrm_render_minor 136\n")
        if with_pci:
            d = base / "bus/pci/devices/0000:0d:00.0"
            d.mkdir(parents=True)
            (d / "numa_node").write_text("1\n")
            (d / "local_cpulist").write_text("64-127,192-255\n")
        if with_link:
            ln = nodes / "3" / "io_links" / "0"
            ln.mkdir(parents=True)
            (ln / "properties").write_text("type 2\nnode_from 3\nnode_to 1\n")
            nd = base / "devices/system/node/node1"
            nd.mkdir(parents=True)
            (nd / "cpulist").write_text("64-127,192-255\n")

    want = (1, set(range(64, 128)) | set(range(192, 256)))
    for name, pci, link in (("pci", True, False), ("link", False, True), ("both", True, True)):
        base = tmp_path / name
        tree(base, pci, link)
        assert bench.gpu_local_cpus(0, str(base)) == want, name
    base = tmp_path / "neither"
    tree(base, False, False)
    assert bench.gpu_local_cpus(0, str(base)) is None


def test_cpu_baseline_child_reports_a_steady_point_under_the_cgroup_quota(tmp_path, monkeypatch):
    """the CPU baseline runs in its own pinned process, never with more threads than the container's CPU quota
    (the GPU boxes show 256 logical CPUs and grant 16), and `value` is the median region rate of the fastest thread count whose
    regions hold together, with every measured point listed."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    q = bench.cpu_quota()
    assert q is None or q > 0
    import builtins
    real_open = builtins.open

    def fake_open(path, *a, **k):
        if path == "/sys/fs/cgroup/cpu.max":
            return real_open(tmp_path / "cpu.max", *a, **k)
        return real_open(path, *a, **k)

    (tmp_path / "cpu.max").write_text("1600000 100000\n")
    monkeypatch.setattr(builtins, "open", fake_open)
    assert bench.cpu_quota() == 16.0
    (tmp_path / "cpu.max").write_text("max 100000\n")
    assert bench.cpu_quota() is None
    monkeypatch.undo()
    p, line = _run_bench(["--cpu-baseline-child", "flight_easy,3,512,0.6"],
                         env_extra={"OMP_PROC_BIND": "close", "OMP_PLACES": "cores", "OMP_DYNAMIC": "false"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert line["kind"] == "port" and line["unit"] == "env-steps/s" and line["value"] > 0
    assert str(line["cores"]) in line["measured_points"] and line["cores"] <= line["pinning"]["physical_cores"]
    p10, med, p90 = line["region_rate_p10_median_p90"]
    assert p10 <= med <= p90 and med == line["value"] and abs(line["p90_over_p10"] - p90 / p10) < 1e-9
    assert line["steady"] == (line["p90_over_p10"] < bench.STEADY_SPAN) or not line["steady"]
    assert line["pinning"]["OMP_PROC_BIND"] == "close" and line["pinning"]["OMP_PLACES"] == "cores"


def test_bench_launcher_propagates_rank_failure():
    """No GPU in this container: the real (non-dry) ranks must fail loudly and the launcher must return non-zero
    without printing a result line."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a GPU-less host")
    p, line = _run_bench(["--gpus", "2", "--steps", "20", "--warmup", "5"])
    assert p.returncode != 0 and line is None
    assert "needs an MI355X" in p.stderr


def test_bench_rejects_world_size_mismatch():
    p, line = _run_bench(["--gpus", "2", "--dry-run"], env_extra={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and line is None and "WORLD_SIZE=1" in p.stderr


def test_bench_options_and_output_sample():
    """A plain run has no process group at N = 1 unless asked for; --full tries one (--pg auto).  --dump-outputs: every env
    while the arrays fit in DUMP_MAX_BYTES, else the same fixed, seeded sample of envs for every array, as float32 (the
    env indices as float64)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod5", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.parse_args([]).pg == "off" and not bench.parse_args([]).full and bench.parse_args([]).dump_outputs is None
    assert bench.parse_args(["--full"]).pg == "auto" and bench.parse_args(["--full", "--pg", "off"]).pg == "off"
    assert bench.parse_args(["--force-pg"]).pg == "on" and bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    B = 64
    small = {"reward": torch.arange(B, dtype=torch.float32), "terminated": torch.arange(B, dtype=torch.uint8) % 2 == 1,
             "obs": torch.arange(B * 12, dtype=torch.float32).reshape(B, 3, 4)}
    got = bench.output_sample(small, B)
    assert got["env_index"].dtype == np.float64 and np.array_equal(got["env_index"], np.arange(B))
    assert got["terminated"].dtype == np.float32 and np.array_equal(got["terminated"], np.arange(B) % 2)
    assert np.array_equal(got["obs"], small["obs"].numpy())
    # a batch too big for the ceiling: flight-width obs rows (3 x 2504 floats per env)
    B = 8192
    big = {"reward": torch.arange(B, dtype=torch.float32), "obs": torch.zeros(B, 3, 2504).add_(torch.arange(B).view(B, 1, 1))}
    a, b = bench.output_sample(big, B), bench.output_sample(big, B)
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES < 64e6
    idx = a["env_index"]
    assert 1000 < len(idx) < B and np.array_equal(idx, b["env_index"]) and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["reward"], idx) and np.array_equal(a["obs"][:, 2, 7], idx)
