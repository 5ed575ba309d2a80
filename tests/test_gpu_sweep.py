"""GPU tests of the sweep kernel (cs_sweep_episodes, csrc/sweep.h): it equals the definition (sweep.sweep_episodes_torch) in
every element of first, new_cells and seen_cells, and sweep_batch / collect_sweep_data work on what a real collector records.
Everything is torch.equal on integers: no tolerance."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import sweep as sw
from test_gpu_compact import flight, fused_agents

pytestmark = pytest.mark.gpu
NAMES = ("first", "new_cells", "seen_cells")


def random_table(E, T1, n, g, k=0, tail=45):
    """(states float32 [E, T1, 4n + tail], counts int32 [E]): positions uniform over the map with exactly -1 and exactly +1 among
    them, counts drawn from 0..T1 with T1, then 0 and 1 (swapped for odd k) forced in, as many as E allows, the rows at and past each count
    filled with NaN and 1e30 in turn.  4n + 45 floats per row: rows are not 16-byte aligned."""
    states = torch.rand(E, T1, 4 * n + tail, generator=g) * 2 - 1
    pos = torch.rand(E, T1, n, 2, generator=g) * 2 - 1
    edge = torch.randint(0, 6, pos.shape, generator=g)
    pos = torch.where(edge == 0, -torch.ones_like(pos), torch.where(edge == 1, torch.ones_like(pos), pos))
    pos[0, 0, 0, 0], pos[0, 0, 0, 1] = -1.0, 1.0
    ag = states[..., :4 * n].reshape(E, T1, n, 4).clone()
    ag[..., :2] = pos
    states[..., :4 * n] = ag.reshape(E, T1, 4 * n)
    counts = torch.randint(0, T1 + 1, (E,), generator=g, dtype=torch.int32)
    forced = [T1, k % 2, 1 - k % 2]
    for e in range(min(E, 3)):
        counts[e] = forced[e]
    for e in range(E):
        c = int(counts[e])
        states[e, c::2] = float("nan")
        states[e, c + 1::2] = 1e30
    return states.contiguous(), counts


def explain(got, want, what, side):
    """pytest.fail naming the first differing episode and row or cell."""
    for name, g, w in zip(NAMES, got, want):
        g = g.cpu()
        if not torch.equal(g, w):
            bad = (g != w).nonzero()
            e, j = bad[0].tolist()
            where = f"cell ({j // side}, {j % side})" if name == "first" else f"row {j}"
            pytest.fail(f"{what}: {len(bad)} elements of {name} differ, first episode {e} {where}: kernel {int(g[e, j])}, "
                        f"definition {int(w[e, j])}")


def compare(states, counts, n, side, vr, what):
    want = sw.sweep_episodes_torch(states, counts, n, side, vr)
    got = cs.sweep_episodes(states.cuda(), counts.cuda(), n, side, vr)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in got)
    explain(got, want, what, side)
    return want


# ---- 1. the kernel equals the definition ------------------------------------------------------------------------------------

@pytest.mark.parametrize("vr", [0, 1, 7, 20])
@pytest.mark.parametrize("E, T1, n, side", [(1, 1, 1, 50), (3, 5, 3, 50), (65, 33, 5, 50), (7, 12, 8, 64), (5, 9, 2, 7), (2, 201, 3, 50)])
def test_kernel_equals_the_definition(E, T1, n, side, vr):
    """One row and one episode; fewer rows than a chunk; more than one block's worth of episodes; the widest team on the largest
    map (16 cells per thread); 49 cells (fewer than the block has threads); 201 rows (three chunks and a part of a fourth)."""
    g = torch.Generator().manual_seed(100000 * E + 1000 * T1 + 100 * n + side + vr)
    states, counts = random_table(E, T1, n, g, k=vr)
    want = compare(states, counts, n, side, vr, f"E {E}, T1 {T1}, n {n}, side {side}, view_range {vr}")
    if vr == 20 and E > 2:
        assert int(want.new_cells.sum()) > 0


def test_counts_outside_the_table_are_clamped_and_an_exact_centre_is_swept_at_view_range_zero():
    g = torch.Generator().manual_seed(3)
    states, counts = random_table(6, 70, 2, g)
    counts[3], counts[4], counts[5] = -5, 71, 2 ** 31 - 1
    states[3:] = torch.rand(3, 70, states.shape[2], generator=g) * 2 - 1   # (their rows are all valid or all invalid)
    compare(states, counts, 2, 50, 7, "clamped counts")
    # view_range 0: only a cell on whose centre (16 i + 8) an agent stands exactly
    onc = torch.zeros(1, 3, 8 + 45)
    onc[0, :, 0] = torch.tensor([-0.5, 0.5, 0.02])    # X = 200, 600, 408: the centres of cells 12, 37 and 25
    onc[0, :, 1] = torch.tensor([-0.5, 0.5, 0.02])
    onc[0, :, 4:6] = 5.0                               # the second agent is far off the map
    want = compare(onc, torch.tensor([3], dtype=torch.int32), 2, 50, 0, "view_range 0")
    assert want.seen_cells.tolist() == [[1, 1, 1]] and want.new_cells.tolist() == [[1, 1, 1]]


def test_outputs_filled_with_garbage_are_fully_overwritten():
    E, T1, n, side = 5, 70, 3, 50
    states, counts = random_table(E, T1, n, torch.Generator().manual_seed(8))
    want = sw.sweep_episodes_torch(states, counts, n, side, 7)
    outs = [torch.full((E, side * side), -7, dtype=torch.int32, device="cuda"), torch.full((E, T1), 12345, dtype=torch.int32, device="cuda"),
            torch.full((E, T1), -2 ** 31, dtype=torch.int32, device="cuda")]
    _lib.torch_ops().sweep_episodes(states.cuda(), counts.cuda(), *outs, n, side, 7)
    explain(outs, want, "garbage in the outputs", side)


# ---- 2. episode batches of a real collector -----------------------------------------------------------------------------------

def test_sweep_batch_on_a_dense_and_on_a_map_once_batch_of_a_coverage_run():
    """flight_easy, B = 8, 3 agents, the coverage policy: its episodes end early, so the counts differ."""
    B = 8
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=3), batch=B, seeds=np.arange(B, dtype=np.uint32) + 77)
    dense, *_ = cs.EpisodeCollector(env).generate_episodes(policy=cs.CoverageAgents(env).policy(), init=True)
    steps = (1 - dense["padded"]).sum(1).view(-1)
    assert len(set(steps.tolist())) > 1 and float(steps.min()) < env.time_limit
    twin = cs.compact_from_dense(dense)
    a, b = cs.sweep_batch(dense, env), cs.sweep_batch(twin, env)
    want = cs.sweep_batch({k: v.cpu() for k, v in dense.items()}, env, impl="torch")
    explain(a, want, "dense batch", env.map_size)
    explain(b, want, "map-once batch", env.map_size)
    assert a.new_cells.shape == (B, env.time_limit + 1) and a.new_cells[:, 0].tolist() == [156] * B
    bonus = cs.sweep_bonus(dense, env, 0.5)
    assert bonus.shape == (B, env.time_limit, 1) and torch.equal(bonus.view(B, -1), a.new_cells[:, 1:].float() * 0.5)
    assert not bool((bonus * dense["padded"]).any())
    out = cs.with_sweep_bonus(dense, env, 0.5)
    assert torch.equal(out["r"], dense["r"] + bonus) and out["s"] is dense["s"]


def test_sweep_batch_on_the_collectors_two_formats_of_one_flight_run():
    """The flight variant with the shipped QMIX checkpoint: generate_episodes(compact=True) and compact=False from the same
    seeds record the same episodes, and their sweeps are identical and equal the definition's."""
    B, res = 8, []
    for compact in (False, True):
        args, env = flight(3, B, time_limit=40)
        batch, *_ = cs.EpisodeCollector(env).generate_episodes(agents=fused_agents(args, B, trained=True), evaluate=True, compact=compact)
        assert ("s_full" in batch) == compact
        res.append(cs.sweep_batch(batch, args))
    want = cs.sweep_batch({k: v.cpu() for k, v in batch.items()}, args, impl="torch")
    explain(res[0], want, "dense flight batch", args.map_size)
    explain(res[1], want, "map-once flight batch", args.map_size)


def test_coverage_sweeps_more_of_the_map_than_random():
    """collect_sweep_data, 256 envs, one batch, 3 agents: percent of the map swept by row 60, both measured here on the same env."""
    B = 256
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=3), batch=B, seeds=np.arange(B, dtype=np.uint32) + 300)
    col = cs.EpisodeCollector(env)
    cov = cs.collect_sweep_data(col, cs.CoverageAgents(env).policy(), batches=1)
    rnd = cs.collect_sweep_data(col, cs.random_policy(torch.Generator(device="cuda").manual_seed(3)), batches=1)
    print(f"percent of the map swept by row 60 / 200: coverage {cov['curve'][60]:.2f} / {cov['curve'][200]:.2f}, random "
          f"{rnd['curve'][60]:.2f} / {rnd['curve'][200]:.2f}; efficiency {cov['efficiency']:.3f} / {rnd['efficiency']:.3f}; "
          f"targets {cov['targets_find']:.2f} / {rnd['targets_find']:.2f}; steps {cov['steps']:.1f} / {rnd['steps']:.1f}")
    assert cov["curve"].shape == (env.time_limit + 1,) and cov["curve"].dtype == np.float64 and cov["episodes"] == B
    assert cov["curve"][60] > rnd["curve"][60]
    assert 0 < rnd["efficiency"] < 1 and 0 < cov["steps"] <= env.time_limit and 0 < cov["targets_find"] <= env.target_num


# ---- 3. refusals and synchronisation ----------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    E, T1, n, side = 4, 6, 3, 50
    ops = _lib.torch_ops()
    states, counts = (t.cuda() for t in random_table(E, T1, n, torch.Generator().manual_seed(2)))
    first = torch.full((E, side * side), 1234, dtype=torch.int32, device="cuda")
    new = torch.full((E, T1), -7, dtype=torch.int32, device="cuda")
    seen = torch.full((E, T1), -9, dtype=torch.int32, device="cuda")
    bad = [dict(states=states.to(torch.float64)), dict(states=states[:, :, :4 * n - 1].contiguous()), dict(states=states[:-1].contiguous()),
           dict(states=states[:, :, :-1]), dict(states=states.cpu()), dict(states=states[0]),
           dict(counts=counts.to(torch.int64)), dict(counts=counts[:-1].contiguous()), dict(counts=counts.repeat(2)[::2]),
           dict(first=first.to(torch.int64)), dict(first=first[:, :-1].contiguous()), dict(first=first.t().contiguous().t()),
           dict(new=new.to(torch.int16)), dict(new=new[:, :-1].contiguous()), dict(new=new.t().contiguous().t()),
           dict(seen=seen.to(torch.float32)), dict(seen=seen[:-1].contiguous()), dict(seen=seen.cpu())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.sweep_episodes(kw.get("states", states), kw.get("counts", counts), kw.get("first", first), kw.get("new", new),
                               kw.get("seen", seen), n, side, 7)
    for args in ((0, side, 7), (9, side, 7), (n, 0, 7), (n, 65, 7), (n, side, -1), (n, side, 65)):
        with pytest.raises(RuntimeError, match="sweep_episodes"):
            ops.sweep_episodes(states, counts, first, new, seen, *args)
    torch.cuda.synchronize()
    assert bool((first == 1234).all()) and bool((new == -7).all()) and bool((seen == -9).all())
    with pytest.raises(ValueError, match="not on a GPU"):
        cs.sweep_episodes(states.cpu(), counts.cpu(), n, side, 7)


def test_a_call_never_synchronises_and_runs_on_the_current_stream():
    E, T1, n, side = 16, 70, 3, 50
    states, counts = random_table(E, T1, n, torch.Generator().manual_seed(4))
    ds, dc = states.cuda(), counts.cuda()
    cs.sweep_episodes(ds, dc, n, side, 7)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            got = cs.sweep_episodes(ds, dc, n, side, 7)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    stream.synchronize()
    explain(got, sw.sweep_episodes_torch(states, counts, n, side, 7), "side stream", side)
