"""GPU tests of the coverage kernel (cs_coverage_actions, csrc/coverage.h): it equals the definition
(baseline.coverage_actions_torch) in every element of the actions and of the grid, and CoverageAgents drops into the collector.
Everything is torch.equal on integers: no tolerance."""
import math

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl

pytestmark = pytest.mark.gpu
KEEP = 6554


def random_state(B, n, g, tail=45):
    """State rows float32 [B, 4n + tail]: positions uniform over the map with exactly 0 and exactly map_size among them, headings
    drawn from the env's 36 values (float32 cosf / sinf), and a tail the policy never reads."""
    pos = torch.rand(B, n, 2, generator=g) * 2 - 1
    edge = torch.randint(0, 6, (B, n, 2), generator=g)
    pos = torch.where(edge == 0, -torch.ones_like(pos), torch.where(edge == 1, torch.ones_like(pos), pos))
    pos[0, 0, 0], pos[0, 0, 1] = -1.0, 1.0
    ang = (torch.randint(0, 36, (B, n), generator=g).to(torch.float64) * (math.pi / 18)).to(torch.float32)
    ag = torch.cat([pos, torch.cos(ang)[..., None], torch.sin(ang)[..., None]], -1).reshape(B, 4 * n)
    return torch.cat([ag, torch.rand(B, tail, generator=g)], 1).contiguous()


def random_grid(B, side, g):
    """int32 [B, side * side] in 0..65536 with both end values; every third row all zero."""
    grid = torch.randint(0, 65537, (B, side * side), generator=g, dtype=torch.int32)
    grid[:, 0], grid[:, -1] = 0, 65536
    grid[2::3] = 0
    return grid


def compare(state, grid, n, side, vr, regrow, la, misalign=False):
    want_g = grid.clone()
    want_a = bl.coverage_actions_torch(state, want_g, n, side, vr, KEEP, regrow, la)
    B = state.shape[0]
    if misalign:   # a grid whose rows are not 16-byte aligned: the one-cell-per-lane path at a side whose rows are whole 16-byte pieces
        got_g = torch.empty(B * side * side + 1, dtype=torch.int32, device="cuda")[1:].view(B, side * side)
        got_g.copy_(grid)
        assert got_g.data_ptr() % 16 != 0 and got_g.is_contiguous()
    else:
        got_g = grid.cuda()
    got_a = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
    _lib.torch_ops().coverage_actions(state.cuda(), got_g, got_a, n, side, vr, KEEP, regrow, la)
    what = f"view_range {vr}, lookahead {la}, regrow {regrow}, misaligned {misalign}"
    if not torch.equal(got_g.cpu(), want_g):
        bad = (got_g.cpu() != want_g).nonzero()
        b, c = bad[0].tolist()
        pytest.fail(f"{what}: {len(bad)} grid cells differ, first env {b} cell ({c // side}, {c % side}): kernel {int(got_g[b, c])}, "
                    f"definition {int(want_g[b, c])}")
    if not torch.equal(got_a.cpu(), want_a):
        bad = (got_a.cpu() != want_a).nonzero()
        b, i = bad[0].tolist()
        pytest.fail(f"{what}: {len(bad)} actions differ, first env {b} agent {i}: kernel {int(got_a[b, i])}, definition {int(want_a[b, i])}")
    return want_a


# ---- 1. the kernel equals the definition ------------------------------------------------------------------------------------

@pytest.mark.parametrize("B, n, side", [(1, 1, 50), (3, 3, 50), (65, 5, 50), (7, 8, 64), (5, 2, 7)])
def test_kernel_equals_the_definition(B, n, side):
    """view_range 1, 7 and 20 (at 20 a footprint's box holds up to 41 x 41 cells, more than the block has threads) by lookahead
    0, 7 and 30 (those that fit the map), regrow 1 and 8 in turn; random grids, and one fresh grid per shape so that ties occur.
    Side 50 and 64 take the 16-byte path, side 7 (49 cells) one cell per lane."""
    g = torch.Generator().manual_seed(1000 * B + 10 * n + side)
    k = 0
    for vr in (1, 7, 20):
        for la in (0, 7, 30):
            if la > side:
                continue
            state, regrow = random_state(B, n, g), (1, 8)[k % 2]
            compare(state, random_grid(B, side, g), n, side, vr, regrow, la)
            k += 1
    fresh = torch.full((B, side * side), 65536, dtype=torch.int32)
    a = compare(random_state(B, n, g), fresh, n, side, 7, 8, min(7, side))
    assert bool(((a >= 0) & (a <= 2)).all())


def test_kernel_equals_the_definition_on_ties_walls_and_unaligned_rows():
    g = torch.Generator().manual_seed(5)
    side, n = 50, 3
    # lookahead 0: the three scores of every agent tie exactly, the lowest action wins
    state = random_state(6, n, g)
    a = compare(state, torch.full((6, side * side), 65536, dtype=torch.int32), n, side, 7, 8, 0)
    assert not bool(a[:, 0].any())
    # lookahead = map_size from the corners and walls, every heading: the look-ahead point clamps
    pts = [(-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0), (0.0, -1.0), (0.0, 1.0), (-1.0, 0.0), (1.0, 0.0)]
    rows = []
    for x, y in pts:
        for h in range(36):
            ang = torch.tensor(h * math.pi / 18, dtype=torch.float64).to(torch.float32)
            rows.append([x, y, float(torch.cos(ang)), float(torch.sin(ang))] * n + [0.0] * 45)
    walls = torch.tensor(rows, dtype=torch.float32)
    compare(walls, random_grid(len(rows), side, g), n, side, 7, 8, side)
    compare(walls, random_grid(len(rows), side, g), n, side, 20, 1, side)
    # rows that are not 16-byte aligned
    compare(random_state(5, n, g), random_grid(5, side, g), n, side, 7, 8, 7, misalign=True)
    # rows no env emits: NaN, infinities and huge values are clamped the same way on both sides
    odd = random_state(4, n, g)
    odd[0, 0], odd[1, 1], odd[2, 2], odd[3, 3], odd[3, 4] = float("nan"), float("inf"), float("nan"), -1e30, 1e30
    compare(odd, random_grid(4, side, g), n, side, 7, 8, 7)
    # cells outside 0..65536 are read as the nearer bound on both sides
    wild = torch.randint(-200000, 200000, (4, side * side), generator=g, dtype=torch.int32)
    wild[0, :3] = torch.tensor([-2 ** 31, 2 ** 31 - 1, 65537], dtype=torch.int32)
    compare(random_state(4, n, g), wild, n, side, 7, 8, 7)
    compare(random_state(4, n, g), wild, n, side, 7, 1, 7, misalign=True)


# ---- 2. closed loop through the collector -----------------------------------------------------------------------------------

def collect(variant, B, impl, seeds, calls=1):
    env = cs.BatchedFlightEnv(cs.make_env_args(variant, n_agents=3), batch=B, seeds=seeds)
    ag = cs.CoverageAgents(env, impl=impl)
    out = []
    for _ in range(calls):
        env.seed(seeds)
        episode, reward, win, found = cs.EpisodeCollector(env).generate_episodes(policy=ag.policy(), init=True)
        out.append((episode, found.clone(), ag.grid.clone()))
    return out


@pytest.mark.parametrize("variant, B", [("flight_easy", 33), ("flight", 9)])
def test_closed_loop_kernel_and_definition_fly_the_same_episodes(variant, B):
    """flight's observations are wide (the map); the policy never reads them."""
    seeds = np.arange(B, dtype=np.uint32) + 77
    (ep_h, found_h, grid_h), = collect(variant, B, "hip", seeds)
    (ep_t, found_t, grid_t), = collect(variant, B, "torch", seeds)
    assert ep_h["u"].shape == (B, 200, 3, 1)
    assert torch.equal(ep_h["u"], ep_t["u"]) and torch.equal(grid_h, grid_t) and torch.equal(found_h, found_t)
    assert torch.equal(ep_h["s"], ep_t["s"]) and torch.equal(ep_h["padded"], ep_t["padded"])


def test_the_grid_resets_at_step_zero_and_reruns_are_bit_identical():
    B = 33
    seeds = np.arange(B, dtype=np.uint32) + 5
    (e0, f0, g0), (e1, f1, g1) = collect("flight_easy", B, "hip", seeds, calls=2)
    (e2, f2, g2), = collect("flight_easy", B, "hip", seeds)
    for k in e0:
        assert torch.equal(e0[k], e1[k]) and torch.equal(e0[k], e2[k]), k
    assert torch.equal(g0, g1) and torch.equal(g0, g2) and torch.equal(f0, f1)


def test_coverage_finds_more_than_random():
    """collect_experiment_data, 256 envs, one batch, 3 agents: percent of targets found by step 60 and by step 200, both measured
    here on the same env."""
    B = 256
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=3), batch=B, seeds=np.arange(B, dtype=np.uint32) + 300)
    cov = cs.collect_experiment_data(env, cs.CoverageAgents(env).policy(), batches=1)
    rnd = cs.collect_experiment_data(env, cs.random_policy(torch.Generator(device="cuda").manual_seed(3)), batches=1)
    print(f"percent found by step 60 / 200: coverage {cov[59]:.2f} / {cov[199]:.2f}, random {rnd[59]:.2f} / {rnd[199]:.2f}")
    assert cov[59] > rnd[59] and cov[199] > rnd[199]


# ---- 3. refusals and synchronisation ----------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops = _lib.torch_ops()
    state = random_state(B, n, torch.Generator().manual_seed(2)).cuda()
    grid = torch.full((B, side * side), 1234, dtype=torch.int32, device="cuda")
    actions = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
    bad = [dict(grid=grid.to(torch.int64)), dict(grid=grid[:, :-1].contiguous()), dict(grid=grid[:-1].contiguous()),
           dict(grid=grid.t().contiguous().t()), dict(state=state.to(torch.float64)), dict(state=state[:, :4 * n - 1].contiguous()),
           dict(state=state[:-1].contiguous()), dict(state=state.cpu()), dict(actions=actions.to(torch.int32)),
           dict(actions=actions[:, :2].contiguous())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.coverage_actions(kw.get("state", state), kw.get("grid", grid), kw.get("actions", actions), n, side, 7, KEEP, 8, 7)
    for args in ((9, side, 7, KEEP, 8, 7), (n, 65, 7, KEEP, 8, 7), (n, side, 65, KEEP, 8, 7), (n, side, 7, 65537, 8, 7), (n, side, 7, KEEP, 0, 7),
                 (n, side, 7, KEEP, 8, side + 1)):
        with pytest.raises(RuntimeError, match="coverage_actions"):
            ops.coverage_actions(state, grid, actions, *args)
    assert bool((grid == 1234).all()) and bool((actions == -7).all())
    ag = cs.CoverageAgents(cs.make_env_args("flight_easy"), batch=B, device="cuda")
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state.to(torch.float64))
    ag.grid = ag.grid.to(torch.int64)
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state)
    with pytest.raises(ValueError, match="not a GPU"):
        cs.CoverageAgents(cs.make_env_args("flight_easy"), batch=B, device="cpu")


def test_a_call_never_synchronises_and_runs_on_the_current_stream():
    B, n = 16, 3
    state = random_state(B, n, torch.Generator().manual_seed(4)).cuda()
    ag = cs.CoverageAgents(cs.make_env_args("flight_easy"), batch=B, device="cuda")
    ag.choose_action(state)
    ag.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            a = ag.choose_action(state)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    want_g = torch.full((B, 2500), 65536, dtype=torch.int32)
    want_a = bl.coverage_actions_torch(state.cpu(), want_g, n, 50, 7, KEEP, 8, 7)
    assert torch.equal(a.cpu(), want_a) and torch.equal(ag.grid.cpu(), want_g)
