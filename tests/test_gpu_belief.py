"""GPU tests of the belief kernel (cs_belief_actions, csrc/belief.h): it equals the definition (belief.belief_actions_torch) in
every element of the grid, of the stored positions and of the actions, and BeliefAgents drops into the collector on a
MovingTargetEnv.  Everything is torch.equal on integers: no tolerance."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import belief as be
from cooperative_search_amd import motion as mo

pytestmark = pytest.mark.gpu
KEEP, VR = 6554, 7
CAP = be.CAP


def env_state(B, n, steps=3):
    """get_state() rows float32 [B, 4n + 45] of a flight_easy env after a few random steps, on the CPU."""
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=np.arange(B, dtype=np.uint32) + 11 * n)
    g = torch.Generator().manual_seed(B + n)
    for _ in range(steps):
        env.step(torch.randint(0, 3, (B, n), generator=g).cuda())
    return env.get_state().cpu().contiguous()


def make_grid(B, side, g, k):
    """int32 [B, side * side]; env b holds kind (b + k) % 5: 0 random in 0..CAP with zeros, 1 random in 0..65536 with most cells
    zero, 2 cells outside 0..CAP, 3 all mass in one cell, 4 a full-CAP map (the overflow bound)."""
    cells = side * side
    grid = torch.empty(B, cells, dtype=torch.int32)
    for b in range(B):
        kind = (b + k) % 5
        if kind == 0:
            row = torch.randint(0, CAP + 1, (cells,), generator=g, dtype=torch.int32)
            row[torch.rand(cells, generator=g) < 0.2] = 0
            row[0], row[-1] = 0, CAP
        elif kind == 1:
            row = torch.randint(0, 65537, (cells,), generator=g, dtype=torch.int32)
            row[torch.rand(cells, generator=g) < 0.9] = 0
        elif kind == 2:
            row = torch.randint(-(1 << 21), 1 << 21, (cells,), generator=g, dtype=torch.int32)
            row[:3] = torch.tensor([-2 ** 31, 2 ** 31 - 1, CAP + 1], dtype=torch.int32)[:min(3, cells)]
        elif kind == 3:
            row = torch.zeros(cells, dtype=torch.int32)
            row[int(torch.randint(0, cells, (1,), generator=g))] = CAP
        else:
            row = torch.full((cells,), CAP, dtype=torch.int32)
        grid[b] = row
    return grid


def make_prev(B, side, g):
    """int32 [B, 8, 2]: on the map, off it (beyond the +-2^15 clamp too), exactly on a cell centre."""
    prev = torch.randint(0, 16 * side + 1, (B, 8, 2), generator=g, dtype=torch.int32)
    off = torch.randint(-40000, 40000, (B, 8, 2), generator=g, dtype=torch.int32)
    prev = torch.where(torch.rand(B, 8, 1, generator=g) < 0.25, off, prev)
    prev[0, 0] = torch.tensor([16 * (side // 2) + 8, 16 * (side // 3) + 8], dtype=torch.int32)
    if B > 1:
        prev[1, 0] = torch.tensor([2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    return prev


def compare(state, grid, prev, n, side, model, moved, vr=VR, la=None, misalign=False):
    la = min(vr, side) if la is None else la
    want_g, want_p = grid.clone(), prev.clone()
    want_a = be.belief_actions_torch(state, want_g, want_p, n, side, vr, KEEP, model, moved, la)
    B = state.shape[0]
    if misalign:   # rows that are not 16-byte aligned: one cell per lane at a side whose rows are whole 16-byte pieces
        got_g = torch.empty(B * side * side + 1, dtype=torch.int32, device="cuda")[1:].view(B, side * side)
        got_g.copy_(grid)
        assert got_g.data_ptr() % 16 != 0 and got_g.is_contiguous()
    else:
        got_g = grid.cuda()
    got_p = prev.cuda()
    got_a = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
    _lib.torch_ops().belief_actions(state.cuda(), got_g, got_p, got_a, n, side, vr, KEEP, la, model.mode, moved, model.sense16,
                                    list(model.dx), list(model.dy))
    what = f"mode {model.mode}, dx[0] {model.dx[0]}, sense16 {model.sense16}, moved {moved}, view_range {vr}, misaligned {misalign}"
    if not torch.equal(got_g.cpu(), want_g):
        bad = (got_g.cpu() != want_g).nonzero()
        b, c = bad[0].tolist()
        pytest.fail(f"{what}: {len(bad)} grid cells differ, first env {b} cell ({c // side}, {c % side}): kernel {int(got_g[b, c])}, "
                    f"definition {int(want_g[b, c])}")
    assert torch.equal(got_p.cpu(), want_p), what
    if not torch.equal(got_a.cpu(), want_a):
        bad = (got_a.cpu() != want_a).nonzero()
        b, i = bad[0].tolist()
        pytest.fail(f"{what}: {len(bad)} actions differ, first env {b} agent {i}: kernel {int(got_a[b, i])}, definition {int(want_a[b, i])}")
    return want_a


# ---- 1. the kernel equals the definition ------------------------------------------------------------------------------------

@pytest.mark.parametrize("B, n, side", [(1, 1, 50), (3, 3, 50), (65, 5, 50), (7, 8, 64), (5, 2, 7)])
def test_kernel_equals_the_definition(B, n, side):
    """walk and evade x speed 0.25, 1.0, 3.5 and map_size x moved 0 and 1 x sense 0, 10 and 2 map_size: 48 calls per shape, each on
    grids of the five kinds of make_grid (rotated so that B = 1 meets them all), prev on and off the map, state rows of an env.
    Side 50 and 64 take the 16-byte path, side 7 (49 cells, fewer than the block has threads) one cell per lane."""
    g = torch.Generator().manual_seed(1000 * B + 10 * n + side)
    state = env_state(B, n)
    k = 0
    for mode in ("walk", "evade"):
        for speed in (0.25, 1.0, 3.5, float(side)):
            for sense in (0.0, 10.0, 2.0 * side):
                model = be.BeliefModel.from_motion(mo.TargetMotion(mode=mode, speed=speed, sense=sense), side)
                for moved in (0, 1):
                    a = compare(state, make_grid(B, side, g, k), make_prev(B, side, g), n, side, model, moved)
                    assert bool(((a >= 0) & (a <= 2)).all())
                    k += 1


def test_kernel_equals_the_definition_on_odd_rows_unaligned_rows_and_wide_views():
    g = torch.Generator().manual_seed(5)
    side, n, B = 50, 3, 5
    evade = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), side)
    walk = be.BeliefModel.from_motion(mo.TargetMotion(mode="walk", speed=3.5), side)
    state = env_state(B, n)
    # rows no env emits: NaN, infinities and huge values are clamped the same way on both sides
    odd = state.clone()
    odd[0, 0], odd[1, 1], odd[2, 2], odd[3, 3], odd[3, 4], odd[4, 5] = float("nan"), float("inf"), float("nan"), -1e30, 1e30, 7.5
    for k, (model, moved) in enumerate(((evade, 1), (walk, 1), (evade, 0))):
        compare(odd, make_grid(B, side, g, k), make_prev(B, side, g), n, side, model, moved)
        # rows that are not 16-byte aligned
        compare(state, make_grid(B, side, g, k), make_prev(B, side, g), n, side, model, moved, misalign=True)
        # a view wider than the block has threads per footprint, no view at all, lookahead 0 and map_size
        compare(state, make_grid(B, side, g, k), make_prev(B, side, g), n, side, model, moved, vr=20, la=30)
        compare(state, make_grid(B, side, g, k), make_prev(B, side, g), n, side, model, moved, vr=0, la=0)
        compare(state, make_grid(B, side, g, k), make_prev(B, side, g), n, side, model, moved, vr=1, la=side)


# ---- 2. closed loop through the collector -----------------------------------------------------------------------------------

def collect(variant, B, impl, every):
    args = cs.make_env_args(variant, n_agents=3)
    args.time_limit = 60
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=every, seed=2)
    seeds = np.arange(B, dtype=np.uint32) + 77
    env = cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion)
    ag = cs.BeliefAgents(env, impl=impl)
    assert ag.motion is motion
    env.seed(seeds)
    episode, reward, win, found = cs.EpisodeCollector(env).generate_episodes(policy=ag.policy(), init=True)
    return episode, found.clone(), ag.grid.clone(), ag.prev.clone(), (ag, env)


@pytest.mark.parametrize("variant, B", [("flight_easy", 33), ("flight", 9)])
@pytest.mark.parametrize("every", [1, 3])
def test_closed_loop_kernel_and_definition_fly_the_same_episodes(variant, B, every):
    """60 steps against evading targets; a rerun on a fresh env is bit-identical (a second episode of the SAME env is another
    one: the walk headings are keyed by the env's episode counter) and the grid resets at t = 0."""
    ep_h, found_h, grid_h, prev_h, (ag, env) = collect(variant, B, "hip", every)
    ep_2, found_2, grid_2, prev_2, _ = collect(variant, B, "hip", every)
    ep_t, found_t, grid_t, prev_t, _ = collect(variant, B, "torch", every)
    assert ep_h["u"].shape == (B, 60, 3, 1)
    assert torch.equal(ep_h["u"], ep_t["u"]) and torch.equal(grid_h, grid_t) and torch.equal(prev_h, prev_t) and torch.equal(found_h, found_t)
    assert torch.equal(ep_h["s"], ep_t["s"]) and torch.equal(ep_h["padded"], ep_t["padded"])
    for k in ep_h:
        assert torch.equal(ep_h[k], ep_2[k]), k
    assert torch.equal(grid_h, grid_2) and torch.equal(prev_h, prev_2) and torch.equal(found_h, found_2)
    assert not bool((grid_h == be.FRESH).all()) and int(found_h.sum()) > 0
    # t = 0 resets: the used object's first decision of a new episode is a fresh object's
    s0 = ep_h["s"][:, 0].contiguous()
    fresh = cs.BeliefAgents(env)
    assert torch.equal(ag.policy()(None, s0, None, 0), fresh.choose_action(s0, 0))
    assert torch.equal(ag.grid, fresh.grid) and torch.equal(ag.prev, fresh.prev) and not torch.equal(ag.grid, grid_h)


def test_belief_finds_more_evaders_than_coverage():
    """collect_experiment_data, 256 envs, one batch, 3 agents, evade at speed 1.0 with sense 10: targets found by step 200, both
    measured here on the same env."""
    B = 256
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, seed=1)
    env = cs.MovingTargetEnv(cs.make_env_args("flight_easy", n_agents=3), batch=B, seeds=np.arange(B, dtype=np.uint32) + 300, target_motion=motion)
    bel = cs.collect_experiment_data(env, cs.BeliefAgents(env).policy(), batches=1)
    cov = cs.collect_experiment_data(env, cs.CoverageAgents(env).policy(), batches=1)
    m = env.target_num / 100
    print(f"evaders found of {env.target_num} by step 60 / 120 / 200: belief {bel[59] * m:.2f} / {bel[119] * m:.2f} / {bel[199] * m:.2f}, "
          f"coverage {cov[59] * m:.2f} / {cov[119] * m:.2f} / {cov[199] * m:.2f}")
    assert bel[199] > cov[199]


# ---- 3. refusals and synchronisation ----------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops = _lib.torch_ops()
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), side)
    state = env_state(B, n).cuda()
    grid = torch.full((B, side * side), 1234, dtype=torch.int32, device="cuda")
    prev = torch.full((B, 8, 2), 99, dtype=torch.int32, device="cuda")
    actions = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
    ints = (n, side, 7, KEEP, 7, m.mode, 1, m.sense16, list(m.dx), list(m.dy))
    bad = [dict(grid=grid.to(torch.int64)), dict(grid=grid[:, :-1].contiguous()), dict(grid=grid[:-1].contiguous()),
           dict(grid=grid.t().contiguous().t()), dict(grid=grid.cpu()), dict(state=state.to(torch.float64)),
           dict(state=state[:, :4 * n - 1].contiguous()), dict(state=state[:-1].contiguous()), dict(state=state.cpu()),
           dict(state=state[:, ::2]), dict(actions=actions.to(torch.int32)), dict(actions=actions[:, :2].contiguous()), dict(actions=actions.cpu()),
           dict(prev=prev.to(torch.int64)), dict(prev=prev[:, :3].contiguous()), dict(prev=prev[:-1].contiguous()),
           dict(prev=prev.transpose(1, 2).contiguous().transpose(1, 2)), dict(prev=prev.cpu())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.belief_actions(kw.get("state", state), kw.get("grid", grid), kw.get("prev", prev), kw.get("actions", actions), *ints)
    for pos, value in ((0, 9), (1, 65), (2, 65), (3, 65537), (4, side + 1), (5, 2), (6, 2), (7, 2049), (8, [0] * 15), (9, [1025] + [0] * 15)):
        args = list(ints)
        args[pos] = value
        with pytest.raises(RuntimeError, match="belief_actions"):
            ops.belief_actions(state, grid, prev, actions, *args)
    assert bool((grid == 1234).all()) and bool((prev == 99).all()) and bool((actions == -7).all())
    ag = cs.BeliefAgents(cs.make_env_args("flight_easy"), batch=B, device="cuda")
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state.to(torch.float64), 1)
    with pytest.raises(ValueError, match="state must be"):
        ag.choose_action(state[:-1], 1)
    ag.grid = ag.grid.to(torch.int64)
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state, 1)
    with pytest.raises(ValueError, match="not a GPU"):
        cs.BeliefAgents(cs.make_env_args("flight_easy"), batch=B, device="cpu")


def test_a_call_never_synchronises_and_runs_on_the_current_stream():
    B, n = 16, 3
    state = env_state(B, n).cuda()
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    ag = cs.BeliefAgents(cs.make_env_args("flight_easy"), motion=motion, batch=B, device="cuda")
    ag.choose_action(state, 1)
    ag.reset()
    ag.prev.fill_(300)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            a = ag.choose_action(state, 1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    want_g = torch.full((B, 2500), 65536, dtype=torch.int32)
    want_p = torch.full((B, 8, 2), 300, dtype=torch.int32)
    want_a = be.belief_actions_torch(state.cpu(), want_g, want_p, n, 50, 7, KEEP, ag.model, 1, 7)
    assert torch.equal(a.cpu(), want_a) and torch.equal(ag.grid.cpu(), want_g) and torch.equal(ag.prev.cpu(), want_p)
