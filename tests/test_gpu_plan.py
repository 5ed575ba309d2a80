"""GPU tests of the planner kernel (cs_plan_actions, csrc/plan.h): it equals the definition (plan.plan_actions_torch) in every
action, plan and score, leaves the grid alone, and PlanAgents flies the same episodes with the kernels as with the definitions.
Everything is torch.equal on integers: no tolerance."""
import math

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import motion as mo
from cooperative_search_amd import plan as pl

pytestmark = pytest.mark.gpu
CAP = pl.CAP
# (depth, stride, view_range, discount): the full cross, 45 combinations
COMBOS = [(D, S, vr, discount) for D, S in ((1, 1), (2, 4), (4, 3), (5, 2), (5, 8)) for vr in (0, 7, 64) for discount in (0, 230, 256)]


def env_state(B, n, steps=3):
    """get_state() rows float32 [B, 4n + 45] of a flight_easy env after a few random steps, on the CPU."""
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=np.arange(B, dtype=np.uint32) + 13 * n)
    g = torch.Generator().manual_seed(B + n)
    for _ in range(steps):
        env.step(torch.randint(0, 3, (B, n), generator=g).cuda())
    return env.get_state().cpu().contiguous()


def wall_state(state, n, k):
    """The same rows with agent 0 of every env in a corner facing out of it (the corner rotates with k and the env), agent 1 (if
    any) on a wall heading along it, agent 2 (if any) just off the map."""
    s = state.clone()
    for b in range(s.shape[0]):
        q = (b + k) % 4
        cx, cy = (1.0, -1.0)[q & 1], (1.0, -1.0)[q >> 1]
        ang = math.atan2(cy, cx)
        s[b, 0:4] = torch.tensor([cx, cy, math.cos(ang), math.sin(ang)])
        if n > 1:
            s[b, 4:8] = torch.tensor([-1.0, 0.3, 0.0, 1.0 if q & 1 else -1.0])
        if n > 2:
            s[b, 8:12] = torch.tensor([1.1, -1.2, -1.0, 0.0])
    return s


def make_grid(B, side, g, k):
    """int32 [B, side * side]; env b holds kind (b + k) % 5: 0 random in 0..CAP with zeros, 1 uniform (all ties), 2 all zero, 3 cells
    outside 0..CAP, 4 a few cells of mass in an empty map."""
    cells = side * side
    grid = torch.empty(B, cells, dtype=torch.int32)
    for b in range(B):
        kind = (b + k) % 5
        if kind == 0:
            row = torch.randint(0, CAP + 1, (cells,), generator=g, dtype=torch.int32)
            row[torch.rand(cells, generator=g) < 0.2] = 0
            row[0], row[-1] = 0, CAP
        elif kind == 1:
            row = torch.full((cells,), CAP if b % 2 else 65536, dtype=torch.int32)
        elif kind == 2:
            row = torch.zeros(cells, dtype=torch.int32)
        elif kind == 3:
            row = torch.randint(-(1 << 21), 1 << 21, (cells,), generator=g, dtype=torch.int32)
            row[:3] = torch.tensor([-2 ** 31, 2 ** 31 - 1, CAP + 1], dtype=torch.int32)[:min(3, cells)]
        else:
            row = torch.zeros(cells, dtype=torch.int32)
            row[torch.randint(0, cells, (5,), generator=g)] = torch.randint(1, CAP + 1, (5,), generator=g, dtype=torch.int32)
        grid[b] = row
    return grid


def compare(state, grid, n, side, vr, D, S, discount, misalign=False):
    """state and grid on the CPU; the definition runs on the GPU (stock torch ops on the same values)."""
    B = state.shape[0]
    want = pl.plan_actions_torch(state.cuda(), grid.cuda(), n, side, vr, D, S, discount, return_plans=True)
    if misalign:   # rows that are not 16-byte aligned: one cell per lane at a side whose rows are whole 16-byte pieces
        got_g = torch.empty(B * side * side + 1, dtype=torch.int32, device="cuda")[1:].view(B, side * side)
        got_g.copy_(grid)
        assert got_g.data_ptr() % 16 != 0 and got_g.is_contiguous()
    else:
        got_g = grid.cuda()
    got = [torch.full((B, n), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
    _lib.torch_ops().plan_actions(state.cuda(), got_g, *got, n, side, vr, D, S, discount)
    what = f"depth {D}, stride {S}, view_range {vr}, discount {discount}, misaligned {misalign}"
    assert torch.equal(got_g.cpu(), grid), what + ": the grid changed"
    for name, g_, w_ in zip(("scores", "plans", "actions"), got[::-1], want[::-1]):
        if not torch.equal(g_, w_):
            bad = (g_ != w_).nonzero()
            b, i = bad[0].tolist()
            pytest.fail(f"{what}: {len(bad)} {name} differ, first env {b} agent {i}: kernel {int(g_[b, i])}, definition {int(w_[b, i])}")
    return want


# ---- 1. the kernel equals the definition ------------------------------------------------------------------------------------

@pytest.mark.parametrize("B, n, side", [(1, 1, 50), (3, 3, 50), (65, 5, 50), (7, 8, 64), (5, 2, 7)])
def test_kernel_equals_the_definition(B, n, side):
    """The 45 combinations of COMBOS per shape, each on grids of the five kinds of make_grid (rotated so that B = 1 meets them all),
    on an env's state rows and on the same rows with agents in corners, on walls and off the map, alternately.  Side 50 and 64
    take the 16-byte path, side 7 (49 cells, fewer than the block has threads) one cell per lane."""
    g = torch.Generator().manual_seed(1000 * B + 10 * n + side)
    state = env_state(B, n)
    seen = set()
    for k, (D, S, vr, discount) in enumerate(COMBOS):
        rows = wall_state(state, n, k) if k % 2 else state
        a, p, s = compare(rows, make_grid(B, side, g, k), n, side, vr, D, S, discount)
        assert bool(((a >= 0) & (a <= 2)).all()) and bool(((p >= 0) & (p < 3 ** D)).all()) and bool((s >= 0).all())
        assert torch.equal(a, p // 3 ** (D - 1))
        seen |= set(a.flatten().tolist())
    assert B * n < 5 or seen == {0, 1, 2}


def test_kernel_equals_the_definition_on_odd_rows_and_unaligned_rows():
    g = torch.Generator().manual_seed(5)
    n, B = 3, 5
    state = env_state(B, n)
    # rows no env emits: NaN, infinities and huge values are clamped the same way on both sides
    odd = state.clone()
    odd[0, 0], odd[1, 1], odd[2, 2], odd[3, 3], odd[3, 4], odd[4, 5] = float("nan"), float("inf"), float("nan"), -1e30, 1e30, 7.5
    for k, (side, (D, S, vr, discount)) in enumerate(((50, (4, 3, 7, 230)), (64, (5, 2, 9, 256)), (50, (2, 8, 20, 128)))):
        compare(odd, make_grid(B, side, g, k), n, side, vr, D, S, discount)
        compare(state, make_grid(B, side, g, k), n, side, vr, D, S, discount, misalign=True)
        compare(state[:, :4 * n].contiguous(), make_grid(B, side, g, k + 2), n, side, vr, D, S, discount)   # the narrowest row
    # the overflow bound: a full map of CAP under a view that holds all of it from the middle of the map: 2^31 in the first gain
    full = torch.full((2, 4096), 2 ** 31 - 1, dtype=torch.int32)
    middle = torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]] * 2)
    a, p, s = compare(middle, full, 2, 64, 64, 5, 1, 256)
    assert s[:, 0].tolist() == [256 * 4096 * CAP] * 2 and not s[:, 1].any() and not p.any()


# ---- 2. closed loop through the collector -----------------------------------------------------------------------------------

def collect(variant, B, base, impl, every, steps):
    args = cs.make_env_args(variant, n_agents=3)
    args.time_limit = steps
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=every, seed=2)
    seeds = np.arange(B, dtype=np.uint32) + 77
    env = cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion)
    ag = cs.PlanAgents(env, base=base, impl=impl)
    assert ag.motion is motion and ag.base.impl == impl and (ag.depth, ag.stride, ag.discount) == (4, 3, 230)
    alone = type(ag.base)(env, impl=impl)   # the base alone, shown every state the planner is shown
    pol, pol_alone = ag.policy(), alone.policy()

    def policy(obs, state, last, t):
        pol_alone(obs, state, last, t)
        return pol(obs, state, last, t)
    env.seed(seeds)
    episode, reward, win, found = cs.EpisodeCollector(env).generate_episodes(policy=policy, init=True)
    assert torch.equal(alone.grid, ag.grid)   # the planner leaves the base's grid what the base alone holds
    return episode, found.clone(), ag, env


@pytest.mark.parametrize("variant, B", [("flight_easy", 33), ("flight", 9)])
@pytest.mark.parametrize("base", ["coverage", "belief"])
@pytest.mark.parametrize("every", [1, 3])
def test_closed_loop_kernel_and_definition_fly_the_same_episodes(variant, B, base, every):
    """80 steps against evading targets: the kernels and the definitions take the same actions, find the same targets and leave the
    same grid, plans and scores; the planner turns (a team that only ever flew straight would prove little)."""
    steps = 80
    ep_h, found_h, ag_h, env = collect(variant, B, base, "hip", every, steps)
    ep_t, found_t, ag_t, _ = collect(variant, B, base, "torch", every, steps)
    assert ep_h["u"].shape == (B, steps, 3, 1)
    assert torch.equal(ep_h["u"], ep_t["u"]) and torch.equal(found_h, found_t)
    assert torch.equal(ep_h["s"], ep_t["s"]) and torch.equal(ep_h["padded"], ep_t["padded"])
    assert torch.equal(ag_h.grid, ag_t.grid) and torch.equal(ag_h.plans, ag_t.plans) and torch.equal(ag_h.scores, ag_t.scores)
    assert set(ep_h["u"].flatten().tolist()) == {0.0, 1.0, 2.0} and int(found_h.sum()) > 0
    # t = 0 resets
    s0 = ep_h["s"][:, 0].contiguous()
    fresh = cs.PlanAgents(env, base=base)
    assert torch.equal(ag_h.policy()(None, s0, None, 0), fresh.choose_action(s0, 0)) and torch.equal(ag_h.grid, fresh.grid)


# ---- 3. refusals and synchronisation ----------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops = _lib.torch_ops()
    state = env_state(B, n).cuda()
    grid = torch.full((B, side * side), 1234, dtype=torch.int32, device="cuda")
    outs = {k: torch.full((B, n), -7, dtype=torch.int64, device="cuda") for k in ("actions", "plans", "scores")}
    ints = (n, side, 7, 4, 3, 230)
    bad = [dict(grid=grid.to(torch.int64)), dict(grid=grid[:, :-1].contiguous()), dict(grid=grid[:-1].contiguous()),
           dict(grid=grid.t().contiguous().t()), dict(grid=grid.cpu()), dict(state=state.to(torch.float64)),
           dict(state=state[:, :4 * n - 1].contiguous()), dict(state=state[:-1].contiguous()), dict(state=state.cpu()),
           dict(state=state[:, ::2]), dict(state=state[:, 1:])]
    for k, t in outs.items():
        bad += [{k: t.to(torch.int32)}, {k: t[:, :2].contiguous()}, {k: t[:-1].contiguous()}, {k: t.cpu()}, {k: t.t().contiguous().t()}]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.plan_actions(kw.get("state", state), kw.get("grid", grid), kw.get("actions", outs["actions"]), kw.get("plans", outs["plans"]),
                             kw.get("scores", outs["scores"]), *ints)
    for pos, values in ((0, (0, 9)), (1, (0, 65)), (2, (-1, 65)), (3, (0, 6)), (4, (0, 9)), (5, (-1, 257))):
        for value in values:
            args = list(ints)
            args[pos] = value
            with pytest.raises(RuntimeError, match="plan_actions"):
                ops.plan_actions(state, grid, outs["actions"], outs["plans"], outs["scores"], *args)
    assert bool((grid == 1234).all()) and all(bool((t == -7).all()) for t in outs.values())
    ag = cs.PlanAgents(cs.make_env_args("flight_easy"), batch=B, device="cuda")
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state.to(torch.float64), 1)
    with pytest.raises(ValueError, match="state must be"):
        ag.choose_action(state[:-1], 1)
    ag.plans = ag.plans.to(torch.int32)
    with pytest.raises(RuntimeError, match="plans"):
        ag.choose_action(state, 1)
    with pytest.raises(ValueError, match="not a GPU"):
        cs.PlanAgents(cs.make_env_args("flight_easy"), batch=B, device="cpu")
    with pytest.raises(ValueError, match="plan:"):
        cs.PlanAgents(cs.make_env_args("flight_easy"), batch=B, device="cuda", depth=6)


@pytest.mark.parametrize("base", ["coverage", "belief"])
def test_a_call_never_synchronises_and_runs_on_the_current_stream(base):
    B, n = 16, 3
    state = env_state(B, n).cuda()
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    ag = cs.PlanAgents(cs.make_env_args("flight_easy"), base=base, motion=motion, batch=B, device="cuda")
    ag.choose_action(state, 1)
    ag.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            a = ag.choose_action(state, 1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    ref = cs.PlanAgents(cs.make_env_args("flight_easy"), base=base, motion=motion, batch=B, device="cpu", impl="torch")
    want = ref.choose_action(state.cpu(), 1)
    assert torch.equal(a.cpu(), want) and torch.equal(ag.grid.cpu(), ref.grid)
    assert torch.equal(ag.plans.cpu(), ref.plans) and torch.equal(ag.scores.cpu(), ref.scores)
