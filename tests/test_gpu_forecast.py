"""GPU tests of the forecast kernels (cs_belief_forecast and cs_plan_forecast_actions, csrc/forecast.h): each equals its
definition (forecast.forecast_torch, forecast.plan_forecast_actions_torch) in every element and leaves its inputs alone, identical
levels give cs_plan_actions' outputs kernel against kernel, and ForecastAgents flies the same episodes with the kernels as with
the definitions.  Everything is torch.equal on integers: no tolerance."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import belief as be
from cooperative_search_amd import forecast as fc
from cooperative_search_amd import motion as mo
from test_gpu_plan import COMBOS, env_state, make_grid, wall_state

pytestmark = pytest.mark.gpu
CAP = fc.CAP
SHAPES = [(1, 1, 50), (3, 3, 50), (65, 5, 50), (7, 8, 64), (5, 2, 7)]   # (B, n_agents, side)
MOVES = [(0, 0, 0), (8, 8, 8, 8, 8), (3, 3, 3, 3), (1, 0, 2, 0, 8)]


def models(side):
    """walk 0.5; evade 1.0 inside 10 cells; evade with sense 0; a walk whose step is the widest the entry point takes (dx reaches
    +-1024: every destination clamps to a wall)."""
    def of(**kw):
        return be.BeliefModel.from_motion(mo.TargetMotion(**kw), side)
    return [of(mode="walk", speed=0.5), of(mode="evade", speed=1.0, sense=10.0), of(mode="evade", speed=1.0, sense=0.0),
            be.BeliefModel(mode=0, sense16=0, dx=tuple(int(round(1024 * v)) for v in mo.CX), dy=tuple(int(round(1024 * v)) for v in mo.CY))]


def make_pos(B, side, g):
    """int32 [B, 8, 2]: positions on the map in sub-units; env 0 holds an agent beyond the clamp and one just off the map."""
    pos = torch.randint(0, 16 * side + 1, (B, 8, 2), generator=g, dtype=torch.int32)
    pos[0, 0] = torch.tensor([-2 ** 31, 2 ** 31 - 1], dtype=torch.int32)
    if B > 1:
        pos[1, 0] = torch.tensor([-40, 16 * side + 90], dtype=torch.int32)
    return pos


def offset_by_one(t):
    """A contiguous GPU copy of t whose storage starts 4 bytes off a 16-byte boundary."""
    out = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def compare_forecast(grid, pos, n, side, mdl, moves, misalign=False):
    """grid and pos on the CPU; the definition runs on the GPU (stock torch ops on the same values)."""
    B = grid.shape[0]
    want = fc.forecast_torch(grid.cuda(), pos.cuda(), n, side, mdl, moves)
    got_g = offset_by_one(grid) if misalign else grid.cuda()
    got_p = pos.cuda()
    stack = torch.full((B, len(moves), side * side), -7, dtype=torch.int32, device="cuda")
    if misalign:
        stack = offset_by_one(stack)
    _lib.torch_ops().belief_forecast(got_g, got_p, stack, n, side, mdl.mode, mdl.sense16, list(mdl.dx), list(mdl.dy), list(moves))
    what = f"mode {mdl.mode}, sense16 {mdl.sense16}, dx[0] {mdl.dx[0]}, moves {moves}, misaligned {misalign}"
    assert torch.equal(got_g.cpu(), grid) and torch.equal(got_p.cpu(), pos), what + ": an input changed"
    if not torch.equal(stack, want):
        bad = (stack != want).nonzero()
        b, d, c = bad[0].tolist()
        pytest.fail(f"{what}: {len(bad)} cells differ, first env {b} level {d} cell {c}: kernel {int(stack[b, d, c])}, definition {int(want[b, d, c])}")
    return want


# ---- 1. the forecast kernel equals its definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("B, n, side", SHAPES)
def test_forecast_kernel_equals_the_definition(B, n, side):
    """Four models by four move lists per shape, each on grids of the five kinds of test_gpu_plan.make_grid (random, uniform, all
    zero, out of range, a few cells; rotated so that B = 1 meets them all).  Sides 50 and 64 take the 16-byte path, side 7 one
    cell per lane."""
    g = torch.Generator().manual_seed(100 * B + 10 * n + side)
    pos = make_pos(B, side, g)
    k = 0
    for mdl in models(side):
        for moves in MOVES:
            stack = compare_forecast(make_grid(B, side, g, k), pos, n, side, mdl, moves)
            assert int(stack.min()) >= 0 and int(stack.max()) <= CAP
            k += 1


def test_forecast_kernel_on_unaligned_rows_and_a_full_map():
    g = torch.Generator().manual_seed(11)
    B, n = 5, 3
    for k, side in enumerate((50, 64)):
        pos = make_pos(B, side, g)
        for mdl in models(side)[:2]:
            compare_forecast(make_grid(B, side, g, k), pos, n, side, mdl, (1, 0, 2, 0, 8), misalign=True)
    # the overflow bound: every cell at its cap and every destination one wall cell or corner: 2^31 lands on few words
    full = torch.full((2, 4096), 2 ** 31 - 1, dtype=torch.int32)
    stack = compare_forecast(full, make_pos(2, 64, g), 8, 64, models(64)[3], (1, 1))
    assert int(stack.max()) == CAP


# ---- 2. the planner kernel equals its definition ------------------------------------------------------------------------------

def make_stack(B, side, D, g, k, pos, n):
    """int32 [B, D, side * side] of kind k % 3: 0 a forecast of a make_grid grid (evade, one move per level), 1 identical levels,
    2 independent levels (a kernel that reads the wrong level cannot pass these)."""
    if k % 3 == 0:
        mdl = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), side)
        return fc.forecast_torch(make_grid(B, side, g, k).cuda(), pos.cuda(), n, side, mdl, (1,) * D).cpu()
    if k % 3 == 1:
        return make_grid(B, side, g, k).unsqueeze(1).repeat(1, D, 1)
    return torch.stack([make_grid(B, side, g, k + d) for d in range(D)], 1)


def compare_plan(state, stack, n, side, vr, D, S, discount, misalign=False):
    B = state.shape[0]
    want = fc.plan_forecast_actions_torch(state.cuda(), stack.cuda(), n, side, vr, D, S, discount, return_plans=True)
    got_s = offset_by_one(stack) if misalign else stack.cuda()
    got = [torch.full((B, n), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
    _lib.torch_ops().plan_forecast_actions(state.cuda(), got_s, *got, n, side, vr, D, S, discount)
    what = f"depth {D}, stride {S}, view_range {vr}, discount {discount}, misaligned {misalign}"
    assert torch.equal(got_s.cpu(), stack), what + ": the stack changed"
    for name, g_, w_ in zip(("scores", "plans", "actions"), got[::-1], want[::-1]):
        if not torch.equal(g_, w_):
            bad = (g_ != w_).nonzero()
            b, i = bad[0].tolist()
            pytest.fail(f"{what}: {len(bad)} {name} differ, first env {b} agent {i}: kernel {int(g_[b, i])}, definition {int(w_[b, i])}")
    return want


@pytest.mark.parametrize("B, n, side", SHAPES)
def test_planner_kernel_equals_the_definition(B, n, side):
    """test_gpu_plan's 45 combinations of (depth, stride, view_range, discount) per shape, on stacks of the three kinds of
    make_stack in turn, on an env's state rows and on the same rows with agents in corners, on walls and off the map, alternately.
    (7, 8, 64) at depth 5 is the shape that needs more than 64 KB of LDS."""
    g = torch.Generator().manual_seed(1000 * B + 10 * n + side)
    state, pos = env_state(B, n), make_pos(B, side, g)
    seen = set()
    for k, (D, S, vr, discount) in enumerate(COMBOS):
        rows = wall_state(state, n, k) if k % 2 else state
        a, p, s = compare_plan(rows, make_stack(B, side, D, g, k, pos, n), n, side, vr, D, S, discount)
        assert bool(((a >= 0) & (a <= 2)).all()) and bool(((p >= 0) & (p < 3 ** D)).all()) and bool((s >= 0).all())
        assert torch.equal(a, p // 3 ** (D - 1))
        seen |= set(a.flatten().tolist())
    assert B * n < 5 or seen == {0, 1, 2}


def test_planner_kernel_on_odd_rows_unaligned_rows_and_identical_levels():
    g = torch.Generator().manual_seed(5)
    n, B = 3, 5
    state = env_state(B, n)
    odd = state.clone()   # rows no env emits: NaN, infinities and huge values are clamped the same way on both sides
    odd[0, 0], odd[1, 1], odd[2, 2], odd[3, 3], odd[3, 4], odd[4, 5] = float("nan"), float("inf"), float("nan"), -1e30, 1e30, 7.5
    ops = _lib.torch_ops()
    for k, (side, (D, S, vr, discount)) in enumerate(((50, (4, 3, 7, 230)), (64, (5, 2, 9, 256)), (50, (2, 8, 20, 128)))):
        pos = make_pos(B, side, g)
        compare_plan(odd, make_stack(B, side, D, g, 2, pos, n), n, side, vr, D, S, discount)
        compare_plan(state, make_stack(B, side, D, g, 2, pos, n), n, side, vr, D, S, discount, misalign=True)
        compare_plan(state[:, :4 * n].contiguous(), make_stack(B, side, D, g, 0, pos, n), n, side, vr, D, S, discount)   # the narrowest row
        # identical levels: cs_plan_actions' outputs, kernel against kernel
        grid = make_grid(B, side, g, k).cuda()
        one = [torch.full((B, n), -7, dtype=torch.int64, device="cuda") for _ in range(3)]
        many = [torch.full((B, n), -8, dtype=torch.int64, device="cuda") for _ in range(3)]
        ops.plan_actions(state.cuda(), grid, *one, n, side, vr, D, S, discount)
        ops.plan_forecast_actions(state.cuda(), grid.unsqueeze(1).repeat(1, D, 1), *many, n, side, vr, D, S, discount)
        assert all(torch.equal(a, b) for a, b in zip(one, many))
    # the overflow bound: every level a full map of CAP under a view that holds all of it: 2^31 in the first gain
    full = torch.full((2, 5, 4096), 2 ** 31 - 1, dtype=torch.int32)
    middle = torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]] * 2)
    a, p, s = compare_plan(middle, full, 2, 64, 64, 5, 1, 256)
    assert s[:, 0].tolist() == [256 * 4096 * CAP] * 2 and not s[:, 1].any() and not p.any()


# ---- 3. closed loop through the collector -------------------------------------------------------------------------------------

def collect(variant, B, mode, impl, every, steps, policy_of=None):
    args = cs.make_env_args(variant, n_agents=3)
    args.time_limit = steps
    motion = mo.TargetMotion(mode=mode, speed=1.0 if mode == "evade" else 0.5, sense=10.0 if mode == "evade" else 0.0, every=every, seed=2)
    seeds = np.arange(B, dtype=np.uint32) + 77
    env = cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion)
    ag = (policy_of or cs.ForecastAgents)(env, impl=impl)
    env.seed(seeds)
    episode, reward, win, found = cs.EpisodeCollector(env).generate_episodes(policy=ag.policy(), init=True)
    return episode, found.clone(), ag, env


@pytest.mark.parametrize("variant, B", [("flight_easy", 33), ("flight", 9)])
@pytest.mark.parametrize("mode", ["walk", "evade"])
@pytest.mark.parametrize("every", [1, 3])
def test_closed_loop_kernels_and_definitions_fly_the_same_episodes(variant, B, mode, every):
    steps = 80
    ep_h, found_h, ag_h, env = collect(variant, B, mode, "hip", every, steps)
    ep_t, found_t, ag_t, _ = collect(variant, B, mode, "torch", every, steps)
    assert ag_h.motion is env.motion and (ag_h.depth, ag_h.stride, ag_h.discount) == (4, 3, 230) and ag_h.base.impl == "hip"
    assert ep_h["u"].shape == (B, steps, 3, 1)
    assert torch.equal(ep_h["u"], ep_t["u"]) and torch.equal(found_h, found_t)
    assert torch.equal(ep_h["s"], ep_t["s"]) and torch.equal(ep_h["padded"], ep_t["padded"])
    assert torch.equal(ag_h.grid, ag_t.grid) and torch.equal(ag_h.plans, ag_t.plans) and torch.equal(ag_h.scores, ag_t.scores)
    assert torch.equal(ag_h.stack, ag_t.stack) and bool(ag_h.stack.any())
    assert set(ep_h["u"].flatten().tolist()) == {0.0, 1.0, 2.0} and int(found_h.sum()) > 0


def test_the_forecast_finds_more_fast_evaders_than_the_plain_planner():
    """256 envs of flight_easy, evade at speed 1.0 inside 10 cells, a move before every step, 200 steps: strictly more targets
    found by step 200 than PlanAgents over the same filter (the filter alone is printed beside them)."""
    B, steps, n = 256, 200, 3
    curves = {}
    for name, policy_of in (("forecast", cs.ForecastAgents), ("plan over belief", lambda env, impl: cs.PlanAgents(env, base="belief", impl=impl)),
                            ("belief", cs.BeliefAgents)):
        ep, _, _, _ = collect("flight_easy", B, "evade", "hip", 1, steps, policy_of)
        count = (ep["s_next"][:, :, 4 * n + 2::3] > 0.5).sum(-1).cummax(1).values.double().mean(0)   # (padded rows are zero)
        curves[name] = [float(count[k - 1]) for k in (60, 120, 200)]
    print("evaders found of 15 at steps 60 / 120 / 200: " + ", ".join(f"{k} " + " / ".join(f"{v:.2f}" for v in c) for k, c in curves.items()))
    assert curves["forecast"][2] > curves["plan over belief"][2]


# ---- 4. refusals and synchronisation ------------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    B, n, side, D = 4, 3, 50, 4
    ops = _lib.torch_ops()
    state = env_state(B, n).cuda()
    grid = torch.full((B, side * side), 1234, dtype=torch.int32, device="cuda")
    pos = torch.full((B, 8, 2), 99, dtype=torch.int32, device="cuda")
    stack = torch.full((B, D, side * side), -7, dtype=torch.int32, device="cuda")
    mdl = models(side)[1]
    f_ints = (n, side, mdl.mode, mdl.sense16, list(mdl.dx), list(mdl.dy), [3, 3, 3, 3])
    bad = [dict(grid=grid.to(torch.int64)), dict(grid=grid[:, :-1].contiguous()), dict(grid=grid[:-1].contiguous()), dict(grid=grid.t().contiguous().t()),
           dict(grid=grid.cpu()), dict(pos=pos.to(torch.int64)), dict(pos=pos[:, :7].contiguous()), dict(pos=pos[:-1].contiguous()), dict(pos=pos.cpu()),
           dict(pos=pos.transpose(1, 2).contiguous().transpose(1, 2)), dict(stack=stack.to(torch.int64)), dict(stack=stack[:, :3].contiguous()),
           dict(stack=stack[:, :, :-1].contiguous()), dict(stack=stack[:-1].contiguous()), dict(stack=stack.cpu()),
           dict(stack=stack.transpose(1, 2).contiguous().transpose(1, 2))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.belief_forecast(kw.get("grid", grid), kw.get("pos", pos), kw.get("stack", stack), *f_ints)
    for at, values in ((0, (0, 9)), (1, (0, 65)), (2, (-1, 2)), (3, (-1, 2049)), (4, ([0] * 15, [1025] + [0] * 15)), (5, ([0] * 17, [0] * 15 + [-1025])),
                       (6, ([], [1] * 6, [3, 3, 3], [3, 3, 3, 3, 3], [3, 9, 3, 3], [-1, 3, 3, 3]))):   # (the wrong number of levels among them)
        for value in values:
            args = list(f_ints)
            args[at] = value
            with pytest.raises(RuntimeError, match="belief_forecast"):
                ops.belief_forecast(grid, pos, stack, *args)
    outs = {k: torch.full((B, n), -7, dtype=torch.int64, device="cuda") for k in ("actions", "plans", "scores")}
    p_ints = (n, side, 7, D, 3, 230)
    bad = [dict(stack=stack.to(torch.int64)), dict(stack=stack[:, :3].contiguous()), dict(stack=stack[:, 0].contiguous()), dict(stack=stack[:-1].contiguous()),
           dict(stack=stack[:, :, :-1].contiguous()), dict(stack=stack.transpose(1, 2).contiguous().transpose(1, 2)), dict(stack=stack.cpu()),
           dict(state=state.to(torch.float64)), dict(state=state[:, :4 * n - 1].contiguous()), dict(state=state[:-1].contiguous()), dict(state=state.cpu()),
           dict(state=state[:, ::2]), dict(state=state[:, 1:])]
    for k, t in outs.items():
        bad += [{k: t.to(torch.int32)}, {k: t[:, :2].contiguous()}, {k: t[:-1].contiguous()}, {k: t.cpu()}, {k: t.t().contiguous().t()}]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.plan_forecast_actions(kw.get("state", state), kw.get("stack", stack), kw.get("actions", outs["actions"]),
                                      kw.get("plans", outs["plans"]), kw.get("scores", outs["scores"]), *p_ints)
    for at, values in ((0, (0, 9)), (1, (0, 65)), (2, (-1, 65)), (3, (0, 3, 5, 6)), (4, (0, 9)), (5, (-1, 257))):   # (depth 3 and 5: not the stack's)
        for value in values:
            args = list(p_ints)
            args[at] = value
            with pytest.raises(RuntimeError, match="plan_forecast_actions"):
                ops.plan_forecast_actions(state, stack, outs["actions"], outs["plans"], outs["scores"], *args)
    assert bool((grid == 1234).all()) and bool((pos == 99).all()) and bool((stack == -7).all()) and all(bool((t == -7).all()) for t in outs.values())
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    ag = cs.ForecastAgents(cs.make_env_args("flight_easy"), motion=motion, batch=B, device="cuda")
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state.to(torch.float64), 1, 1)
    with pytest.raises(ValueError, match="state must be"):
        ag.choose_action(state[:-1], 1, 1)
    ag.stack = ag.stack.to(torch.int64)
    with pytest.raises(RuntimeError, match="stack"):
        ag.choose_action(state, 1, 1)
    with pytest.raises(ValueError, match="not a GPU"):
        cs.ForecastAgents(cs.make_env_args("flight_easy"), batch=B, device="cpu")
    with pytest.raises(ValueError, match="base must be a BeliefAgents"):
        cs.ForecastAgents(cs.make_env_args("flight_easy"), base=cs.CoverageAgents(cs.make_env_args("flight_easy"), batch=B, device="cuda"))


def test_a_call_never_synchronises_and_runs_on_the_current_stream():
    B, n = 16, 3
    state = env_state(B, n).cuda()
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    ag = cs.ForecastAgents(cs.make_env_args("flight_easy"), motion=motion, batch=B, device="cuda")
    ag.choose_action(state, 1, 1)
    ag.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            a = ag.choose_action(state, 1, 1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    ref = cs.ForecastAgents(cs.make_env_args("flight_easy"), motion=motion, batch=B, device="cpu", impl="torch")
    want = ref.choose_action(state.cpu(), 1, 1)
    assert torch.equal(a.cpu(), want) and torch.equal(ag.grid.cpu(), ref.grid) and torch.equal(ag.stack.cpu(), ref.stack)
    assert torch.equal(ag.plans.cpu(), ref.plans) and torch.equal(ag.scores.cpu(), ref.scores) and bool(ref.stack.any())
