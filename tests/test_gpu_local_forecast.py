"""GPU tests of the forecast planner on private grids (cs_local_belief_forecast and cs_local_plan_forecast_actions,
csrc/local_forecast.h): both kernels equal their definitions (local_forecast.py) in every element, from aligned
and from 4-byte-offset bases, and leave what they only read alone; the op layer and a bare ctypes call give the same; the entry points
refuse bad arguments and launch nothing; LocalForecastAgents flies the same episodes with the kernels as with the definitions, and
ForecastAgents' at an unlimited range.  Everything is torch.equal on integers: no tolerance, and nothing is asserted about what a
policy finds.  The references are local_forecast_util's cached definitions, computed once on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import motion as mo
from local_forecast_util import MIXED, MOVES, PARAMS3, SHAPES, forecast_case, mdl, plan_case
from local_util import walk

pytestmark = pytest.mark.gpu
DEV = "cuda"


def place(t, offset):
    """The same values in a contiguous device tensor; with `offset` it starts one element behind a 16-byte boundary."""
    if not offset:
        out = t.to(DEV).contiguous()
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(*t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def run_forecast(grids, prev, heard, n, side, m, moves, off_in=False, off_out=False):
    B = grids.shape[0]
    g, p, h = place(grids, off_in), prev.to(DEV), heard.to(DEV)
    stacks = place(torch.full((B, n, len(moves), side * side), -7, dtype=torch.int32), off_out)
    _lib.torch_ops().local_belief_forecast(g, p, h, stacks, n, side, m.mode, m.sense16, list(m.dx), list(m.dy), list(moves))
    assert torch.equal(g.cpu(), grids) and torch.equal(p.cpu(), prev) and torch.equal(h.cpu(), heard), "an input changed"
    return stacks.cpu()


def run_search(state, stacks, n, side, vr, depth, stride, discount, comm, offset=False):
    B = state.shape[0]
    s = place(stacks, offset)
    got = [torch.full((B, n), -7, dtype=torch.int64, device=DEV) for _ in range(3)]
    _lib.torch_ops().local_plan_forecast_actions(state.to(DEV), s, *got, n, side, vr, depth, stride, discount, comm)
    assert torch.equal(s.cpu(), stacks), "the stacks changed"
    return [t.cpu() for t in got]


def check(got, want, what):
    for name, g_, w_ in zip(("scores", "plans", "actions"), got[::-1], want[::-1]):
        if not torch.equal(g_, w_):
            bad = (g_ != w_).nonzero()
            b, i = bad[0].tolist()
            pytest.fail(f"{what}: {len(bad)} {name} differ, first env {b} agent {i}: kernel {int(g_[b, i])}, definition {int(w_[b, i])}")


# ---- 1. the kernels equal their definitions ------------------------------------------------------------------------------------

@pytest.mark.parametrize("moves", MOVES)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_forecast_kernel_equals_the_definition(B, n, side, vr, moves):
    """Grids with cells below 0 and above 2^19, heard over all 32 bits, prev beyond +-2^15; side 50 and 64 take the 16-byte paths
    from aligned bases, side 7 (49 cells) and every offset base one cell per lane; each vector flag is switched off alone."""
    grids, prev, heard, want = forecast_case(B, n, side, moves)
    m = mdl(side)
    for off_in, off_out in ((False, False), (True, False), (False, True), (True, True)):
        got = run_forecast(grids, prev, heard, n, side, m, moves, off_in, off_out)
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            b, i, d, c = bad[0].tolist()
            pytest.fail(f"moves {moves}, offset in {off_in} out {off_out}: {len(bad)} cells differ, first env {b} agent {i} level {d} cell {c}: "
                        f"kernel {int(got[b, i, d, c])}, definition {int(want[b, i, d, c])}")
    allheard = run_forecast(grids, prev, torch.full_like(heard, -1), n, side, m, moves)
    assert int((allheard != want).sum()) >= 80   # a kernel that ignored the mask would not pass


@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_forecast_kernel_in_walk_mode_ignores_the_mask(B, n, side, vr):
    moves = MOVES[1]
    grids, prev, heard, want = forecast_case(B, n, side, moves, "walk")
    m = mdl(side, "walk")
    assert torch.equal(run_forecast(grids, prev, heard, n, side, m, moves), want)
    assert torch.equal(run_forecast(grids, prev, torch.zeros_like(heard), n, side, m, moves), want)
    assert not torch.equal(want, forecast_case(B, n, side, moves)[3])


@pytest.mark.parametrize("depth, stride, discount", PARAMS3)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_search_kernel_equals_the_definition(B, n, side, vr, depth, stride, discount):
    """Stacks that differ per agent and per level, with cells below 0 and above 2^19; the mixed range, range 0 and the unlimited
    range; depth 5 at side 64 takes 85.4 KB of LDS, past the limit the entry point has to raise; side 7 goes level by level at a
    pitch of 52 words."""
    results = {}
    for comm in (MIXED[B, n, side], 0, -1):
        state, stacks, want = plan_case(B, n, side, vr, depth, stride, discount, comm)
        for offset in (False, True):
            got = run_search(state, stacks, n, side, vr, depth, stride, discount, comm, offset)
            check(got, want, f"depth {depth}, stride {stride}, discount {discount}, comm_range {comm}, offset {offset}")
        results[comm] = got
    mixed, differs = results[MIXED[B, n, side]], lambda a, b: not (torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]))
    assert differs(mixed, results[0]) or differs(mixed, results[-1])   # a kernel that heard every claim, or none, would not pass


# ---- 2. the bindings and the refusals -----------------------------------------------------------------------------------------

def test_the_op_layer_and_a_ctypes_call_agree():
    B, n, side, vr = SHAPES[0]
    L = _lib.load()
    moves = MOVES[0]
    grids, prev, heard, want = forecast_case(B, n, side, moves)
    m = mdl(side)
    p = _lib.CsForecastParams(n, side, len(moves), m.mode, m.sense16)
    for k in range(16):
        p.dx[k], p.dy[k] = m.dx[k], m.dy[k]
    for d, v in enumerate(moves):
        p.moves[d] = v
    g, pv, h = grids.to(DEV), prev.to(DEV), heard.to(DEV)
    stacks = torch.full(want.shape, -7, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.cs_local_belief_forecast(C.byref(p), g.data_ptr(), pv.data_ptr(), h.data_ptr(), B, stacks.data_ptr(), stream) == 0
    assert torch.equal(stacks.cpu(), want) and torch.equal(stacks.cpu(), run_forecast(grids, prev, heard, n, side, m, moves))
    depth, stride, discount = PARAMS3[0]
    comm = MIXED[B, n, side]
    state, stk, want = plan_case(B, n, side, vr, depth, stride, discount, comm)
    q = _lib.CsLocalPlanParams(n, side, vr, depth, stride, discount, state.shape[1], comm, 0)
    s_dev, k_dev = state.to(DEV), stk.to(DEV)
    outs = [torch.full((B, n), -7, dtype=torch.int64, device=DEV) for _ in range(3)]
    assert L.cs_local_plan_forecast_actions(C.byref(q), s_dev.data_ptr(), B, k_dev.data_ptr(), *(t.data_ptr() for t in outs), stream) == 0
    got = [t.cpu() for t in outs]
    check(got, want, "ctypes")
    check(got, run_search(state, stk, n, side, vr, depth, stride, discount, comm), "ctypes against the op")
    # refused with its code, and nothing launched: the outputs keep what they held
    stacks.fill_(-7)
    for field, value in (("levels", 6), ("n_agents", 9), ("reserved", 1), ("sense16", 2049)):
        bad = _lib.CsForecastParams.from_buffer_copy(p)
        setattr(bad, field, value)
        assert L.cs_local_belief_forecast(C.byref(bad), g.data_ptr(), pv.data_ptr(), h.data_ptr(), B, stacks.data_ptr(), stream) == -1
        assert L.cs_episodes_last_error().decode().startswith("cs_local_belief_forecast")
    bad = _lib.CsForecastParams.from_buffer_copy(p)
    bad.moves[4] = 1   # beyond `levels`
    assert L.cs_local_belief_forecast(C.byref(bad), g.data_ptr(), pv.data_ptr(), h.data_ptr(), B, stacks.data_ptr(), stream) == -1
    assert L.cs_local_belief_forecast(C.byref(p), g.data_ptr(), pv.data_ptr(), h.data_ptr() + 2, B, stacks.data_ptr(), stream) == -1
    for t in outs:
        t.fill_(-7)
    for field, value in (("depth", 6), ("stride", 0), ("comm_range", 129), ("state_width", 11), ("reserved", 1)):
        bad = _lib.CsLocalPlanParams.from_buffer_copy(q)
        setattr(bad, field, value)
        assert L.cs_local_plan_forecast_actions(C.byref(bad), s_dev.data_ptr(), B, k_dev.data_ptr(), *(t.data_ptr() for t in outs), stream) == -1
        assert L.cs_episodes_last_error().decode().startswith("cs_local_plan_forecast_actions")
    assert L.cs_local_plan_forecast_actions(C.byref(q), s_dev.data_ptr(), 0, k_dev.data_ptr(), *(t.data_ptr() for t in outs), stream) == -1
    torch.cuda.synchronize()
    assert bool((stacks == -7).all()) and all(bool((t == -7).all()) for t in outs)


def test_wrong_tensors_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops = _lib.torch_ops()
    m = mdl(side)
    grids = torch.full((B, n, side * side), 1234, dtype=torch.int32, device=DEV)
    prev = torch.zeros(B, 8, 2, dtype=torch.int32, device=DEV)
    heard = torch.zeros(B, 8, dtype=torch.int32, device=DEV)
    stacks = torch.full((B, n, 4, side * side), -7, dtype=torch.int32, device=DEV)
    model_ints = (n, side, m.mode, m.sense16, list(m.dx), list(m.dy), [1, 1, 1, 1])
    bad = [dict(grids=grids.to(torch.int64)), dict(grids=grids[:-1].contiguous()), dict(grids=grids.cpu()),
           dict(grids=grids.transpose(1, 2).contiguous().transpose(1, 2)), dict(prev=prev.to(torch.int64)), dict(prev=prev.cpu()),
           dict(prev=prev[:, :, :1].contiguous()), dict(heard=heard.to(torch.int64)), dict(heard=heard.cpu()), dict(heard=heard[:, :7].contiguous()),
           dict(stacks=stacks.to(torch.int64)), dict(stacks=stacks.cpu()), dict(stacks=stacks[:, :, :3].contiguous()),
           dict(stacks=stacks.transpose(1, 2).contiguous().transpose(1, 2))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.local_belief_forecast(kw.get("grids", grids), kw.get("prev", prev), kw.get("heard", heard), kw.get("stacks", stacks), *model_ints)
    state = walk(B, n, 1, 3, tail=45)[0].cuda()
    outs = {k: torch.full((B, n), -7, dtype=torch.int64, device=DEV) for k in ("actions", "plans", "scores")}
    ints = (n, side, 7, 4, 3, 230, 10)
    bad = [dict(stacks=stacks.to(torch.int64)), dict(stacks=stacks[:-1].contiguous()), dict(stacks=stacks[:, :2].contiguous()),
           dict(stacks=stacks[:, :, :3].contiguous()), dict(stacks=stacks.cpu()), dict(stacks=stacks.transpose(1, 2).contiguous().transpose(1, 2)),
           dict(state=state.to(torch.float64)), dict(state=state[:, :4 * n - 1].contiguous()), dict(state=state.cpu()), dict(state=state[:, ::2])]
    for k, t in outs.items():
        bad += [{k: t.to(torch.int32)}, {k: t[:, :2].contiguous()}, {k: t.cpu()}, {k: t.t().contiguous().t()}]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.local_plan_forecast_actions(kw.get("state", state), kw.get("stacks", stacks), kw.get("actions", outs["actions"]),
                                            kw.get("plans", outs["plans"]), kw.get("scores", outs["scores"]), *ints)
    for pos, values in ((0, (0, 9)), (1, (0, 65)), (2, (-1, 65)), (3, (0, 6)), (4, (0, 9)), (5, (-1, 257)), (6, (-2, 129))):
        for value in values:
            args = list(ints)
            args[pos] = value
            with pytest.raises(RuntimeError, match="local_plan_forecast_actions"):
                ops.local_plan_forecast_actions(state, stacks, outs["actions"], outs["plans"], outs["scores"], *args)
    torch.cuda.synchronize()
    assert bool((grids == 1234).all()) and bool((stacks == -7).all()) and all(bool((t == -7).all()) for t in outs.values())
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalForecastAgents(cs.make_env_args("flight_easy"), 10, batch=B, device="cpu")
    ag = cs.LocalForecastAgents(cs.make_env_args("flight_easy"), 10, motion=mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), batch=B, device=DEV)
    ag.stacks = ag.stacks.to(torch.int64)
    with pytest.raises(RuntimeError, match="stacks"):
        ag.choose_action(state, 1, 0)


# ---- 3. the closed loop -------------------------------------------------------------------------------------------------------

STEPS, ENVS = 12, 4


def fly(agents_of, every=1):
    """One batch of 12-step episodes on a fresh MovingTargetEnv of fixed seeds (evaders at speed 1.0) -> (episode dict, found, agents)."""
    args = cs.make_env_args("flight_easy", n_agents=3)
    args.time_limit = STEPS
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=every, seed=2)
    seeds = np.arange(ENVS, dtype=np.uint32) + 77
    env = cs.MovingTargetEnv(args, batch=ENVS, seeds=seeds, target_motion=motion)
    ag = agents_of(env)
    assert ag.motion is motion
    env.seed(seeds)
    episode, reward, win, found = cs.EpisodeCollector(env).generate_episodes(policy=ag.policy(), init=True)
    return episode, found.clone(), ag


@pytest.mark.parametrize("every", [1, 2])
def test_closed_loop_kernels_and_definitions_fly_the_same_episodes(every):
    comm = MIXED[3, 3, 50]
    ep_h, found_h, hip = fly(lambda env: cs.LocalForecastAgents(env, comm), every)
    ep_t, found_t, ref = fly(lambda env: cs.LocalForecastAgents(env, comm, impl="torch"), every)
    assert ep_h["u"].shape == (ENVS, STEPS, 3, 1) and hip.base.impl == "hip" and ref.base.impl == "torch"
    for k in ep_h:
        assert torch.equal(ep_h[k], ep_t[k]), k
    assert torch.equal(hip.grids, ref.grids) and torch.equal(hip.plans, ref.plans) and torch.equal(hip.scores, ref.scores)
    assert torch.equal(hip.stacks, ref.stacks) and torch.equal(hip.base.heard, ref.base.heard) and torch.equal(found_h, found_t)
    assert bool((hip.stacks[:, :, 0] != hip.stacks[:, :, -1]).any())   # a forecast, not copies of one level
    ep_p, _, plain = fly(lambda env: cs.LocalPlanAgents(env, comm, base="belief"), every)
    assert not torch.equal(plain.scores, hip.scores)   # ... and the plain planner scores the same flight's end otherwise
    print(f"every {every}, comm_range {comm}: found {float(found_h.double().mean()):.2f} of 15 in {STEPS} steps")


def test_closed_loop_at_unlimited_range_is_forecast_agents():
    ep_f, found_f, shared = fly(lambda env: cs.ForecastAgents(env))
    ep_l, found_l, local = fly(lambda env: cs.LocalForecastAgents(env, None))
    assert shared.impl == local.impl == "hip"
    for k in ep_f:
        assert torch.equal(ep_f[k], ep_l[k]), k
    assert torch.equal(found_f, found_l) and torch.equal(local.plans, shared.plans) and torch.equal(local.scores, shared.scores)
    for i in range(3):
        assert torch.equal(local.grids[:, i], shared.grid) and torch.equal(local.stacks[:, i], shared.stack), i


def test_a_call_never_synchronises_and_runs_on_the_current_stream():
    B, n = 16, 3
    state = walk(B, n, 1, 4, tail=45)[0].cuda()
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    ag = cs.LocalForecastAgents(cs.make_env_args("flight_easy"), 15, motion=motion, batch=B, device=DEV)
    ag.choose_action(state, 1, 0)
    ag.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            a = ag.choose_action(state, 1, 0)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    ref = cs.LocalForecastAgents(cs.make_env_args("flight_easy"), 15, motion=motion, batch=B, device="cpu", impl="torch")
    want = ref.choose_action(state.cpu(), 1, 0)
    assert torch.equal(a.cpu(), want) and torch.equal(ag.grids.cpu(), ref.grids) and torch.equal(ag.stacks.cpu(), ref.stacks)
    assert torch.equal(ag.plans.cpu(), ref.plans) and torch.equal(ag.scores.cpu(), ref.scores)
