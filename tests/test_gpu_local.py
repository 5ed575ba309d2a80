"""GPU tests of the local coverage kernel (cs_local_coverage_actions, csrc/local.h): it equals the definition
(local.local_coverage_actions_torch) in every element of the n grids and of the actions, at an unlimited range it equals
cs_coverage_actions, and LocalCoverageAgents drops into the collector.  Everything is torch.equal on integers: no tolerance."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from local_util import KEEP, SIDE, VR, boundary_rows, far_rows, fresh, random_grids, run_definition, tie_rows, walk, wall_rows

pytestmark = pytest.mark.gpu
CALLS = 6


def behind(shape, dtype):
    """A contiguous GPU tensor of `shape` that starts one element behind a 16-byte boundary."""
    numel = int(np.prod(shape))
    t = torch.empty(numel + 1, dtype=dtype, device="cuda")[1:].view(*shape)
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


def kernel(state, grids, n, side, vr, comm, regrow=8, la=None):
    """One launch on GPU tensors: grids in place -> actions."""
    la = min(vr, side) if la is None else la
    actions = torch.full((state.shape[0], n), -7, dtype=torch.int64, device="cuda")
    _lib.torch_ops().local_coverage_actions(state, grids, actions, n, side, vr, KEEP, regrow, la, comm)
    return actions


def compare(states, grids, n, side, vr, comm, regrow=8, la=None, sliced=False, misalign=False):
    """Consecutive calls of the kernel against the definition's, grids and actions after every call."""
    want = run_definition(states, grids, n, side, vr, comm, regrow, la)
    got_g = behind(grids.shape, torch.int32) if misalign else torch.empty_like(grids, device="cuda")
    got_g.copy_(grids)
    what = f"B {grids.shape[0]}, n {n}, side {side}, view_range {vr}, comm_range {comm}, lookahead {la}, sliced {sliced}, misaligned {misalign}"
    for t, s in enumerate(states):
        if sliced:   # the state rows as a slice of a wider tensor, one float behind a 16-byte boundary
            sd = behind(s.shape, torch.float32)
            sd.copy_(s)
        else:
            sd = s.cuda()
        got_a = kernel(sd, got_g, n, side, vr, comm, regrow, la)
        wg, wa = want[t]
        if not torch.equal(got_g.cpu(), wg):
            bad = (got_g.cpu() != wg).nonzero()
            b, i, c = bad[0].tolist()
            pytest.fail(f"{what}, call {t}: {len(bad)} grid cells differ, first env {b} agent {i} cell ({c // side}, {c % side}): kernel "
                        f"{int(got_g[b, i, c])}, definition {int(wg[b, i, c])}")
        if not torch.equal(got_a.cpu(), wa):
            bad = (got_a.cpu() != wa).nonzero()
            b, i = bad[0].tolist()
            pytest.fail(f"{what}, call {t}: {len(bad)} actions differ, first env {b} agent {i}: kernel {int(got_a[b, i])}, definition "
                        f"{int(wa[b, i])}")
    return want


# ---- 1. the kernel equals the definition ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B, n, side, comm", [(1, 1, 50, 0), (3, 3, 50, 10), (3, 3, 50, 0), (65, 5, 50, 20), (7, 8, 64, -1), (5, 2, 7, 3)])
def test_kernel_equals_the_definition(B, n, side, comm):
    """Six consecutive calls along a walk that reaches and passes the walls, from different random grids per agent; then the same
    with the state rows as an unaligned slice.  Side 50 and 64 take the 16-byte path, side 7 (49 cells: odd agents' rows are not
    aligned) one cell per lane."""
    vr = 2 if side == 7 else 7
    states = walk(B, n, CALLS, 1000 * B + 10 * n + side)
    grids = random_grids(B, n, side, B + n)
    compare(states, grids, n, side, vr, comm)
    compare(states, grids, n, side, vr, comm, sliced=True)


def test_kernel_on_boundary_far_tie_and_wall_rows():
    """The CPU file's hand rows through the kernel: the strict boundary, positions that need the 64-bit link test, exact ties
    (lookahead 0, and two agents on one spot, linked and not), look-ahead points clamped at the walls; grids one word behind a
    16-byte boundary (the one-cell-per-lane path at side 50); cells outside 0..65536."""
    for comm in (10, 9, 11):
        compare([boundary_rows(10)] * 2, fresh(2, 2, SIDE), 2, SIDE, VR, comm)
    skew = fresh(1, 2, SIDE)
    skew[0, 0] = 1000
    for comm in (128, 0, -1):
        want = compare([far_rows()] * 2, skew, 2, SIDE, VR, comm)
        assert torch.equal(want[0][0][0, 0], want[0][0][0, 1]) == (comm == -1)
    for comm in (5, 0):
        want = compare([tie_rows()] * 2, fresh(1, 2, SIDE), 2, SIDE, VR, comm)
        assert (int(want[0][1][0, 0]) != int(want[0][1][0, 1])) == (comm == 5)
    states = walk(6, 3, 2, 5)
    want = compare(states, fresh(6, 3, SIDE), 3, SIDE, VR, 20, la=0)
    assert not bool(want[0][1].any())   # lookahead 0: the three scores tie, the lowest action wins
    walls = wall_rows(3)
    compare([walls], random_grids(walls.shape[0], 3, SIDE, 3), 3, SIDE, VR, 10, la=SIDE)
    compare([walls], random_grids(walls.shape[0], 3, SIDE, 4), 3, SIDE, 20, -1, regrow=1, la=SIDE)
    compare(states, random_grids(6, 3, SIDE, 6), 3, SIDE, VR, 10, misalign=True)
    g = torch.Generator().manual_seed(8)
    wild = torch.randint(-200000, 200000, (6, 3, SIDE * SIDE), generator=g, dtype=torch.int32)
    wild[0, 0, :3] = torch.tensor([-2 ** 31, 2 ** 31 - 1, 65537], dtype=torch.int32)
    compare(states, wild, 3, SIDE, VR, 10)
    odd = [s.clone() for s in states]
    odd[0][0, 0], odd[0][1, 1], odd[0][2, 2], odd[0][3, 3], odd[0][3, 4] = float("nan"), float("inf"), float("nan"), -1e30, 1e30
    compare(odd, random_grids(6, 3, SIDE, 7), 3, SIDE, VR, 10)


@pytest.mark.parametrize("side, vr, la", [(50, 0, 0), (50, 0, 7), (64, 64, 64), (64, 64, 0), (1, 1, 1), (1, 0, 0), (7, 7, 3)])
def test_kernel_at_the_edge_parameters(side, vr, la):
    """view_range 0 and 64, lookahead 0, side 1: boxes that are one cell or empty, and boxes that are the whole map."""
    B, n = 3, 3
    states = walk(B, n, 2, side + vr)
    states[0][0, :2] = 0.0   # agent 0 of env 0 on the centre of the map: at an odd side that is a cell centre, view_range 0 sees it
    compare(states, random_grids(B, n, side, 2), n, side, vr, 3, la=la)
    compare(states, fresh(B, n, side), n, side, vr, -1, la=la)


# ---- 2. unlimited range equals cs_coverage_actions, on the GPU --------------------------------------------------------------------

@pytest.mark.parametrize("B, n, side", [(3, 3, 50), (7, 8, 64)])
def test_unlimited_range_equals_the_coverage_kernel(B, n, side):
    states = walk(B, n, CALLS, 31 * B + n)
    grids = random_grids(B, n, side, 9, equal=True).cuda()
    shared = grids[:, 0].clone()
    for t, s in enumerate(states):
        sd = s.cuda()
        got = kernel(sd, grids, n, side, 7, -1)
        want = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
        _lib.torch_ops().coverage_actions(sd, shared, want, n, side, 7, KEEP, 8, 7)
        assert torch.equal(got, want), t
        for i in range(n):
            assert torch.equal(grids[:, i], shared), (t, i)


# ---- 3. closed loop through the collector -------------------------------------------------------------------------------------------

def collect(impl, seeds, calls=1, steps=60, comm=10):
    B = len(seeds)
    args = cs.make_env_args("flight_easy", n_agents=3)
    args.time_limit = steps
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds)
    ag = cs.LocalCoverageAgents(env, comm, impl=impl)
    out = []
    for _ in range(calls):
        env.seed(seeds)
        episode, reward, win, found = cs.EpisodeCollector(env).generate_episodes(policy=ag.policy(), init=True)
        out.append((episode, found.clone(), ag.grids.clone()))
    return out


@pytest.mark.parametrize("comm", [10, 2])
def test_closed_loop_kernel_and_definition_fly_the_same_episodes_and_reruns_are_bit_identical(comm):
    """flight_easy, 33 envs, 3 agents, comm_range 10 (and 2: links that break early), 60 steps: impl 'hip' and 'torch' fly the same
    episodes; the grids reset at t = 0 (a second collection on the same agents equals the first) and a rerun on fresh agents is
    bit-identical."""
    B = 33
    seeds = np.arange(B, dtype=np.uint32) + 77
    (e0, f0, g0), (e1, f1, g1) = collect("hip", seeds, calls=2, comm=comm)
    (e2, f2, g2), = collect("hip", seeds, comm=comm)
    (et, ft, gt), = collect("torch", seeds, comm=comm)
    assert e0["u"].shape == (B, 60, 3, 1) and g0.shape == (B, 3, 2500)
    for k in e0:
        assert torch.equal(e0[k], e1[k]) and torch.equal(e0[k], e2[k]) and torch.equal(e0[k], et[k]), k
    assert torch.equal(g0, g1) and torch.equal(g0, g2) and torch.equal(g0, gt)
    assert torch.equal(f0, f1) and torch.equal(f0, f2) and torch.equal(f0, ft)
    print(f"comm_range {comm}: envs whose agents 0 and 1 end with different grids: {int((g0[:, 0] != g0[:, 1]).any(1).sum())} of {B}")


# ---- 4. refusals and synchronisation ------------------------------------------------------------------------------------------------

def test_wrong_tensors_and_parameters_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops = _lib.torch_ops()
    state = walk(B, n, 1, 2, tail=45)[0].cuda()
    grids = torch.full((B, n, side * side), 1234, dtype=torch.int32, device="cuda")
    actions = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
    bad = [dict(grids=grids.to(torch.int64)), dict(grids=grids[:, :, :-1].contiguous()), dict(grids=grids[:-1].contiguous()),
           dict(grids=grids[:, :2].contiguous()), dict(grids=grids[:, 0].contiguous()), dict(grids=grids.transpose(1, 2).contiguous().transpose(1, 2)),
           dict(grids=grids.cpu()), dict(state=state.to(torch.float64)), dict(state=state[:, :4 * n - 1].contiguous()), dict(state=state[:, :20]),
           dict(state=state[:-1].contiguous()), dict(state=state.cpu()), dict(actions=actions.to(torch.int32)),
           dict(actions=actions[:, :2].contiguous())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.local_coverage_actions(kw.get("state", state), kw.get("grids", grids), kw.get("actions", actions), n, side, 7, KEEP, 8, 7, 10)
    for args in ((9, side, 7, KEEP, 8, 7, 10), (n, 65, 7, KEEP, 8, 7, 10), (n, side, 65, KEEP, 8, 7, 10), (n, side, 7, 65537, 8, 7, 10),
                 (n, side, 7, KEEP, 0, 7, 10), (n, side, 7, KEEP, 8, side + 1, 10), (n, side, 7, KEEP, 8, 7, -2), (n, side, 7, KEEP, 8, 7, 129)):
        with pytest.raises(RuntimeError, match="local_coverage_actions"):
            ops.local_coverage_actions(state, grids, actions, *args)
    torch.cuda.synchronize()
    assert bool((grids == 1234).all()) and bool((actions == -7).all())
    ag = cs.LocalCoverageAgents(cs.make_env_args("flight_easy"), 10, batch=B, device="cuda")
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state.to(torch.float64))
    with pytest.raises(ValueError, match="state must be"):
        ag.choose_action(state[:-1])
    ag.grids = ag.grids.to(torch.int64)
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state)
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalCoverageAgents(cs.make_env_args("flight_easy"), 10, batch=B, device="cpu")


def test_a_call_never_synchronises_and_runs_on_the_current_stream():
    B, n = 16, 3
    state = walk(B, n, 1, 4, tail=45)[0]
    sd = state.cuda()
    ag = cs.LocalCoverageAgents(cs.make_env_args("flight_easy"), 10, batch=B, device="cuda")
    ag.choose_action(sd)
    ag.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            a = ag.choose_action(sd)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    (want_g, want_a), = run_definition([state], fresh(B, n, 50), n, 50, 7, 10)
    assert torch.equal(a.cpu(), want_a) and torch.equal(ag.grids.cpu(), want_g)
