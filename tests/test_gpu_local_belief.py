"""GPU tests of the local belief kernel (cs_local_belief_actions, csrc/local_belief.h): it equals the definition
(local_belief.local_belief_actions_torch) in every element of the n grids, of prev, of heard and of the actions; in a closed loop
it flies BeliefAgents' episodes at an unlimited range and n lone filters' at range 0; and LocalBeliefAgents drops into the
collector.  Everything is torch.equal on integers: no tolerance, and nothing is asserted about what the policy finds."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import belief as be
from cooperative_search_amd import local_belief as lb
from cooperative_search_amd import motion as mo
from local_belief_util import CAP, model, random_heard
from local_util import KEEP, SIDE, VR, far_rows, tie_rows, walk, wall_rows
from test_gpu_belief import env_state, make_grid, make_prev
from test_gpu_local import behind

pytestmark = pytest.mark.gpu


def make_grids(B, n, side, g, k):
    """int32 [B, n, side * side]: agent i of env b holds kind (b + i + k) % 5 of test_gpu_belief.make_grid (random with zeros, mostly
    zero, cells outside 0..CAP, all mass in one cell, a full-CAP map), so the grids of an env differ in kind; an env with
    (b + k) % 6 == 5 holds full-CAP maps in EVERY private grid: the 2^31 bound of the accumulator and of the scores."""
    grids = torch.stack([make_grid(B, side, g, k + i) for i in range(n)], 1)
    for b in range(B):
        if (b + k) % 6 == 5:
            grids[b] = CAP
    return grids.contiguous()


def compare(state, grids, prev, heard, n, side, mdl, moved, comm, vr=VR, la=None, misalign=False, sliced=False):
    """One launch against one call of the definition (on the CPU): grids, prev, heard and actions."""
    la = min(vr, side) if la is None else la
    want_g, want_p, want_h = grids.clone(), prev.clone(), heard.clone()
    want_a = lb.local_belief_actions_torch(state, want_g, want_p, want_h, n, side, vr, KEEP, mdl, moved, comm, la)
    B = state.shape[0]
    got_g = behind(grids.shape, torch.int32) if misalign else torch.empty_like(grids, device="cuda")
    got_g.copy_(grids)
    if sliced:   # the state rows one float behind a 16-byte boundary
        sd = behind(state.shape, torch.float32)
        sd.copy_(state)
    else:
        sd = state.cuda()
    got_p, got_h = prev.cuda(), heard.cuda()
    got_a = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
    _lib.torch_ops().local_belief_actions(sd, got_g, got_p, got_h, got_a, n, side, vr, KEEP, la, mdl.mode, moved, mdl.sense16, list(mdl.dx),
                                          list(mdl.dy), comm)
    what = (f"B {B}, n {n}, side {side}, mode {mdl.mode}, dx[0] {mdl.dx[0]}, sense16 {mdl.sense16}, moved {moved}, comm_range {comm}, "
            f"view_range {vr}, lookahead {la}, misaligned {misalign}, sliced {sliced}")
    if not torch.equal(got_g.cpu(), want_g):
        bad = (got_g.cpu() != want_g).nonzero()
        b, i, c = bad[0].tolist()
        pytest.fail(f"{what}: {len(bad)} grid cells differ, first env {b} agent {i} cell ({c // side}, {c % side}): kernel "
                    f"{int(got_g[b, i, c])}, definition {int(want_g[b, i, c])}")
    assert torch.equal(got_p.cpu(), want_p), what
    assert torch.equal(got_h.cpu(), want_h), what
    if not torch.equal(got_a.cpu(), want_a):
        bad = (got_a.cpu() != want_a).nonzero()
        b, i = bad[0].tolist()
        pytest.fail(f"{what}: {len(bad)} actions differ, first env {b} agent {i}: kernel {int(got_a[b, i])}, definition {int(want_a[b, i])}")
    return want_g, want_h, want_a


# ---- 1. the kernel equals the definition ------------------------------------------------------------------------------------------

MODES, SPEEDS, SENSES, COMMS = ("evade", "walk"), (1.0, 0.25, 3.5, None), (10.0, 0.0, None), (10, -1, 0, 2, 128)   # None: map_size, 2 map_size
SETTINGS = [(MODES[k % 2], SPEEDS[(k + k // 4) % 4], SENSES[k % 3], COMMS[k % 5], 0 if k in (3, 10) else 1) for k in range(12)]


def test_the_settings_hold_every_value():
    """The product is trimmed to twelve calls per shape; every value of every factor is among them, with moved = 1 for both modes,
    every speed and every range."""
    assert {s[0] for s in SETTINGS} == set(MODES) and {s[1] for s in SETTINGS} == set(SPEEDS) and {s[2] for s in SETTINGS} == set(SENSES)
    assert {s[3] for s in SETTINGS} == set(COMMS) and {s[4] for s in SETTINGS} == {0, 1}
    on = [s for s in SETTINGS if s[4] == 1]
    assert {s[0] for s in on} == set(MODES) and {s[1] for s in on} == set(SPEEDS) and {s[3] for s in on} >= {10, -1, 0, 2}
    assert ("evade", 1.0, 10.0, 10, 1) in SETTINGS and any(s[0] == "evade" and s[2] is None and s[4] == 1 for s in SETTINGS)


@pytest.mark.parametrize("B, n, side", [(1, 1, 50), (3, 3, 50), (65, 5, 50), (7, 8, 64), (5, 2, 7)])
def test_kernel_equals_the_definition(B, n, side):
    """Twelve settings per shape (SETTINGS), each on grids of the kinds of make_grids (rotated so that B = 1 meets them all), prev on
    and off the map, heard random over all 32 bits, state rows of an env.  Side 50 and 64 take the 16-byte path, side 7 (49 cells,
    fewer than the block has threads, odd agents' rows unaligned) one cell per lane."""
    g = torch.Generator().manual_seed(1000 * B + 10 * n + side)
    state = env_state(B, n)
    vr = 2 if side == 7 else VR
    for k, (mode, speed, sense, comm, moved) in enumerate(SETTINGS):
        mdl = model(mode, float(side) if speed is None else speed, 2.0 * side if sense is None else sense, side)
        _, h, a = compare(state, make_grids(B, n, side, g, k), make_prev(B, side, g), random_heard(B, 50 * k + n), n, side, mdl, moved, comm, vr=vr)
        assert bool(((a >= 0) & (a <= 2)).all()) and bool(((h[:, :n] >= 1) & (h[:, :n] < 1 << n)).all())


def test_kernel_on_odd_unaligned_far_tie_and_wall_rows():
    """Rows no env emits (NaN, infinities, huge values); state rows and grid bases one word behind a 16-byte boundary (the
    one-cell-per-lane path at side 50); positions that need the 64-bit link test; two agents on one spot, linked and not;
    look-ahead points clamped at the walls."""
    g = torch.Generator().manual_seed(5)
    side, n, B = 50, 3, 5
    evade, wander = model("evade", 1.0, 10.0), model("walk", 3.5, 0.0)
    state = env_state(B, n)
    odd = state.clone()
    odd[0, 0], odd[1, 1], odd[2, 2], odd[3, 3], odd[3, 4], odd[4, 5] = float("nan"), float("inf"), float("nan"), -1e30, 1e30, 7.5
    for k, (mdl, moved) in enumerate(((evade, 1), (wander, 1), (evade, 0))):
        compare(odd, make_grids(B, n, side, g, k), make_prev(B, side, g), random_heard(B, k), n, side, mdl, moved, 10)
        compare(state, make_grids(B, n, side, g, k), make_prev(B, side, g), random_heard(B, k), n, side, mdl, moved, 10, misalign=True)
        compare(state, make_grids(B, n, side, g, k), make_prev(B, side, g), random_heard(B, k), n, side, mdl, moved, 2, sliced=True)
    for comm in (128, 0, -1):
        skew = make_grids(1, 2, side, g, 0)
        want_g, want_h, _ = compare(far_rows(), skew, make_prev(1, side, g), random_heard(1, 7), 2, side, evade, 1, comm)
        assert want_h[0, :2].tolist() == ([3, 3] if comm == -1 else [1, 2]) and torch.equal(want_g[0, 0], want_g[0, 1]) == (comm == -1)
    for comm in (5, 0):
        fresh2 = torch.full((1, 2, side * side), 65536, dtype=torch.int32)
        compare(tie_rows(), fresh2, make_prev(1, side, g), random_heard(1, 8), 2, side, evade, 1, comm)
        # (nothing moved: the grids stay equal, and only a claim can part the two agents)
        _, _, a = compare(tie_rows(), fresh2, make_prev(1, side, g), random_heard(1, 8), 2, side, evade, 0, comm)
        assert (int(a[0, 0]) != int(a[0, 1])) == (comm == 5)
    walls = wall_rows(3)
    W = walls.shape[0]
    compare(walls, make_grids(W, 3, side, g, 1), make_prev(W, side, g), random_heard(W, 9), 3, side, evade, 1, 10, la=SIDE)


@pytest.mark.parametrize("side, vr, la", [(50, 0, 0), (50, 0, 50), (64, 64, 64), (64, 64, 0), (1, 1, 1), (7, 7, 3)])
def test_kernel_at_the_edge_parameters(side, vr, la):
    """view_range 0 and 64, lookahead 0 and side, side 1: boxes that are one cell or empty, and boxes that are the whole map (a
    full-CAP map under a whole-map footprint is the 2^31 score)."""
    B, n = 6, 3
    g = torch.Generator().manual_seed(side + vr + la)
    states = walk(B, n, 2, side + vr)
    states[0][0, :2] = 0.0   # agent 0 of env 0 on the centre of the map: at an odd side that is a cell centre, view_range 0 sees it
    evade = model("evade", 1.0, 10.0 if side > 7 else 2.0, side)
    for k, (s, comm) in enumerate(zip(states, (3, -1))):
        compare(s, make_grids(B, n, side, g, k + 4), make_prev(B, side, g), random_heard(B, k), n, side, evade, 1, comm, vr=vr, la=la)
    compare(states[0], torch.full((B, n, side * side), CAP, dtype=torch.int32), make_prev(B, side, g), random_heard(B, 2), n, side, evade, 0, -1,
            vr=vr, la=la)


# ---- 2. the closed loop -------------------------------------------------------------------------------------------------------------

STEPS, ENVS = 40, 33


def fly(agents_of, every):
    """One batch of episodes on a fresh MovingTargetEnv of fixed seeds -> (episode dict, found, the agents object)."""
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


@pytest.mark.parametrize("comm", [2, 10])
@pytest.mark.parametrize("every", [1, 3])
def test_closed_loop_kernel_and_definition_fly_the_same_episodes(every, comm):
    """flight_easy against evaders, 33 envs, 3 agents, 40 steps: impl 'hip' and 'torch' take the same actions at every step and end
    with the same grids, stored positions and masks."""
    ep_h, found_h, hip = fly(lambda env: cs.LocalBeliefAgents(env, comm), every)
    ep_t, found_t, ref = fly(lambda env: cs.LocalBeliefAgents(env, comm, impl="torch"), every)
    assert ep_h["u"].shape == (ENVS, STEPS, 3, 1)
    for k in ep_h:
        assert torch.equal(ep_h[k], ep_t[k]), k
    assert torch.equal(hip.grids, ref.grids) and torch.equal(hip.prev, ref.prev) and torch.equal(hip.heard, ref.heard)
    assert torch.equal(found_h, found_t)
    assert not bool((hip.grids == be.FRESH).all())
    print(f"every {every}, comm_range {comm}: envs whose agents 0 and 1 end with different grids: "
          f"{int((hip.grids[:, 0] != hip.grids[:, 1]).any(1).sum())} of {ENVS}; found {float(found_h.double().mean()):.2f} of 15")


@pytest.mark.parametrize("every", [1, 3])
def test_closed_loop_at_unlimited_range_is_belief_agents_and_at_range_zero_n_lone_filters(every):
    """Identity A through the kernel: at comm_range None the episode equals BeliefAgents' own and every private grid ends as its
    grid.  Identity B: at range 0, agent i's grid ends as that of a one-agent BeliefAgents fed agent i's floats of the same rows."""
    ep_b, found_b, shared = fly(lambda env: cs.BeliefAgents(env), every)
    ep_l, found_l, local = fly(lambda env: cs.LocalBeliefAgents(env, None), every)
    for k in ep_b:
        assert torch.equal(ep_b[k], ep_l[k]), k
    assert torch.equal(found_b, found_l) and torch.equal(local.prev, shared.prev)
    for i in range(3):
        assert torch.equal(local.grids[:, i], shared.grid), i
    ep_0, _, lone = fly(lambda env: cs.LocalBeliefAgents(env, 0), every)
    one = cs.make_env_args("flight_easy", n_agents=1)
    for i in range(3):
        solo = cs.BeliefAgents(one, motion=lone.motion, batch=ENVS, device="cuda")
        pol = solo.policy()
        for t in range(STEPS):
            a = pol(None, ep_0["s"][:, t, 4 * i:4 * i + 4].contiguous(), None, t)
            assert torch.equal(a.view(-1), ep_0["u"][:, t, i, 0].to(torch.int64)), (i, t)
        assert torch.equal(solo.grid, lone.grids[:, i]), i


# ---- 3. refusals, synchronisation, drop-ins -------------------------------------------------------------------------------------------

def test_wrong_tensors_and_parameters_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops, m = _lib.torch_ops(), model()
    state = env_state(B, n).cuda()
    grids = torch.full((B, n, side * side), 1234, dtype=torch.int32, device="cuda")
    prev = torch.full((B, 8, 2), 99, dtype=torch.int32, device="cuda")
    heard = torch.full((B, 8), 5, dtype=torch.int32, device="cuda")
    actions = torch.full((B, n), -7, dtype=torch.int64, device="cuda")
    ints = (n, side, 7, KEEP, 7, m.mode, 1, m.sense16, list(m.dx), list(m.dy), 10)
    bad = [dict(grids=grids.to(torch.int64)), dict(grids=grids[:, :, :-1].contiguous()), dict(grids=grids[:-1].contiguous()),
           dict(grids=grids[:, :2].contiguous()), dict(grids=grids[:, 0].contiguous()),
           dict(grids=grids.transpose(1, 2).contiguous().transpose(1, 2)),
           dict(grids=grids.cpu()), dict(state=state.to(torch.float64)), dict(state=state[:, :4 * n - 1].contiguous()), dict(state=state[:, ::2]),
           dict(state=state[:-1].contiguous()), dict(state=state.cpu()), dict(actions=actions.to(torch.int32)),
           dict(actions=actions[:, :2].contiguous()),
           dict(actions=actions.cpu()), dict(prev=prev.to(torch.int64)), dict(prev=prev[:, :3].contiguous()), dict(prev=prev[:-1].contiguous()),
           dict(prev=prev.transpose(1, 2).contiguous().transpose(1, 2)), dict(prev=prev.cpu()), dict(heard=heard.to(torch.int64)),
           dict(heard=heard[:, :3].contiguous()), dict(heard=heard[:-1].contiguous()), dict(heard=heard.t().contiguous().t()),
           dict(heard=heard.cpu())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.local_belief_actions(kw.get("state", state), kw.get("grids", grids), kw.get("prev", prev), kw.get("heard", heard),
                                     kw.get("actions", actions), *ints)
    for pos, value in ((0, 9), (1, 65), (2, 65), (3, 65537), (4, side + 1), (5, 2), (6, 2), (7, 2049), (8, [0] * 15), (9, [1025] + [0] * 15),
                       (10, -2), (10, 129)):
        args = list(ints)
        args[pos] = value
        with pytest.raises(RuntimeError, match="local_belief_actions"):
            ops.local_belief_actions(state, grids, prev, heard, actions, *args)
    torch.cuda.synchronize()
    assert bool((grids == 1234).all()) and bool((prev == 99).all()) and bool((heard == 5).all()) and bool((actions == -7).all())
    ag = cs.LocalBeliefAgents(cs.make_env_args("flight_easy"), 10, batch=B, device="cuda")
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state.to(torch.float64), 1)
    with pytest.raises(ValueError, match="state must be"):
        ag.choose_action(state[:-1], 1)
    ag.heard = ag.heard.to(torch.int64)
    with pytest.raises(RuntimeError, match="coopsearch"):
        ag.choose_action(state, 1)
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalBeliefAgents(cs.make_env_args("flight_easy"), 10, batch=B, device="cpu")


def test_a_call_never_synchronises_and_runs_on_the_current_stream():
    B, n = 16, 3
    state = env_state(B, n)
    sd = state.cuda()
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    ag = cs.LocalBeliefAgents(cs.make_env_args("flight_easy"), 10, motion=motion, batch=B, device="cuda")
    ag.choose_action(sd, 1)
    ag.reset()
    ag.prev.fill_(300)
    ag.heard.fill_(0b101)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            a = ag.choose_action(sd, 1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    want_g = torch.full((B, n, 2500), 65536, dtype=torch.int32)
    want_p, want_h = torch.full((B, 8, 2), 300, dtype=torch.int32), torch.full((B, 8), 0b101, dtype=torch.int32)
    want_a = lb.local_belief_actions_torch(state, want_g, want_p, want_h, n, 50, 7, KEEP, ag.model, 1, 10, 7)
    assert torch.equal(a.cpu(), want_a) and torch.equal(ag.grids.cpu(), want_g) and torch.equal(ag.prev.cpu(), want_p)
    assert torch.equal(ag.heard.cpu(), want_h)


def test_the_policy_drops_into_the_collector_evaluate_sweep_data_and_label_episodes():
    B = 8
    args = cs.make_env_args("flight_easy", n_agents=3)
    args.time_limit = 20
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, seed=3)
    env = cs.MovingTargetEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 5, target_motion=motion)
    ag = cs.LocalBeliefAgents(env, 10)
    collector = cs.EpisodeCollector(env)
    episode, reward, win, found = collector.generate_episodes(policy=ag.policy(), init=True)
    assert episode["u"].shape == (B, 20, 3, 1) and found.shape[0] == B
    win_rate, ep_reward, targets = cs.evaluate(env, ag.policy())
    assert 0.0 <= win_rate <= 1.0 and 0.0 <= targets <= env.target_num
    swept = cs.collect_sweep_data(collector, ag.policy())
    assert swept["episodes"] == B and 0.0 < swept["curve"][-1] <= 100.0
    labels = cs.label_episodes(ag, episode, impl="rows")
    assert labels.shape == (B, 20, 3) and torch.equal(labels, episode["u"][..., 0].to(torch.int64) * (1 - episode["padded"]).to(torch.int64))
    with pytest.raises(ValueError, match="CoverageAgents or a BeliefAgents"):
        cs.label_episodes(ag, episode, impl="hip")
