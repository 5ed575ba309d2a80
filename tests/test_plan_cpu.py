"""CPU tests of the receding-horizon planner (plan.py, include/coopsearch.h: cs_plan_actions): the definition
(plan.plan_actions_torch) equals an independent brute force in plain Python integers, breaks ties and discounts as DESIGN.md
section 21 says, turns toward mass abeam that the myopic policies cannot see, refuses what it must, and the boundary declares,
exports and registers the kernel.  Everything is integer: no tolerance."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import motion as mo
from cooperative_search_amd import plan as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 19
TURN = (0, 1, 35)


@pytest.fixture(autouse=True)
def one_thread():
    """The definition's tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


# ---- the independent brute force: plain Python ints, one env, one sequence at a time -------------------------------------------

def discs_of(x, y, h, s, side, vr, D, S):
    """The D discs (sets of cells) of sequence s flown from pose (x, y, h)."""
    ct, st = bl.trig_tables()
    out = []
    for d in range(D):
        a = (s // 3 ** (D - 1 - d)) % 3
        for _ in range(S):
            h = (h + TURN[a]) % 36
            x = min(max(x + ((16 * ct[h]) >> 14), 0), 16 * side)
            y = min(max(y + ((16 * st[h]) >> 14), 0), 16 * side)
        out.append({(ix, iy) for ix in range(side) for iy in range(side)
                    if (16 * ix + 8 - x) ** 2 + (16 * iy + 8 - y) ** 2 <= (16 * vr) ** 2})
    return out


def brute(X, Y, H, cells, n, side, vr, D, S, discount):
    """One env: (actions, plans, scores) as lists of n Python ints."""
    W = [min(max(int(c), 0), CAP) for c in cells]
    acts, plans, scores = [], [], []
    for i in range(n):
        best = None
        for s in range(3 ** D):
            seen, score, w = set(), 0, 256
            for disc in discs_of(X[i], Y[i], H[i], s, side, vr, D, S):
                score += w * sum(W[ix * side + iy] for ix, iy in disc - seen)
                seen |= disc
                w = (w * discount) >> 8
            if best is None or score > best[0]:
                best = (score, s, seen)
        for ix, iy in best[2]:
            W[ix * side + iy] = 0
        acts.append(best[1] // 3 ** (D - 1))
        plans.append(best[1])
        scores.append(best[0])
    return acts, plans, scores


def poses(B, n, g, tail=5):
    """State rows float32 [B, 4n + tail]: random poses; env 0 sits in a corner and env 1 on a wall, both facing out."""
    xy = torch.rand(B, n, 2, generator=g) * 2 - 1
    ang = torch.rand(B, n, generator=g) * 2 * math.pi
    xy[0, :, :] = torch.tensor([1.0, 1.0])
    ang[0] = math.pi / 4
    if B > 1:
        xy[1, :, 0] = -1.0
        ang[1] = math.pi
    ag = torch.cat([xy, torch.cos(ang)[..., None], torch.sin(ang)[..., None]], -1).reshape(B, 4 * n)
    return torch.cat([ag, torch.rand(B, tail, generator=g)], 1).to(torch.float32).contiguous()


def random_grid(B, side, g):
    """int32 [B, side * side]: values in 0..CAP, a fifth of them zero, with cells below 0 and above CAP."""
    grid = torch.randint(0, CAP + 1, (B, side * side), generator=g, dtype=torch.int32)
    grid[torch.rand(B, side * side, generator=g) < 0.2] = 0
    wild = torch.randint(-(1 << 21), 1 << 21, (B, side * side), generator=g, dtype=torch.int32)
    grid = torch.where(torch.rand(B, side * side, generator=g) < 0.1, wild, grid)
    grid[:, 0], grid[:, -1] = -2 ** 31, 2 ** 31 - 1
    return grid


@pytest.mark.parametrize("side, n, vr, D, S", [(7, 2, 1, 3, 1), (13, 3, 3, 4, 2), (50, 3, 7, 2, 3), (9, 1, 0, 5, 1), (8, 8, 9, 1, 8)])
@pytest.mark.parametrize("discount", [230, 256])
def test_definition_equals_the_brute_force(side, n, vr, D, S, discount):
    B = 3
    g = torch.Generator().manual_seed(100 * side + 10 * n + D)
    state, grid = poses(B, n, g), random_grid(B, side, g)
    before = grid.clone()
    acts, plans, scores = pl.plan_actions_torch(state, grid, n, side, vr, D, S, discount, return_plans=True)
    assert torch.equal(grid, before)   # read only
    assert acts.dtype == plans.dtype == scores.dtype == torch.int64 and acts.shape == plans.shape == scores.shape == (B, n)
    assert torch.equal(acts, pl.plan_actions_torch(state, grid, n, side, vr, D, S, discount))
    X, Y, H = bl.quantise(state, n, side)
    for b in range(B):
        want = brute(X[b].tolist(), Y[b].tolist(), H[b].tolist(), grid[b].tolist(), n, side, vr, D, S, discount)
        assert (acts[b].tolist(), plans[b].tolist(), scores[b].tolist()) == want, f"env {b}"


def test_a_large_batch_goes_block_by_block_and_gives_the_same(monkeypatch):
    g = torch.Generator().manual_seed(3)
    state, grid = poses(5, 2, g), random_grid(5, 13, g)
    whole = pl.plan_actions_torch(state, grid, 2, 13, 3, 3, 2, 200, return_plans=True)
    monkeypatch.setattr(pl, "_CHUNK", 2 * 27 * 169)   # two envs at a time
    for got, want in zip(pl.plan_actions_torch(state, grid, 2, 13, 3, 3, 2, 200, return_plans=True), whole):
        assert torch.equal(got, want)


# ---- ties and discount ---------------------------------------------------------------------------------------------------------

def centre_row(ix, iy, heading, side, tail=5):
    """One state row with one agent on the centre of cell (ix, iy), heading index `heading` (of 36)."""
    half = side / 2
    ang = heading * math.pi / 18
    return torch.tensor([[(ix + 0.5 - half) / half, (iy + 0.5 - half) / half, math.cos(ang), math.sin(ang)] + [0.0] * tail], dtype=torch.float32)


def test_ties_take_the_lowest_sequence():
    g = torch.Generator().manual_seed(9)
    state = poses(4, 3, g)
    # all zero: every score is 0
    a, p, s = pl.plan_actions_torch(state, torch.zeros(4, 2500, dtype=torch.int32), 3, 50, 7, 4, 3, 256, return_plans=True)
    assert not a.any() and not p.any() and not s.any()
    # uniform, and a view that holds the whole map from anywhere: the first disc takes everything, every sequence ties
    state = poses(4, 2, g)
    a, p, s = pl.plan_actions_torch(state, torch.full((4, 49), 1000, dtype=torch.int32), 2, 7, 64, 3, 2, 256, return_plans=True)
    assert not a.any() and not p.any()
    assert s.tolist() == [[256 * 49 * 1000, 0]] * 4   # and the second agent finds nothing left


def test_a_later_sequence_strictly_wins_and_discount_zero_counts_first_segments_only():
    """view_range 0: a disc is the one cell whose centre IS the point.  From the centre of (10, 10) at heading 8 (80 degrees) only
    action 1 reaches heading 9 (CT = 0, ST = 16384: a step of exactly (0, 16)) and with it the centre of (10, 11); action 0 steps
    by ((16 * 2845) >> 14, (16 * 16135) >> 14) = (2, 15) and action 2 by (5, 15), onto no centre.  (1, 0) goes on to (10, 12)."""
    side = 20
    state = centre_row(10, 10, 8, side)
    X, Y, H = bl.quantise(state, 1, side)
    assert (int(X), int(Y), int(H)) == (168, 168, 8)
    grid = torch.full((1, side * side), 77, dtype=torch.int32)
    grid[0, 10 * side + 11], grid[0, 10 * side + 12], grid[0, 10 * side + 10] = 1000, 500, CAP
    a, p, s = pl.plan_actions_torch(state, grid, 1, side, 0, 2, 1, 128, return_plans=True)
    assert (int(a), int(p), int(s)) == (1, 3, 256 * 1000 + 128 * 500)
    a, p, s = pl.plan_actions_torch(state, grid, 1, side, 0, 2, 1, 0, return_plans=True)   # (1, 0), (1, 1), (1, 2) tie: the lowest
    assert (int(a), int(p), int(s)) == (1, 3, 256 * 1000)
    a, p, s = pl.plan_actions_torch(state, grid, 1, side, 0, 1, 1, 256, return_plans=True)
    assert (int(a), int(p), int(s)) == (1, 1, 256 * 1000)
    assert pl.weights(5, 230) == [256, 230, 206, 185, 166] and pl.weights(3, 0) == [256, 0, 0] and pl.weights(3, 256) == [256] * 3
    assert pl.step_tables()[0][:2] == [16, 15] and pl.step_tables()[1][35] == -3   # the shift floors


# ---- the case the feature exists for -------------------------------------------------------------------------------------------

def edge_row(ix, iy, side, tail=45):
    """One state row with one agent at heading 0, on the middle of the edge between cells (ix, iy - 1) and (ix, iy)."""
    half = side / 2
    return torch.tensor([[(ix + 0.5 - half) / half, (iy - half) / half, 1.0, 0.0] + [0.0] * tail], dtype=torch.float32)


@pytest.mark.parametrize("iy0, turn", [(34, 1), (13, 2)])
def test_mass_abeam_turns_the_planner_and_not_the_myopic_policies(iy0, turn):
    """One agent in the middle of flight_easy's map at (25.5, 25.0), heading 0, and mass only in a 3 x 3 blob 10.5 cells abeam.
    The three look-ahead discs of the myopic step miss it: three equal scores, action 0.  Four segments of three steps turn 120
    degrees on a circle of radius 18 / pi = 5.7 cells and end about 5 cells from the blob; no sequence that starts with another
    action reaches it."""
    side, vr, D, S = 50, 7, 4, 3
    state = edge_row(25, 25, side)
    X, Y, H = (int(t) for t in bl.quantise(state, 1, side))
    assert (X, Y, H) == (408, 400, 0)
    blob = {(ix, iy) for ix in (24, 25, 26) for iy in range(iy0, iy0 + 3)}
    grid = torch.zeros(1, side * side, dtype=torch.int32)
    for ix, iy in blob:
        grid[0, ix * side + iy] = 65536
    # the coverage baseline: regrow = 16 leaks (65536 - 0) >> 16 = 1 into every empty cell and nothing into the blob; each of the
    # three footprints holds 94 cells at this pose and none of the blob
    left = grid.clone()
    a, sc = bl.coverage_actions_torch(state, left, 1, side, vr, 6554, regrow=16, return_scores=True)
    assert sc.tolist() == [[[94, 94, 94]]] and int(a) == 0   # three equal scores: the tie rule flies straight on
    prev = torch.zeros(1, 8, 2, dtype=torch.int32)
    a, sc = be.belief_actions_torch(state, grid.clone(), prev, 1, side, vr, 6554, be.BeliefModel(), 0, return_scores=True)
    assert sc.tolist() == [[[0, 0, 0]]] and int(a) == 0      # the filter's choice step: the same
    for g in (left, grid):   # the grid the coverage call left (ones around the blob), and the bare blob
        a, p, s = pl.plan_actions_torch(state, g, 1, side, vr, D, S, 230, return_plans=True)
        assert int(a) == turn and int(s) >= 166 * 65536
        assert set().union(*discs_of(X, Y, H, int(p), side, vr, D, S)) & blob
    for s_ in range(3 ** D):   # the geometry: only sequences that start with `turn` reach the blob
        if s_ // 27 != turn:
            assert not set().union(*discs_of(X, Y, H, s_, side, vr, D, S)) & blob, s_


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_the_definition_refuses_bad_ranges_and_shapes():
    state, grid = torch.zeros(2, 17), torch.zeros(2, 2500, dtype=torch.int32)
    good = dict(n_agents=3, side=50, view_range=7, depth=4, stride=3, discount=230)

    def call(state=state, grid=grid, **kw):
        return pl.plan_actions_torch(state, grid, **dict(good, **kw))

    assert call().shape == (2, 3)
    for kw in (dict(n_agents=0), dict(n_agents=9), dict(side=0, grid=torch.zeros(2, 0, dtype=torch.int32)), dict(side=65), dict(view_range=-1),
               dict(view_range=65), dict(depth=0), dict(depth=6), dict(stride=0), dict(stride=9), dict(discount=-1), dict(discount=257),
               dict(state=state[:, :11]), dict(state=state[0]), dict(state=state.double()), dict(state=state[:0]), dict(grid=grid[:1]),
               dict(grid=grid[:, :-1]), dict(grid=grid.long()), dict(grid=grid.view(2, 50, 50))):
        with pytest.raises(ValueError, match="plan:"):
            call(**kw)
    with pytest.raises(TypeError, match="plan:"):
        call(grid=grid.tolist())


def good_params():
    return _lib.CsPlanParams(3, 50, 7, 4, 3, 230, 57, 0)


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("view_range", -1, "view_range"),
    ("view_range", 65, "view_range"), ("depth", 0, "depth"), ("depth", 6, "depth"), ("stride", 0, "stride"), ("stride", 9, "stride"),
    ("discount", -1, "discount"), ("discount", 257, "discount"), ("state_width", 11, "state_width"), ("reserved", 1, "reserved"),
    ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("ptr", 3, "NULL"), ("ptr", 4, "NULL"), ("params", None, "NULL"),
    ("align", 0, "aligned"), ("align", 1, "aligned"), ("align", 2, "aligned"), ("align", 3, "aligned"), ("align", 4, "aligned")])
def test_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = good_params()
    B, ptrs = 4, [256, 512, 1024, 2048, 4096]   # state, grid, actions, plans, scores
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2 if value < 2 else 4
    elif field == "B":
        B = value
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_plan_actions(None if field == "params" else C.byref(p), ptrs[0], B, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None)
    assert rc == -1   # CS_E_CONFIG
    assert msg in L.cs_episodes_last_error().decode() and "cs_plan_actions" in L.cs_episodes_last_error().decode()


def test_the_op_refuses_bad_integers_shapes_and_cpu_tensors():
    ops = _lib.torch_ops()
    state, grid = torch.zeros(2, 57), torch.full((2, 2500), 65536, dtype=torch.int32)
    outs = [torch.full((2, 3), -7, dtype=torch.int64) for _ in range(3)]
    good = dict(n_agents=3, side=50, view_range=7, depth=4, stride=3, discount=230)

    def call(state=state, grid=grid, outs=outs, **kw):
        a = dict(good, **kw)
        ops.plan_actions(state, grid, *outs, a["n_agents"], a["side"], a["view_range"], a["depth"], a["stride"], a["discount"])

    for kw, msg in ((dict(n_agents=9), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"), (dict(depth=0), "depth"),
                    (dict(depth=6), "depth"), (dict(stride=0), "stride"), (dict(stride=9), "stride"), (dict(discount=257), "discount"),
                    (dict(discount=-1), "discount"), (dict(grid=grid[:1]), "grid must be"), (dict(state=state[:, :11]), "state must be"),
                    (dict(outs=[outs[0][:, :2], outs[1], outs[2]]), "actions must be"), (dict(outs=[outs[0], outs[1][:1], outs[2]]), "plans must be"),
                    (dict(outs=[outs[0], outs[1], outs[2][:, :2]]), "scores must be")):
        with pytest.raises(RuntimeError, match="plan_actions: " + msg):   # integers and shapes come first
            call(**kw)
    with pytest.raises(RuntimeError, match="GPU"):   # a CPU tensor must be refused, not dereferenced
        call()
    assert all(bool((o == -7).all()) for o in outs)


# ---- wiring ----------------------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    version = re.search(r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    assert "cs_plan_params and cs_plan_actions" in version and "no existing export or struct changed" in version
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_plan_actions\s*\(\s*const\s+cs_plan_params\s*\*", header)
    assert "cs_plan_actions" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.cs_plan_actions.argtypes) == 8 and L.cs_plan_actions.restype is C.c_int
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_plan_params \{(.*?)\}", header, flags=re.S).group(1)
    want = ["n_agents", "side", "view_range", "depth", "stride", "discount", "state_width", "reserved"]
    assert re.findall(r"int32_t\s+(\w+);", fields) == want
    assert [k for k, _ in _lib.CsPlanParams._fields_] == want and C.sizeof(_lib.CsPlanParams) == 32
    schema = str(_lib.torch_ops().plan_actions.default._schema)
    assert schema == ("coopsearch::plan_actions(Tensor state, Tensor grid, Tensor(a!) actions, Tensor(b!) plans, Tensor(c!) scores, "
                      "int n_agents, int side, int view_range, int depth, int stride, int discount) -> ()")
    from cooperative_search_amd import build
    assert "plan.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "plan_actions")
    assert cs.PlanAgents is pl.PlanAgents and cs.plan_actions_torch is pl.plan_actions_torch
    src = open(os.path.join(ROOT, "cooperative-search_amd", "csrc", "plan.h")).read()
    assert int(re.search(r"PLAN_CAP\s*=\s*1\s*<<\s*(\d+)", src).group(1)) == 19 and pl.CAP == be.CAP == 1 << 19
    assert int(re.search(r"PLAN_MAX_NODES\s*=\s*(\d+)", src).group(1)) == sum(3 ** d for d in range(1, pl.MAX_DEPTH + 1)) == 363


@pytest.mark.parametrize("base", ["coverage", "belief"])
def test_plan_agents_run_the_definition_on_the_cpu_and_leave_the_bases_grid_alone(base):
    B, n = 3, 3
    args = cs.make_env_args("flight_easy", n_agents=n)
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=2)
    ag = cs.PlanAgents(args, base=base, motion=motion, depth=2, stride=3, batch=B, device="cpu", impl="torch")
    alone = (cs.CoverageAgents(args, batch=B, device="cpu", impl="torch") if base == "coverage"
             else cs.BeliefAgents(args, motion=motion, batch=B, device="cpu", impl="torch"))
    assert type(ag.base) is type(alone) and ag.grid is ag.base.grid and (ag.depth, ag.stride, ag.discount) == (2, 3, 230)
    assert ag.motion is motion
    g = torch.Generator().manual_seed(4)
    policy, policy_alone = ag.policy(), alone.policy()
    ag.grid.fill_(5)   # t == 0 resets
    for t in range(4):
        state = poses(B, n, g, tail=45)
        a = policy(None, state, None, t)
        policy_alone(None, state, None, t)
        assert a.shape == (B, n) and a.dtype == torch.int64 and bool(((a >= 0) & (a <= 2)).all())
        assert torch.equal(ag.grid, alone.grid)
        want = pl.plan_actions_torch(state, alone.grid, n, 50, 7, 2, 3, 230, return_plans=True)
        assert torch.equal(a, want[0]) and torch.equal(ag.plans, want[1]) and torch.equal(ag.scores, want[2])
    if base == "belief":
        assert torch.equal(ag.base.prev, alone.prev)
    ag.reset()
    assert bool((ag.grid == bl.FRESH).all())
    wrapped = cs.PlanAgents(args, base=alone, impl="torch")   # an instance: shared, not copied
    assert wrapped.base is alone and wrapped.batch == B and wrapped.device.type == "cpu"
    assert torch.equal(wrapped.choose_action(state, 0), pl.plan_actions_torch(state, alone.grid, n, 50, 7, 4, 3, 230))


def test_plan_agents_refuse_what_they_cannot_run():
    args = cs.make_env_args("flight_easy")
    with pytest.raises(ValueError, match="not a GPU"):
        cs.PlanAgents(args, batch=4, device="cpu", impl="hip")
    with pytest.raises(ValueError, match="not a GPU"):
        cs.PlanAgents(args, base="belief", batch=4, device="cpu")
    with pytest.raises(ValueError, match="impl"):
        cs.PlanAgents(args, batch=4, device="cpu", impl="eager")
    with pytest.raises(ValueError, match="base must be"):
        cs.PlanAgents(args, base="random", batch=4, device="cpu", impl="torch")
    with pytest.raises(ValueError, match="batch"):
        cs.PlanAgents(args, device="cpu", impl="torch")
    for kw in (dict(depth=0), dict(depth=6), dict(stride=0), dict(stride=9), dict(discount=257), dict(discount=-1)):
        with pytest.raises(ValueError, match="plan:"):
            cs.PlanAgents(args, batch=4, device="cpu", impl="torch", **kw)
    base = cs.CoverageAgents(args, batch=4, device="cpu", impl="torch")
    with pytest.raises(ValueError, match="the base runs"):
        cs.PlanAgents(args, base=base, impl="hip")
    with pytest.raises(ValueError, match="batch 5"):
        cs.PlanAgents(args, base=base, batch=5, impl="torch")
    with pytest.raises(TypeError, match="motion"):
        cs.PlanAgents(args, motion="walk", batch=4, device="cpu", impl="torch")
