"""CPU tests of the target-density filter policy (belief.py, include/coopsearch.h: cs_belief_actions): the boundary declares,
exports and registers it; the definition (belief.belief_actions_torch) does what DESIGN.md section 20 says on hand cases; and
driving the C oracle in a closed loop against evading targets it finds more of them than the coverage baseline on the same seeds."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import motion as mo
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, VR, KEEP = 50, 7, 6554   # flight_easy: map_size, view_range, rint(0.1 * 65536)
OFF = (-1.0, -1.0)             # an agent in the corner (0, 0)


@pytest.fixture()
def one_thread():
    """The definition's tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def rows(agents, tail=45):
    """State rows float32 [1, 4n + tail] of agents (xn, yn), heading 0."""
    row = []
    for xn, yn in agents:
        row += [xn, yn, 1.0, 0.0]
    return torch.tensor([row + [0.0] * tail], dtype=torch.float32)


def model(mode="walk", speed=0.5, sense=0.0, side=SIDE):
    return be.BeliefModel.from_motion(mo.TargetMotion(mode=mode, speed=speed, sense=sense), side)


def prev_of(points, B=1):
    p = torch.zeros(B, 8, 2, dtype=torch.int32)
    for i, (x, y) in enumerate(points):
        p[:, i, 0], p[:, i, 1] = x, y
    return p


def predict(grid, prev, mdl, n=1, side=SIDE, agents=(OFF,)):
    """One call with moved = 1 that sweeps nothing (view_range 0 and an agent on a cell corner, which is no cell centre): grid
    becomes the prediction of its clamped self."""
    be.belief_actions_torch(rows(agents).expand(grid.shape[0], -1).contiguous(), grid, prev, n, side, 0, KEEP, mdl, 1)
    return grid


# ---- 1. the boundary ----------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    assert "cs_belief_params and cs_belief_actions" in re.search(r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_belief_actions\s*\(\s*const\s+cs_belief_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_belief_actions" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "cs_belief_actions") and L.cs_belief_actions.argtypes is not None
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_belief_params \{(.*?)\}", header, flags=re.S).group(1)
    want = ["n_agents", "side", "view_range", "keep", "lookahead", "state_width", "mode", "moved", "sense16", "dx[16]", "dy[16]", "reserved"]
    assert re.findall(r"int32_t\s+(\w+(?:\[16\])?);", fields) == want
    assert [k + ("[16]" if t is not C.c_int32 else "") for k, t in _lib.CsBeliefParams._fields_] == want
    assert C.sizeof(_lib.CsBeliefParams) == 4 * (9 + 32 + 1)
    schema = str(_lib.torch_ops().belief_actions.default._schema)
    assert schema == ("coopsearch::belief_actions(Tensor state, Tensor(a!) grid, Tensor(b!) prev, Tensor(c!) actions, int n_agents, "
                      "int side, int view_range, int keep, int lookahead, int mode, int moved, int sense16, int[] dx, int[] dy) -> ()")
    from cooperative_search_amd import build
    assert "belief.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "belief_actions")
    assert cs.BeliefAgents is be.BeliefAgents and cs.belief_actions_torch is be.belief_actions_torch and cs.BeliefModel is be.BeliefModel
    assert (mo.MODES["walk"], mo.MODES["evade"]) == (0, 1)


def test_the_kernel_header_holds_the_definitions_heading_tables():
    src = open(os.path.join(ROOT, "cooperative-search_amd", "csrc", "belief.h")).read()
    cq, sq = be.heading_tables()
    for name, want in (("BEL_CQ", cq), ("BEL_SQ", sq)):
        body = re.search(name + r"\[BEL_HEADINGS\]\s*=\s*\{(.*?)\}", src, flags=re.S).group(1)
        assert [int(v) for v in body.split(",")] == want, name
    assert cq == [int(v) for v in np.rint(16384 * np.array(mo.CX))] and sq == [int(v) for v in np.rint(16384 * np.array(mo.CY))]
    assert int(re.search(r"BEL_CAP\s*=\s*1\s*<<\s*(\d+)", src).group(1)) == 19 and be.CAP == 1 << 19


def good_params():
    m = model("evade", 1.0, 10.0)
    return _lib.CsBeliefParams(3, SIDE, VR, KEEP, 7, 57, m.mode, 1, m.sense16, (C.c_int32 * 16)(*m.dx), (C.c_int32 * 16)(*m.dy), 0)


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("view_range", -1, "view_range"),
    ("view_range", 65, "view_range"), ("keep", -1, "keep"), ("keep", 65537, "keep"), ("lookahead", -1, "lookahead"),
    ("lookahead", 51, "lookahead"), ("state_width", 11, "state_width"), ("mode", 2, "mode"), ("mode", -1, "mode"), ("moved", 2, "moved"),
    ("moved", -1, "moved"), ("sense16", -1, "sense16"), ("sense16", 2049, "sense16"), ("dx", (3, 1025), "dx and dy"),
    ("dx", (0, -1025), "dx and dy"), ("dy", (15, 1025), "dx and dy"), ("dy", (7, -1025), "dx and dy"), ("reserved", 1, "reserved"),
    ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("ptr", 3, "NULL"), ("params", None, "NULL"),
    ("align", 1, "aligned"), ("align", 2, "aligned"), ("align", 3, "aligned")])
def test_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = good_params()
    B, ptrs = 4, [256, 512, 1024, 2048]   # state, grid, prev, actions
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2 if value < 3 else 4
    elif field == "B":
        B = value
    elif field in ("dx", "dy"):
        getattr(p, field)[value[0]] = value[1]
    elif field != "params":
        setattr(p, field, value)
    pp = None if field == "params" else C.byref(p)
    rc = L.cs_belief_actions(pp, ptrs[0], B, ptrs[1], ptrs[2], ptrs[3], None)
    assert rc == -1   # CS_E_CONFIG
    assert msg in L.cs_episodes_last_error().decode() and "cs_belief_actions" in L.cs_episodes_last_error().decode()


def test_op_and_agents_refuse_bad_integers_and_a_cpu_device():
    ops, m = _lib.torch_ops(), model("evade", 1.0, 10.0)
    state, grid, prev, act = torch.zeros(2, 57), torch.full((2, SIDE * SIDE), 65536, dtype=torch.int32), prev_of([], 2), torch.zeros(2, 3, dtype=torch.int64)
    good = dict(n_agents=3, side=SIDE, view_range=VR, keep=KEEP, lookahead=7, mode=1, moved=1, sense16=m.sense16, dx=list(m.dx), dy=list(m.dy))

    def call(state=state, grid=grid, prev=prev, act=act, **kw):
        a = dict(good, **kw)
        ops.belief_actions(state, grid, prev, act, a["n_agents"], a["side"], a["view_range"], a["keep"], a["lookahead"], a["mode"], a["moved"],
                           a["sense16"], a["dx"], a["dy"])

    for kw, msg in ((dict(n_agents=9), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"), (dict(keep=65537), "keep"),
                    (dict(lookahead=51), "lookahead"), (dict(mode=2), "mode"), (dict(moved=2), "moved"), (dict(sense16=2049), "sense16"),
                    (dict(dx=[0] * 15), "16 integers"), (dict(dy=[0] * 15 + [1025]), "-1024..1024"), (dict(dx=[-1025] + [0] * 15), "-1024..1024"),
                    (dict(grid=grid[:1]), "grid must be"), (dict(prev=prev[:, :3]), "prev must be"), (dict(act=act[:, :2]), "actions must be"),
                    (dict(state=state[:, :11]), "state must be")):
        with pytest.raises(RuntimeError, match=msg):   # integers and shapes come first: the CPU tensors are not reached
            call(**kw)
    with pytest.raises(RuntimeError, match="GPU"):   # a CPU tensor must be refused, not dereferenced
        call()
    assert bool((grid == 65536).all()) and bool((prev == 0).all()) and bool((act == 0).all())
    with pytest.raises(ValueError, match="not a GPU"):
        cs.BeliefAgents(cs.make_env_args("flight_easy"), batch=4, device="cpu")
    with pytest.raises(ValueError, match="batch"):
        cs.BeliefAgents(cs.make_env_args("flight_easy"), device="cpu", impl="torch")
    with pytest.raises(ValueError, match="impl"):
        cs.BeliefAgents(cs.make_env_args("flight_easy"), batch=4, device="cpu", impl="eager")
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=3)
    a = cs.BeliefAgents(cs.make_env_args("flight_easy", n_agents=5), motion=motion, batch=4, device="cpu", impl="torch")
    assert (a.n_agents, a.side, a.view_range, a.keep, a.lookahead, a.motion, a.model) == (5, 50, 7, KEEP, 7, motion, model("evade", 1.0, 10.0))
    assert a.grid.dtype == torch.int32 and a.grid.shape == (4, 2500) and bool((a.grid == be.FRESH).all())
    assert a.prev.dtype == torch.int32 and a.prev.shape == (4, 8, 2)
    args = cs.make_env_args("flight_easy")   # from an args namespace
    args.target_speed, args.target_motion, args.target_sense = 0.5, "evade", 4.0
    assert cs.BeliefAgents(args, batch=1, device="cpu", impl="torch").model == model("evade", 0.5, 4.0)
    env_like = types.SimpleNamespace(n_agents=3, map_size=50, view_range=7, detect_prob=0.9, batch=2, device="cpu", motion=motion)   # from an env
    assert cs.BeliefAgents(env_like, impl="torch").motion is motion


def test_belief_model_from_motion_written_out():
    def both(q):   # one quadrant (k = 0..3) -> the 16 headings of dx and of dy
        a, b, c, d = q
        dx = (a, b, c, d, 0, -d, -c, -b, -a, -b, -c, -d, 0, d, c, b)
        return dx, dx[12:] + dx[:12]
    for speed, quadrant in ((0.0, (0, 0, 0, 0)), (0.25, (4, 4, 3, 2)), (1.0, (16, 15, 11, 6)), (3.5, (56, 52, 40, 21))):
        m = be.BeliefModel.from_motion(mo.TargetMotion(mode="walk", speed=speed), SIDE)
        assert (m.dx, m.dy) == both(quadrant) and (m.mode, m.sense16) == (0, 0), speed
    assert be.BeliefModel.from_motion(mo.TargetMotion(mode="walk", speed=1.0), SIDE).dy == (0, 6, 11, 15, 16, 15, 11, 6, 0, -6, -11, -15, -16, -15, -11, -6)
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=50.0, sense=100.0), SIDE)
    assert (m.mode, m.sense16, m.dx[0], m.dy[4], m.dx[8], m.dx[2]) == (1, 1600, 800, 800, -800, 566)
    assert be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.03), SIDE).sense16 == 160
    with pytest.raises(ValueError, match="speed"):
        be.BeliefModel.from_motion(mo.TargetMotion(speed=51.0), SIDE)
    with pytest.raises(ValueError, match="dx and dy"):
        be.BeliefModel(dx=(1025,) + (0,) * 15)
    with pytest.raises(ValueError, match="sense16"):
        be.BeliefModel(mode=1, sense16=2049)


# ---- 2. the definition on hand cases ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, side", [(1, 50), (3, 50), (5, 64), (2, 7)])
def test_without_a_move_it_is_the_coverage_step_without_regrowth(n, side):
    """moved = 0 on cells in 1..65536: coverage_actions_torch with regrow = 16 adds (65536 - v) >> 16 = 0 to such a cell, so its grid
    and its actions are an independent statement of steps 3 and 4."""
    g = torch.Generator().manual_seed(10 * n + side)
    B = 6
    state = torch.cat([torch.rand(B, 2 * n, generator=g).view(B, n, 2) * 2 - 1,
                       torch.tensor([1.0, 0.0]).expand(B, n, 2)], -1).reshape(B, 4 * n).contiguous()
    grid = torch.randint(1, 65537, (B, side * side), generator=g, dtype=torch.int32)
    grid[0], grid[1, 0] = 65536, 1
    want_g, got_g, prev = grid.clone(), grid.clone(), prev_of([(123, -5)] * 8, B)
    want = bl.coverage_actions_torch(state, want_g, n, side, VR, KEEP, regrow=16)
    got = be.belief_actions_torch(state, got_g, prev, n, side, VR, KEEP, model("evade", 1.0, 10.0, side), 0)
    assert torch.equal(got, want) and torch.equal(got_g, want_g) and not torch.equal(got_g, grid)
    X, Y, _ = bl.quantise(state, n, side)
    assert torch.equal(prev[:, :n, 0], X.to(torch.int32)) and torch.equal(prev[:, :n, 1], Y.to(torch.int32))
    assert bool((prev[:, n:, 0] == 123).all()) and bool((prev[:, n:, 1] == -5).all())   # slots >= n keep their content


@pytest.mark.parametrize("speed", [0.25, 0.5, 0.9])
def test_a_walk_leaves_a_uniform_interior_exactly_uniform(speed):
    """A uniform grid of 65536: every piece is 65536 wx wy / 4096 = 16 wx wy, exact, and a cell at least 2 cells from a wall receives
    the pieces of a full neighbourhood, 16 * 16 headings * 256 / 16 = 65536."""
    g = predict(torch.full((1, SIDE * SIDE), 65536, dtype=torch.int32), prev_of([(400, 400)]), model("walk", speed)).view(SIDE, SIDE)
    assert bool((g[2:-2, 2:-2] == 65536).all())
    # the walls too: dx and dy are symmetric under k -> k + 8, so what a wall cell keeps of the mass that would have left the map
    # equals what cells beyond the wall would have sent in
    assert bool((g == 65536).all())


def test_the_total_never_grows_under_prediction():
    gen = torch.Generator().manual_seed(7)
    for side in (50, 7):
        for mode in ("walk", "evade"):
            for speed in (0.25, 1.0, 3.5, float(side)):
                grid = torch.randint(0, be.CAP + 1, (4, side * side), generator=gen, dtype=torch.int32)
                grid[1] = torch.where(torch.rand(side * side, generator=gen) < 0.9, 0, 1).to(torch.int32) * grid[1]
                grid[2] = be.CAP
                before = grid.to(torch.int64).sum(1)
                prev = prev_of([(int(v), int(w)) for v, w in torch.randint(-100, 16 * side + 100, (3, 2), generator=gen)], 4)
                predict(grid, prev, model(mode, speed, 10.0, side), n=3, side=side, agents=(OFF,) * 3)
                after = grid.to(torch.int64).sum(1)
                assert bool((after <= before).all()) and bool((grid >= 0).all()) and bool((grid <= be.CAP).all()), (side, mode, speed)


@pytest.mark.parametrize("offset", [(40, 0), (30, 25), (0, 37), (-33, 20), (-50, -3), (-20, -60), (5, -70), (64, -64)])
def test_mass_near_an_agent_moves_away_from_it(offset):
    """One cell of mass inside `sense` of one agent, speed 2: every cell the mass lands on is farther from the agent than the source
    was (a displacement of 2 cells outruns the bilinear split's one cell), and at most 4 units are lost to the four floors."""
    ix, iy, mass = 25, 20, 65531
    ax, ay = 16 * ix + 8 - offset[0], 16 * iy + 8 - offset[1]
    grid = torch.zeros(1, SIDE * SIDE, dtype=torch.int32)
    grid[0, ix * SIDE + iy] = mass
    g = predict(grid, prev_of([(ax, ay)]), model("evade", 2.0, 10.0)).view(SIDE, SIDE)
    assert mass - 4 <= int(g.sum()) <= mass
    d2 = offset[0] ** 2 + offset[1] ** 2
    for jx, jy in g.nonzero().tolist():
        assert (16 * jx + 8 - ax) ** 2 + (16 * jy + 8 - ay) ** 2 > d2, (jx, jy)
    assert 1 <= len(g.nonzero()) <= 4
    # the same cell outside the radius diffuses instead: 16 headings
    g2 = predict(grid.zero_().index_fill_(1, torch.tensor([ix * SIDE + iy]), mass), prev_of([(ax, ay)]), model("evade", 2.0, 2.0))
    assert len(g2.nonzero()) > 16


def test_mass_shoved_at_a_wall_stays_in_the_wall_cells():
    for speed in (3.5, 50.0):
        grid = torch.zeros(1, SIDE * SIDE, dtype=torch.int32)
        cells = [(0, 20), (1, 21), (2, 19)]
        for ix, iy in cells:
            grid[0, ix * SIDE + iy] = 65536
        g = predict(grid, prev_of([(100, 16 * 20 + 8)]), model("evade", speed, 10.0)).view(SIDE, SIDE)   # the agent is at larger x
        assert int(g[0].sum()) >= 3 * 65536 - 12 and int(g[1:].sum()) == 0, speed


def test_a_cell_out_of_range_is_read_as_the_bound():
    gen = torch.Generator().manual_seed(1)
    wild = torch.randint(-(1 << 21), 1 << 21, (2, SIDE * SIDE), generator=gen, dtype=torch.int32)
    wild[0, :3] = torch.tensor([-2 ** 31, 2 ** 31 - 1, be.CAP + 1], dtype=torch.int32)
    state = rows([(0.3, 0.1), (-0.5, 0.7)]).expand(2, -1).contiguous()
    for moved in (0, 1):
        g, c = wild.clone(), wild.clamp(0, be.CAP)
        p1, p2 = prev_of([(300, 300), (500, 100)], 2), prev_of([(300, 300), (500, 100)], 2)
        m = model("evade", 1.0, 10.0)
        assert torch.equal(be.belief_actions_torch(state, g, p1, 2, SIDE, VR, KEEP, m, moved),
                           be.belief_actions_torch(state, c, p2, 2, SIDE, VR, KEEP, m, moved))
        assert torch.equal(g, c) and bool((g >= 0).all()) and bool((g <= be.CAP).all())
    # prev is read clamped to +-2^15
    far, lim = prev_of([(2 ** 31 - 1, -2 ** 31)]), prev_of([(1 << 15, -(1 << 15))])
    g = torch.randint(0, 65537, (1, SIDE * SIDE), generator=gen, dtype=torch.int32)
    assert torch.equal(predict(g.clone(), far, model("evade", 1.0, 100.0)), predict(g.clone(), lim, model("evade", 1.0, 100.0)))


def test_evade_with_sense_zero_is_the_walk_except_under_an_agent():
    gen = torch.Generator().manual_seed(3)
    grid = torch.randint(0, 65537, (1, SIDE * SIDE), generator=gen, dtype=torch.int32)
    off_centre, on_centre = prev_of([(16 * 10 + 7, 16 * 12 + 8)]), prev_of([(16 * 10 + 8, 16 * 12 + 8)])
    walk = predict(grid.clone(), off_centre, model("walk", 1.0))
    assert torch.equal(predict(grid.clone(), off_centre, model("evade", 1.0, 0.0)), walk)
    under = predict(grid.clone(), on_centre, model("evade", 1.0, 0.0))
    assert not torch.equal(under, walk)
    # the cell under the agent takes heading 0 with all its mass; take that cell out and the two agree again
    grid[0, 10 * SIDE + 12] = 0
    assert torch.equal(predict(grid.clone(), on_centre, model("evade", 1.0, 0.0)), predict(grid.clone(), on_centre, model("walk", 1.0)))


def test_policy_passes_moved_as_specified():
    calls = []

    def agents(**kw):
        ag = cs.BeliefAgents(cs.make_env_args("flight_easy", n_agents=1), motion=mo.TargetMotion(**kw), batch=1, device="cpu", impl="torch")
        real = ag.choose_action
        ag.choose_action = lambda state, moved: (calls.append(bool(moved)), real(state, moved))[1]
        return ag
    s = rows([(0.2, 0.2)])
    T, F = True, False
    for kw, want in ((dict(mode="evade", speed=1.0, sense=10.0, every=1), [F, T, T, T, T, T, T, T]),
                     (dict(mode="walk", speed=0.5, every=3), [F, T, F, F, T, F, F, T]),
                     (dict(mode="walk", speed=0.0, every=1), [F] * 8)):
        calls.clear()
        ag = agents(**kw)
        pol = ag.policy()
        acts = [pol(None, s, None, t) for t in range(8)]
        assert calls == want, kw
        # against the hand-made call sequence on a second object
        ref = cs.BeliefAgents(cs.make_env_args("flight_easy", n_agents=1), motion=mo.TargetMotion(**kw), batch=1, device="cpu", impl="torch")
        for t in range(8):
            assert torch.equal(ref.choose_action(s, want[t]), acts[t])
        assert torch.equal(ref.grid, ag.grid) and torch.equal(ref.prev, ag.prev)
        g7 = ag.grid.clone()
        a0 = pol(None, s, None, 0)   # t = 0 resets
        assert torch.equal(a0, acts[0]) and not torch.equal(ag.grid, g7) and a0.dtype == torch.int64 and a0.shape == (1, 1)


# ---- 3. closed loop on the C oracle -------------------------------------------------------------------------------------------

def found_curve(policy, motion, args, B, T, n, seeds):
    """Mean number of targets found after every step, float64 [T], of `policy(state float32 [B, S], t) -> int [B, n]` on the C
    oracle; before every step the targets are moved by motion.move_targets_torch on arrays assembled from the oracle."""
    ob = orc.OracleBatch(orc.make_config(variant="flight_easy", n_agents=n), B, seeds)
    ob.reset(init=True, threads=4)
    envs = [ob.env(b) for b in range(B)]
    m = envs[0].m
    state = np.stack([e.get_state() for e in envs]).astype(np.float32)
    curve = np.zeros(T)
    tgt, agent, hdr = torch.zeros(B, 16, 2, dtype=torch.float64), torch.zeros(B, 8, 4, dtype=torch.float64), torch.zeros(B, 16, dtype=torch.int32)
    for t in range(T):
        actions = np.asarray(policy(torch.from_numpy(state), t), dtype=np.int32)
        for b, e in enumerate(envs):
            pos, found = e.targets()
            c = e.counters()
            tgt[b, :m] = torch.from_numpy(pos)
            agent[b, :n, :2] = torch.from_numpy(e.agents()[0])
            hdr[b, _lib.H_FOUND] = int(sum(1 << j for j in range(m) if found[j]))
            hdr[b, _lib.H_FLAGS], hdr[b, _lib.H_TIME_STEP] = (1 if c["win"] else 0), c["time_step"]
        moved = mo.move_targets_torch(tgt, agent, hdr, motion, args).numpy()
        for b, e in enumerate(envs):
            e.set_targets(moved[b, :m])
        ob.step(actions, freeze_done=True, threads=4)
        state = ob.state.copy()
        curve[t] = (state[:, 4 * n + 2::3] > 0.5).sum(1).mean()
    return curve


def test_belief_finds_more_evaders_than_coverage_on_the_oracle(one_thread):
    """flight_easy, 3 agents, 32 envs, seeds 1000..1031, 200 steps, freeze_done; evade, speed 1.0, sense 10, a move before every
    step: strictly more targets found by step 200 than the coverage baseline on the same seeds.  Both sides are measured here
    (a prototype with other walk headings gave 12.06 against about 9.3: the expectation, not the assertion)."""
    B, T, n = 32, 200, 3
    seeds = np.arange(B, dtype=np.uint32) + 1000
    args = cs.make_env_args("flight_easy", n_agents=n)
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    bel = cs.BeliefAgents(args, motion=motion, batch=B, device="cpu", impl="torch").policy()
    cov = cs.CoverageAgents(args, batch=B, device="cpu", impl="torch").policy()
    b = found_curve(lambda s, t: bel(None, s, None, t).numpy(), motion, args, B, T, n, seeds)
    c = found_curve(lambda s, t: cov(None, s, None, t).numpy(), motion, args, B, T, n, seeds)
    print(f"evaders found of 15 at steps 60 / 120 / 200: belief {b[59]:.2f} / {b[119]:.2f} / {b[199]:.2f}, "
          f"coverage {c[59]:.2f} / {c[119]:.2f} / {c[199]:.2f}")
    assert b[199] > c[199]
