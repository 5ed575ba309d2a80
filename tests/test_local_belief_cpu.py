"""CPU tests of the density filter under a communication range (local_belief.py, include/coopsearch.h: cs_local_belief_actions): the
boundary declares, exports and registers it and refuses bad arguments before any launch; the definition
(local_belief.local_belief_actions_torch) is BeliefAgents' definition at an unlimited range (identity A), n lone filters at range 0
(B), LocalCoverageAgents' definition without regrowth when nothing moved (C), its mask over agents is the same as parking the
unheard agents far off the map (D), and in between it does what DESIGN.md section 26 says on hand cases.  Everything is
torch.equal on integers: no tolerance, and no threshold on what the policy finds."""
import ctypes as C
import dataclasses
import os
import re
import types

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import local as lc
from cooperative_search_amd import local_belief as lb
from cooperative_search_amd import motion as mo
from local_belief_util import CAP, FAR, model, moved_at, own_bits, random_heard, random_prev, run_definition
from local_util import KEEP, LINE, SIDE, VR, boundary_rows, fresh, landed, random_grids, rows_at, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def one_thread():
    """The definition's tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def zeros_heard(B):
    return torch.zeros(B, 8, dtype=torch.int32)


def zeros_prev(B):
    return torch.zeros(B, 8, 2, dtype=torch.int32)


# ---- 1. the boundary ------------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    assert "cs_local_belief_params and" in re.search(r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_local_belief_actions\s*\(\s*const\s+cs_local_belief_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_local_belief_actions" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "cs_local_belief_actions") and len(L.cs_local_belief_actions.argtypes) == 8
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_local_belief_params \{(.*?)\}", header, flags=re.S).group(1)
    want = ["n_agents", "side", "view_range", "keep", "lookahead", "state_width", "mode", "moved", "sense16", "dx[16]", "dy[16]",
            "comm_range", "reserved"]
    assert re.findall(r"int32_t\s+(\w+(?:\[16\])?);", fields) == want
    assert [k + ("[16]" if t is not C.c_int32 else "") for k, t in _lib.CsLocalBeliefParams._fields_] == want
    assert want[:-2] == [k + ("[16]" if t is not C.c_int32 else "") for k, t in _lib.CsBeliefParams._fields_][:-1]   # cs_belief_params' fields first
    assert C.sizeof(_lib.CsLocalBeliefParams) == 4 * (9 + 32 + 2)
    schema = str(_lib.torch_ops().local_belief_actions.default._schema)
    assert schema == ("coopsearch::local_belief_actions(Tensor state, Tensor(a!) grids, Tensor(b!) prev, Tensor(c!) heard, Tensor(d!) actions, "
                      "int n_agents, int side, int view_range, int keep, int lookahead, int mode, int moved, int sense16, int[] dx, int[] dy, "
                      "int comm_range) -> ()")
    from cooperative_search_amd import build
    assert "local_belief.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "local_belief_actions")   # one ops object, no ctypes twin
    assert cs.LocalBeliefAgents is lb.LocalBeliefAgents and cs.local_belief_actions_torch is lb.local_belief_actions_torch
    # the definition imports its parts; it does not restate them
    assert lb.quantise is bl.quantise and lb.cell_centres is bl.cell_centres and lb.disc_mask is bl.disc_mask
    assert lb.greedy_choose is bl.greedy_choose and lb.links is lc.links and lb.predict_torch is be.predict_torch
    assert lb.BeliefModel is be.BeliefModel and lb.CAP is be.CAP and lb._check_comm is lc._check_comm


def good_params():
    m = model()
    return _lib.CsLocalBeliefParams(3, SIDE, VR, KEEP, 7, 57, m.mode, 1, m.sense16, (C.c_int32 * 16)(*m.dx), (C.c_int32 * 16)(*m.dy), 10, 0)


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("view_range", -1, "view_range"),
    ("view_range", 65, "view_range"), ("keep", -1, "keep"), ("keep", 65537, "keep"), ("lookahead", -1, "lookahead"),
    ("lookahead", 51, "lookahead"), ("state_width", 11, "state_width"), ("mode", 2, "mode"), ("mode", -1, "mode"), ("moved", 2, "moved"),
    ("moved", -1, "moved"), ("sense16", -1, "sense16"), ("sense16", 2049, "sense16"), ("dx", (3, 1025), "dx and dy"),
    ("dy", (7, -1025), "dx and dy"), ("comm_range", -2, "comm_range"), ("comm_range", 129, "comm_range"), ("reserved", 1, "reserved"),
    ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("ptr", 3, "NULL"), ("ptr", 4, "NULL"),
    ("params", None, "NULL"), ("align", 0, "aligned"), ("align", 1, "aligned"), ("align", 2, "aligned"), ("align", 3, "aligned"),
    ("align", 4, "aligned")])
def test_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = good_params()
    B, ptrs = 4, [256, 512, 1024, 2048, 4096]   # state, grids, prev, heard, actions
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2 if value < 4 else 4
    elif field == "B":
        B = value
    elif field in ("dx", "dy"):
        getattr(p, field)[value[0]] = value[1]
    elif field != "params":
        setattr(p, field, value)
    pp = None if field == "params" else C.byref(p)
    assert L.cs_local_belief_actions(pp, ptrs[0], B, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None) == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_local_belief_actions") and msg in err


def test_op_definition_and_agents_refuse_wrong_tensors_and_parameters():
    ops, m = _lib.torch_ops(), model()
    state, grids, prev, heard, act = torch.zeros(2, 57), fresh(2, 3, SIDE), zeros_prev(2), zeros_heard(2), torch.zeros(2, 3, dtype=torch.int64)
    good = dict(n_agents=3, side=SIDE, view_range=VR, keep=KEEP, lookahead=7, mode=1, moved=1, sense16=m.sense16, dx=list(m.dx), dy=list(m.dy),
                comm_range=10)

    def call(state=state, grids=grids, prev=prev, heard=heard, act=act, **kw):
        a = dict(good, **kw)
        ops.local_belief_actions(state, grids, prev, heard, act, a["n_agents"], a["side"], a["view_range"], a["keep"], a["lookahead"], a["mode"],
                                 a["moved"], a["sense16"], a["dx"], a["dy"], a["comm_range"])

    for kw, msg in ((dict(n_agents=9), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"), (dict(keep=65537), "keep"),
                    (dict(lookahead=51), "lookahead"), (dict(mode=2), "mode"), (dict(moved=2), "moved"), (dict(sense16=2049), "sense16"),
                    (dict(dx=[0] * 15), "16 integers"), (dict(dy=[0] * 15 + [1025]), "-1024..1024"), (dict(comm_range=-2), "comm_range"),
                    (dict(comm_range=129), "comm_range"), (dict(grids=grids[:, 0]), "grids must be"), (dict(grids=grids[:, :2]), "grids must be"),
                    (dict(prev=prev[:, :3]), "prev must be"), (dict(heard=heard[:, :3]), "heard must be"), (dict(heard=prev), "heard must be"),
                    (dict(act=act[:, :2]), "actions must be"), (dict(state=state[:, :11]), "state must be")):
        with pytest.raises(RuntimeError, match=msg):   # integers and shapes come first: the CPU tensors are not reached
            call(**kw)
    with pytest.raises(RuntimeError, match="GPU"):   # a CPU tensor must be refused, not dereferenced
        call()
    assert bool((grids == 65536).all()) and bool((prev == 0).all()) and bool((heard == 0).all()) and bool((act == 0).all())

    def define(state=state, grids=grids, prev=prev, heard=heard, mdl=m, moved=1, comm=10, n=3, la=None):
        return lb.local_belief_actions_torch(state, grids, prev, heard, n, SIDE, VR, KEEP, mdl, moved, comm, la)
    for kw, err, msg in ((dict(comm=-2), ValueError, "comm_range"), (dict(comm=129), ValueError, "comm_range"), (dict(moved=2), ValueError, "moved"),
                         (dict(la=51), ValueError, "lookahead"), (dict(n=9), ValueError, "n_agents"), (dict(mdl=(1, 160)), TypeError, "BeliefModel"),
                         (dict(grids=grids[:, 0]), ValueError, "grids must be"), (dict(grids=grids.to(torch.int64)), ValueError, "grids must be"),
                         (dict(prev=prev[:, :3]), ValueError, "prev must be"), (dict(heard=heard.to(torch.int64)), ValueError, "heard must be"),
                         (dict(heard=heard[:, :3]), ValueError, "heard must be"), (dict(state=state[:, :11]), ValueError, "state must be")):
        with pytest.raises(err, match=msg):
            define(**kw)
    args = cs.make_env_args("flight_easy")
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalBeliefAgents(args, 10, batch=4, device="cpu")
    with pytest.raises(ValueError, match="batch"):
        cs.LocalBeliefAgents(args, 10, device="cpu", impl="torch")
    with pytest.raises(ValueError, match="impl"):
        cs.LocalBeliefAgents(args, 10, batch=4, device="cpu", impl="triton")
    for comm in (-1, 2.5, 129):
        with pytest.raises(ValueError, match="comm_range"):
            cs.LocalBeliefAgents(args, comm, batch=4, device="cpu", impl="torch")
    with pytest.raises(TypeError, match="TargetMotion"):
        cs.LocalBeliefAgents(args, 10, motion="evade", batch=4, device="cpu", impl="torch")
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=3)
    a = cs.LocalBeliefAgents(cs.make_env_args("flight_easy", n_agents=5), None, motion=motion, batch=4, device="cpu", impl="torch")
    assert (a.n_agents, a.side, a.view_range, a.keep, a.lookahead, a.comm_range, a.motion, a.model) == (5, 50, 7, KEEP, 7, -1, motion, model())
    assert a.grids.dtype == torch.int32 and a.grids.shape == (4, 5, 2500) and bool((a.grids == bl.FRESH).all())
    assert a.prev.dtype == torch.int32 and a.prev.shape == (4, 8, 2) and a.heard.dtype == torch.int32 and a.heard.shape == (4, 8)
    assert cs.LocalBeliefAgents(args, 0, batch=1, device="cpu", impl="torch").comm_range == 0
    env_like = types.SimpleNamespace(n_agents=3, map_size=50, view_range=7, detect_prob=0.9, batch=2, device="cpu", motion=motion)   # from an env
    assert cs.LocalBeliefAgents(env_like, 10, impl="torch").motion is motion


# ---- 2. identities A and B ----------------------------------------------------------------------------------------------------------

SHAPES = [(3, 3, 50, 7), (2, 5, 7, 2), (2, 8, 64, 7)]   # B, n, side, view_range
MODELS = [("walk", 0.25), ("evade", 1.0), ("evade", 3.5)]


@pytest.mark.parametrize("mode, speed", MODELS)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_identity_a_unlimited_range_is_the_shared_filter(B, n, side, vr, mode, speed):
    """All n grids start equal: over 30 calls (the targets move before every call but the first) every private grid equals the grid
    belief_actions_torch leaves, and actions and prev are equal."""
    mdl = model(mode, speed, 10.0, side)
    states = walk(B, n, 30, 100 * n + side)
    grids, prev, heard = random_grids(B, n, side, 7, equal=True), random_prev(B, side, 3), zeros_heard(B)
    shared, shared_prev, taken = grids[:, 0].clone(), prev.clone(), set()
    for t, s in enumerate(states):
        got = lb.local_belief_actions_torch(s, grids, prev, heard, n, side, vr, KEEP, mdl, moved_at(t), -1)
        taken |= {int(a) for a in got.view(-1)}
        want = be.belief_actions_torch(s, shared, shared_prev, n, side, vr, KEEP, mdl, moved_at(t))
        assert torch.equal(got, want), t
        assert torch.equal(prev, shared_prev), t
        for i in range(n):
            assert torch.equal(grids[:, i], shared), (t, i)
        assert bool((heard[:, :n] == (1 << n) - 1).all()) and bool((heard[:, n:] == 0).all())
    assert len(taken) > 1


@pytest.mark.parametrize("mode, speed", MODELS)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_identity_b_range_zero_is_n_lone_filters(B, n, side, vr, mode, speed):
    """Different random grids per agent: over 30 calls agent i's grid and action equal belief_actions_torch with n_agents = 1 on its
    own four floats, with a grid and a prev of its own; the lone agent's position sits in slot 0 of that prev."""
    mdl = model(mode, speed, 10.0, side)
    states = walk(B, n, 30, 200 * n + side)
    grids, prev, heard = random_grids(B, n, side, 8), random_prev(B, side, 4), zeros_heard(B)
    lone = [grids[:, i].clone() for i in range(n)]
    lone_prev = [zeros_prev(B) for _ in range(n)]
    for i in range(n):
        lone_prev[i][:, 0] = prev[:, i]
    for t, s in enumerate(states):
        got = lb.local_belief_actions_torch(s, grids, prev, heard, n, side, vr, KEEP, mdl, moved_at(t), 0)
        for i in range(n):
            want = be.belief_actions_torch(s[:, 4 * i:4 * i + 4].contiguous(), lone[i], lone_prev[i], 1, side, vr, KEEP, mdl, moved_at(t))
            assert torch.equal(got[:, i:i + 1], want), (t, i)
            assert torch.equal(grids[:, i], lone[i]), (t, i)
            assert torch.equal(prev[:, i], lone_prev[i][:, 0]), (t, i)
        assert torch.equal(heard, own_bits(B) * (torch.arange(8) < n))


# ---- 3. identities C and D ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B, n, side, vr", SHAPES)
@pytest.mark.parametrize("comm", [-1, 0, 4])
def test_identity_c_without_a_move_it_is_local_coverage_without_regrowth(B, n, side, vr, comm):
    """moved = 0 on cells in 1..65536: local_coverage_actions_torch with regrow = 16 adds (65536 - G) >> 16 = 0 to such a cell."""
    start = random_grids(B, n, side, 9)
    start[start == 0] = 1
    for t, s in enumerate(walk(B, n, 4, 300 * n + side)):   # (one call each: a swept cell may reach 0, which regrow 16 lifts to 1)
        grids, want_g, prev, heard = start.clone(), start.clone(), random_prev(B, side, 5), random_heard(B, 6)
        got = lb.local_belief_actions_torch(s, grids, prev, heard, n, side, vr, KEEP, model("evade", 1.0, 10.0, side), 0, comm)
        want = lc.local_coverage_actions_torch(s, want_g, n, side, vr, KEEP, comm, regrow=16)
        assert torch.equal(got, want) and torch.equal(grids, want_g) and not torch.equal(grids, start), t


@pytest.mark.parametrize("B, n, side", [(3, 3, 50), (2, 5, 7), (2, 8, 64)])
def test_identity_d_the_mask_equals_parking_the_unheard_agents_off_the_map(B, n, side):
    """The prediction of agent i under its mask equals predict_torch on a copy of prev in which every agent that i did not hear
    stands at (-2^15, -2^15): a cell centre is at most 1016, so such an agent is farther than the largest sense16 (2048) from every
    cell.  Seen through the definition at range 0 and view_range 0 (no merge; a sweep only of a cell an agent stands on)."""
    assert (16 * 63 + 8 - FAR) > be.MAX_SENSE16
    mdl = dataclasses.replace(model("evade", 1.0, 10.0, side), sense16=be.MAX_SENSE16)   # the largest radius the entry point takes
    g = torch.Generator().manual_seed(n)
    state = walk(B, n, 1, 17 * n)[0]
    grids = random_grids(B, n, side, 10)
    prev = torch.randint(0, 16 * side + 1, (B, 8, 2), generator=g, dtype=torch.int32)   # on the map: every agent matters somewhere
    heard = torch.randint(0, 1 << n, (B, 8), generator=g, dtype=torch.int32)
    masks = lb.heard_masks(heard, n)
    assert not bool(masks.all()) and bool(masks.diagonal(dim1=1, dim2=2).all())
    got_g, got_p, got_h = grids.clone(), prev.clone(), heard.clone()
    lb.local_belief_actions_torch(state, got_g, got_p, got_h, n, side, 0, KEEP, mdl, 1, 0)
    differs = 0
    for i in range(n):
        parked = prev.clone()
        parked[:, :n][~masks[:, i]] = FAR
        want_g, everyone = grids.clone(), torch.full((B, 8), -1, dtype=torch.int32)
        lb.local_belief_actions_torch(state, want_g, parked, everyone, n, side, 0, KEEP, mdl, 1, 0)
        assert torch.equal(got_g[:, i], want_g[:, i]), i
        all_g = grids.clone()
        lb.local_belief_actions_torch(state, all_g, prev.clone(), everyone.clone(), n, side, 0, KEEP, mdl, 1, 0)
        differs += int(not torch.equal(all_g[:, i], got_g[:, i]))
    assert differs > 0   # the mask is not vacuous: hearing everybody predicts another grid


# ---- 4. hand cases --------------------------------------------------------------------------------------------------------------------

def spread_by_hand(ix, iy, d, m, headings, mdl, side):
    """Where the mass d of cell (ix, iy) goes along `headings` with weight m, in plain Python integers -> {cell index: mass}."""
    out = {}
    for k in headings:
        ux, uy = 16 * ix + mdl.dx[k], 16 * iy + mdl.dy[k]
        i0, fx, j0, fy = ux >> 4, ux & 15, uy >> 4, uy & 15
        for di, wx in ((0, 16 - fx), (1, fx)):
            for dj, wy in ((0, 16 - fy), (1, fy)):
                ci, cj = min(max(i0 + di, 0), side - 1), min(max(j0 + dj, 0), side - 1)
                out[ci * side + cj] = out.get(ci * side + cj, 0) + ((d * m * wx * wy) >> 12)
    return {c: min(v, CAP) for c, v in out.items() if v}


APART = [(0, 0, 0), (0, 800, 0), (800, 0, 0)]   # three cell corners, 50 cells apart: nobody is linked at range 10, nothing is swept at view_range 0


def test_an_agent_predicts_with_the_agents_it_heard_and_no_others():
    """A - B - C in a row, 8 cells apart, comm_range 10.  Call 1 (nothing moved) stores the poses and the masks: A heard A and B,
    B all three, C heard B and C.  All mass, 65536, sits in cell (30, 25), centre (488, 408): 64 sub-units from C (inside sense
    160), 192 from B and 320 from A (outside).  Call 2 (the targets moved; the agents now far apart on cell corners with view_range
    0, so nothing is swept or merged): in C's grid, and in B's, who heard C, the cell EVADES C: ex = 64, ey = 0, heading 0, dx = 16:
    all of it lands in cell (31, 25) = 1575: (65536 * 16 * 16 * 16) >> 12 = 65536.  In A's grid, whose mask lacks C, it spreads one
    sixteenth along each heading; of that, cell (31, 25) collects 4096 from heading 0 (weight 16 * 16), 2400 each from headings 1
    and 15 (15 * 10), 880 each from 2 and 14 (11 * 5) and 96 each from 3 and 13 (6 * 1): 10848."""
    n, comm, mdl = 3, 10, model("evade", 1.0, 10.0)
    assert (mdl.dx[:4], mdl.dy[:4], mdl.sense16) == ((16, 15, 11, 6), (0, 6, 11, 15), 160)
    line = rows_at([LINE], SIDE)
    assert landed(line, n, SIDE) == [[(x, y) for x, y, _ in LINE]]
    src, dst = 30 * SIDE + 25, 31 * SIDE + 25
    grids = torch.zeros(1, n, SIDE * SIDE, dtype=torch.int32)
    grids[:, :, src] = 65536
    prev, heard = zeros_prev(1), zeros_heard(1)
    lb.local_belief_actions_torch(line, grids, prev, heard, n, SIDE, 0, KEEP, mdl, 0, comm)
    assert heard[0, :3].tolist() == [0b011, 0b111, 0b110] and not bool(heard[0, 3:].any())
    assert prev[0, :3].tolist() == [[x, y] for x, y, _ in LINE]
    assert bool((grids[0, :, src] == 65536).all()) and int(grids.sum()) == 3 * 65536   # nobody stands on (30, 25): nothing swept
    apart = rows_at([APART], SIDE)
    assert landed(apart, n, SIDE) == [[(x, y) for x, y, _ in APART]]
    lb.local_belief_actions_torch(apart, grids, prev, heard, n, SIDE, 0, KEEP, mdl, 1, comm)
    evaded = torch.zeros(SIDE * SIDE, dtype=torch.int32)
    evaded[dst] = 65536
    assert dst == 1575 and torch.equal(grids[0, 2], evaded) and torch.equal(grids[0, 1], evaded)
    by_hand = spread_by_hand(30, 25, 65536, 1, range(16), mdl, SIDE)
    assert by_hand[dst] == 4096 + 2 * 2400 + 2 * 880 + 2 * 96 == 10848 and by_hand == spread_by_hand(30, 25, 65536, 1, range(16), mdl, SIDE)
    assert spread_by_hand(30, 25, 65536, 16, [0], mdl, SIDE) == {dst: 65536}
    diffused = torch.zeros(SIDE * SIDE, dtype=torch.int32)
    for c, v in by_hand.items():
        diffused[c] = v
    assert torch.equal(grids[0, 0], diffused) and int(grids[0, 0, dst]) == 10848
    assert heard[0, :3].tolist() == [0b001, 0b010, 0b100]   # and now nobody hears anybody


def test_the_minimum_merge_keeps_the_lower_estimate():
    """The same two calls with the agents still in line at call 2: A hears B, whose post-sweep grid holds the evaded mass -- 65536 in
    (31, 25) and 0 elsewhere -- while A's own holds the diffusion.  The minimum keeps 10848 in (31, 25) and nothing else, in A's grid
    and in B's, who hears A: mass is lost where predictions disagree (the module docstring says so).  C hears B and not A: the
    merge reads post-sweep grids, one hop per call, so C, who agrees with B, keeps all of it."""
    n, mdl = 3, model("evade", 1.0, 10.0)
    line = rows_at([LINE], SIDE)
    grids = torch.zeros(1, n, SIDE * SIDE, dtype=torch.int32)
    grids[:, :, 30 * SIDE + 25] = 65536
    prev, heard = zeros_prev(1), zeros_heard(1)
    for moved in (0, 1):
        lb.local_belief_actions_torch(line, grids, prev, heard, n, SIDE, 0, KEEP, mdl, moved, 10)
    assert [int(g.sum()) for g in grids[0]] == [10848, 10848, 65536] and int(grids[0, 0, 1575]) == int(grids[0, 1, 1575]) == 10848


def test_the_link_test_is_strict_and_shows_in_heard():
    """Exactly 16 comm_range sub-units apart: not linked; one sub-unit less: linked."""
    state = boundary_rows(10)
    assert landed(state, 2, SIDE) == [[(168, 408), (328, 408)], [(168, 408), (327, 408)]]
    grids, prev, heard = fresh(2, 2, SIDE), zeros_prev(2), random_heard(2, 1)
    keep = heard[:, 2:].clone()
    lb.local_belief_actions_torch(state, grids, prev, heard, 2, SIDE, VR, KEEP, model(), 0, 10)
    assert heard[:, :2].tolist() == [[0b01, 0b10], [0b11, 0b11]]
    assert torch.equal(heard[:, 2:], keep)   # slots >= n keep their content
    assert not torch.equal(grids[0, 0], grids[0, 1]) and torch.equal(grids[1, 0], grids[1, 1])


@pytest.mark.parametrize("mode", ["walk", "evade"])
def test_garbage_bits_and_a_missing_own_bit_in_heard_do_not_matter(mode):
    B, n, side = 3, 3, 50
    mdl = model(mode, 1.0, 10.0)
    states = walk(B, n, 2, 41)
    g = torch.Generator().manual_seed(2)
    clean = torch.randint(0, 1 << n, (B, 8), generator=g, dtype=torch.int32) | own_bits(B)
    dirty = (clean & ~own_bits(B)) | (random_heard(B, 3) & ~((1 << n) - 1))   # own bit cleared, bits at and above n random
    dirty[:, n:] = random_heard(B, 4)[:, n:]
    assert bool((dirty[:, :n] != clean[:, :n]).all())
    grids, prev = random_grids(B, n, side, 11), random_prev(B, side, 12)
    always = lambda t: 1
    want = run_definition(states, grids, prev, clean, n, side, VR, mdl, 10, moved=always)
    got = run_definition(states, grids, prev, dirty, n, side, VR, mdl, 10, moved=always)
    for (wg, wp, wh, wa), (gg, gp, gh, ga) in zip(want, got):
        assert torch.equal(wg, gg) and torch.equal(wp, gp) and torch.equal(wa, ga) and torch.equal(wh[:, :n], gh[:, :n])
    assert torch.equal(got[0][2][:, n:], dirty[:, n:])


def test_the_first_call_after_reset_with_a_move_is_well_defined():
    """heard is zero after reset(): with moved = 1 each agent evades only itself -- the result of a call whose masks hold the own
    bits, and (three agents within sense of one another) another one than hearing everybody gives."""
    B, n = 2, 3
    args = cs.make_env_args("flight_easy", n_agents=n)
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    ag = cs.LocalBeliefAgents(args, 10, motion=motion, batch=B, device="cpu", impl="torch")
    ag.heard.fill_(-1)
    ag.grids.fill_(7)
    ag.reset()
    assert not bool(ag.heard.any()) and not bool(ag.prev.any()) and bool((ag.grids == bl.FRESH).all())
    close = rows_at([[(392, 392, 0), (408, 408, 3), (424, 392, 7)]] * B, SIDE, tail=45)
    ag.prev[:, :n] = torch.tensor([[392, 392], [408, 408], [424, 392]], dtype=torch.int32)
    prev0 = ag.prev.clone()
    got = ag.choose_action(close, 1)
    results = []
    for h in (own_bits(B), torch.full((B, 8), -1, dtype=torch.int32)):
        g, p = fresh(B, n, SIDE), prev0.clone()
        a = lb.local_belief_actions_torch(close, g, p, h, n, SIDE, VR, KEEP, ag.model, 1, 10)
        results.append((g, a))
    assert torch.equal(ag.grids, results[0][0]) and torch.equal(got, results[0][1])
    assert not torch.equal(ag.grids, results[1][0])
    assert bool((ag.heard[:, :n] == 0b111).all())


@pytest.mark.parametrize("mode, speed, comm", [("walk", 0.25, 10), ("evade", 1.0, 10), ("evade", 3.5, 2), ("evade", 1.0, -1)])
def test_mass_is_monotone(mode, speed, comm):
    """Floors, the cap, the sweep and the minimum only lose mass: the sum over each private grid never grows over 30 calls."""
    B, n, side = 3, 3, 50
    states = walk(B, n, 30, 77)
    out = run_definition(states, random_grids(B, n, side, 13), random_prev(B, side, 14), zeros_heard(B), n, side, VR,
                         model(mode, speed, 10.0), comm, moved=lambda t: 1)
    sums = torch.stack([g.to(torch.int64).sum(-1) for g, _, _, _ in out])   # [calls, B, n]
    assert bool((sums[1:] <= sums[:-1]).all()) and bool((sums[-1] < sums[0]).all())


# ---- 5. the class as a policy -----------------------------------------------------------------------------------------------------------

def test_policy_resets_at_step_zero_and_passes_moved_as_specified():
    args = cs.make_env_args("flight_easy", n_agents=3)
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=3)
    ag = cs.LocalBeliefAgents(args, 10, motion=motion, batch=2, device="cpu", impl="torch")
    seen = []
    inner = ag.choose_action
    ag.choose_action = lambda state, moved: (seen.append(bool(moved)), inner(state, moved))[1]
    pol = ag.policy()
    states = walk(2, 3, 6, 9, tail=45)
    first = [pol(None, s, None, t) for t, s in enumerate(states)]
    assert seen == [be.targets_moved(motion, t) for t in range(6)] == [False, True, False, False, True, False]
    g_end = ag.grids.clone()
    again = [pol(None, s, None, t) for t, s in enumerate(states)]   # t = 0 resets: the second flight equals the first
    assert all(torch.equal(a, b) for a, b in zip(first, again)) and torch.equal(ag.grids, g_end)
    assert first[0].shape == (2, 3) and first[0].dtype == torch.int64


def test_label_episodes_takes_the_class_through_the_rows_path():
    """Unlimited range labels recorded rows as BeliefAgents does; the second episode ends after three rows."""
    E, T, n = 2, 5, 3
    s = torch.stack(walk(E, n, T, 12, tail=45), 1)
    padded = torch.zeros(E, T, 1)
    padded[1, 3:] = 1.0
    batch = {"s": s, "padded": padded}
    args = cs.make_env_args("flight_easy", n_agents=n)
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    local = cs.LocalBeliefAgents(args, None, motion=motion, batch=E, device="cpu", impl="torch")
    shared = cs.BeliefAgents(args, motion=motion, batch=E, device="cpu", impl="torch")
    got, want = cs.label_episodes(local, batch, impl="rows"), cs.label_episodes(shared, batch, impl="rows")
    assert torch.equal(got, want) and got.shape == (E, T, n) and not bool(got[1, 3:].any())
    assert bool((local.grids == bl.FRESH).all()) and not bool(local.heard.any())   # the rows path ends with reset()
