"""CPU tests of the forecast planner on private grids (local_forecast.py, include/coopsearch.h: cs_local_belief_forecast and
cs_local_plan_forecast_actions): the boundary declares, exports and registers both and refuses bad arguments before any launch; the
definitions are ForecastAgents' with all-heard masks, an unlimited range and equal inputs (identity A), n lone forecasters and planners
with own-bit masks and range 0 (B), do not let a later agent change an earlier one (C), read a mask as parking the unheard agents far
away (D), are local_plan's on identical levels (E), ignore the mask in walk mode (F), and in between do what a restatement per env and
per agent says; LocalForecastAgents is LocalPlanAgents(base="belief") on static targets and ForecastAgents at an unlimited range.
Everything is torch.equal on integers: no tolerance, and no threshold on what the policy finds.  Every test that relies on two results
being different asserts that they are."""
import ctypes as C
import os
import re

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import forecast as fc
from cooperative_search_amd import gridobs as go
from cooperative_search_amd import imitate as im
from cooperative_search_amd import local as lc
from cooperative_search_amd import local_belief as lb
from cooperative_search_amd import local_forecast as lf
from cooperative_search_amd import local_plan as lp
from cooperative_search_amd import localobs as lo
from cooperative_search_amd import motion as mo
from cooperative_search_amd import plan as pl
from local_belief_util import FAR, own_bits
from local_forecast_util import (CAP, MIXED, MOVES, PARAMS3, SHAPES, forecast_by_hand, forecast_case, forecast_inputs, mdl, moves_for,
                                 plan_by_hand, plan_case, plan_inputs)
from local_util import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = torch.full((1, 8), -1, dtype=torch.int32)   # every bit set: everybody heard everybody


@pytest.fixture(autouse=True)
def one_thread():
    """The definitions' tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def same(got, want):
    return all(torch.equal(g, w) for g, w in zip(got, want))


def plan(state, stacks, n, side, vr, depth, stride, discount, comm):
    return lf.local_plan_forecast_actions_torch(state, stacks, n, side, vr, depth, stride, discount, comm, return_plans=True)


# ---- 1. the boundary ------------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    version = re.search(r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    assert "cs_local_belief_forecast and" in version and "cs_local_plan_forecast_actions" in version
    assert "no existing export or struct changed" in version
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_local_belief_forecast\s*\(\s*const\s+cs_forecast_params\s*\*", header)
    assert re.search(r"\bint\s+cs_local_plan_forecast_actions\s*\(\s*const\s+cs_local_plan_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_local_belief_forecast" in _lib.EXPORTS and "cs_local_plan_forecast_actions" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.cs_local_belief_forecast.argtypes) == 7 and L.cs_local_belief_forecast.restype is C.c_int
    assert len(L.cs_local_plan_forecast_actions.argtypes) == 8 and L.cs_local_plan_forecast_actions.restype is C.c_int
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    ops = _lib.torch_ops()
    assert str(ops.local_belief_forecast.default._schema) == (
        "coopsearch::local_belief_forecast(Tensor grids, Tensor prev, Tensor heard, Tensor(a!) stacks, int n_agents, int side, int mode, "
        "int sense16, int[] dx, int[] dy, int[] moves) -> ()")
    assert str(ops.local_plan_forecast_actions.default._schema) == (
        "coopsearch::local_plan_forecast_actions(Tensor state, Tensor stacks, Tensor(a!) actions, Tensor(b!) plans, Tensor(c!) scores, "
        "int n_agents, int side, int view_range, int depth, int stride, int discount, int comm_range) -> ()")
    from cooperative_search_amd import build
    assert "local_forecast.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "local_belief_forecast")   # one ops object, no ctypes twin
    assert cs.LocalForecastAgents is lf.LocalForecastAgents and cs.local_forecast_torch is lf.local_forecast_torch
    assert cs.local_plan_forecast_actions_torch is lf.local_plan_forecast_actions_torch
    # the definitions import their parts; they do not restate them
    assert lf.forecast_torch is fc.forecast_torch and lf.plan_forecast_actions_torch is fc.plan_forecast_actions_torch
    assert lf.segment_moves is fc.segment_moves and lf.heard_masks is lb.heard_masks and lf.heard_prev is lb.heard_prev
    assert lf.links is lc.links and lf._check_comm is lc._check_comm and lf.sequence_points is pl.sequence_points and lf.CAP is pl.CAP
    assert lf.quantise is bl.quantise and lf.cell_centres is bl.cell_centres and lf.disc_mask is bl.disc_mask
    episodes = open(os.path.join(ROOT, "cooperative-search_amd", "csrc", "episodes.hip")).read()
    assert episodes.index('#include "forecast.h"') < episodes.index('#include "local_forecast.h"') > episodes.index('#include "local_plan.h"')
    table = open(os.path.join(ROOT, "profiles", "kernel_resources.txt")).read()
    for kernel in ("k_local_belief_forecast", "k_local_plan_forecast_actions"):
        line = re.search(rf"^{kernel}\s.*$", table, flags=re.M).group(0)
        assert re.search(r"vgpr_spill\s+0\s+scratch\s+0\b", line), line


def forecast_params():
    p = _lib.CsForecastParams(3, 50, 4, 1, 160)
    for d in range(4):
        p.moves[d] = 1
    return p


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("levels", 0, "levels"),
    ("levels", 6, "levels"), ("mode", 2, "mode"), ("sense16", -1, "sense16"), ("sense16", 2049, "sense16"), ("reserved", 1, "reserved"),
    ("moves", (0, -1), "moves"), ("moves", (1, 9), "moves"), ("moves", (4, 1), "moves"), ("dx", 1025, "dx and dy"), ("dy", -1025, "dx and dy"),
    ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("ptr", 3, "NULL"), ("params", None, "NULL"),
    ("align", 0, "aligned"), ("align", 1, "aligned"), ("align", 2, "aligned"), ("align", 3, "aligned")])
def test_forecast_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = forecast_params()
    B, ptrs = 4, [256, 512, 1024, 2048]   # grids, prev, heard, stacks
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2
    elif field == "B":
        B = value
    elif field == "moves":
        p.moves[value[0]] = value[1]
    elif field in ("dx", "dy"):
        getattr(p, field)[5] = value
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_local_belief_forecast(None if field == "params" else C.byref(p), ptrs[0], ptrs[1], ptrs[2], B, ptrs[3], None)
    assert rc == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_local_belief_forecast") and msg in err


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("view_range", -1, "view_range"),
    ("view_range", 65, "view_range"), ("depth", 0, "depth"), ("depth", 6, "depth"), ("stride", 0, "stride"), ("stride", 9, "stride"),
    ("discount", -1, "discount"), ("discount", 257, "discount"), ("state_width", 11, "state_width"), ("comm_range", -2, "comm_range"),
    ("comm_range", 129, "comm_range"), ("reserved", 1, "reserved"), ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"),
    ("ptr", 2, "NULL"), ("ptr", 3, "NULL"), ("ptr", 4, "NULL"), ("params", None, "NULL"), ("align", 0, "aligned"), ("align", 1, "aligned"),
    ("align", 2, "aligned"), ("align", 3, "aligned"), ("align", 4, "aligned")])
def test_plan_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    L = _lib.load()
    p = _lib.CsLocalPlanParams(3, 50, 7, 4, 3, 230, 57, 10, 0)
    B, ptrs = 4, [256, 512, 1024, 2048, 4096]   # state, stacks, actions, plans, scores
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2 if value < 2 else 4
    elif field == "B":
        B = value
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_local_plan_forecast_actions(None if field == "params" else C.byref(p), ptrs[0], B, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None)
    assert rc == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_local_plan_forecast_actions") and msg in err


def test_the_ops_refuse_bad_integers_shapes_and_cpu_tensors():
    ops = _lib.torch_ops()
    m = mdl(50)
    grids, prev, heard = torch.zeros(2, 3, 2500, dtype=torch.int32), torch.zeros(2, 8, 2, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32)
    stacks = torch.full((2, 3, 4, 2500), -7, dtype=torch.int32)

    def forecast(grids=grids, prev=prev, heard=heard, stacks=stacks, n=3, side=50, mode=m.mode, sense16=m.sense16, dx=m.dx, dy=m.dy,
                 moves=(1, 1, 1, 1)):
        ops.local_belief_forecast(grids, prev, heard, stacks, n, side, mode, sense16, list(dx), list(dy), list(moves))

    for kw, msg in ((dict(n=9), "n_agents"), (dict(side=65), "side"), (dict(mode=2), "mode"), (dict(sense16=2049), "sense16"),
                    (dict(dx=m.dx[:15]), "dx"), (dict(moves=()), "moves must hold"), (dict(moves=(1,) * 6), "moves must hold"),
                    (dict(moves=(1, 9, 1, 1)), "moves must be"), (dict(moves=(1, -1, 1, 1)), "moves must be"),
                    (dict(grids=grids[:, 0]), "grids must be"), (dict(grids=grids[:, :2]), "grids must be"),
                    (dict(grids=grids[:, :, :-1]), "grids must be"), (dict(prev=prev[:, :7]), "prev must be"), (dict(heard=heard[:1]), "heard must be"),
                    (dict(stacks=stacks[:, :, :3]), "stacks must be"), (dict(stacks=stacks[:, :2]), "stacks must be")):
        with pytest.raises(RuntimeError, match="local_belief_forecast: " + msg):   # integers and shapes come first
            forecast(**kw)
    with pytest.raises(RuntimeError, match="GPU"):   # a CPU tensor must be refused, not dereferenced
        forecast()
    state = torch.zeros(2, 57)
    outs = [torch.full((2, 3), -7, dtype=torch.int64) for _ in range(3)]
    good = dict(n_agents=3, side=50, view_range=7, depth=4, stride=3, discount=230, comm_range=10)

    def search(state=state, stacks=stacks, outs=outs, **kw):
        a = dict(good, **kw)
        ops.local_plan_forecast_actions(state, stacks, *outs, a["n_agents"], a["side"], a["view_range"], a["depth"], a["stride"], a["discount"],
                                        a["comm_range"])

    for kw, msg in ((dict(n_agents=9), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"), (dict(depth=0), "depth"),
                    (dict(depth=6), "depth"), (dict(stride=0), "stride"), (dict(stride=9), "stride"), (dict(discount=257), "discount"),
                    (dict(comm_range=-2), "comm_range"), (dict(comm_range=129), "comm_range"), (dict(stacks=stacks[:, 0]), "stacks must be"),
                    (dict(stacks=stacks[:, :, :3]), "stacks must be"), (dict(depth=3), "stacks must be"), (dict(stacks=stacks[:1]), "stacks must be"),
                    (dict(state=state[:, :11]), "state must be"), (dict(outs=[outs[0][:, :2], outs[1], outs[2]]), "actions must be"),
                    (dict(outs=[outs[0], outs[1][:1], outs[2]]), "plans must be"), (dict(outs=[outs[0], outs[1], outs[2][:, :2]]), "scores must be")):
        with pytest.raises(RuntimeError, match="local_plan_forecast_actions: " + msg):
            search(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        search()
    assert all(bool((o == -7).all()) for o in outs) and bool((stacks == -7).all())


def test_the_definitions_refuse_bad_moves_shapes_and_dtypes():
    m = mdl(50)
    grids, prev, heard = torch.zeros(2, 3, 2500, dtype=torch.int32), torch.zeros(2, 8, 2, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32)

    def forecast(grids=grids, prev=prev, heard=heard, n=3, side=50, model=m, moves=(1, 0, 2)):
        return lf.local_forecast_torch(grids, prev, heard, n, side, model, moves)

    out = forecast()
    assert out.shape == (2, 3, 3, 2500) and out.dtype == torch.int32
    for kw in (dict(moves=()), dict(moves=(1,) * 6), dict(moves=(1, 9)), dict(moves=(-1,)), dict(n=9, grids=torch.zeros(2, 9, 2500, dtype=torch.int32)),
               dict(side=65, grids=torch.zeros(2, 3, 4225, dtype=torch.int32))):
        with pytest.raises(ValueError, match="forecast: "):
            forecast(**kw)
    for kw in (dict(grids=grids[:, 0]), dict(grids=grids[:, :2]), dict(n=0), dict(grids=grids[:, :, :-1]), dict(grids=grids.long())):
        with pytest.raises(ValueError, match="forecast: grid"):
            forecast(**kw)
    for kw in (dict(prev=prev[:, :7]), dict(prev=prev.long()), dict(prev=prev[:1])):
        with pytest.raises(ValueError, match="forecast: pos must be"):
            forecast(**kw)
    for kw in (dict(heard=heard[:, :7]), dict(heard=heard.long()), dict(heard=heard[:1])):
        with pytest.raises(ValueError, match="local forecast: heard must be"):
            forecast(**kw)
    with pytest.raises(TypeError, match="BeliefModel"):
        forecast(model="evade")
    with pytest.raises(TypeError, match="local forecast:"):
        forecast(heard=heard.tolist())
    state, stacks = torch.zeros(2, 17), torch.zeros(2, 3, 4, 2500, dtype=torch.int32)
    good = dict(n_agents=3, side=50, view_range=7, depth=4, stride=3, discount=230, comm_range=10)

    def search(state=state, stacks=stacks, **kw):
        return lf.local_plan_forecast_actions_torch(state, stacks, **dict(good, **kw))

    assert search().shape == (2, 3) and all(t.shape == (2, 3) and t.dtype == torch.int64 for t in search(return_plans=True))
    for kw in (dict(comm_range=-2), dict(comm_range=129)):
        with pytest.raises(ValueError, match="comm_range"):
            search(**kw)
    for kw in (dict(n_agents=0), dict(n_agents=9), dict(side=65), dict(view_range=65), dict(depth=0), dict(depth=6), dict(stride=0),
               dict(stride=9), dict(discount=-1), dict(discount=257)):
        with pytest.raises(ValueError, match="plan:"):
            search(**kw)
    for kw in (dict(state=state[:, :11]), dict(state=state[0]), dict(state=state.double())):
        with pytest.raises(ValueError, match="local forecast plan: state must be"):
            search(**kw)
    for kw in (dict(stacks=stacks[:, 0]), dict(stacks=stacks[:, :2]), dict(stacks=stacks[:1]), dict(stacks=stacks[:, :, :3]), dict(depth=3),
               dict(stacks=stacks.long()), dict(stacks=stacks[..., :-1])):
        with pytest.raises(ValueError, match="local forecast plan: stacks must be"):
            search(**kw)
    with pytest.raises(TypeError, match="local forecast plan:"):
        search(stacks=stacks.tolist())
    assert not bool(stacks.any()) and not bool(grids.any())   # read only


# ---- 2. the forecast: identities A, B, C, D and F, and the restatement -------------------------------------------------------------

@pytest.mark.parametrize("moves", MOVES)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_forecast_identities_a_and_b_and_the_mask_matters(B, n, side, vr, moves):
    grids, prev, heard, masked = forecast_case(B, n, side, moves)
    before = [t.clone() for t in (grids, prev, heard)]
    m = mdl(side)
    equal = grids[:, :1].expand(B, n, side * side).contiguous()
    shared = fc.forecast_torch(equal[:, 0], prev, n, side, m, moves)
    got = lf.local_forecast_torch(equal, prev, ALL.expand(B, 8).contiguous(), n, side, m, moves)   # A: everybody heard everybody
    lone = lf.local_forecast_torch(grids, prev, own_bits(B), n, side, m, moves)                     # B: everybody heard itself alone
    zeros = lf.local_forecast_torch(grids, prev, torch.zeros(B, 8, dtype=torch.int32), n, side, m, moves)   # (the own bit is set on reading)
    for i in range(n):
        assert torch.equal(got[:, i], shared), i
        pos = prev.clone()
        pos[:, 0] = prev[:, i]
        assert torch.equal(lone[:, i], fc.forecast_torch(grids[:, i], pos, 1, side, m, moves)), i
    assert torch.equal(zeros, lone)
    allheard = lf.local_forecast_torch(grids, prev, ALL.expand(B, 8).contiguous(), n, side, m, moves)
    assert int((masked != allheard).sum()) >= 80 and int((masked != lone).sum()) >= 80   # the random masks are neither extreme
    assert masked.shape == (B, n, len(moves), side * side) and int(masked.min()) >= 0 and int(masked.max()) <= CAP
    if moves[0] == 0:   # level 0 is a copy of the clamped grid
        assert torch.equal(masked[:, :, 0], grids.clamp(0, CAP))
    assert same((grids, prev, heard), before)   # read only


@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_forecast_identities_c_d_f_and_the_restatement_by_hand(B, n, side, vr):
    moves = MOVES[1]
    grids, prev, heard, masked = forecast_case(B, n, side, moves)
    m = mdl(side)
    for k in range(1, n):   # C: the bits of agents k .. n-1 in the words of agents < k are dropped when the team ends at k
        part = lf.local_forecast_torch(grids[:, :k].contiguous(), prev, heard, k, side, m, moves)
        low = heard & ((1 << k) - 1)
        assert torch.equal(part, lf.local_forecast_torch(grids, prev, low, n, side, m, moves)[:, :k]), k
    known = lb.heard_masks(heard, n)
    for i in range(n):   # D: the mask is parking every unheard agent at (-2^15, -2^15)
        parked = prev.clone()
        parked[:, :n] = torch.where(known[:, i].unsqueeze(-1), prev[:, :n], torch.full_like(prev[:, :n], FAR))
        assert torch.equal(masked[:, i], fc.forecast_torch(grids[:, i], parked, n, side, m, moves)), i
    assert torch.equal(masked, forecast_by_hand(grids, prev, heard, n, side, m, moves))
    w = mdl(side, "walk")   # F: a random walk senses nobody
    walked = forecast_case(B, n, side, moves, "walk")[3]
    assert torch.equal(walked, lf.local_forecast_torch(grids, prev, own_bits(B), n, side, w, moves))
    assert torch.equal(walked, lf.local_forecast_torch(grids, prev, ALL.expand(B, 8).contiguous(), n, side, w, moves))
    assert not torch.equal(walked, masked)


# ---- 3. the search: identities A, B, C and E, and the restatement ------------------------------------------------------------------

@pytest.mark.parametrize("depth, stride, discount", PARAMS3)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_search_identities_a_b_and_e(B, n, side, vr, depth, stride, discount):
    state, stacks = plan_inputs(B, n, side, depth)
    before = stacks.clone()
    equal = stacks[:, :1].expand(B, n, depth, side * side).contiguous()
    shared = fc.plan_forecast_actions_torch(state, equal[:, 0].contiguous(), n, side, vr, depth, stride, discount, return_plans=True)
    assert same(plan(state, equal, n, side, vr, depth, stride, discount, -1), shared)                      # A
    assert same(plan(state, equal, n, side, vr, depth, stride, discount, 128), shared)                     # (128 cells reach across any map)
    zero = plan_case(B, n, side, vr, depth, stride, discount, 0)[2]
    for i in range(n):                                                                                     # B
        lone = fc.plan_forecast_actions_torch(state[:, 4 * i:4 * i + 4].contiguous(), stacks[:, i].contiguous(), 1, side, vr, depth, stride,
                                              discount, return_plans=True)
        assert same([t[:, i:i + 1] for t in zero], lone), i
    comm = MIXED[B, n, side]
    level = stacks[:, :, depth - 1].contiguous()                                                           # E: identical levels
    flat = level.unsqueeze(2).expand(B, n, depth, side * side).contiguous()
    plain = lp.local_plan_actions_torch(state, level, n, side, vr, depth, stride, discount, comm, return_plans=True)
    assert same(plan(state, flat, n, side, vr, depth, stride, discount, comm), plain)
    mixed = plan_case(B, n, side, vr, depth, stride, discount, comm)[2]
    assert bool((mixed[2] != plain[2]).any(0).all())   # on the forecast every agent scores otherwise than on one level of it
    unforecast = lp.local_plan_actions_torch(state, forecast_inputs(B, n, side)[0], n, side, vr, depth, stride, discount, comm, return_plans=True)
    assert bool((mixed[2] != unforecast[2]).any(0).all())   # ... and otherwise than the plain local planner on the grid it was forecast from
    assert torch.equal(stacks, before)
    assert torch.equal(mixed[0], lf.local_plan_forecast_actions_torch(state, stacks, n, side, vr, depth, stride, discount, comm))
    assert torch.equal(mixed[0], mixed[1] // 3 ** (depth - 1)) and bool(((mixed[1] >= 0) & (mixed[1] < 3 ** depth)).all())


@pytest.mark.parametrize("depth, stride, discount", PARAMS3)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_search_identity_c_and_a_mixed_range_is_neither_extreme(B, n, side, vr, depth, stride, discount):
    state, stacks = plan_inputs(B, n, side, depth)
    results = {}
    for comm in (-1, 0, MIXED[B, n, side]):
        full = results[comm] = plan_case(B, n, side, vr, depth, stride, discount, comm)[2]
        for k in range(1, n):
            part = plan(state[:, :4 * k].contiguous(), stacks[:, :k].contiguous(), k, side, vr, depth, stride, discount, comm)
            assert same([t[:, :k] for t in full], part), (comm, k)
    mixed, differs = results[MIXED[B, n, side]], lambda a, b: not (torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]))
    assert differs(mixed, results[0]) or differs(mixed, results[-1])
    if (depth, stride, discount) == PARAMS3[0]:
        assert differs(mixed, results[0]) and differs(mixed, results[-1])


@pytest.mark.parametrize("depth, stride, discount", [PARAMS3[0], PARAMS3[2]])
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_search_equals_the_restatement_by_hand_at_the_mixed_range(B, n, side, vr, depth, stride, discount):
    comm = MIXED[B, n, side]
    state, stacks, got = plan_case(B, n, side, vr, depth, stride, discount, comm)
    X, Y, _ = bl.quantise(state, n, side)
    adj = lc.links(X, Y, comm)
    off = ~torch.eye(n, dtype=torch.bool)
    assert bool(adj[:, off].any()) and not bool(adj[:, off].all())
    assert same(got, plan_by_hand(state, stacks, n, side, vr, depth, stride, discount, comm))


# ---- 4. the class -----------------------------------------------------------------------------------------------------------------

def fly(agents, T, seed, n=3, B=4):
    pol, out = agents.policy(), []
    for t, s in enumerate(walk(B, n, T, seed, tail=45)):
        out.append(pol(None, s, None, t).clone())
    return out


def test_static_targets_fly_the_plain_local_planner():
    """speed 0: no move falls into any horizon, nothing is forecast and the call IS LocalPlanAgents(base='belief').choose_action."""
    args, B, T = cs.make_env_args("flight_easy", n_agents=3), 4, 12
    still = mo.TargetMotion(mode="evade", speed=0.0, sense=10.0)
    ours = cs.LocalForecastAgents(args, 15, motion=still, depth=3, batch=B, device="cpu", impl="torch")
    plain = cs.LocalPlanAgents(args, 15, base="belief", motion=still, depth=3, batch=B, device="cpu", impl="torch")
    assert same(fly(ours, T, 21), fly(plain, T, 21))
    assert same((ours.grids, ours.plans, ours.scores), (plain.grids, plain.plans, plain.scores)) and not bool(ours.stacks.any())
    moving = cs.LocalForecastAgents(args, 15, motion=mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), depth=3, batch=B, device="cpu",
                                    impl="torch")
    assert not same(fly(moving, T, 21), fly(plain, T, 21)) and bool(moving.stacks.any())   # with moves it is another policy


@pytest.mark.parametrize("every", [1, 2])
def test_unlimited_range_flies_forecast_agents(every):
    args, B, T = cs.make_env_args("flight_easy", n_agents=3), 4, 12
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=every)
    ours = cs.LocalForecastAgents(args, None, motion=motion, depth=3, batch=B, device="cpu", impl="torch")
    shared = cs.ForecastAgents(args, motion=motion, depth=3, batch=B, device="cpu", impl="torch")
    pol, pol_shared, taken = ours.policy(), shared.policy(), set()
    for t, s in enumerate(walk(B, 3, T, 23, tail=45)):
        a = pol(None, s, None, t)
        assert torch.equal(a, pol_shared(None, s, None, t)) and torch.equal(ours.plans, shared.plans) and torch.equal(ours.scores, shared.scores), t
        if t > 0:   # (at t == 0 nobody has heard anybody yet: heard is this call's links from the first call on)
            for i in range(3):
                assert torch.equal(ours.stacks[:, i], shared.stack) and torch.equal(ours.grids[:, i], shared.grid), (t, i)
        taken |= set(a.flatten().tolist())
    assert len(taken) >= 2


@pytest.mark.parametrize("every", [1, 2])
def test_choose_action_forecasts_with_the_moves_of_the_schedule(every, monkeypatch):
    """Against a MovingTargetEnv's schedule (a move precedes step u iff u % every == 0): the moves handed to the forecast are
    segment_moves' of the step, the forecast reads what the base just left, and the decision is the two definitions'."""
    args, B, T, depth, stride = cs.make_env_args("flight_easy", n_agents=3), 4, 12, 3, 3
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=every)
    ag = cs.LocalForecastAgents(args, 15, motion=motion, depth=depth, stride=stride, batch=B, device="cpu", impl="torch")
    twin = cs.LocalBeliefAgents(args, 15, motion=motion, batch=B, device="cpu", impl="torch")
    seen, real = [], lf.local_forecast_torch
    monkeypatch.setattr(lf, "local_forecast_torch", lambda g, p, h, n, side, model, moves: (seen.append(tuple(moves)), real(g, p, h, n, side, model, moves))[1])
    pol = ag.policy()
    for t, s in enumerate(walk(B, 3, T, 24, tail=45)):
        if t == 0:
            twin.reset()
        a = pol(None, s, None, t)
        twin.choose_action(s, be.targets_moved(motion, t))
        want = tuple(sum(1 for u in range(t + d * stride, t + (d + 1) * stride) if u % every == 0) for d in range(depth))
        assert seen[-1] == want == fc.segment_moves(t, depth, stride, every, 1.0) and sum(want) == (9 if every == 1 else 5 - t % 2), t
        assert same((ag.grids, ag.base.prev, ag.base.heard), (twin.grids, twin.prev, twin.heard)), t
        stacks = real(twin.grids, twin.prev, twin.heard, 3, 50, twin.model, want)
        assert torch.equal(ag.stacks, stacks), t
        got = plan(s, stacks, 3, 50, 7, depth, stride, 230, 15)
        assert same((a, ag.plans, ag.scores), got), t
    assert len(seen) == T
    ag.grids.fill_(5)   # what a previous episode left behind: t == 0 resets
    first = pol(None, walk(B, 3, 1, 24, tail=45)[0], None, 0)
    fresh = cs.LocalForecastAgents(args, 15, motion=motion, depth=depth, stride=stride, batch=B, device="cpu", impl="torch")
    assert torch.equal(first, fresh.choose_action(walk(B, 3, 1, 24, tail=45)[0], 0, 0))


def test_local_forecast_agents_refuse_what_they_cannot_run():
    args = cs.make_env_args("flight_easy")
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalForecastAgents(args, 10, batch=4, device="cpu")
    with pytest.raises(ValueError, match="impl"):
        cs.LocalForecastAgents(args, 10, batch=4, device="cpu", impl="eager")
    for base in ("coverage", cs.LocalCoverageAgents(args, 10, batch=4, device="cpu", impl="torch"),
                 cs.BeliefAgents(args, motion=motion, batch=4, device="cpu", impl="torch")):
        with pytest.raises(ValueError, match="a coverage base has no motion model to forecast with"):   # ForecastAgents' reason
            cs.LocalForecastAgents(args, 10, base=base, batch=4, device="cpu", impl="torch")
    for comm in (-1, 2.5, 129):
        with pytest.raises(ValueError, match="comm_range"):
            cs.LocalForecastAgents(args, comm, batch=4, device="cpu", impl="torch")
    for kw in (dict(depth=0), dict(depth=6), dict(stride=0), dict(stride=9), dict(discount=257)):
        with pytest.raises(ValueError, match="plan:"):
            cs.LocalForecastAgents(args, 10, batch=4, device="cpu", impl="torch", **kw)
    with pytest.raises(TypeError, match="motion"):
        cs.LocalForecastAgents(args, 10, motion="walk", batch=4, device="cpu", impl="torch")
    base = cs.LocalBeliefAgents(args, 10, motion=motion, batch=4, device="cpu", impl="torch")
    with pytest.raises(ValueError, match="the base runs"):
        cs.LocalForecastAgents(args, 10, base=base, impl="hip")
    with pytest.raises(ValueError, match="batch 5"):
        cs.LocalForecastAgents(args, 10, base=base, batch=5, impl="torch")
    with pytest.raises(ValueError, match="device"):
        cs.LocalForecastAgents(args, 10, base=base, device="cuda", impl="torch")
    for comm in (0, 11, None):
        with pytest.raises(ValueError, match="comm_range .* is not the base's"):
            cs.LocalForecastAgents(args, comm, base=base, impl="torch")
    ag = cs.LocalForecastAgents(args, 10, base=base, depth=2, impl="torch")   # an instance: shared, not copied
    assert isinstance(ag, cs.LocalPlanAgents) and ag.base is base and ag.grids is base.grids and ag.motion is motion
    assert ag.stacks.shape == (4, 3, 2, 2500) and ag.stacks.dtype == torch.int32 and ag.plans.shape == ag.scores.shape == (4, 3)
    assert "491 MB" in cs.LocalForecastAgents.__doc__
    state = walk(4, 3, 1, 3, tail=45)[0]
    with pytest.raises(ValueError, match="must be"):   # a batch that is not the base's
        ag.choose_action(state[:-1], 1, 0)
    built = cs.LocalForecastAgents(cs.make_env_args("flight_easy", n_agents=5), 20, motion=motion, batch=3, device="cpu", impl="torch")
    assert type(built.base) is cs.LocalBeliefAgents and built.base.comm_range == 20 and built.motion is motion
    assert (built.depth, built.stride, built.discount) == (4, 3, 230) and built.stacks.shape == (3, 5, 4, 2500)


def test_distil_local_grid_labels_with_the_class_through_the_rows_path(monkeypatch):
    """Iteration 0 flown by the expert, one DAgger iteration: its labels are T policy() calls of the LocalForecastAgents expert, which
    get t (the forecast's schedule) and end with reset()."""
    from imitate_util import bc_args, synthetic_batch
    from localobs_util import episodes
    args = bc_args(T=4)
    B, calls = 3, []

    class StubCollector:
        def __init__(self, env):
            self.k = 0

        def generate_episodes(self, policy=None, agents=None, evaluate=True, init=False, **kw):
            batch = synthetic_batch(args, B, 20 + self.k)
            batch["s"] = episodes(B, args.n_agents, 4, 30 + self.k, tail=args.state_shape - 4 * args.n_agents) * (1 - batch["padded"])
            self.k += 1
            del batch["u_expert"]
            return batch, None, None, torch.tensor([3, 4, 5])

    class StubAgents:
        def __init__(self, net):
            self.net = net

        def policy(self):
            return lambda obs, state, last, t: None

        def sync_weights(self):
            pass

    monkeypatch.setattr(lo, "EpisodeCollector", StubCollector)
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    learner = go.GridImitationLearner(args, device="cpu", unroll="torch")
    filt = cs.LocalBeliefAgents(args, 10, motion=motion, batch=B, device="cpu", impl="torch")
    expert = cs.LocalForecastAgents(args, 10, motion=motion, depth=2, batch=B, device="cpu", impl="torch")
    inner = expert.choose_action
    expert.choose_action = lambda state, moved=0, t=0: (calls.append(t), inner(state, moved, t))[1]
    ring = go.FeatureRing(args, 16, device="cpu")
    history = lo.distil_local_grid(None, expert, filt, learner, StubAgents(learner.eval_rnn), ring, iterations=2, updates=1, sample=4,
                                   generator=torch.Generator().manual_seed(0), impl="rows")
    assert [h["flown_by"] for h in history] == ["expert", "student"] and ring.current_size == 2 * B
    assert calls == [0, 1, 2, 3]   # one relabelling, of the student's batch
    second = {k: v[B:2 * B] for k, v in ring.buffers.items()}
    relabel = cs.LocalForecastAgents(args, 10, motion=motion, depth=2, batch=B, device="cpu", impl="torch")
    want = im.label_episodes(relabel, second, impl="rows")
    assert torch.equal(second["u_expert"].squeeze(3).long(), want) and set(want.flatten().tolist()) <= {0, 1, 2}
    plain = im.label_episodes(cs.LocalPlanAgents(args, 10, base="belief", motion=motion, depth=2, batch=B, device="cpu", impl="torch"), second,
                              impl="rows")
    assert not torch.equal(want, plain)   # the forecast decides otherwise than the plain planner on these rows
    assert bool((expert.grids == bl.FRESH).all())   # the rows path ends with reset()
