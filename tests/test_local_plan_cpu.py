"""CPU tests of the planner on private grids under a communication range (local_plan.py, include/coopsearch.h: cs_local_plan_actions):
the boundary declares, exports and registers it and refuses bad arguments before any launch; the definition
(local_plan.local_plan_actions_torch) is PlanAgents' definition at an unlimited range on equal grids (identity A), n lone planners at
range 0 (B), does not let a later agent change an earlier one (C), and in between does what a restatement in plain Python integers
and a hand case (D) say; LocalPlanAgents flies PlanAgents' decisions at an unlimited range and n lone planners' at range 0.
Everything is torch.equal on integers: no tolerance, and no threshold on what the policy finds."""
import ctypes as C
import os
import re

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import local as lc
from cooperative_search_amd import local_plan as lp
from cooperative_search_amd import motion as mo
from cooperative_search_amd import plan as pl
from local_plan_util import MIXED, PARAMS, SHAPES, by_hand, inputs, points_by_hand
from local_util import LINE, SIDE, VR, disc, fresh, landed, random_grids, rows_at, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def one_thread():
    """The definition's tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def define(state, grids, n, side, vr, depth, stride, discount, comm):
    return lp.local_plan_actions_torch(state, grids, n, side, vr, depth, stride, discount, comm, return_plans=True)


def same(got, want):
    return all(torch.equal(g, w) for g, w in zip(got, want))


# ---- 1. the boundary ------------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    version = re.search(r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    assert "cs_local_plan_params and cs_local_plan_actions" in version and "no existing export or struct changed" in version
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_local_plan_actions\s*\(\s*const\s+cs_local_plan_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_local_plan_actions" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.cs_local_plan_actions.argtypes) == 8 and L.cs_local_plan_actions.restype is C.c_int
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_local_plan_params \{(.*?)\}", header, flags=re.S).group(1)
    want = ["n_agents", "side", "view_range", "depth", "stride", "discount", "state_width", "comm_range", "reserved"]
    assert re.findall(r"int32_t\s+(\w+);", fields) == want
    assert [k for k, _ in _lib.CsLocalPlanParams._fields_] == want and C.sizeof(_lib.CsLocalPlanParams) == 36
    assert want[:-2] == [k for k, _ in _lib.CsPlanParams._fields_][:-1]   # cs_plan_params' fields first, in its order
    schema = str(_lib.torch_ops().local_plan_actions.default._schema)
    assert schema == ("coopsearch::local_plan_actions(Tensor state, Tensor grids, Tensor(a!) actions, Tensor(b!) plans, Tensor(c!) scores, "
                      "int n_agents, int side, int view_range, int depth, int stride, int discount, int comm_range) -> ()")
    from cooperative_search_amd import build
    assert "local_plan.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "local_plan_actions")   # one ops object, no ctypes twin
    assert cs.LocalPlanAgents is lp.LocalPlanAgents and cs.local_plan_actions_torch is lp.local_plan_actions_torch
    # the definition imports its parts; it does not restate them
    assert lp.quantise is bl.quantise and lp.cell_centres is bl.cell_centres and lp.disc_mask is bl.disc_mask
    assert lp.links is lc.links and lp._check_comm is lc._check_comm and lp.CAP is pl.CAP and lp._check_params is pl._check_params
    assert lp.plan_actions_torch is pl.plan_actions_torch and lp.step_tables is pl.step_tables and lp.weights is pl.weights
    assert lp.TURN is pl.TURN and lp.MAX_DEPTH is pl.MAX_DEPTH
    episodes = open(os.path.join(ROOT, "cooperative-search_amd", "csrc", "episodes.hip")).read()
    assert episodes.index('#include "plan.h"') < episodes.index('#include "local_plan.h"') > episodes.index('#include "local.h"')


def good_params():
    return _lib.CsLocalPlanParams(3, 50, 7, 4, 3, 230, 57, 10, 0)


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("view_range", -1, "view_range"),
    ("view_range", 65, "view_range"), ("depth", 0, "depth"), ("depth", 6, "depth"), ("stride", 0, "stride"), ("stride", 9, "stride"),
    ("discount", -1, "discount"), ("discount", 257, "discount"), ("state_width", 11, "state_width"), ("comm_range", -2, "comm_range"),
    ("comm_range", 129, "comm_range"), ("reserved", 1, "reserved"), ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"),
    ("ptr", 2, "NULL"), ("ptr", 3, "NULL"), ("ptr", 4, "NULL"), ("params", None, "NULL"), ("align", 0, "aligned"), ("align", 1, "aligned"),
    ("align", 2, "aligned"), ("align", 3, "aligned"), ("align", 4, "aligned")])
def test_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = good_params()
    B, ptrs = 4, [256, 512, 1024, 2048, 4096]   # state, grids, actions, plans, scores
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2 if value < 2 else 4
    elif field == "B":
        B = value
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_local_plan_actions(None if field == "params" else C.byref(p), ptrs[0], B, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None)
    assert rc == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_local_plan_actions") and msg in err


def test_the_op_refuses_bad_integers_shapes_and_cpu_tensors():
    ops = _lib.torch_ops()
    state, grids = torch.zeros(2, 57), fresh(2, 3, SIDE)
    outs = [torch.full((2, 3), -7, dtype=torch.int64) for _ in range(3)]
    good = dict(n_agents=3, side=SIDE, view_range=VR, depth=4, stride=3, discount=230, comm_range=10)

    def call(state=state, grids=grids, outs=outs, **kw):
        a = dict(good, **kw)
        ops.local_plan_actions(state, grids, *outs, a["n_agents"], a["side"], a["view_range"], a["depth"], a["stride"], a["discount"],
                               a["comm_range"])

    for kw, msg in ((dict(n_agents=9), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"), (dict(depth=0), "depth"),
                    (dict(depth=6), "depth"), (dict(stride=0), "stride"), (dict(stride=9), "stride"), (dict(discount=257), "discount"),
                    (dict(discount=-1), "discount"), (dict(comm_range=-2), "comm_range"), (dict(comm_range=129), "comm_range"),
                    (dict(grids=grids[:, 0]), "grids must be"), (dict(grids=grids[:, :2]), "grids must be"), (dict(grids=grids[:1]), "grids must be"),
                    (dict(state=state[:, :11]), "state must be"), (dict(outs=[outs[0][:, :2], outs[1], outs[2]]), "actions must be"),
                    (dict(outs=[outs[0], outs[1][:1], outs[2]]), "plans must be"), (dict(outs=[outs[0], outs[1], outs[2][:, :2]]), "scores must be")):
        with pytest.raises(RuntimeError, match="local_plan_actions: " + msg):   # integers and shapes come first: the CPU tensors are not reached
            call(**kw)
    with pytest.raises(RuntimeError, match="GPU"):   # a CPU tensor must be refused, not dereferenced
        call()
    assert all(bool((o == -7).all()) for o in outs) and bool((grids == bl.FRESH).all())


def test_the_definition_refuses_bad_ranges_and_shapes():
    state, grids = torch.zeros(2, 17), torch.zeros(2, 3, 2500, dtype=torch.int32)
    good = dict(n_agents=3, side=50, view_range=7, depth=4, stride=3, discount=230, comm_range=10)

    def call(state=state, grids=grids, **kw):
        return lp.local_plan_actions_torch(state, grids, **dict(good, **kw))

    assert call().shape == (2, 3) and call().dtype == torch.int64
    assert all(t.shape == (2, 3) and t.dtype == torch.int64 for t in call(return_plans=True))
    for kw in (dict(comm_range=-2), dict(comm_range=129)):
        with pytest.raises(ValueError, match="comm_range"):
            call(**kw)
    for kw in (dict(n_agents=0), dict(n_agents=9), dict(side=65), dict(view_range=-1), dict(view_range=65), dict(depth=0), dict(depth=6),
               dict(stride=0), dict(stride=9), dict(discount=-1), dict(discount=257)):
        with pytest.raises(ValueError, match="plan:"):
            call(**kw)
    for kw in (dict(state=state[:, :11]), dict(state=state[0]), dict(state=state.double()), dict(state=state[:0])):
        with pytest.raises(ValueError, match="local plan: state must be"):
            call(**kw)
    for kw in (dict(grids=grids[:, 0]), dict(grids=grids[:, :2]), dict(grids=grids[:1]), dict(grids=grids[:, :, :-1]), dict(grids=grids.long()),
               dict(grids=grids.view(2, 3, 50, 50))):
        with pytest.raises(ValueError, match="local plan: grids must be"):
            call(**kw)
    with pytest.raises(TypeError, match="local plan:"):
        call(grids=grids.tolist())
    assert not bool(grids.any())   # read only


def test_local_plan_agents_refuse_what_they_cannot_run():
    args = cs.make_env_args("flight_easy")
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalPlanAgents(args, 10, batch=4, device="cpu", impl="hip")
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalPlanAgents(args, 10, base="belief", batch=4, device="cpu")
    with pytest.raises(ValueError, match="impl"):
        cs.LocalPlanAgents(args, 10, batch=4, device="cpu", impl="eager")
    with pytest.raises(ValueError, match="base must be"):
        cs.LocalPlanAgents(args, 10, base="random", batch=4, device="cpu", impl="torch")
    with pytest.raises(ValueError, match="base must be"):   # a centralised filter keeps no private grids
        cs.LocalPlanAgents(args, 10, base=cs.CoverageAgents(args, batch=4, device="cpu", impl="torch"), impl="torch")
    with pytest.raises(ValueError, match="batch"):
        cs.LocalPlanAgents(args, 10, device="cpu", impl="torch")
    for comm in (-1, 2.5, 129):
        with pytest.raises(ValueError, match="comm_range"):
            cs.LocalPlanAgents(args, comm, batch=4, device="cpu", impl="torch")
    for kw in (dict(depth=0), dict(depth=6), dict(stride=0), dict(stride=9), dict(discount=257), dict(discount=-1)):
        with pytest.raises(ValueError, match="plan:"):
            cs.LocalPlanAgents(args, 10, batch=4, device="cpu", impl="torch", **kw)
    with pytest.raises(TypeError, match="motion"):
        cs.LocalPlanAgents(args, 10, motion="walk", batch=4, device="cpu", impl="torch")
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0)
    for base in (cs.LocalCoverageAgents(args, 10, batch=4, device="cpu", impl="torch"),
                 cs.LocalBeliefAgents(args, 10, motion=motion, batch=4, device="cpu", impl="torch")):
        with pytest.raises(ValueError, match="the base runs"):
            cs.LocalPlanAgents(args, 10, base=base, impl="hip")
        with pytest.raises(ValueError, match="batch 5"):
            cs.LocalPlanAgents(args, 10, base=base, batch=5, impl="torch")
        with pytest.raises(ValueError, match="device"):
            cs.LocalPlanAgents(args, 10, base=base, device="cuda", impl="torch")
        for comm in (0, 11, None):
            with pytest.raises(ValueError, match="comm_range .* is not the base's"):
                cs.LocalPlanAgents(args, comm, base=base, impl="torch")
        wrapped = cs.LocalPlanAgents(args, 10, base=base, impl="torch")   # an instance: shared, not copied
        assert wrapped.base is base and wrapped.grids is base.grids and (wrapped.batch, wrapped.device.type, wrapped.comm_range) == (4, "cpu", 10)
    unlimited = cs.LocalCoverageAgents(args, None, batch=4, device="cpu", impl="torch")
    assert cs.LocalPlanAgents(args, None, base=unlimited, impl="torch").comm_range == -1
    with pytest.raises(ValueError, match="is not the base's"):
        cs.LocalPlanAgents(args, 10, base=unlimited, impl="torch")
    built = cs.LocalPlanAgents(cs.make_env_args("flight_easy", n_agents=5), 20, base="belief", motion=motion, depth=2, batch=3, device="cpu", impl="torch")
    assert type(built.base) is cs.LocalBeliefAgents and built.base.comm_range == 20 and built.motion is motion
    assert (built.n_agents, built.side, built.view_range, built.depth, built.stride, built.discount) == (5, 50, 7, 2, 3, 230)
    assert built.grids.shape == (3, 5, 2500) and built.plans.shape == built.scores.shape == (3, 5) and built.plans.dtype == torch.int64


# ---- 2. identities A, B and C, and the range in between ---------------------------------------------------------------------------

@pytest.mark.parametrize("depth, stride, discount", PARAMS)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_identity_a_unlimited_range_on_equal_grids_is_the_shared_planner(B, n, side, vr, depth, stride, discount):
    state, grids = inputs(B, n, side)
    before = grids.clone()
    got = define(state, grids, n, side, vr, depth, stride, discount, -1)
    assert same(got, pl.plan_actions_torch(state, grids[:, 0].contiguous(), n, side, vr, depth, stride, discount, return_plans=True))
    assert torch.equal(grids, before)
    assert torch.equal(got[0], lp.local_plan_actions_torch(state, grids, n, side, vr, depth, stride, discount, -1))
    assert same(got, define(state, grids, n, side, vr, depth, stride, discount, 128))   # 128 cells reach across any map


@pytest.mark.parametrize("depth, stride, discount", PARAMS)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_identity_b_range_zero_is_n_lone_planners(B, n, side, vr, depth, stride, discount):
    state = walk(B, n, 1, 5)[0]
    for grids in (inputs(B, n, side)[1], random_grids(B, n, side, 4)):   # equal grids, and a grid of its own per agent
        got = define(state, grids, n, side, vr, depth, stride, discount, 0)
        for i in range(n):
            lone = pl.plan_actions_torch(state[:, 4 * i:4 * i + 4].contiguous(), grids[:, i].contiguous(), 1, side, vr, depth, stride, discount,
                                         return_plans=True)
            assert same([t[:, i:i + 1] for t in got], lone), i


@pytest.mark.parametrize("depth, stride, discount", PARAMS)
@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_identity_c_an_agent_does_not_depend_on_those_that_decide_after_it(B, n, side, vr, depth, stride, discount):
    state, grids = inputs(B, n, side)
    for comm in (-1, 0, MIXED[B, n, side]):
        full = define(state, grids, n, side, vr, depth, stride, discount, comm)
        for k in range(1, n):
            part = define(state[:, :4 * k].contiguous(), grids[:, :k].contiguous(), k, side, vr, depth, stride, discount, comm)
            assert same([t[:, :k] for t in full], part), (comm, k)


@pytest.mark.parametrize("B, n, side, vr", SHAPES)
def test_a_mixed_range_is_neither_identity_and_equals_the_restatement_by_hand(B, n, side, vr):
    """At these ranges some pairs are linked and others are not (asserted on the inputs), and the scores differ from the unlimited
    range's AND from range 0's (asserted too): neither a shared-grid planner nor n lone planners pass.  What it must give is the
    restatement of local_plan_util.by_hand: links, claim points and claimed discs in plain Python integers."""
    depth, stride, discount = PARAMS[0]
    comm = MIXED[B, n, side]
    state, grids = inputs(B, n, side)
    X, Y, _ = bl.quantise(state, n, side)
    adj = lc.links(X, Y, comm)
    off = ~torch.eye(n, dtype=torch.bool)
    assert bool(adj[:, off].any()) and not bool(adj[:, off].all())
    got = define(state, grids, n, side, vr, depth, stride, discount, comm)
    unlimited, zero = (define(state, grids, n, side, vr, depth, stride, discount, c) for c in (-1, 0))
    assert int((got[2] != unlimited[2]).sum()) > 0 and int((got[2] != zero[2]).sum()) > 0
    assert same(got, by_hand(state, grids, n, side, vr, depth, stride, discount, comm))
    own = random_grids(B, n, side, 4)   # and with a grid of its own per agent
    assert same(define(state, own, n, side, vr, depth, stride, discount, comm), by_hand(state, own, n, side, vr, depth, stride, discount, comm))


def test_the_range_that_links_without_changing_a_score_is_not_used():
    """Range 30 at side 50 links some pairs of the three agents and not others, yet no score differs from range 0's on these inputs:
    the reason the mixed range of that shape is 15."""
    B, n, side, vr = SHAPES[0]
    state, grids = inputs(B, n, side)
    X, Y, _ = bl.quantise(state, n, side)
    off = ~torch.eye(n, dtype=torch.bool)
    adj = lc.links(X, Y, 30)
    assert bool(adj[:, off].any()) and not bool(adj[:, off].all())
    assert same(define(state, grids, n, side, vr, 4, 3, 230, 30), by_hand(state, grids, n, side, vr, 4, 3, 230, 30))


# ---- 3. the hand case and the edge values -----------------------------------------------------------------------------------------

def test_identity_d_a_claim_is_heard_by_the_linked_agents_and_no_others():
    """A - B - C on a line, 8 cells apart, all heading east: at range 10 A-B and B-C are linked, A-C (16 cells) is not.  depth 1,
    stride 8, fresh grids: every agent's best single segment is counted in plain Python.  A takes its disc whole.  B hears A: the
    gain of each of its three candidate discs is the disc less its overlap with A's CLAIMED disc.  C hears B and not A: less B's
    claimed disc only.  (A's claim lies 16 cells behind C and touches none of C's candidates, so the unlimited range gives C the same
    score; the next test has an unheard claim that does overlap.)"""
    n, depth, stride = 3, 1, 8
    state = rows_at([LINE], SIDE)
    assert landed(state, n, SIDE) == [[(x, y) for x, y, _ in LINE]]
    grids = fresh(1, n, SIDE)

    def candidates(i):
        return [disc(*points_by_hand(*LINE[i], s, SIDE, depth, stride)[0], SIDE, VR) for s in range(3)]

    def best(i, claimed):
        gains = [int((d & ~claimed).sum()) * 65536 * 256 for d in candidates(i)]
        s = gains.index(max(gains))   # the lowest of the largest
        return s, gains[s], candidates(i)[s]

    nothing = torch.zeros(SIDE * SIDE, dtype=torch.bool)
    sa, ga, da = best(0, nothing)
    sb, gb, db = best(1, da)
    sc, gc, dc = best(2, db)
    assert ga == int(da.sum()) * 65536 * 256 and gb < ga and gc < ga        # both claims bite
    a, p, s = define(state, grids, n, SIDE, VR, depth, stride, 230, 10)
    assert p.tolist() == [[sa, sb, sc]] and s.tolist() == [[ga, gb, gc]] and torch.equal(a, p)
    a, p, s = define(state, grids, n, SIDE, VR, depth, stride, 230, 0)     # range 0: every agent takes its full disc
    full = [best(i, nothing) for i in range(n)]
    assert p.tolist() == [[f[0] for f in full]] and s.tolist() == [[f[1] for f in full]]
    assert s[0, 0] == s[0, 1] == s[0, 2] == ga
    a, p, s = define(state, grids, n, SIDE, VR, depth, stride, 230, -1)    # unlimited: C hears A too
    assert s.tolist() == [[ga, gb, best(2, da | db)[1]]]


def test_an_unheard_claim_that_overlaps_is_not_subtracted():
    """Two agents 12 cells apart flying toward each other, depth 1, stride 8: their end points lie 4 cells apart and the discs overlap.
    At range 10 they are not linked and the second takes its disc whole; at range 13 it loses the overlap, counted in plain Python."""
    pair = [(168, 408, 0), (360, 408, 18)]
    state = rows_at([pair], SIDE)
    assert landed(state, 2, SIDE) == [[(168, 408), (360, 408)]]
    discs = [[disc(*points_by_hand(*pair[i], s, SIDE, 1, 8)[0], SIDE, VR) for s in range(3)] for i in range(2)]
    whole = [[int(d.sum()) * 65536 * 256 for d in discs[i]] for i in range(2)]
    first = whole[0].index(max(whole[0]))
    less = [int((d & ~discs[0][first]).sum()) * 65536 * 256 for d in discs[1]]
    assert max(less) < max(whole[1])
    for comm, want in ((10, max(whole[1])), (0, max(whole[1])), (13, max(less)), (-1, max(less))):
        a, p, s = define(state, fresh(1, 2, SIDE), 2, SIDE, VR, 1, 8, 230, comm)
        assert s.tolist() == [[max(whole[0]), want]] and p[0, 0] == first, comm


@pytest.mark.parametrize("depth, stride, vr, discount", [(1, 3, 7, 230), (5, 3, 7, 230), (4, 1, 7, 230), (4, 8, 7, 230), (4, 3, 0, 230),
                                                         (4, 3, 64, 230), (4, 3, 7, 0), (1, 8, 64, 0), (5, 1, 0, 256)])
def test_edge_values_of_every_parameter(depth, stride, vr, discount):
    """depth 1 and 5, stride 1 and 8, view_range 0 and 64, discount 0: identities A and B and the restatement by hand at the mixed range."""
    B, n, side, _ = SHAPES[0]
    state, grids = inputs(B, n, side)
    assert same(define(state, grids, n, side, vr, depth, stride, discount, -1),
                pl.plan_actions_torch(state, grids[:, 0].contiguous(), n, side, vr, depth, stride, discount, return_plans=True))
    own = random_grids(B, n, side, 6)
    zero = define(state, own, n, side, vr, depth, stride, discount, 0)
    for i in range(n):
        lone = pl.plan_actions_torch(state[:, 4 * i:4 * i + 4].contiguous(), own[:, i].contiguous(), 1, side, vr, depth, stride, discount,
                                     return_plans=True)
        assert same([t[:, i:i + 1] for t in zero], lone), i
    got = define(state, own, n, side, vr, depth, stride, discount, MIXED[B, n, side])
    assert same(got, by_hand(state, own, n, side, vr, depth, stride, discount, MIXED[B, n, side]))
    assert bool(((got[1] >= 0) & (got[1] < 3 ** depth)).all()) and torch.equal(got[0], got[1] // 3 ** (depth - 1)) and bool((got[2] >= 0).all())


def test_sequence_points_are_the_points_walked_by_hand():
    state = walk(4, 3, 1, 8)[0]
    X, Y, h = bl.quantise(state, 3, 50)
    g = torch.Generator().manual_seed(1)
    for depth, stride in ((1, 1), (4, 3), (5, 8)):
        plans = torch.randint(0, 3 ** depth, (4, 3), generator=g)
        for i in range(3):
            px, py = pl.sequence_points(X[:, i], Y[:, i], h[:, i], plans[:, i], 50, depth, stride)
            for b in range(4):
                want = points_by_hand(int(X[b, i]), int(Y[b, i]), int(h[b, i]), int(plans[b, i]), 50, depth, stride)
                assert list(zip(px[b].tolist(), py[b].tolist())) == want


# ---- 4. the class ---------------------------------------------------------------------------------------------------------------------

MOTION = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=2)   # the targets move before every second call: moved calls included


def build(kind, cls, args, B, *comm, **kw):
    if kind == "belief":
        kw["motion"] = MOTION
    return cls(args, *comm, batch=B, device="cpu", impl="torch", **kw)


@pytest.mark.parametrize("kind", ["coverage", "belief"])
def test_unlimited_range_flies_the_centralised_planner(kind):
    B, n, T = 2, 3, 30
    args = cs.make_env_args("flight_easy", n_agents=n)
    local = build(kind, cs.LocalPlanAgents, args, B, None, base=kind, depth=3)
    shared = build(kind, cs.PlanAgents, args, B, base=kind, depth=3)
    assert local.motion == shared.motion and local.grids is local.base.grids
    pol, pol_shared = local.policy(), shared.policy()
    moved, taken = 0, set()
    for t, s in enumerate(walk(B, n, T, 21, tail=45)):
        moved += int(be.targets_moved(local.motion, t))
        a, want = pol(None, s, None, t), pol_shared(None, s, None, t)
        assert torch.equal(a, want) and torch.equal(local.plans, shared.plans) and torch.equal(local.scores, shared.scores), t
        for i in range(n):
            assert torch.equal(local.grids[:, i], shared.grid), (t, i)
        taken |= set(a.flatten().tolist())
    assert taken == {0, 1, 2} and moved == (15 if kind == "belief" else 0)   # the belief base met moved calls


@pytest.mark.parametrize("kind", ["coverage", "belief"])
def test_range_zero_flies_n_lone_planners(kind):
    B, n, T = 2, 3, 30
    local = build(kind, cs.LocalPlanAgents, cs.make_env_args("flight_easy", n_agents=n), B, 0, base=kind, depth=3)
    lone = [build(kind, cs.PlanAgents, cs.make_env_args("flight_easy", n_agents=1), B, base=kind, depth=3) for _ in range(n)]
    pol, pol_lone = local.policy(), [p.policy() for p in lone]
    for t, s in enumerate(walk(B, n, T, 22, tail=45)):
        a = pol(None, s, None, t)
        for i in range(n):
            want = pol_lone[i](None, s[:, 4 * i:4 * i + 4].contiguous(), None, t)
            assert torch.equal(a[:, i:i + 1], want) and torch.equal(local.plans[:, i:i + 1], lone[i].plans), (t, i)
            assert torch.equal(local.scores[:, i:i + 1], lone[i].scores) and torch.equal(local.grids[:, i], lone[i].grid), (t, i)


def test_policy_resets_at_step_zero_and_passes_moved_as_specified():
    args = cs.make_env_args("flight_easy", n_agents=3)
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=3)
    ag = cs.LocalPlanAgents(args, 10, base="belief", motion=motion, depth=2, batch=2, device="cpu", impl="torch")
    seen = []
    inner = ag.choose_action
    ag.choose_action = lambda state, moved=0: (seen.append(bool(moved)), inner(state, moved))[1]
    base_seen = []
    base_inner = ag.base.choose_action
    ag.base.choose_action = lambda state, moved: (base_seen.append(bool(moved)), base_inner(state, moved))[1]
    pol = ag.policy()
    states = walk(2, 3, 6, 9, tail=45)
    first = [pol(None, s, None, t) for t, s in enumerate(states)]
    assert seen == base_seen == [be.targets_moved(motion, t) for t in range(6)] == [False, True, False, False, True, False]
    g_end, p_end = ag.grids.clone(), ag.plans.clone()
    ag.grids.fill_(5)   # what a previous episode left behind
    again = [pol(None, s, None, t) for t, s in enumerate(states)]   # t = 0 resets: the second flight equals the first
    assert all(torch.equal(a, b) for a, b in zip(first, again)) and torch.equal(ag.grids, g_end) and torch.equal(ag.plans, p_end)
    assert first[0].shape == (2, 3) and first[0].dtype == torch.int64
    ag.reset()
    assert bool((ag.grids == bl.FRESH).all()) and not bool(ag.base.heard.any())
    cov = cs.LocalPlanAgents(args, 10, base="coverage", depth=2, batch=2, device="cpu", impl="torch")   # a coverage base ignores moved
    assert cov.policy()(None, states[0], None, 0).shape == (2, 3) and cov.choose_action(states[1], 1).shape == (2, 3)


class RecordingOps:
    """Stands in for the op layer: records every op that is asked for (none should be, on the rows path of a torch expert)."""

    def __init__(self):
        self.asked = []

    def __getattr__(self, name):
        self.asked.append(name)
        raise AssertionError(f"the op layer was asked for {name}")


def test_label_episodes_takes_the_class_through_the_rows_path(monkeypatch):
    """An expert imitate.label_episodes does not know: no one-launch path, T policy() calls.  At an unlimited range the labels are
    PlanAgents'; the second episode ends after three rows."""
    E, T, n = 2, 5, 3
    s = torch.stack(walk(E, n, T, 12, tail=45), 1)
    padded = torch.zeros(E, T, 1)
    padded[1, 3:] = 1.0
    batch = {"s": s, "padded": padded}
    args = cs.make_env_args("flight_easy", n_agents=n)
    local = cs.LocalPlanAgents(args, None, base="belief", motion=MOTION, depth=2, batch=E, device="cpu", impl="torch")
    shared = cs.PlanAgents(args, base="belief", motion=MOTION, depth=2, batch=E, device="cpu", impl="torch")
    ops = RecordingOps()
    monkeypatch.setattr(_lib, "torch_ops", lambda: ops)
    monkeypatch.setattr(_lib, "torch_ops_for", lambda what: ops)
    calls = []
    inner = local.policy
    local.policy = lambda: (lambda pol: (lambda obs, state, last, t: (calls.append(t), pol(obs, state, last, t))[1]))(inner())
    for impl in ("auto", "rows"):
        calls.clear()
        got = cs.label_episodes(local, batch, impl=impl)
        assert calls == list(range(T)) and not ops.asked, impl
        assert torch.equal(got, cs.label_episodes(shared, batch, impl="rows")) and got.shape == (E, T, n) and not bool(got[1, 3:].any())
        assert bool((local.grids == bl.FRESH).all())   # the rows path ends with reset()
    with pytest.raises(ValueError, match="needs a CoverageAgents or a BeliefAgents"):
        cs.label_episodes(local, batch, impl="hip")
    mixed = cs.LocalPlanAgents(args, 10, base="belief", motion=MOTION, depth=2, batch=E, device="cpu", impl="torch")
    flown = torch.stack([mixed.policy()(None, s[:, t].contiguous(), None, t) for t in range(T)], 1)
    live = torch.arange(T).view(1, T, 1) < torch.tensor([T, 3]).view(E, 1, 1)
    assert torch.equal(cs.label_episodes(mixed, batch, impl="rows"), torch.where(live, flown, torch.zeros_like(flown)))
