"""CPU tests of coverage under a communication range (local.py, include/coopsearch.h: cs_local_coverage_actions): the boundary
declares, exports and registers it and refuses bad arguments before any launch; the definition (local.local_coverage_actions_torch)
is CoverageAgents' definition at an unlimited range and n lone agents at range 0, and in between does what DESIGN.md section 25 says
on hand cases.  Everything is torch.equal on integers: no tolerance."""
import ctypes as C
import os
import re

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import local as lc
from local_util import (KEEP, LINE, REGROWN, SIDE, SWEPT, SWEPT_TWICE, VR, boundary_rows, disc, far_rows, fresh, landed, random_grids,
                        rows_at, tie_rows, walk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def one_thread():
    """The definition's tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


# ---- 1. the boundary ------------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    assert "cs_local_params and cs_local_coverage_actions" in header   # the ABI comment notes the addition
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_local_coverage_actions\s*\(\s*const\s+cs_local_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_local_coverage_actions" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "cs_local_coverage_actions") and L.cs_local_coverage_actions.argtypes is not None
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_local_params \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", fields) == [k for k, _ in _lib.CsLocalParams._fields_]
    schema = str(_lib.torch_ops().local_coverage_actions.default._schema)
    assert schema == ("coopsearch::local_coverage_actions(Tensor state, Tensor(a!) grids, Tensor(b!) actions, int n_agents, int side, "
                      "int view_range, int keep, int regrow, int lookahead, int comm_range) -> ()")
    from cooperative_search_amd import build
    assert "local.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "local_coverage_actions")   # one ops object, no ctypes twin
    assert cs.LocalCoverageAgents is lc.LocalCoverageAgents and cs.local_coverage_actions_torch is lc.local_coverage_actions_torch
    assert lc.quantise is bl.quantise and lc.trig_tables is bl.trig_tables and lc.keep_of is bl.keep_of and lc.FRESH is bl.FRESH


@pytest.mark.parametrize("field, value, msg", [("n_agents", 9, "n_agents"), ("side", 65, "side"), ("view_range", -1, "view_range"),
                                               ("keep", 65537, "keep"), ("regrow", 0, "regrow"), ("regrow", 17, "regrow"),
                                               ("lookahead", 51, "lookahead"), ("state_width", 11, "state_width"),
                                               ("comm_range", -2, "comm_range"), ("comm_range", 129, "comm_range"),
                                               ("reserved", 1, "reserved"), (None, None, "B must"), ("ptr", None, "NULL"),
                                               ("align", None, "aligned")])
def test_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = _lib.CsLocalParams(3, SIDE, VR, KEEP, 8, 7, 57, 10, 0)
    B, ptrs = 4, [C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)]
    if field == "ptr":
        ptrs[1] = None
    elif field == "align":
        ptrs[1] = C.c_void_p(514)
    elif field is None:
        B = 0
    else:
        setattr(p, field, value)
    assert L.cs_local_coverage_actions(C.byref(p), ptrs[0], B, ptrs[1], ptrs[2], None) == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_local_coverage_actions") and msg in err


def test_op_definition_and_agents_refuse_wrong_tensors_and_parameters():
    ops = _lib.torch_ops()
    state, acts = torch.zeros(2, 57), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):   # a CPU tensor must be refused, not dereferenced
        ops.local_coverage_actions(state, fresh(2, 3, SIDE), acts, 3, SIDE, VR, KEEP, 8, 7, 10)
    with pytest.raises(RuntimeError, match="grids must be"):
        ops.local_coverage_actions(state, fresh(2, 3, SIDE)[:, 0], acts, 3, SIDE, VR, KEEP, 8, 7, 10)
    with pytest.raises(RuntimeError, match="grids must be"):
        ops.local_coverage_actions(state, fresh(2, 2, SIDE), acts, 3, SIDE, VR, KEEP, 8, 7, 10)
    with pytest.raises(RuntimeError, match="actions must be"):
        ops.local_coverage_actions(state, fresh(2, 3, SIDE), acts[:, :2], 3, SIDE, VR, KEEP, 8, 7, 10)
    for comm in (-2, 129):
        with pytest.raises(RuntimeError, match="comm_range"):
            ops.local_coverage_actions(state, fresh(2, 3, SIDE), acts, 3, SIDE, VR, KEEP, 8, 7, comm)
        with pytest.raises(ValueError, match="comm_range"):
            lc.local_coverage_actions_torch(state, fresh(2, 3, SIDE), 3, SIDE, VR, KEEP, comm)
    with pytest.raises(RuntimeError, match="lookahead"):
        ops.local_coverage_actions(state, fresh(2, 3, SIDE), acts, 3, SIDE, VR, KEEP, 8, SIDE + 1, 10)
    with pytest.raises(ValueError, match="grids must be"):
        lc.local_coverage_actions_torch(state, fresh(2, 3, SIDE)[:, 0], 3, SIDE, VR, KEEP, 10)
    with pytest.raises(ValueError, match="grids must be"):
        lc.local_coverage_actions_torch(state, fresh(2, 3, SIDE).to(torch.int64), 3, SIDE, VR, KEEP, 10)
    with pytest.raises(ValueError, match="state must be"):
        lc.local_coverage_actions_torch(state[:, :11], fresh(2, 3, SIDE), 3, SIDE, VR, KEEP, 10)
    args = cs.make_env_args("flight_easy")
    with pytest.raises(ValueError, match="not a GPU"):
        cs.LocalCoverageAgents(args, 10, batch=4, device="cpu")
    with pytest.raises(ValueError, match="batch"):
        cs.LocalCoverageAgents(args, 10, device="cpu", impl="torch")
    with pytest.raises(ValueError, match="impl"):
        cs.LocalCoverageAgents(args, 10, batch=4, device="cpu", impl="triton")
    for comm in (-1, 2.5, 129):
        with pytest.raises(ValueError, match="comm_range"):
            cs.LocalCoverageAgents(args, comm, batch=4, device="cpu", impl="torch")
    a = cs.LocalCoverageAgents(cs.make_env_args("flight_easy", n_agents=5), None, batch=4, device="cpu", impl="torch")
    assert (a.n_agents, a.side, a.view_range, a.keep, a.regrow, a.lookahead, a.comm_range) == (5, 50, 7, KEEP, 8, 7, -1)
    assert a.grids.dtype == torch.int32 and a.grids.shape == (4, 5, 2500) and bool((a.grids == bl.FRESH).all())
    assert cs.LocalCoverageAgents(args, 0, batch=1, device="cpu", impl="torch").comm_range == 0


# ---- 2. the two identities --------------------------------------------------------------------------------------------------------

CASES = [(3, 3, 50, 7), (2, 5, 7, 2), (2, 8, 64, 7)]   # B, n, side, view_range


@pytest.mark.parametrize("B, n, side, vr", CASES)
def test_unlimited_range_is_the_coverage_baseline_grids_and_actions(B, n, side, vr):
    """All n grids start equal (a random grid): over 30 calls every private grid equals the shared grid coverage_actions_torch
    leaves, and the actions are equal."""
    states = walk(B, n, 30, 100 * n + side)
    grids = random_grids(B, n, side, 7, equal=True)
    shared = grids[:, 0].clone()
    for t, s in enumerate(states):
        got = lc.local_coverage_actions_torch(s, grids, n, side, vr, KEEP, -1)
        want = bl.coverage_actions_torch(s, shared, n, side, vr, KEEP)
        assert torch.equal(got, want), t
        for i in range(n):
            assert torch.equal(grids[:, i], shared), (t, i)
    assert len({int(a) for a in got.view(-1)}) > 1 or n == 1


@pytest.mark.parametrize("B, n, side, vr", CASES)
def test_range_zero_is_n_lone_coverage_agents_grids_and_actions(B, n, side, vr):
    """Different random grids per agent: over 30 calls agent i's grid and action equal coverage_actions_torch with n_agents = 1 on
    its own four floats."""
    states = walk(B, n, 30, 200 * n + side)
    grids = random_grids(B, n, side, 8)
    lone = [grids[:, i].clone() for i in range(n)]
    for t, s in enumerate(states):
        got = lc.local_coverage_actions_torch(s, grids, n, side, vr, KEEP, 0)
        for i in range(n):
            want = bl.coverage_actions_torch(s[:, 4 * i:4 * i + 4].contiguous(), lone[i], 1, side, vr, KEEP)
            assert torch.equal(got[:, i:i + 1], want), (t, i)
            assert torch.equal(grids[:, i], lone[i]), (t, i)


def test_the_walk_reaches_and_passes_the_walls():
    X, Y = bl.quantise_positions(torch.cat(walk(3, 3, 30, 350), 0), 3, 50)
    assert bool((X == 800).any()) and bool((Y == 0).any()) and bool((X < 0).any()) and bool((Y > 800).any())


# ---- 3. hand cases ------------------------------------------------------------------------------------------------------------------

def test_partial_links_relay_one_hop_per_call():
    """A - B - C in a row, 8 cells apart, comm_range 10: A hears B, B hears both, C hears B.  Fresh grids, regrow 8:
    call 1: a fresh cell regrows to 65536 and a swept one becomes (65536 * 6554) >> 16 = 6554.  A's grid is swept on A's and B's disc
            and nowhere else: C's disc is not there yet.
    call 2, same poses: a 6554 cell regrows to 6554 + (58982 >> 8) = 6784, and swept again is (6784 * 6554) >> 16 = 678.  B's
            post-sweep grid holds 678 on its own disc and 6784 on what A and C told it in call 1; A's own holds 678 on A's disc and
            6784 on B's.  A takes the minimum: 678 on A's and B's discs, 6784 = C's FIRST sweep (regrown once, not the second sweep's
            678) on the rest of C's disc, 65536 elsewhere."""
    n, comm = 3, 10
    state = rows_at([LINE], SIDE)
    assert landed(state, n, SIDE) == [[(x, y) for x, y, _ in LINE]]
    assert (SWEPT, REGROWN, SWEPT_TWICE) == (6554, 6784, 678)
    dA, dB, dC = (disc(x, y, SIDE, VR) for x, y, _ in LINE)
    assert bool((dC & ~dA & ~dB).any()) and bool((dB & ~dA).any()) and not bool((dA & dC).any())
    grids = fresh(1, n, SIDE)
    full = torch.full((SIDE * SIDE,), 65536, dtype=torch.int32)

    def paint(*layers):
        g = full.clone()
        for mask, value in layers:
            g[mask] = value
        return g
    lc.local_coverage_actions_torch(state, grids, n, SIDE, VR, KEEP, comm)
    assert torch.equal(grids[0, 0], paint((dA | dB, 6554)))
    assert torch.equal(grids[0, 1], paint((dA | dB | dC, 6554)))
    assert torch.equal(grids[0, 2], paint((dB | dC, 6554)))
    lc.local_coverage_actions_torch(state, grids, n, SIDE, VR, KEEP, comm)
    assert torch.equal(grids[0, 0], paint((dC, 6784), (dA | dB, 678)))
    assert torch.equal(grids[0, 1], paint((dA | dB | dC, 678)))
    assert torch.equal(grids[0, 2], paint((dA, 6784), (dB | dC, 678)))


def test_claims_are_heard_only_over_a_link():
    state = tie_rows()
    assert landed(state, 2, SIDE) == [[(408, 392), (408, 392)]]
    linked, sc_l = lc.local_coverage_actions_torch(state, fresh(1, 2, SIDE), 2, SIDE, VR, KEEP, 5, return_scores=True)
    alone, sc_a = lc.local_coverage_actions_torch(state, fresh(1, 2, SIDE), 2, SIDE, VR, KEEP, 0, return_scores=True)
    assert int(linked[0, 0]) != int(linked[0, 1]) and int(alone[0, 0]) == int(alone[0, 1]) == int(linked[0, 0])
    assert torch.equal(sc_a[0, 0], sc_a[0, 1]) and torch.equal(sc_l[0, 0], sc_a[0, 0])
    assert int(sc_l[0, 1, int(linked[0, 0])]) == 0   # the footprint agent 0 took is worth nothing to the agent that heard it


def test_the_link_test_is_strict():
    """Exactly 16 comm_range sub-units apart: not linked; one sub-unit less: linked.  Seen through agent 1's grid: agent 0's disc
    is in it only over a link."""
    comm = 10
    state = boundary_rows(comm)
    assert landed(state, 2, SIDE) == [[(168, 408), (328, 408)], [(168, 408), (327, 408)]]
    X, Y = bl.quantise_positions(state, 2, SIDE)
    adj = lc.links(X, Y, comm)
    assert adj.tolist() == [[[True, False], [False, True]], [[True, True], [True, True]]]
    grids = fresh(2, 2, SIDE)
    lc.local_coverage_actions_torch(state, grids, 2, SIDE, VR, KEEP, comm)
    own0 = disc(168, 408, SIDE, VR)
    far0 = own0 & ~disc(328, 408, SIDE, VR) & ~disc(327, 408, SIDE, VR)
    assert bool(far0.any())
    assert bool((grids[0, 1][far0] == 65536).all()) and bool((grids[1, 1][far0] == 6554).all())
    assert bool((grids[0, 0][own0] == 6554).all()) and bool((grids[1, 0][own0] == 6554).all())
    # comm_range 0 links nobody, not even two agents on one spot
    same = tie_rows()
    X, Y = bl.quantise_positions(same, 2, SIDE)
    assert lc.links(X, Y, 0).tolist() == [[[True, False], [False, True]]] and bool(lc.links(X, Y, 1).all()) and bool(lc.links(X, Y, -1).all())


def test_the_link_test_is_taken_in_64_bits():
    """+-1e9 clamps to +-2^15 sub-units: the agents sit in opposite corners of the clamped range, 2^16 apart per axis.  A 32-bit
    square of 2^16 is 0 and would link them at any range; at the largest range, 128 cells, they are not linked.  Seen through the
    grids: they start different and nothing off the map sweeps them, so a merge would show."""
    state = far_rows()
    assert landed(state, 2, SIDE) == [[(-32768, -32768), (32768, 32768)]]
    X, Y = bl.quantise_positions(state, 2, SIDE)
    assert lc.links(X, Y, 128).tolist() == [[[True, False], [False, True]]]
    assert ((2 ** 16) ** 2) % 2 ** 32 == 0 and 0 < (16 * 128) ** 2
    grids = fresh(1, 2, SIDE)
    grids[0, 0] = 1000
    lc.local_coverage_actions_torch(state, grids, 2, SIDE, VR, KEEP, 128)
    assert bool((grids[0, 0] == 1000 + ((65536 - 1000) >> 8)).all()) and bool((grids[0, 1] == 65536).all())
    lc.local_coverage_actions_torch(state, grids, 2, SIDE, VR, KEEP, -1)   # (unlimited: now they do merge)
    assert torch.equal(grids[0, 0], grids[0, 1]) and int(grids[0, 1, 0]) < 65536


def test_agents_drop_into_a_policy_callable_and_reset_at_step_zero():
    args = cs.make_env_args("flight_easy", n_agents=3)
    ag = cs.LocalCoverageAgents(args, 10, batch=2, device="cpu", impl="torch")
    pol = ag.policy()
    states = walk(2, 3, 3, 9, tail=45)
    a0 = pol(None, states[0], None, 0)
    g0 = ag.grids.clone()
    pol(None, states[1], None, 1)
    assert not torch.equal(ag.grids, g0)
    a1 = pol(None, states[0], None, 0)
    assert torch.equal(a0, a1) and torch.equal(ag.grids, g0) and a0.shape == (2, 3) and a0.dtype == torch.int64


def test_label_episodes_takes_the_class_through_the_rows_path():
    """Unlimited range labels recorded rows as CoverageAgents does; the second episode ends after three rows."""
    E, T, n = 2, 5, 3
    s = torch.stack(walk(E, n, T, 12, tail=45), 1)
    padded = torch.zeros(E, T, 1)
    padded[1, 3:] = 1.0
    batch = {"s": s, "padded": padded}
    args = cs.make_env_args("flight_easy", n_agents=n)
    local = cs.LocalCoverageAgents(args, None, batch=E, device="cpu", impl="torch")
    shared = cs.CoverageAgents(args, batch=E, device="cpu", impl="torch")
    got, want = cs.label_episodes(local, batch, impl="rows"), cs.label_episodes(shared, batch, impl="rows")
    assert torch.equal(got, want) and got.shape == (E, T, n) and not bool(got[1, 3:].any())
    assert bool((local.grids == bl.FRESH).all())   # the rows path ends with reset()
