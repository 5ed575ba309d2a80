"""CPU tests of the private-grid observations (localobs.py, include/coopsearch.h: cs_local_grid_features, cs_local_feature_episodes;
DESIGN.md section 27): the boundary declares, exports and registers both entry points and refuses bad arguments before any launch;
the definitions are the centralised ones at an unlimited range (identity A), n lone filters' at range 0 (B) and the rows path's labels
(C); in between they do what a hand case says; the acting class feeds the network [16 features of MY grid | obs | last | id] and
resets with its filter.  Everything is torch.equal on integers or on float bits: no tolerance, and no threshold on what a policy
finds."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import gridobs as go
from cooperative_search_amd import imitate as im
from cooperative_search_amd import local as lc
from cooperative_search_amd import local_belief as lb
from cooperative_search_amd import localobs as lo
from cooperative_search_amd import motion as mo
from imitate_util import bc_args
from local_util import KEEP, LINE, SIDE, SWEPT, VR, disc, fresh, landed, rows_at, walk
from localobs_util import SEED, T, WALK_SHAPES, episodes, lens_for, link_stats, params, ranges_for, same_bits, spoil_past

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def one_thread():
    """The definitions' tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


# ---- 1. the boundary ------------------------------------------------------------------------------------------------------------

LABEL_FIELDS = ["expert", "n_agents", "side", "view_range", "keep", "regrow", "lookahead", "state_width", "mode", "sense16", "every", "moving",
                "dx[16]", "dy[16]"]


def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    assert "cs_local_label_params, cs_local_grid_features and cs_local_feature_episodes" in re.search(
        r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_local_grid_features\s*\(\s*const\s+cs_grid_params\s*\*", header)
    assert re.search(r"\bint\s+cs_local_feature_episodes\s*\(\s*const\s+cs_local_label_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_local_grid_features" in _lib.EXPORTS and "cs_local_feature_episodes" in _lib.EXPORTS
    L = _lib.load()
    assert len(L.cs_local_grid_features.argtypes) == 6 and len(L.cs_local_feature_episodes.argtypes) == 11
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    named = lambda fields: [k + ("[16]" if t is not C.c_int32 else "") for k, t in fields]
    want = LABEL_FIELDS + ["comm_range", "reserved"]
    fields = re.search(r"typedef struct cs_local_label_params \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+(?:\[16\])?);", fields) == want
    assert named(_lib.CsLocalLabelParams._fields_) == want
    assert named(_lib.CsLabelParams._fields_) == LABEL_FIELDS + ["reserved"]   # cs_label_params' fields first
    assert C.sizeof(_lib.CsLocalLabelParams) == 4 * (12 + 32 + 2)
    ops = _lib.torch_ops()
    assert str(ops.local_grid_features.default._schema) == (
        "coopsearch::local_grid_features(Tensor state, Tensor grids, Tensor(a!) feat, int n_agents, int side, int view_range, int lookahead) -> ()")
    assert str(ops.local_feature_episodes.default._schema) == (
        "coopsearch::local_feature_episodes(Tensor s, Tensor lens, Tensor(a!) feat, Tensor(b!)? labels, Tensor(c!) grids, Tensor(d!)? prev_out, "
        "Tensor(e!)? heard_out, int expert, int n_agents, int side, int view_range, int keep, int regrow, int lookahead, int mode, "
        "int sense16, int every, int moving, int[] dx, int[] dy, int comm_range) -> ()")
    from cooperative_search_amd import build
    assert "localobs.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "local_grid_features") and not hasattr(_lib.CtypesOps, "local_feature_episodes")   # no ctypes twin
    for name in ("LocalExpertParams", "LocalGridAgents", "distil_local_grid", "local_expert_params", "local_feature_episodes",
                 "local_feature_episodes_hip", "local_feature_episodes_torch", "local_grid_features", "local_grid_features_hip",
                 "local_grid_features_torch", "local_label_episodes"):
        assert getattr(cs, name) is getattr(lo, name), name
    # the definitions import their parts; they do not restate them
    assert lo.quantise is bl.quantise and lo.cell_centres is bl.cell_centres and lo.disc_mask is bl.disc_mask and lo.greedy_choose is bl.greedy_choose
    assert lo.links is lc.links and lo.local_coverage_actions_torch is lc.local_coverage_actions_torch and lo._check_comm is lc._check_comm
    assert lo.local_belief_actions_torch is lb.local_belief_actions_torch and lo.grid_features_torch is go.grid_features_torch
    assert (lo.REL, lo.DIST, lo.PROBES, lo.SCALE) == (go.REL, go.DIST, go.PROBES, go.SCALE) and lo.CAP is be.CAP and lo.targets_moved is be.targets_moved


def test_kernels_are_included_after_the_helpers_they_call_and_no_existing_header_restates_them():
    csrc = os.path.join(ROOT, "cooperative-search_amd", "csrc")
    ep = open(os.path.join(csrc, "episodes.hip")).read()
    assert ep.index('#include "local_belief.h"') < ep.index('#include "localobs.h"') and ep.index('#include "gridobs.h"') < ep.index('#include "localobs.h"')
    code = re.sub(r"//.*", "", open(os.path.join(csrc, "localobs.h")).read())
    for helper in ("cov_quant", "cov_point", "cov_box", "cov_within", "cov_update", "bel_update", "lbel_scatter", "go_point", "go_probe_sum",
                   "go_feature", "COV_CT", "COV_ST"):
        assert helper + "(" in code or helper + "[" in code, helper
    assert "atomic" not in code   # LDS atomics are bel_spread's only; nothing global
    for helper in ("cov_quant", "cov_update", "bel_update", "lbel_scatter", "go_point", "go_probe_sum", "go_feature"):
        assert not re.search(r"__device__[^;{]*\b" + helper + r"\s*\(", code), helper   # called, not defined again


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("view_range", -1, "view_range"),
    ("view_range", 65, "view_range"), ("lookahead", -1, "lookahead"), ("lookahead", 51, "lookahead"), ("state_width", 11, "state_width"),
    ("reserved", 1, "reserved"), ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("params", None, "NULL"),
    ("align", 0, "aligned"), ("align", 1, "aligned"), ("align", 2, "aligned")])
def test_decision_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = _lib.CsGridParams(3, 50, 7, 7, 57, 0)
    B, ptrs = 4, [256, 512, 1024]   # state, grids, feat
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2
    elif field == "B":
        B = value
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_local_grid_features(None if field == "params" else C.byref(p), ptrs[0], B, ptrs[1], ptrs[2], None)
    assert rc == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_local_grid_features") and msg in err


def good_label_params():
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), 50)
    return _lib.CsLocalLabelParams(1, 3, 50, 7, KEEP, 8, 7, 57, m.mode, m.sense16, 1, 1, (C.c_int32 * 16)(*m.dx), (C.c_int32 * 16)(*m.dy), 10, 0)


@pytest.mark.parametrize("field, value, msg", [
    ("expert", 2, "expert"), ("expert", -1, "expert"), ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"),
    ("side", 65, "side"), ("view_range", -1, "view_range"), ("view_range", 65, "view_range"), ("keep", -1, "keep"), ("keep", 65537, "keep"),
    ("regrow", 0, "regrow"), ("regrow", 17, "regrow"), ("lookahead", -1, "lookahead"), ("lookahead", 51, "lookahead"),
    ("state_width", 11, "state_width"), ("mode", 2, "mode"), ("sense16", -1, "sense16"), ("sense16", 2049, "sense16"), ("every", 0, "every"),
    ("moving", 2, "moving"), ("dx", (3, 1025), "dx and dy"), ("dy", (7, -1025), "dx and dy"), ("comm_range", -2, "comm_range"),
    ("comm_range", 129, "comm_range"), ("reserved", 1, "reserved"), ("E", 0, "E and T"), ("T", 0, "E and T"), ("ptr", 0, "NULL"),
    ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("ptr", 4, "NULL"), ("params", None, "NULL"), ("align", 0, "aligned"), ("align", 1, "aligned"),
    ("align", 2, "aligned"), ("align", 3, "aligned"), ("align", 4, "aligned"), ("align", 5, "aligned"), ("align", 6, "aligned"),
    ("coverage_prev", None, "prev_dev"), ("coverage_heard", None, "heard_dev"), ("expert_with_labels", 2, "expert")])
def test_episode_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    L = _lib.load()
    p = good_label_params()
    E, steps, ptrs = 4, 5, [256, 512, 1024, 2048, 4096, 8192, 16384]   # s, lens, feat, labels, grids, prev, heard
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 4 if value == 3 else 2
    elif field in ("E", "T"):
        E, steps = (value, steps) if field == "E" else (E, value)
    elif field in ("dx", "dy"):
        getattr(p, field)[value[0]] = value[1]
    elif field == "coverage_prev":
        p.expert, ptrs[6] = 0, None
    elif field == "coverage_heard":
        p.expert, ptrs[5] = 0, None
    elif field == "expert_with_labels":
        p.expert = value
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_local_feature_episodes(None if field == "params" else C.byref(p), ptrs[0], ptrs[1], E, steps, ptrs[2], ptrs[3], ptrs[4], ptrs[5],
                                     ptrs[6], None)
    assert rc == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_local_feature_episodes") and msg in err


def test_ops_refuse_bad_integers_shapes_and_cpu_tensors():
    ops = _lib.torch_ops()
    state, grids, feat = torch.zeros(2, 57), torch.zeros(2, 3, 2500, dtype=torch.int32), torch.zeros(2, 3, 16)
    good = dict(n_agents=3, side=50, view_range=7, lookahead=7)

    def one(state=state, grids=grids, feat=feat, **kw):
        a = dict(good, **kw)
        ops.local_grid_features(state, grids, feat, *(a[k] for k in good))

    for kw, msg in [(dict(n_agents=0), "n_agents"), (dict(n_agents=9), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"),
                    (dict(view_range=-1), "view_range"), (dict(lookahead=51), "lookahead"), (dict(state=torch.zeros(2, 11)), "state must be"),
                    (dict(state=torch.zeros(57)), "state must be"), (dict(grids=grids[:, 0]), "grids must be"), (dict(grids=grids[:, :2]), "grids must be"),
                    (dict(grids=grids[:1]), "grids must be"), (dict(feat=feat[:, :2]), "feat must be"), (dict(feat=torch.zeros(2, 3, 8)), "feat must be"),
                    (dict(), "GPU tensor")]:
        with pytest.raises(RuntimeError, match=msg):   # integers and shapes come first: the CPU tensors are not reached
            one(**kw)
    assert not feat.any()
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), 50)
    s, lens, labels = torch.zeros(2, 4, 57), torch.full((2,), 4, dtype=torch.int32), torch.zeros(2, 4, 3, dtype=torch.int64)
    f4, prev, heard = torch.zeros(2, 4, 3, 16), torch.zeros(2, 8, 2, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32)
    good = dict(expert=1, n_agents=3, side=50, view_range=7, keep=KEEP, regrow=8, lookahead=7, mode=1, sense16=m.sense16, every=1, moving=1,
                dx=list(m.dx), dy=list(m.dy), comm_range=10)

    def many(s=s, lens=lens, feat=f4, labels=labels, grids=grids, prev=prev, heard=heard, **kw):
        a = dict(good, **kw)
        ops.local_feature_episodes(s, lens, feat, labels, grids, prev, heard, *(a[k] for k in good))

    for kw, msg in [(dict(expert=2), "expert"), (dict(n_agents=0), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"),
                    (dict(keep=65537), "keep"), (dict(regrow=0), "regrow"), (dict(lookahead=51), "lookahead"), (dict(mode=2), "mode"),
                    (dict(sense16=2049), "sense16"), (dict(every=0), "every"), (dict(moving=2), "moving"), (dict(dx=[0] * 15), "16 integers"),
                    (dict(dy=[1025] + [0] * 15), "-1024..1024"), (dict(comm_range=-2), "comm_range"), (dict(comm_range=129), "comm_range"),
                    (dict(s=torch.zeros(2, 57)), "s must be"), (dict(s=torch.zeros(2, 4, 11)), "s must be"), (dict(lens=lens[:1]), "lens must be"),
                    (dict(feat=f4[:, :3]), "feat must be"), (dict(feat=torch.zeros(2, 4, 3, 8)), "feat must be"),
                    (dict(labels=labels[:, :3]), "labels must be"), (dict(grids=grids[:, 0]), "grids must be"), (dict(grids=grids[:, :, :7]), "grids must be"),
                    (dict(prev=prev[:, :7]), "prev_out must be"), (dict(heard=heard[:, :7]), "heard_out must be"), (dict(heard=prev), "heard_out must be"),
                    (dict(expert=0), "prev_out is the belief"), (dict(expert=0, prev=None), "heard_out is the belief"), (dict(), "GPU tensor"),
                    (dict(labels=None, prev=None, heard=None), "GPU tensor")]:
        with pytest.raises(RuntimeError, match=msg):
            many(**kw)
    with pytest.raises((RuntimeError, TypeError)):   # the workspace is required: None is no tensor
        many(grids=None)
    assert not f4.any() and not labels.any() and not grids.any()


def test_python_layer_and_classes_refuse_bad_arguments():
    state, grids = walk(2, 3, 1, 0)[0], fresh(2, 3, 50)
    for kw in (dict(n_agents=0), dict(n_agents=9), dict(side=65), dict(view_range=65), dict(lookahead=51), dict(lookahead=-1)):
        a = dict(dict(n_agents=3, side=50, view_range=7), **kw)
        with pytest.raises(ValueError):
            lo.local_grid_features_torch(state, grids, **a)
    for bad_state, bad_grids in ((state.double(), grids), (state[0], grids), (state[:, :11], grids), (state, grids.long()), (state, grids[:1]),
                                 (state, grids[:, 0]), (state, grids[:, :2]), (state, grids[:, :, :7]), (state, None)):
        with pytest.raises(ValueError):
            lo.local_grid_features_torch(bad_state, bad_grids, 3, 50, 7)
    with pytest.raises(ValueError, match="impl must be"):
        lo.local_grid_features(state, grids, 3, 50, 7, impl="fused")
    with pytest.raises(ValueError, match="no CPU fallback"):
        lo.local_grid_features(state, grids, 3, 50, 7, impl="hip")
    assert same_bits(lo.local_grid_features(state, grids, 3, 50, 7), lo.local_grid_features_torch(state, grids, 3, 50, 7))   # "auto" on the CPU
    # the parameters
    p = params("coverage", None, 0.0, 3, 50, 7, 10)
    assert dataclass_fields(p)[:-1] == dataclass_fields(im.ExpertParams(im.COVERAGE, 3, 50, 7, KEEP)) and dataclass_fields(p)[-1] == "comm_range"
    assert isinstance(p, im.ExpertParams) and p != im.ExpertParams(im.COVERAGE, 3, 50, 7, KEEP) and p.lookahead == 7
    with pytest.raises(Exception):
        p.comm_range = 3   # frozen
    for comm in (-2, 129):
        with pytest.raises(ValueError, match="comm_range"):
            lo.LocalExpertParams(im.COVERAGE, 3, 50, 7, KEEP, comm_range=comm)
    with pytest.raises(ValueError, match="expert"):
        lo.LocalExpertParams(2, 3, 50, 7, KEEP)
    q = params("belief", "evade", 1.0, 3, 50, 7, -1, every=3)
    twin = im.ExpertParams(im.BELIEF, 3, 50, 7, KEEP, 8, None, q.model, 3, 1)
    assert [q.moved(t) for t in range(9)] == [twin.moved(t) for t in range(9)] == [0, 1, 0, 0, 1, 0, 0, 1, 0]
    assert [p.moved(t) for t in range(4)] == [0, 0, 0, 0]
    args = cs.make_env_args("flight_easy")
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=3)
    cov = cs.LocalCoverageAgents(args, 10, batch=2, device="cpu", impl="torch", regrow=5)
    bel = cs.LocalBeliefAgents(args, None, motion=motion, batch=2, device="cpu", impl="torch")
    assert lo.local_expert_params(cov) == lo.LocalExpertParams(im.COVERAGE, 3, 50, 7, KEEP, 5, 7, comm_range=10)
    assert lo.local_expert_params(bel) == lo.LocalExpertParams(im.BELIEF, 3, 50, 7, KEEP, 8, 7, bel.model, 3, 1, comm_range=-1)
    still = cs.LocalBeliefAgents(args, 0, motion=mo.TargetMotion(mode="walk", speed=0.0), batch=2, device="cpu", impl="torch")
    assert lo.local_expert_params(still).moving == 0 and lo.local_expert_params(still).comm_range == 0

    class Sub(cs.LocalCoverageAgents):
        pass

    for foreign in (cs.CoverageAgents(args, batch=2, device="cpu", impl="torch"), cs.BeliefAgents(args, motion=motion, batch=2, device="cpu", impl="torch"),
                    Sub(args, 10, batch=2, device="cpu", impl="torch"), cs.PlanAgents(args, base="coverage", batch=2, device="cpu", impl="torch")):
        with pytest.raises(TypeError, match="private grids"):
            lo.local_expert_params(foreign)
    # the batch functions
    s, lens = episodes(2, 3, 3), torch.tensor([3, 1], dtype=torch.int32)
    for bad_s, bad_lens in ((s.double(), lens), (s[0], lens), (s[:, :, :11], lens), (s, lens.long()), (s, torch.tensor([4, 0], dtype=torch.int32)),
                            (s, torch.tensor([-1, 0], dtype=torch.int32))):
        with pytest.raises(ValueError):
            lo.local_feature_episodes_torch(bad_s, bad_lens, p)
    for not_params in (dict(expert=0), im.ExpertParams(im.COVERAGE, 3, 50, 7, KEEP)):
        with pytest.raises(TypeError, match="LocalExpertParams"):
            lo.local_feature_episodes_torch(s, lens, not_params)
        with pytest.raises(TypeError, match="LocalExpertParams"):
            lo.local_feature_episodes_hip(s, lens, not_params)
    batch = {"s": s, "padded": torch.zeros(2, 3, 1)}
    with pytest.raises(ValueError, match="impl must be"):
        lo.local_feature_episodes(cov, batch, impl="rows")
    with pytest.raises(ValueError, match="no CPU fallback"):
        lo.local_feature_episodes(cov, batch, impl="hip")
    with pytest.raises(ValueError, match="impl must be"):
        lo.local_label_episodes(cov, batch, impl="torch")
    with pytest.raises(ValueError, match="no CPU fallback"):
        lo.local_label_episodes(cov, batch, impl="hip")
    for fn in (lo.local_feature_episodes, lo.local_label_episodes):
        with pytest.raises(TypeError, match="private grids"):
            fn(cs.CoverageAgents(args, batch=2, device="cpu", impl="torch"), batch)
    with pytest.raises(ValueError, match=r"\[E, T, S\]"):
        lo.local_feature_episodes(cov, {"s": s[0], "padded": torch.zeros(2, 3, 1)})
    feat, labels = lo.local_feature_episodes(cov, batch, labels=True)
    want = lo.local_feature_episodes_torch(s, torch.full((2,), 3, dtype=torch.int32), lo.local_expert_params(cov))
    assert same_bits(feat, want[0]) and torch.equal(labels, want[1]) and same_bits(lo.local_feature_episodes(cov, batch), want[0])
    assert want[3] is None and want[4] is None and bool((cov.grids == bl.FRESH).all())   # the filter's own grids: neither read nor written
    # gridobs and imitate keep refusing the local classes
    with pytest.raises(TypeError):
        go.feature_episodes(cov, batch)
    with pytest.raises(TypeError):
        go.GridAgents(bc_args(), cs.LocalCoverageAgents(bc_args(), 10, batch=4, device="cpu", impl="torch"))
    with pytest.raises(ValueError, match="hip"):
        im.label_episodes(cov, batch, impl="hip")


def dataclass_fields(p):
    import dataclasses
    return [f.name for f in dataclasses.fields(p)]


def test_local_grid_agents_refuse_a_conv_variant_a_foreign_filter_and_a_narrow_net():
    args = bc_args()
    filt = cs.LocalCoverageAgents(args, 10, batch=4, device="cpu", impl="torch")
    with pytest.raises(ValueError, match="32 input columns"):
        lo.LocalGridAgents(bc_args(env="flight", conv=True), filt)
    for foreign in (cs.CoverageAgents(args, batch=4, device="cpu", impl="torch"), cs.PlanAgents(args, base="coverage", batch=4, device="cpu", impl="torch")):
        with pytest.raises(TypeError, match="filter must be"):
            lo.LocalGridAgents(args, foreign)
    with pytest.raises(ValueError, match="the filter serves"):
        lo.LocalGridAgents(args, filt, batch=5)
    with pytest.raises(ValueError, match="the filter serves"):
        lo.LocalGridAgents(bc_args(n_agents=5), filt)
    with pytest.raises(ValueError, match="fc1 must take"):
        lo.LocalGridAgents(args, filt, net=cs.AgentRNN(cs.rnn_input_shape(args), args))


# ---- 2. identities A and B of one decision, over a walk ------------------------------------------------------------------------------

def fly(kind, states, n, side, vr, comm, centralised=False):
    """The coverage or belief (evade 1.0) step definition over consecutive rows from fresh grids -> the grids after every row: [B, n,
    cells] of the local definition, [B, cells] of the centralised one."""
    B = states[0].shape[0]
    model = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), side)
    prev, heard, out = torch.zeros(B, 8, 2, dtype=torch.int32), torch.zeros(B, 8, dtype=torch.int32), []
    g = torch.full((B, side * side), bl.FRESH, dtype=torch.int32) if centralised else fresh(B, n, side)
    for t, s in enumerate(states):
        moved = 1 if t > 0 else 0
        if centralised:
            if kind == "coverage":
                bl.coverage_actions_torch(s, g, n, side, vr, KEEP)
            else:
                be.belief_actions_torch(s, g, prev, n, side, vr, KEEP, model, moved)
        elif kind == "coverage":
            lc.local_coverage_actions_torch(s, g, n, side, vr, KEEP, comm)
        else:
            lb.local_belief_actions_torch(s, g, prev, heard, n, side, vr, KEEP, model, moved, comm)
        out.append(g.clone())
    return out


@pytest.mark.parametrize("kind", ["coverage", "belief"])
@pytest.mark.parametrize("B, n, side, vr", WALK_SHAPES[1:])
def test_identity_a_and_b_of_one_decision(B, n, side, vr, kind):
    """A, unlimited range: the n grids stay equal, and every agent's row equals grid_features_torch on the shared grid.  B, range 0:
    row i equals grid_features_torch with n_agents = 1 on agent i's four floats and grid i -- and there the private features DO
    differ from the shared-grid ones (coverage, 12 calls of local_util.walk(.., seed 5): 498 of 1728, 1380 of 1920 and 1720 of 3072
    entries), so the test cannot pass on a shared grid."""
    states = walk(B, n, T, SEED)
    shared = fly(kind, states, n, side, vr, -1, centralised=True)
    whole = fly(kind, states, n, side, vr, -1)
    alone = fly(kind, states, n, side, vr, 0)
    differ = total = 0
    for t, s in enumerate(states):
        want = go.grid_features_torch(s, shared[t], n, side, vr)
        assert all(torch.equal(whole[t][:, i], shared[t]) for i in range(n)), t
        assert same_bits(lo.local_grid_features_torch(s, whole[t], n, side, vr), want), t
        got, sums = lo.local_grid_features_torch(s, alone[t], n, side, vr, return_sums=True)
        by_rows = [go.grid_features_torch(s, alone[t][:, i].contiguous(), n, side, vr, return_sums=True) for i in range(n)]
        assert same_bits(got, torch.stack([by_rows[i][0][:, i] for i in range(n)], 1)), t   # the definition's vectorised form IS row i of
        assert torch.equal(sums, torch.stack([by_rows[i][1][:, i] for i in range(n)], 1)), t   # grid_features_torch(state, grids[:, i])
        for i in range(n):
            lone, lone_sums = go.grid_features_torch(s[:, 4 * i:4 * i + 4].contiguous(), alone[t][:, i].contiguous(), 1, side, vr, return_sums=True)
            assert same_bits(got[:, i], lone[:, 0]) and torch.equal(sums[:, i], lone_sums[:, 0]), (t, i)
        differ += int((got != want).sum())
        total += got.numel()
    print(f"identity B, {kind}, {(B, n, side, vr)}: {differ} of {total} private features differ from the shared grid's")
    assert total == B * n * 16 * T and differ > 0


# ---- 3. identities A and C of a recorded batch ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind, mode, speed", [("coverage", None, 0.0), ("belief", "evade", 1.0), ("belief", "walk", 0.25)])
@pytest.mark.parametrize("E, n, side, vr", WALK_SHAPES)
def test_identity_a_unlimited_range_is_the_centralised_walk(E, n, side, vr, kind, mode, speed):
    s, lens = episodes(E, n), lens_for(E, shift=n)
    p = params(kind, mode, speed, n, side, vr, -1, every=3 if speed == 1.0 else 1)
    central = im.ExpertParams(p.expert, n, side, vr, KEEP, 8, None, p.model, p.every, p.moving)
    feat, labels, grids, prev, heard = lo.local_feature_episodes_torch(spoil_past(s, lens), lens, p)
    want = go.feature_episodes_torch(s, lens, central)
    assert same_bits(feat, want[0]) and torch.equal(labels, want[1])
    assert all(torch.equal(grids[:, i], want[2]) for i in range(n))
    if kind == "belief":
        assert torch.equal(prev, want[3])
        full = torch.where(lens.view(E, 1) > 0, (1 << n) - 1, 0)
        assert torch.equal(heard[:, :n], full.expand(E, n).to(torch.int32)) and not heard[:, n:].any()
    else:
        assert prev is None and heard is None and want[3] is None
    assert bool(feat.any()) or int(lens.max()) == 0


def rows_expert(kind, mode, speed, n, side, vr, comm, every, E):
    env_like = types.SimpleNamespace(n_agents=n, map_size=side, view_range=vr, detect_prob=0.9, batch=E, device="cpu")
    if kind == "coverage":
        return cs.LocalCoverageAgents(env_like, None if comm < 0 else comm, impl="torch")
    motion = mo.TargetMotion(mode=mode, speed=speed, sense=10.0, every=every)
    return cs.LocalBeliefAgents(env_like, None if comm < 0 else comm, motion=motion, impl="torch")


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("kind, mode, speed, every", [("coverage", None, 0.0, 1), ("belief", "evade", 1.0, 3), ("belief", "walk", 0.25, 1)])
@pytest.mark.parametrize("E, n, side, vr", WALK_SHAPES)
def test_identity_c_the_rows_path(E, n, side, vr, kind, mode, speed, every, which):
    """The labels equal imitate.label_episodes(expert, batch, impl="rows") with the definition-backed experts, at every range (which:
    unlimited, 0, the mixed one); on full-length episodes the final grids, prev and heard equal what the expert holds after flying its
    own policy() over the rows."""
    s = episodes(E, n)
    comm = ranges_for(s, n, side)[which]
    expert = rows_expert(kind, mode, speed, n, side, vr, comm, every, E)
    p = lo.local_expert_params(expert)
    assert p == params(kind, mode, speed, n, side, vr, comm, every)
    lens = lens_for(E, shift=which)
    batch = {"s": spoil_past(s, lens), "padded": (torch.arange(T).view(1, T, 1) >= lens.view(E, 1, 1)).float()}
    assert torch.equal(im.episode_lens(batch), lens)
    feat, labels = lo.local_feature_episodes(expert, batch, labels=True, impl="torch")
    safe = dict(batch, s=torch.where(batch["padded"].bool(), torch.zeros_like(s), s))   # (the rows path flies the padded rows too)
    assert torch.equal(labels, lo.local_label_episodes(expert, safe)), comm   # on the CPU: imitate.label_episodes(..., impl="rows")
    assert bool((expert.grids == bl.FRESH).all())   # the rows path ends with expert.reset()
    full = torch.full((E,), T, dtype=torch.int32)
    _, full_labels, grids, prev, heard = lo.local_feature_episodes_torch(s, full, p)
    policy = expert.policy()
    flown = torch.stack([policy(None, s[:, t].contiguous(), None, t) for t in range(T)], 1)
    assert torch.equal(full_labels, flown) and torch.equal(grids, expert.grids), comm
    live = torch.arange(T).view(1, T, 1) < lens.view(E, 1, 1)
    assert torch.equal(labels, torch.where(live, flown, torch.zeros_like(flown)))   # an episode's labels do not depend on where it ends
    if kind == "belief":
        assert torch.equal(prev, expert.prev) and torch.equal(heard, expert.heard), comm
        assert bool((heard[:, :n] & (1 << torch.arange(n, dtype=torch.int32))).all()) and not heard[:, n:].any() and not prev[:, n:].any()


def test_local_label_episodes_defers_to_the_rows_path(monkeypatch):
    seen = []
    monkeypatch.setattr(im, "label_episodes", lambda expert, batch, impl="auto": seen.append(impl) or "labels")
    cov = cs.LocalCoverageAgents(cs.make_env_args("flight_easy"), 10, batch=2, device="cpu", impl="torch")
    batch = {"s": episodes(2, 3, 3), "padded": torch.zeros(2, 3, 1)}
    assert lo.local_label_episodes(cov, batch, impl="rows") == "labels" and lo.local_label_episodes(cov, batch) == "labels" and seen == ["rows", "rows"]


def test_the_mixed_ranges_are_mixed_and_range_ten_is_not():
    """The condition the GPU tests rely on, asserted on the inputs: at the mixed range of every shape the walk has linked and unlinked
    pairs and links that flip between rows; range 10 at side 50 links nobody on that walk (it is range 0 again)."""
    for E, n, side, vr in WALK_SHAPES[1:]:
        s = episodes(E, n)
        linked, pairs, flips = link_stats(s, n, side, ranges_for(s, n, side)[2])
        print(f"{(E, n, side)}: {linked} of {pairs} ordered pairs linked, {flips} flips")
        assert 0 < linked < pairs and flips > 0
    assert link_stats(episodes(3, 3), 3, 50, 10)[0] == 0


# ---- 4. a hand case, the probe limits and the rows past the end ----------------------------------------------------------------------

def test_hand_case_a_line_of_three_at_range_ten():
    """A - B - C of local_util.LINE, 8 cells apart, heading +x, at range 10: A-B and B-C are linked, A-C is not.  After one coverage
    call from fresh grids agent i's grid holds SWEPT = 6554 in the discs of the agents it heard and 65536 elsewhere, so a probe sum is
    6554 k + 65536 (cells - k) with k the probe's cells inside the heard discs.  B heard both: its rear probe (ring 0, bearing 18) lies
    on A's look-ahead probe (ring 0, bearing 0) and sees A's disc as A does; C's rear probe is C's view toward B."""
    state = rows_at([LINE], SIDE)
    assert landed(state, 3, SIDE) == [[(x, y) for x, y, _ in LINE]]
    grids = fresh(1, 3, SIDE)
    lc.local_coverage_actions_torch(state, grids, 3, SIDE, VR, KEEP, 10)
    feat, sums = lo.local_grid_features_torch(state, grids, 3, SIDE, VR, return_sums=True)
    discs = [disc(x, y, SIDE, VR) for x, y, _ in LINE]
    heard = {0: discs[0] | discs[1], 1: discs[0] | discs[1] | discs[2], 2: discs[1] | discs[2]}
    look = 16 * VR
    for i, (x, y, _) in enumerate(LINE):
        for k, px in ((0, x + look), (7, x - look)):   # ring 0: straight ahead (toward the next agent) and straight behind
            foot = disc(px, y, SIDE, VR)
            inside, cells = int((foot & heard[i]).sum()), int(foot.sum())
            assert cells == (149 if px >= look else 121) and int(sums[0, i, k]) == SWEPT * inside + 65536 * (cells - inside), (i, k)   # (A's rear probe: the wall)
            assert float(feat[0, i, k]) == float((SWEPT * inside + 65536 * (cells - inside)) >> 8) * 2.0 ** -15
    # The same probe points read on B's grid (B heard everybody: its grid is the shared one).  Ring 0 of A looks at B, whom A heard:
    # no difference.  Ring 1 of A (three look-aheads ahead) looks past B at C's disc, of which A has not heard: the difference is
    # exactly C's share of that footprint, (65536 - 6554) per cell.  C's rear probes mirror it.
    b_grid = go.grid_features_torch(state, grids[:, 1].contiguous(), 3, SIDE, VR, return_sums=True)[1]
    for i, k_near, k_far, sign, other in ((0, 0, 8, 1, 2), (2, 7, 15, -1, 0)):
        x = LINE[i][0]
        assert int(sums[0, i, k_near]) == int(b_grid[0, i, k_near])
        unheard = int((disc(x + sign * 3 * look, 408, SIDE, VR) & discs[other] & ~heard[i]).sum())
        assert unheard > 0 and int(sums[0, i, k_far]) - int(b_grid[0, i, k_far]) == (65536 - SWEPT) * unheard == 58982 * unheard, (i, unheard)
    shared = torch.full((1, SIDE * SIDE), bl.FRESH, dtype=torch.int32)
    bl.coverage_actions_torch(state, shared, 3, SIDE, VR, KEEP)
    assert torch.equal(grids[:, 1], shared) and same_bits(feat[:, 1], go.grid_features_torch(state, shared, 3, SIDE, VR)[:, 1])   # B knows all


def test_probe_limits_lookahead_zero_and_view_range_zero_and_sixty_four():
    n, side = 3, 50
    state = walk(2, n, 3, 1)[2]
    g = torch.Generator().manual_seed(2)
    grids = torch.randint(-70000, 600000, (2, n, side * side), generator=g, dtype=torch.int32)   # below 0 and above CAP too
    feat = lo.local_grid_features_torch(state, grids, n, side, 7, 0)
    assert bool((feat == feat[:, :, :1]).all()) and feat[:, :, 0].unique().numel() > 1   # sixteen equal features, other ones per agent
    assert same_bits(feat, lo.local_grid_features_torch(state, grids.clamp(0, be.CAP), n, side, 7, 0))
    assert same_bits(lo.local_grid_features_torch(state, grids, n, side, 7), lo.local_grid_features_torch(state, grids, n, side, 7, 7))
    centre = rows_at([[(408, 408, 0), (400, 408, 9), (408, 408, 18)]], side)   # agents 0 and 2 on the centre of cell (25, 25), agent 1 between centres
    cells = (torch.arange(side * side, dtype=torch.int32) * 100 + 300).view(1, 1, -1) + torch.tensor([0, 1 << 8, 2 << 8], dtype=torch.int32).view(1, 3, 1)
    feat, sums = lo.local_grid_features_torch(centre, cells.contiguous(), n, side, 0, 0, return_sums=True)
    own = 25 * side + 25
    assert bool((sums[0, 0] == own * 100 + 300).all()) and not sums[0, 1].any() and bool((sums[0, 2] == own * 100 + 300 + 512).all())
    full = torch.full((2, 8, 64 * 64), be.CAP, dtype=torch.int32)
    full[:, 1::2] = 1
    feat, sums = lo.local_grid_features_torch(walk(2, 8, 1, 4)[0], full, 8, 64, 64, return_sums=True)
    assert int(sums[:, 0::2].max()) <= 1 << 31 and int(sums[:, 0::2].min()) > 1 << 19 and int(sums[:, 1::2].max()) <= 4096
    assert bool(torch.isfinite(feat).all()) and float(feat.max()) <= 256.0
    middle = torch.tensor([[0.0, 0.0, 1.0, 0.0] * 8] * 2)
    feat, sums = lo.local_grid_features_torch(middle, full, 8, 64, 64, 0, return_sums=True)   # from the centre: the whole map
    assert bool((sums[:, 0::2] == 1 << 31).all()) and bool((feat[:, 0::2] == 256.0).all()) and bool((sums[:, 1::2] == 4096).all())


@pytest.mark.parametrize("kind, mode, speed", [("coverage", None, 0.0), ("belief", "evade", 1.0)])
def test_rows_past_the_end_are_never_read(kind, mode, speed):
    E, n, side, vr = 4, 3, 50, 7
    s, lens = episodes(E, n, 6), torch.tensor([6, 0, 4, 1], dtype=torch.int32)
    p = params(kind, mode, speed, n, side, vr, 30)
    poisoned = spoil_past(s, lens)
    keep_s, keep_lens = poisoned.clone(), lens.clone()
    got, want = lo.local_feature_episodes_torch(poisoned, lens, p), lo.local_feature_episodes_torch(s, lens, p)
    assert same_bits(got[0], want[0]) and all(a is None and b is None or torch.equal(a, b) for a, b in zip(got[1:], want[1:]))
    assert torch.equal(lens, keep_lens) and same_bits(poisoned, keep_s)
    feat, labels, grids, prev, heard = got
    for e in range(E):
        tail = feat[e, int(lens[e]):]
        assert same_bits(tail, torch.zeros_like(tail)) and not labels[e, int(lens[e]):].any()   # +0.0, not -0.0 or NaN
    assert bool((grids[1] == bl.FRESH).all()) and bool(feat[0].any()) and not same_bits(feat[0, 0], feat[0, 5])
    if kind == "belief":
        assert not prev[1].any() and not heard[1].any()
    # an ended episode keeps its state: the same rows as a shorter batch
    short = lo.local_feature_episodes_torch(s[:, :4].contiguous(), torch.tensor([4, 0, 4, 1], dtype=torch.int32), p)
    assert torch.equal(short[2][2], grids[2]) and same_bits(short[0][2], feat[2, :4])


# ---- 5. the acting class --------------------------------------------------------------------------------------------------------------

class RecordingOps:
    """Stands in for the op layer of a LocalGridAgents on the CPU: records what cs_policy_forward would have been given."""

    def __init__(self):
        self.calls = []

    def policy_forward(self, packed, obs, obs_stride, obs_offset, last, feat, rows_per_feat, hidden, q, actions, rows, n_agents, n_actions, *rest):
        self.calls.append(dict(obs=obs.clone(), obs_stride=obs_stride, obs_offset=obs_offset, last=last.clone(), feat=feat.clone(),
                               rows_per_feat=rows_per_feat, hidden=hidden.clone(), rows=rows, n_agents=n_agents, n_actions=n_actions))
        actions.fill_(2)


@pytest.mark.parametrize("kind", ["coverage", "belief"])
def test_local_grid_agents_input_row_layout_and_policy_reset(kind):
    """With the definition-backed filter on the CPU: one decision advances the filter once, reads every agent's OWN grid and hands
    cs_policy_forward [16 features | obs(4) | last | id] rows, one feature row per agent row; policy() resets the filter and the
    hidden state at t == 0 and tells the filter whether the targets moved."""
    args, B, n = bc_args(), 4, 3
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=2)
    filt = (cs.LocalCoverageAgents(args, 30, batch=B, device="cpu", impl="torch") if kind == "coverage"
            else cs.LocalBeliefAgents(args, 30, motion=motion, batch=B, device="cpu", impl="torch"))
    agents = lo.LocalGridAgents(args, filt, seed=3)
    assert isinstance(agents, cs.FusedAgents) and agents.net.fc1.in_features == cs.rnn_input_shape(args) + 16 == 16 + 4 + 3 + 3
    assert agents.filter is filt and tuple(agents.features.shape) == (B, n, 16) and agents.batch == B
    with pytest.raises(NotImplementedError):
        agents.forward_raw(torch.zeros(B * n, 26))
    ops = agents._ops = RecordingOps()
    moved_seen = []
    real = filt.choose_action
    filt.choose_action = (lambda state, moved=None: (moved_seen.append(moved), real(state) if kind == "coverage" else real(state, moved))[1])
    states = walk(B, n, 5, 9, tail=args.state_shape - 4 * n)
    obs = [s[:, :4 * n].reshape(B, n, 4).contiguous() for s in states]
    twin = type(filt)(args, 30, batch=B, device="cpu", impl="torch") if kind == "coverage" else type(filt)(args, 30, motion=motion, batch=B, device="cpu", impl="torch")
    policy, trace = agents.policy(trace=torch.full((5, B, n, 16), -1.0)), None
    for episode in range(2):
        filt.grids.fill_(1234)        # what a previous episode left behind
        agents.hidden.fill_(1.0)
        agents.actions.fill_(1)
        twin.reset()
        for t, s in enumerate(states):
            out = policy(obs[t], s, None, t)
            twin.choose_action(s) if kind == "coverage" else twin.choose_action(s, be.targets_moved(motion, t))
            call = ops.calls[-1]
            assert torch.equal(filt.grids, twin.grids), (episode, t)   # reset at t == 0, then advanced once per decision
            want = lo.local_grid_features_torch(s, twin.grids, n, 50, 7)
            assert same_bits(call["feat"], want) and same_bits(agents.features, want) and call["rows_per_feat"] == 1
            assert same_bits(call["obs"], obs[t]) and (call["obs_stride"], call["obs_offset"]) == (4, 0)
            assert (call["rows"], call["n_agents"], call["n_actions"]) == (B * n, n, 3)
            assert bool((call["last"] == (-1 if t == 0 else 2)).all())   # init_hidden at t == 0, then the action just chosen
            assert not call["hidden"].any() and out is agents.actions and bool((out == 2).all())
    want_moved = [be.targets_moved(motion, t) if kind == "belief" else None for t in range(5)] * 2
    assert moved_seen == want_moved and (kind == "coverage" or want_moved[:5] == [False, True, False, True, False])
    assert len(ops.calls) == 10 and agents.calls == 10


def test_distil_local_grid_call_order_labels_and_history(monkeypatch):
    from imitate_util import synthetic_batch
    args = bc_args(T=4)
    B, calls = 3, []

    class StubCollector:
        def __init__(self, env):
            self.k = 0

        def generate_episodes(self, policy=None, agents=None, evaluate=True, init=False, **kw):
            calls.append(("fly", getattr(policy, "tag", "expert")))
            batch = synthetic_batch(args, B, 20 + self.k)
            rows = episodes(B, args.n_agents, 4, 30 + self.k, tail=args.state_shape - 4 * args.n_agents)
            batch["s"] = rows * (1 - batch["padded"])
            self.k += 1
            del batch["u_expert"]
            return batch, None, None, torch.tensor([3, 4, 5])

    class StubAgents:
        def __init__(self, net):
            self.net, self.synced = net, 0

        def policy(self):
            fn = lambda obs, state, last, t: None
            fn.tag = "student"
            return fn

        def sync_weights(self):
            calls.append(("sync",))
            self.synced += 1

    monkeypatch.setattr(lo, "EpisodeCollector", StubCollector)
    learner = go.GridImitationLearner(args, device="cpu", unroll="torch")
    agents = StubAgents(learner.eval_rnn)
    filt = cs.LocalCoverageAgents(args, 30, batch=B, device="cpu", impl="torch")
    real_label, labelled = im.label_episodes, []

    def label(expert, batch, impl="auto"):
        calls.append(("label", type(expert).__name__))
        labelled.append(real_label(expert, batch, impl))
        return labelled[-1]

    monkeypatch.setattr(im, "label_episodes", label)
    # (a) the expert is of the filter's class with equal parameters: labels and features from one call, label_episodes never runs
    ring = go.FeatureRing(args, 16, device="cpu")
    expert = cs.LocalCoverageAgents(args, 30, batch=B, device="cpu", impl="torch")
    history = lo.distil_local_grid(None, expert, filt, learner, agents, ring, iterations=2, updates=2, sample=5, generator=torch.Generator().manual_seed(0))
    assert calls == [("fly", "expert"), ("sync",), ("fly", "student"), ("sync",)]
    assert [h["flown_by"] for h in history] == ["expert", "student"] and ring.current_size == 2 * B and agents.synced == 2
    assert all(set(h) == {"iteration", "flown_by", "loss", "agreement", "targets_find"} for h in history)
    stored = {k: v[:B] for k, v in ring.buffers.items()}
    feat, labels = lo.local_feature_episodes(filt, stored, labels=True)
    assert same_bits(stored["f"], feat) and torch.equal(stored["u_expert"].squeeze(3).long(), labels) and bool(feat.any())
    # (b) the same class at ANOTHER range decides differently: iteration 0 clones the actions flown, iteration 1 asks label_episodes
    del calls[:]
    ring = go.FeatureRing(args, 16, device="cpu")
    other = cs.LocalCoverageAgents(args, 0, batch=B, device="cpu", impl="torch")
    history = lo.distil_local_grid(None, other, filt, learner, agents, ring, iterations=2, updates=0, sample=1)
    assert [c[0] for c in calls] == ["fly", "sync", "fly", "label", "sync"] and calls[3] == ("label", "LocalCoverageAgents")
    assert history[0]["loss"] is None and history[1]["agreement"] is None
    assert torch.equal(ring.buffers["u_expert"][:B], ring.buffers["u"][:B])
    assert torch.equal(ring.buffers["u_expert"][B:2 * B].squeeze(3).long(), labelled[0])
    assert same_bits(ring.buffers["f"][B:2 * B], lo.local_feature_episodes(filt, {k: v[B:2 * B] for k, v in ring.buffers.items()}))
    with pytest.raises(ValueError):
        lo.distil_local_grid(None, expert, filt, learner, agents, ring, iterations=0, updates=1, sample=1)
    with pytest.raises(TypeError, match="private grids"):
        lo.distil_local_grid(None, expert, cs.CoverageAgents(args, batch=B, device="cpu", impl="torch"), learner, agents, ring, 1, 0, 1)
