"""CPU tests of the grid observations (gridobs.py, include/coopsearch.h: cs_grid_features, cs_feature_episodes; DESIGN.md section
24): the boundary declares, exports and registers both entry points and refuses bad arguments before any launch; the feature
definition equals the policies' own scores where they overlap, a plain-Python probe sum elsewhere, and is exact; the episode
definition is the labeller's loop with the probes taken after every step; the learner, the ring and the acting class do what their
docstrings say."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import gridobs as go
from cooperative_search_amd import imitate as im
from cooperative_search_amd import motion as mo
from gridobs_util import FORWARD_SEED, clear_fraction, forward_case, grids, probe_sum_python, rows, same_bits, twin_of, twin_step
from imitate_util import KEEP, bc_args, belief_params, coverage_params, mixed_lens, state_rows, synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def one_thread():
    """The definitions' tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


# ---- 1. the boundary ----------------------------------------------------------------------------------------------------------

GRID_FIELDS = ["n_agents", "side", "view_range", "lookahead", "state_width", "reserved"]


def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    assert "cs_grid_params, cs_grid_features and" in re.search(r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_grid_features\s*\(\s*const\s+cs_grid_params\s*\*", header)
    assert re.search(r"\bint\s+cs_feature_episodes\s*\(\s*const\s+cs_label_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_grid_features" in _lib.EXPORTS and "cs_feature_episodes" in _lib.EXPORTS
    L = _lib.load()
    assert L.cs_grid_features.argtypes is not None and L.cs_feature_episodes.argtypes is not None
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_grid_params \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", fields) == GRID_FIELDS
    assert [k for k, _ in _lib.CsGridParams._fields_] == GRID_FIELDS and C.sizeof(_lib.CsGridParams) == 4 * len(GRID_FIELDS)
    ops = _lib.torch_ops()
    assert str(ops.grid_features.default._schema) == (
        "coopsearch::grid_features(Tensor state, Tensor grid, Tensor(a!) feat, int n_agents, int side, int view_range, int lookahead) -> ()")
    assert str(ops.feature_episodes.default._schema) == (
        "coopsearch::feature_episodes(Tensor s, Tensor lens, Tensor(a!) feat, Tensor(b!)? labels, Tensor(c!)? grid_out, Tensor(d!)? prev_out, "
        "int expert, int n_agents, int side, int view_range, int keep, int regrow, int lookahead, int mode, int sense16, int every, "
        "int moving, int[] dx, int[] dy) -> ()")
    from cooperative_search_amd import build
    assert "gridobs.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "grid_features") and not hasattr(_lib.CtypesOps, "feature_episodes")
    for name in ("FeatureRing", "GridAgents", "GridImitationLearner", "distil_grid", "feature_episodes", "feature_episodes_hip",
                 "feature_episodes_torch", "grid_features", "grid_features_hip", "grid_features_torch"):
        assert getattr(cs, name) is getattr(go, name), name


def test_kernels_are_included_after_the_helpers_they_call_and_the_tables_match():
    csrc = os.path.join(ROOT, "cooperative-search_amd", "csrc")
    ep = open(os.path.join(csrc, "episodes.hip")).read()
    assert ep.index('#include "label.h"') < ep.index('#include "gridobs.h"')
    code = re.sub(r"//.*", "", open(os.path.join(csrc, "gridobs.h")).read())
    for helper in ("cov_quant", "cov_update", "cov_point", "cov_box", "cov_within", "bel_scatter", "bel_update"):
        assert helper + "(" in code, helper
    assert "atomic" not in code   # LDS atomics are bel_spread's only; nothing global
    rel = [int(v) for v in re.search(r"GO_REL\[8\]\s*=\s*\{([^}]*)\}", code).group(1).split(",")]
    dist = [int(v) for v in re.search(r"GO_DIST\[2\]\s*=\s*\{([^}]*)\}", code).group(1).split(",")]
    assert tuple(rel) == go.REL == (0, 1, 35, 4, 32, 9, 27, 18) and tuple(dist) == go.DIST == (1, 3)
    assert go.PROBES == 16 == len(go.REL) * len(go.DIST)


@pytest.mark.parametrize("field, value, msg", [
    ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"), ("side", 65, "side"), ("view_range", -1, "view_range"),
    ("view_range", 65, "view_range"), ("lookahead", -1, "lookahead"), ("lookahead", 51, "lookahead"), ("state_width", 11, "state_width"),
    ("reserved", 1, "reserved"), ("B", 0, "B must"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("params", None, "NULL"),
    ("align", 0, "aligned"), ("align", 1, "aligned"), ("align", 2, "aligned")])
def test_feature_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = _lib.CsGridParams(3, 50, 7, 7, 57, 0)
    B, ptrs = 4, [256, 512, 1024]   # state, grid, feat
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 2
    elif field == "B":
        B = value
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_grid_features(None if field == "params" else C.byref(p), ptrs[0], B, ptrs[1], ptrs[2], None)
    assert rc == -1   # CS_E_CONFIG
    assert msg in L.cs_episodes_last_error().decode() and "cs_grid_features" in L.cs_episodes_last_error().decode()


def good_label_params():
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), 50)
    return _lib.CsLabelParams(1, 3, 50, 7, KEEP, 8, 7, 57, m.mode, m.sense16, 1, 1, (C.c_int32 * 16)(*m.dx), (C.c_int32 * 16)(*m.dy), 0)


@pytest.mark.parametrize("field, value, msg", [
    ("expert", 2, "expert"), ("n_agents", 9, "n_agents"), ("side", 65, "side"), ("view_range", 65, "view_range"), ("keep", 65537, "keep"),
    ("regrow", 0, "regrow"), ("lookahead", 51, "lookahead"), ("state_width", 11, "state_width"), ("mode", 2, "mode"), ("sense16", 2049, "sense16"),
    ("every", 0, "every"), ("moving", 2, "moving"), ("dx", (3, 1025), "dx and dy"), ("dy", (7, -1025), "dx and dy"), ("reserved", 1, "reserved"),
    ("E", 0, "E and T"), ("T", 0, "E and T"), ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("params", None, "NULL"),
    ("align", 0, "aligned"), ("align", 1, "aligned"), ("align", 2, "aligned"), ("align", 3, "aligned"), ("align", 4, "aligned"), ("align", 5, "aligned"),
    ("coverage_prev", None, "prev_out_dev")])
def test_episode_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    L = _lib.load()
    p = good_label_params()
    E, T, ptrs = 4, 5, [256, 512, 1024, 2048, 4096, 8192]   # s, lens, feat, labels, grid_out, prev_out
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 4 if value == 3 else 2
    elif field in ("E", "T"):
        E, T = (value, T) if field == "E" else (E, value)
    elif field in ("dx", "dy"):
        getattr(p, field)[value[0]] = value[1]
    elif field == "coverage_prev":
        p.expert = 0
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_feature_episodes(None if field == "params" else C.byref(p), ptrs[0], E, T, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], None)
    assert rc == -1   # CS_E_CONFIG
    assert msg in L.cs_episodes_last_error().decode() and "cs_feature_episodes" in L.cs_episodes_last_error().decode()


def test_ops_refuse_bad_integers_shapes_and_cpu_tensors():
    ops = _lib.torch_ops()
    state, grid, feat = torch.zeros(2, 57), torch.zeros(2, 2500, dtype=torch.int32), torch.zeros(2, 3, 16)
    good = dict(n_agents=3, side=50, view_range=7, lookahead=7)

    def one(state=state, grid=grid, feat=feat, **kw):
        a = dict(good, **kw)
        ops.grid_features(state, grid, feat, *(a[k] for k in good))

    for kw, msg in [(dict(n_agents=0), "n_agents"), (dict(n_agents=9), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"),
                    (dict(view_range=-1), "view_range"), (dict(lookahead=51), "lookahead"), (dict(state=torch.zeros(2, 11)), "state must be"),
                    (dict(state=torch.zeros(57)), "state must be"), (dict(grid=grid[:, :7]), "grid must be"), (dict(grid=grid[:1]), "grid must be"),
                    (dict(feat=feat[:, :2]), "feat must be"), (dict(feat=torch.zeros(2, 3, 8)), "feat must be"), (dict(), "GPU tensor")]:
        with pytest.raises(RuntimeError, match=msg):
            one(**kw)
    assert not feat.any()
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), 50)
    s, lens, labels = torch.zeros(2, 4, 57), torch.full((2,), 4, dtype=torch.int32), torch.zeros(2, 4, 3, dtype=torch.int64)
    f4, g2, prev = torch.zeros(2, 4, 3, 16), torch.zeros(2, 2500, dtype=torch.int32), torch.zeros(2, 8, 2, dtype=torch.int32)
    good = dict(expert=1, n_agents=3, side=50, view_range=7, keep=KEEP, regrow=8, lookahead=7, mode=1, sense16=m.sense16, every=1, moving=1,
                dx=list(m.dx), dy=list(m.dy))

    def many(s=s, lens=lens, feat=f4, labels=labels, grid=g2, prev=prev, **kw):
        a = dict(good, **kw)
        ops.feature_episodes(s, lens, feat, labels, grid, prev, *(a[k] for k in good))

    for kw, msg in [(dict(expert=2), "expert"), (dict(n_agents=0), "n_agents"), (dict(side=65), "side"), (dict(view_range=65), "view_range"),
                    (dict(keep=65537), "keep"), (dict(regrow=0), "regrow"), (dict(lookahead=51), "lookahead"), (dict(mode=2), "mode"),
                    (dict(sense16=2049), "sense16"), (dict(every=0), "every"), (dict(moving=2), "moving"), (dict(dx=[0] * 15), "16 integers"),
                    (dict(dy=[1025] + [0] * 15), "-1024..1024"), (dict(s=torch.zeros(2, 57)), "s must be"), (dict(s=torch.zeros(2, 4, 11)), "s must be"),
                    (dict(lens=lens[:1]), "lens must be"), (dict(feat=f4[:, :3]), "feat must be"), (dict(feat=torch.zeros(2, 4, 3, 8)), "feat must be"),
                    (dict(labels=labels[:, :3]), "labels must be"), (dict(grid=g2[:, :7]), "grid_out must be"), (dict(prev=prev[:, :7]), "prev_out must be"),
                    (dict(expert=0), "prev_out is the belief"), (dict(), "GPU tensor"), (dict(labels=None, grid=None, prev=None), "GPU tensor")]:
        with pytest.raises(RuntimeError, match=msg):
            many(**kw)


def test_python_layer_refuses_bad_arguments():
    state, grid = rows(2, 3, 57, 0), torch.full((2, 2500), bl.FRESH, dtype=torch.int32)
    for kw in (dict(n_agents=0), dict(n_agents=9), dict(side=65), dict(view_range=65), dict(lookahead=51), dict(lookahead=-1)):
        a = dict(dict(n_agents=3, side=50, view_range=7), **kw)
        with pytest.raises(ValueError):
            go.grid_features_torch(state, grid, **a)
    for bad_state, bad_grid in ((state.double(), grid), (state[0], grid), (state[:, :11], grid), (state, grid.long()), (state, grid[:1]), (state, grid[:, :7])):
        with pytest.raises(ValueError):
            go.grid_features_torch(bad_state, bad_grid, 3, 50, 7)
    with pytest.raises(ValueError, match="impl must be"):
        go.grid_features(state, grid, 3, 50, 7, impl="fused")
    with pytest.raises(ValueError, match="no CPU fallback"):
        go.grid_features(state, grid, 3, 50, 7, impl="hip")
    assert same_bits(go.grid_features(state, grid, 3, 50, 7), go.grid_features_torch(state, grid, 3, 50, 7))   # "auto" on the CPU: the definition
    s, lens = state_rows(2, 3, 3, 57, 0), torch.tensor([3, 1], dtype=torch.int32)
    p = coverage_params(3, 50, 7)
    for bad_s, bad_lens in ((s.double(), lens), (s[0], lens), (s[:, :, :11], lens), (s, lens.long()), (s, torch.tensor([4, 0], dtype=torch.int32)),
                            (s, torch.tensor([-1, 0], dtype=torch.int32))):
        with pytest.raises(ValueError):
            go.feature_episodes_torch(bad_s, bad_lens, p)
    with pytest.raises(TypeError):
        go.feature_episodes_torch(s, lens, dict(expert=0))
    filt = cs.CoverageAgents(cs.make_env_args("flight_easy"), batch=2, device="cpu", impl="torch")
    batch = {"s": s, "padded": torch.zeros(2, 3, 1)}
    with pytest.raises(ValueError, match="impl must be"):
        go.feature_episodes(filt, batch, impl="rows")
    with pytest.raises(ValueError, match="no CPU fallback"):
        go.feature_episodes(filt, batch, impl="hip")
    with pytest.raises(TypeError):
        go.feature_episodes(cs.PlanAgents(cs.make_env_args("flight_easy"), base="coverage", batch=2, device="cpu", impl="torch"), batch)
    feat, labels = go.feature_episodes(filt, batch, labels=True)
    want = go.feature_episodes_torch(s, torch.full((2,), 3, dtype=torch.int32), im.expert_params(filt))
    assert same_bits(feat, want[0]) and torch.equal(labels, want[1]) and same_bits(go.feature_episodes(filt, batch), want[0])


# ---- 2. the feature definition ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side, vr", [(7, 2), (50, 7), (64, 9)])
def test_inner_ring_sums_are_the_scores_the_policies_choose_from(side, vr):
    B, n = 5, 3
    model = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=5.0), side)
    for kind in ("coverage", "belief"):
        grid = torch.full((B, side * side), bl.FRESH, dtype=torch.int32)
        prev = torch.zeros(B, 8, 2, dtype=torch.int32)
        for k in range(3):
            state = rows(B, n, 4 * n + 5, 10 * side + k)
            if kind == "coverage":
                _, scores = bl.coverage_actions_torch(state, grid, n, side, vr, KEEP, return_scores=True)
            else:
                _, scores = be.belief_actions_torch(state, grid, prev, n, side, vr, KEEP, model, 1 if k else 0, return_scores=True)
            feat, sums = go.grid_features_torch(state, grid, n, side, vr, return_sums=True)
            assert torch.equal(sums[:, 0, 0:3], scores[:, 0]), (kind, k)   # agent 0 scores before anybody has claimed anything
            assert sums.dtype == torch.int64 and feat.dtype == torch.float32 and tuple(feat.shape) == (B, n, 16)
        assert int(sums.min()) >= 0 and sums[:, 0, 0:3].unique().numel() > 1   # the case decides something


@pytest.mark.parametrize("n, side, vr, look", [(2, 7, 0, 7), (2, 9, 2, 2), (3, 20, 4, 4), (1, 12, 3, 0), (2, 16, 16, 16)])
def test_every_probe_sum_equals_a_plain_python_sum(n, side, vr, look):
    B = 2
    state = rows(B, n, 4 * n + 3, side + vr)
    for kind in ("belief", "wild"):
        grid = grids(kind, state, n, side, vr, look)
        _, sums = go.grid_features_torch(state, grid, n, side, vr, look, return_sums=True)
        for b in range(B):
            for i in range(n):
                for k in range(16):
                    assert int(sums[b, i, k]) == probe_sum_python(state[b], grid[b], i, k, n, side, vr, look), (kind, b, i, k)


def test_features_are_exact_clamped_bounded_and_write_nothing():
    n, side, vr = 3, 50, 7
    state = rows(4, n, 57, 3, spoil=True)
    state[0, :4] = torch.tensor([float("nan"), 1e9, float("inf"), -1.0])
    for kind in ("fresh", "coverage", "belief", "wild", "cap"):
        grid = grids(kind, state, n, side, vr, vr)
        keep_state, keep_grid = state.clone(), grid.clone()
        feat, sums = go.grid_features_torch(state, grid, n, side, vr, return_sums=True)
        assert torch.equal(grid, keep_grid) and same_bits(state, keep_state)   # read, never written
        assert same_bits(feat, (sums >> 8).to(torch.float32) * 2.0 ** -15)
        assert torch.equal((feat.double() * 2.0 ** 15).long(), sums >> 8)       # nothing was rounded on the way to float32
        clamped = grid.clamp(0, be.CAP)
        assert same_bits(feat, go.grid_features_torch(state, clamped, n, side, vr))   # a cell outside 0..CAP is read as the nearer bound
        if kind == "wild":
            assert not torch.equal(clamped, grid)
    full = torch.full((2, 64 * 64), be.CAP, dtype=torch.int32)   # the largest sums there are
    feat, sums = go.grid_features_torch(rows(2, 8, 32, 4), full, 8, 64, 64, return_sums=True)
    assert 0 < int(sums.min()) and int(sums.max()) <= 1 << 31 and bool(torch.isfinite(feat).all()) and float(feat.max()) <= 256.0
    feat, sums = go.grid_features_torch(torch.tensor([[0.0, 0.0, 1.0, 0.0]] * 2), full, 1, 64, 64, 0, return_sums=True)   # from the centre: the whole map
    assert bool((sums == 1 << 31).all()) and bool((feat == 256.0).all())
    fresh = torch.full((1, 2500), bl.FRESH, dtype=torch.int32)   # the figure the module docstring quotes
    centre = torch.tensor([[0.02, 0.02, 1.0, 0.0]])   # X = Y = 408: the centre of cell (25, 25)
    assert float(go.grid_features_torch(centre, fresh, 1, 50, 7, 0)[0, 0, 0]) == 149 / 128


def test_lookahead_zero_makes_the_sixteen_probes_equal_and_the_default_is_the_policies():
    n, side, vr = 5, 50, 7
    state = rows(3, n, 4 * n, 8)
    grid = grids("belief", state, n, side, vr, vr)
    feat = go.grid_features_torch(state, grid, n, side, vr, 0)
    assert bool((feat == feat[:, :, :1]).all()) and feat[:, :, 0].unique().numel() > 1
    assert same_bits(go.grid_features_torch(state, grid, n, side, vr), go.grid_features_torch(state, grid, n, side, vr, min(vr, side)))
    far = go.grid_features_torch(state, grid, n, side, vr, vr)
    assert not bool((far == far[:, :, :1]).all())
    small = torch.full((3, 16), bl.FRESH, dtype=torch.int32)
    assert same_bits(go.grid_features_torch(state, small, n, 4, 7), go.grid_features_torch(state, small, n, 4, 7, 4))   # min(view_range, side)


# ---- 3. the episode definition -----------------------------------------------------------------------------------------------------

def by_hand(s, lens, p):
    """The step definition and grid_features_torch, one episode and one row at a time."""
    E, T, n = s.shape[0], s.shape[1], p.n_agents
    feat = torch.zeros(E, T, n, 16)
    for e in range(E):
        grid = torch.full((1, p.side * p.side), bl.FRESH, dtype=torch.int32)
        prev = torch.zeros(1, 8, 2, dtype=torch.int32)
        for t in range(int(lens[e])):
            row = s[e, t].view(1, -1).contiguous()
            if p.expert == im.COVERAGE:
                bl.coverage_actions_torch(row, grid, n, p.side, p.view_range, p.keep, p.regrow, p.lookahead)
            else:
                be.belief_actions_torch(row, grid, prev, n, p.side, p.view_range, p.keep, p.model, p.moved(t), p.lookahead)
            feat[e, t] = go.grid_features_torch(row, grid, n, p.side, p.view_range, p.lookahead)[0]
    return feat


@pytest.mark.parametrize("kind", ["coverage", "walk", "evade"])
def test_episode_features_are_the_step_definition_plus_the_feature_definition(kind):
    E, T, n = 4, 6, 2
    p = coverage_params(n, 16, 3) if kind == "coverage" else belief_params(n, 16, 3, kind, speed=1.0, sense=5.0, every=2)
    s, lens = state_rows(E, T, n, 4 * n + 3, 6), torch.tensor([6, 0, 4, 1], dtype=torch.int32)
    want_feat, want = by_hand(s, lens, p), im.label_episodes_torch(s, lens, p)
    s_in = s.clone()
    s_in[1], s_in[2, 4:], s_in[3, 1:] = float("nan"), float("nan"), float("nan")   # rows past lens: never read
    keep_s, keep_lens = s_in.clone(), lens.clone()
    feat, labels, grid, prev = go.feature_episodes_torch(s_in, lens, p)
    assert torch.equal(labels, want[0]) and torch.equal(grid, want[1])
    assert (prev is None and want[2] is None) or torch.equal(prev, want[2])
    assert same_bits(feat, want_feat)
    assert not feat[1].any() and not feat[2, 4:].any() and not feat[3, 1:].any() and bool(feat[0].any())
    assert same_bits(feat[1], torch.zeros_like(feat[1]))   # +0.0, not -0.0 or NaN
    assert torch.equal(lens, keep_lens) and same_bits(s_in, keep_s)
    assert feat[0, 0].unique().numel() > 1 and not same_bits(feat[0, 0], feat[0, T - 1])   # the grid moves on and the features with it


# ---- 4. the learner, the ring and the acting class ----------------------------------------------------------------------------------

def featured_batch(args, E, seed):
    """imitate_util.synthetic_batch plus "f"; the label now depends on a FEATURE (which third f[..., 3] falls in), not on the
    observation: only a learner that reads "f" can lower the loss below the prior's."""
    batch = synthetic_batch(args, E, seed)
    g = torch.Generator().manual_seed(seed)
    live = (1 - batch["padded"]).unsqueeze(3)
    f = torch.rand(E, args.episode_limit, args.n_agents, 16, generator=g) * live
    batch["f"] = f.contiguous()
    batch["u_expert"] = ((f[..., 3] > 1 / 3).long() + (f[..., 3] > 2 / 3).long()).unsqueeze(3).float() * live
    return batch


def test_grid_learner_lowers_the_loss_needs_f_and_keeps_its_own_checkpoint_directory(tmp_path):
    args = bc_args(model_dir=str(tmp_path) + "/")
    learner = go.GridImitationLearner(args, device="cpu", unroll="torch")
    assert learner.eval_rnn.fc1.in_features == cs.rnn_input_shape(args) + 16 == 4 + 3 + 3 + 16
    assert isinstance(learner, im.ImitationLearner)
    twin = go.GridImitationLearner(bc_args(model_dir=str(tmp_path) + "/"), device="cpu", unroll="torch")
    for (k, a), (_, b) in zip(learner.eval_rnn.state_dict().items(), twin.eval_rnn.state_dict().items()):
        assert torch.equal(a, b), k   # the same actor for the same seed
    batch = featured_batch(args, 16, 0)
    with pytest.raises(KeyError, match="'f'"):
        learner.learn({k: v for k, v in batch.items() if k != "f"})
    with pytest.raises(KeyError, match="u_expert"):
        learner.learn({k: v for k, v in batch.items() if k != "u_expert"})
    losses = [float(learner.learn(batch)) for _ in range(30)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and losses[-1] < 0.9 * np.log(3)   # below what ignoring "f" can reach
    assert learner.last_stats.shape == (3,) and abs(float(learner.last_stats[0]) - losses[-1]) < 1e-6
    assert np.isfinite(float(learner.learn(batch, max_episode_len=3)))
    # the features ARE read: the same batch with other features gives another loss
    other = dict(batch, f=batch["f"].flip(3).contiguous())
    probe = go.GridImitationLearner(bc_args(model_dir=str(tmp_path) + "/"), device="cpu", unroll="torch")
    probe2 = go.GridImitationLearner(bc_args(model_dir=str(tmp_path) + "/"), device="cpu", unroll="torch")
    assert float(probe.learn(batch)) != float(probe2.learn(other))
    path = learner.save_model(3)
    assert "_bc_grid_" in path and os.path.exists(path) and learner.model_dir == os.path.dirname(path)
    fresh = go.GridImitationLearner(bc_args(seed=99, model_dir=str(tmp_path) + "/"), device="cpu", unroll="torch")
    fresh.load_model(path)
    for k, v in learner.eval_rnn.state_dict().items():
        assert torch.equal(fresh.eval_rnn.state_dict()[k], v), k
    plain = im.ImitationLearner(bc_args(model_dir=str(tmp_path) + "/"), device="cpu", unroll="torch")
    with pytest.raises(RuntimeError, match="size mismatch"):   # 16 columns wider than the plain actor: not a file Runner can load
        plain.load_model(path)
    with pytest.raises(ValueError, match="flight_easy only"):
        go.GridImitationLearner(bc_args(env="flight", conv=True), device="cpu", unroll="torch")


def test_grid_agents_refuse_a_conv_variant_a_foreign_filter_and_a_narrow_net():
    args = bc_args()
    filt = cs.CoverageAgents(args, batch=4, device="cpu", impl="torch")
    conv = bc_args(env="flight", conv=True)
    with pytest.raises(ValueError, match="32 input columns"):
        go.GridAgents(conv, filt)
    with pytest.raises(TypeError, match="filter must be"):
        go.GridAgents(args, cs.PlanAgents(args, base="coverage", batch=4, device="cpu", impl="torch"))
    with pytest.raises(ValueError, match="the filter serves"):
        go.GridAgents(args, filt, batch=5)
    with pytest.raises(ValueError, match="fc1 must take"):
        go.GridAgents(args, filt, net=cs.AgentRNN(cs.rnn_input_shape(args), args))


def test_feature_ring_stores_and_samples_f_beside_its_episode():
    args = bc_args(T=4)
    ring, labelled = go.FeatureRing(args, 5, device="cpu"), im.LabelledRing(args, 5, device="cpu")
    assert ring.keys == im.LabelledRing.keys + ("f",) and tuple(ring.buffers) == ring.keys and isinstance(ring, im.LabelledRing)
    assert tuple(ring.buffers["f"].shape) == (5, 4, args.n_agents, 16)
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for k, E in enumerate((2, 2, 3, 1)):   # wraps
        batch = featured_batch(args, E, 10 + k)
        ring.store_episode(batch)
        labelled.store_episode(batch)
        assert (ring.current_idx, ring.current_size) == (labelled.current_idx, labelled.current_size)
        a, b = ring.sample(4, ga), labelled.sample(4, gb)
        for key in labelled.keys:
            assert torch.equal(a[key], b[key]), key
        assert a["f"].shape == (4, 4, args.n_agents, 16)
    a = ring.sample(8, ga)   # the features travel with their episode: in every sampled slot the label is the label of that slot's f
    want = ((a["f"][..., 3] > 1 / 3).long() + (a["f"][..., 3] > 2 / 3).long()).unsqueeze(3).float() * (1 - a["padded"]).unsqueeze(3)
    assert torch.equal(a["u_expert"], want)
    with pytest.raises(KeyError):
        ring.store_episode({k: v for k, v in featured_batch(args, 1, 0).items() if k != "f"})


def test_distil_grid_call_order_labels_and_history(monkeypatch):
    args = bc_args(T=4)
    B, calls = 3, []

    class StubCollector:
        def __init__(self, env):
            self.k = 0

        def generate_episodes(self, policy=None, agents=None, evaluate=True, init=False, **kw):
            calls.append(("fly", getattr(policy, "tag", "expert")))
            batch = synthetic_batch(args, B, 20 + self.k)
            batch["s"] = state_rows(B, 4, args.n_agents, args.state_shape, 30 + self.k) * (1 - batch["padded"])
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

    monkeypatch.setattr(go, "EpisodeCollector", StubCollector)
    learner = go.GridImitationLearner(args, device="cpu", unroll="torch")
    agents = StubAgents(learner.eval_rnn)
    filt = cs.CoverageAgents(args, batch=B, device="cpu", impl="torch")
    real_label, labelled = im.label_episodes, []

    def label(expert, batch, impl="auto"):
        calls.append(("label", type(expert).__name__))
        labelled.append(real_label(expert, batch, impl))
        return labelled[-1]

    monkeypatch.setattr(im, "label_episodes", label)
    # (a) the expert is the filter's own class: labels and features from one call, label_episodes never runs
    ring = go.FeatureRing(args, 16, device="cpu")
    expert = cs.CoverageAgents(args, batch=B, device="cpu", impl="torch")
    history = go.distil_grid(None, expert, filt, learner, agents, ring, iterations=2, updates=2, sample=5, generator=torch.Generator().manual_seed(0))
    assert calls == [("fly", "expert"), ("sync",), ("fly", "student"), ("sync",)]
    assert [h["flown_by"] for h in history] == ["expert", "student"] and ring.current_size == 2 * B and agents.synced == 2
    assert all(set(h) == {"iteration", "flown_by", "loss", "agreement", "targets_find"} for h in history)
    assert all(np.isfinite(h["loss"]) and 0 <= h["agreement"] <= 1 and h["targets_find"] == 4.0 for h in history)
    stored = {k: v[:B] for k, v in ring.buffers.items()}
    feat, labels = go.feature_episodes(filt, stored, labels=True)
    assert same_bits(stored["f"], feat) and torch.equal(stored["u_expert"].squeeze(3).long(), labels) and bool(feat.any())
    # (b) a planner over a separate filter: iteration 0 clones the actions flown, iteration 1 asks label_episodes
    del calls[:]
    ring = go.FeatureRing(args, 16, device="cpu")
    planner = cs.PlanAgents(args, base="coverage", depth=2, stride=2, batch=B, device="cpu", impl="torch")
    history = go.distil_grid(None, planner, filt, learner, agents, ring, iterations=2, updates=0, sample=1)
    assert [c[0] for c in calls] == ["fly", "sync", "fly", "label", "sync"] and calls[3] == ("label", "PlanAgents")
    assert history[0]["loss"] is None and history[1]["agreement"] is None
    assert torch.equal(ring.buffers["u_expert"][:B], ring.buffers["u"][:B])
    assert torch.equal(ring.buffers["u_expert"][B:2 * B].squeeze(3).long(), labelled[0])
    assert same_bits(ring.buffers["f"][B:2 * B], go.feature_episodes(filt, {k: v[B:2 * B] for k, v in ring.buffers.items()}))
    with pytest.raises(ValueError):
        go.distil_grid(None, expert, filt, learner, agents, ring, iterations=0, updates=1, sample=1)


# ---- 5. the seed of the GPU forward test ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, B", [(3, 1), (3, 37), (8, 129)])
def test_the_float64_twin_alone_leaves_nine_rows_in_ten_a_clear_top_two_gap(n, B):
    """tests/test_gpu_gridobs.py compares actions only where the float64 top-2 gap exceeds 1e-3 and wants 90 % of the rows that
    clear; FORWARD_SEED is chosen so that the float64 module itself, fed its own greedy actions, gives that on every step."""
    args = bc_args(n_agents=n)
    net, feats, obs = forward_case(args, n, B, seed=FORWARD_SEED)
    m = twin_of(net, torch.float64)
    h, last = torch.zeros(B * n, 64, dtype=torch.float64), torch.full((B, n), -1, dtype=torch.int64)
    for t in range(feats.shape[0]):
        q, h = twin_step(m, feats[t], obs[t], last, h, n, 3)
        share, _ = clear_fraction(q)
        assert share >= 0.9, (t, share)
        last = q.argmax(1).view(B, n)
