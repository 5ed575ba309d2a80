"""CPU tests of the imitation module (imitate.py, include/coopsearch.h: cs_label_episodes, cs_bc_loss):
the boundary declares, exports and registers both entry points and refuses bad arguments before any launch; the labeller's
definition equals the experts' step definitions called row by row; the generic path equals it and shadows a planner; the
loss's definition equals a NumPy float64 statement; the learner, the ring and the distillation loop do what their docstrings say."""
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
from cooperative_search_amd import imitate as im
from cooperative_search_amd import motion as mo
from imitate_util import (KEEP, bc_args, bc_f64, bc_inputs, bc_twin, belief_params, coverage_params, mixed_lens, rel_err, state_rows,
                          synthetic_batch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, VR = 50, 7


@pytest.fixture(autouse=True)
def one_thread():
    """The definitions' tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


# ---- 1. the boundary ----------------------------------------------------------------------------------------------------------

LABEL_FIELDS = ["expert", "n_agents", "side", "view_range", "keep", "regrow", "lookahead", "state_width", "mode", "sense16", "every", "moving",
                "dx[16]", "dy[16]", "reserved"]


def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    assert "cs_label_params, cs_label_episodes and cs_bc_loss" in re.search(r"#define CS_ABI_VERSION 7.*?\*/", header, flags=re.S).group(0)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_label_episodes\s*\(\s*const\s+cs_label_params\s*\*", header)
    assert re.search(r"\bint\s+cs_bc_loss\s*\(\s*const\s+float\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_label_episodes" in _lib.EXPORTS and "cs_bc_loss" in _lib.EXPORTS
    L = _lib.load()
    assert L.cs_label_episodes.argtypes is not None and L.cs_bc_loss.argtypes is not None
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_label_params \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+(?:\[16\])?);", fields) == LABEL_FIELDS
    assert [k + ("[16]" if t is not C.c_int32 else "") for k, t in _lib.CsLabelParams._fields_] == LABEL_FIELDS
    assert C.sizeof(_lib.CsLabelParams) == 4 * (12 + 32 + 1)
    ops = _lib.torch_ops()
    assert str(ops.label_episodes.default._schema) == (
        "coopsearch::label_episodes(Tensor s, Tensor lens, Tensor(a!) labels, Tensor(b!)? grid_out, Tensor(c!)? prev_out, int expert, "
        "int n_agents, int side, int view_range, int keep, int regrow, int lookahead, int mode, int sense16, int every, int moving, "
        "int[] dx, int[] dy) -> ()")
    assert str(ops.bc_loss.default._schema) == (
        "coopsearch::bc_loss(Tensor logits, Tensor avail, Tensor labels, Tensor mask, int rows, int n_agents, int n_actions, "
        "Tensor inv_count, Tensor(a!) dlogits, Tensor(b!) stats, Tensor(c!) scratch) -> ()")
    from cooperative_search_amd import build
    assert "label.h" in build.SOURCES and "bc_loss.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "label_episodes") and not hasattr(_lib.CtypesOps, "bc_loss")
    for name in ("BCLoss", "ExpertParams", "ImitationLearner", "LabelledRing", "bc_loss_torch", "distil", "expert_params", "get_bc_args",
                 "label_episodes", "label_episodes_hip", "label_episodes_torch"):
        assert getattr(cs, name) is getattr(im, name), name
    assert im.BC_BLOCK == int(re.search(r"#define\s+CS_PPO_BLOCK\s+(\d+)", header).group(1))


def test_kernels_are_included_where_their_helpers_are_defined():
    csrc = os.path.join(ROOT, "cooperative-search_amd", "csrc")
    ep, pol = open(os.path.join(csrc, "episodes.hip")).read(), open(os.path.join(csrc, "policy.hip")).read()
    assert ep.index('#include "belief.h"') < ep.index('#include "label.h"')
    assert pol.index('#include "ppo.h"') < pol.index('#include "bc_loss.h"')
    label = open(os.path.join(csrc, "label.h")).read()
    code = re.sub(r"//.*", "", label)
    for helper in ("cov_quant", "cov_update", "cov_point", "cov_box", "cov_within", "bel_scatter", "bel_update"):
        assert helper + "(" in code, helper
    assert "atomicAdd" not in code   # LDS atomics are bel_spread's only; nothing global


def good_label_params():
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), SIDE)
    return _lib.CsLabelParams(1, 3, SIDE, VR, KEEP, 8, 7, 57, m.mode, m.sense16, 1, 1, (C.c_int32 * 16)(*m.dx), (C.c_int32 * 16)(*m.dy), 0)


@pytest.mark.parametrize("field, value, msg", [
    ("expert", 2, "expert"), ("expert", -1, "expert"), ("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"),
    ("side", 65, "side"), ("view_range", -1, "view_range"), ("view_range", 65, "view_range"), ("keep", -1, "keep"), ("keep", 65537, "keep"),
    ("regrow", 0, "regrow"), ("regrow", 17, "regrow"), ("lookahead", -1, "lookahead"), ("lookahead", 51, "lookahead"),
    ("state_width", 11, "state_width"), ("mode", 2, "mode"), ("mode", -1, "mode"), ("sense16", -1, "sense16"), ("sense16", 2049, "sense16"),
    ("every", 0, "every"), ("moving", 2, "moving"), ("moving", -1, "moving"), ("dx", (3, 1025), "dx and dy"), ("dx", (0, -1025), "dx and dy"),
    ("dy", (15, 1025), "dx and dy"), ("dy", (7, -1025), "dx and dy"), ("reserved", 1, "reserved"), ("E", 0, "E and T"), ("T", 0, "E and T"),
    ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("params", None, "NULL"), ("align", 0, "aligned"), ("align", 1, "aligned"),
    ("align", 2, "aligned"), ("align", 3, "aligned"), ("align", 4, "aligned"), ("coverage_prev", None, "prev_out_dev")])
def test_label_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = good_label_params()
    E, T, ptrs = 4, 5, [256, 512, 1024, 2048, 4096]   # s, lens, labels, grid_out, prev_out
    if field == "ptr":
        ptrs[value] = None
    elif field == "align":
        ptrs[value] += 4 if value == 2 else 2
    elif field in ("E", "T"):
        E, T = (value, T) if field == "E" else (E, value)
    elif field in ("dx", "dy"):
        getattr(p, field)[value[0]] = value[1]
    elif field == "coverage_prev":
        p.expert = 0
    elif field != "params":
        setattr(p, field, value)
    rc = L.cs_label_episodes(None if field == "params" else C.byref(p), ptrs[0], E, T, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None)
    assert rc == -1   # CS_E_CONFIG
    assert msg in L.cs_episodes_last_error().decode() and "cs_label_episodes" in L.cs_episodes_last_error().decode()


@pytest.mark.parametrize("field, value", [("ptr", 0), ("ptr", 1), ("ptr", 2), ("ptr", 3), ("ptr", 4), ("ptr", 5), ("ptr", 6), ("ptr", 7),
                                          ("rows", 0), ("rows", 7), ("n_agents", 0), ("n_actions", 1), ("n_actions", 9), ("scratch", 2)])
def test_loss_entry_point_refuses_bad_arguments_before_any_launch(field, value):
    L = _lib.load()
    ptrs = [256 * (k + 1) for k in range(8)]   # logits, avail, labels, mask, inv_count, dlogits, stats, scratch
    rows, n, A, floats = 6, 3, 3, 3
    if field == "ptr":
        ptrs[value] = None
    elif field == "rows":
        rows = value
    elif field == "n_agents":
        n = value
    elif field == "n_actions":
        A = value
    else:
        floats = value
    rc = L.cs_bc_loss(ptrs[0], ptrs[1], ptrs[2], ptrs[3], rows, n, A, ptrs[4], ptrs[5], ptrs[6], ptrs[7], floats, None)
    assert rc == -2   # CS_E_ARG, as cs_ppo_loss
    assert "cs_bc_loss" in L.cs_learn_last_error().decode()
    assert ("scratch holds" if field == "scratch" else "bad argument") in L.cs_learn_last_error().decode()


def test_ops_refuse_bad_integers_and_cpu_tensors():
    ops = _lib.torch_ops()
    m = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), SIDE)
    s, lens, labels = torch.zeros(2, 4, 57), torch.full((2,), 4, dtype=torch.int32), torch.zeros(2, 4, 3, dtype=torch.int64)
    grid, prev = torch.zeros(2, SIDE * SIDE, dtype=torch.int32), torch.zeros(2, 8, 2, dtype=torch.int32)
    good = dict(expert=1, n_agents=3, side=SIDE, view_range=VR, keep=KEEP, regrow=8, lookahead=7, mode=1, sense16=m.sense16, every=1, moving=1,
                dx=list(m.dx), dy=list(m.dy))

    def call(s=s, lens=lens, labels=labels, grid=grid, prev=prev, **kw):
        a = dict(good, **kw)
        ops.label_episodes(s, lens, labels, grid, prev, *(a[k] for k in good))

    for kw, msg in [(dict(expert=2), "expert"), (dict(n_agents=0), "n_agents"), (dict(n_agents=9), "n_agents"), (dict(side=65), "side"),
                    (dict(view_range=65), "view_range"), (dict(keep=65537), "keep"), (dict(regrow=0), "regrow"), (dict(lookahead=51), "lookahead"),
                    (dict(mode=2), "mode"), (dict(sense16=2049), "sense16"), (dict(every=0), "every"), (dict(moving=2), "moving"),
                    (dict(dx=[0] * 15), "16 integers"), (dict(dy=[1025] + [0] * 15), "-1024..1024"), (dict(s=torch.zeros(2, 57)), "s must be"),
                    (dict(s=torch.zeros(2, 4, 11)), "s must be"), (dict(lens=lens[:1]), "lens must be"), (dict(labels=labels[:, :3]), "labels must be"),
                    (dict(grid=grid[:, :7]), "grid_out must be"), (dict(prev=prev[:, :7]), "prev_out must be"),
                    (dict(expert=0), "prev_out is the belief"), (dict(), "GPU tensor")]:
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    z, av, u, mk = torch.zeros(6, 3), torch.ones(6, 3), torch.zeros(6, dtype=torch.int64), torch.ones(2)
    inv, dz, st, sc = torch.ones(1), torch.zeros(6, 3), torch.zeros(3), torch.zeros(3)
    for args, msg in [((z, av, u, mk, 0, 3, 3, inv, dz, st, sc), "multiple of n_agents"), ((z, av, u, mk, 7, 3, 3, inv, dz, st, sc), "multiple of n_agents"),
                      ((z, av, u, mk, 6, 3, 9, inv, dz, st, sc), "2 to 8"), ((z, av, u, mk, 6, 3, 3, inv, dz, st, sc), "GPU tensor")]:
        with pytest.raises(RuntimeError, match=msg):
            ops.bc_loss(*args)


def test_python_definitions_refuse_bad_arguments():
    for kw in (dict(expert=2), dict(n_agents=0), dict(side=65), dict(view_range=65), dict(keep=-1), dict(regrow=17), dict(lookahead=51),
               dict(every=0), dict(moving=2)):
        with pytest.raises(ValueError):
            im.ExpertParams(**dict(dict(expert=0, n_agents=3, side=SIDE, view_range=VR, keep=KEEP), **kw))
    with pytest.raises(TypeError):
        im.ExpertParams(1, 3, SIDE, VR, KEEP, model="walk")
    p = coverage_params(3, SIDE, VR)
    s, lens = state_rows(2, 3, 3, 57, 0), torch.tensor([3, 1], dtype=torch.int32)
    for bad_s, bad_lens in ((s.double(), lens), (s[0], lens), (s[:, :, :11], lens), (s, lens.long()), (s, lens[:1]), (s, torch.tensor([4, 0], dtype=torch.int32)),
                            (s, torch.tensor([-1, 0], dtype=torch.int32))):
        with pytest.raises(ValueError):
            im.label_episodes_torch(bad_s, bad_lens, p)
    with pytest.raises(TypeError):
        im.label_episodes_torch(s, lens, dict(expert=0))
    with pytest.raises(TypeError):
        im.expert_params(object())
    expert = cs.CoverageAgents(cs.make_env_args("flight_easy"), batch=2, device="cpu", impl="torch")
    batch = {"s": s, "padded": torch.zeros(2, 3, 1)}
    with pytest.raises(ValueError, match="impl must be"):
        im.label_episodes(expert, batch, impl="fused")
    with pytest.raises(ValueError, match="no CPU fallback"):
        im.label_episodes(expert, batch, impl="hip")
    with pytest.raises(TypeError, match="policy"):
        im.label_episodes(object(), batch)
    x = bc_inputs(3, 5, 3, 3, False)
    for kw in (dict(logits=x["logits"][..., :1]), dict(avail=x["avail"][:, :4]), dict(labels=x["labels"].float()), dict(mask=x["mask"][:2])):
        a = dict(x, **kw)
        with pytest.raises(ValueError):
            im.bc_loss_torch(a["logits"], a["avail"], a["labels"], a["mask"])
    with pytest.raises(ValueError, match="unroll"):
        im.ImitationLearner(bc_args(), device="cpu", unroll="hip")
    with pytest.raises(ValueError, match="no CPU fallback"):
        im.ImitationLearner(bc_args(), device="cpu", unroll="fused")


# ---- 2. the labeller's definition -----------------------------------------------------------------------------------------------

def by_rows(s, lens, p, moved_of):
    """The experts' step definitions called row by row, ONE EPISODE AT A TIME (the definition under test walks all episodes
    together and masks): -> (labels, grid, prev)."""
    E, T, n = s.shape[0], s.shape[1], p.n_agents
    labels = torch.zeros(E, T, n, dtype=torch.int64)
    grids, prevs = [], []
    for e in range(E):
        grid = torch.full((1, p.side * p.side), bl.FRESH, dtype=torch.int32)
        prev = torch.zeros(1, 8, 2, dtype=torch.int32)
        for t in range(int(lens[e])):
            row = s[e, t].view(1, -1).contiguous()
            if p.expert == im.COVERAGE:
                labels[e, t] = bl.coverage_actions_torch(row, grid, n, p.side, p.view_range, p.keep, p.regrow, p.lookahead)[0]
            else:
                labels[e, t] = be.belief_actions_torch(row, grid, prev, n, p.side, p.view_range, p.keep, p.model, moved_of(t), p.lookahead)[0]
        grids.append(grid)
        prevs.append(prev)
    return labels, torch.cat(grids), torch.cat(prevs)


@pytest.mark.parametrize("regrow", [8, 16])
def test_coverage_labels_are_the_step_definition_row_by_row(regrow):
    E, T, n = 4, 5, 3
    p = coverage_params(n, 20, 4, regrow)
    s, lens = state_rows(E, T, n, 4 * n + 5, 1), torch.tensor([5, 0, 3, 5], dtype=torch.int32)
    want = by_rows(s, lens, p, None)
    s_in = s.clone()
    s_in[1], s_in[2, 3:] = float("nan"), float("nan")   # rows past lens: never read
    keep_s, keep_lens = s_in.clone(), lens.clone()
    labels, grid, prev = im.label_episodes_torch(s_in, lens, p)
    assert prev is None
    assert torch.equal(labels, want[0]) and torch.equal(grid, want[1])
    assert not labels[1].any() and not labels[2, 3:].any() and bool((grid[1] == bl.FRESH).all())
    assert torch.equal(lens, keep_lens) and torch.equal(torch.nan_to_num(s_in, nan=7.0), torch.nan_to_num(keep_s, nan=7.0))
    assert labels.unique().numel() > 1   # the case decides something


@pytest.mark.parametrize("mode, every", [("walk", 1), ("walk", 3), ("evade", 1), ("evade", 3)])
def test_belief_labels_are_the_step_definition_row_by_row_with_the_moved_schedule_written_out(mode, every):
    E, T, n = 3, 8, 2
    p = belief_params(n, 16, 3, mode, speed=1.0, sense=5.0, every=every)
    schedule = {1: [0, 1, 1, 1, 1, 1, 1, 1], 3: [0, 1, 0, 0, 1, 0, 0, 1]}[every]   # moved before row t: t > 0 and (t - 1) % every == 0
    assert [p.moved(t) for t in range(T)] == schedule
    s, lens = state_rows(E, T, n, 4 * n + 3, 2), torch.tensor([8, 0, 5], dtype=torch.int32)
    want = by_rows(s, lens, p, lambda t: schedule[t])
    s_in = s.clone()
    s_in[1], s_in[2, 5:] = float("nan"), float("nan")
    labels, grid, prev = im.label_episodes_torch(s_in, lens, p)
    assert torch.equal(labels, want[0]) and torch.equal(grid, want[1]) and torch.equal(prev, want[2])
    assert not prev[1].any() and bool((grid[1] == bl.FRESH).all()) and not prev[:, n:].any()
    still = dataclass_replace(p, moving=0)
    assert [still.moved(t) for t in range(T)] == [0] * T
    assert not torch.equal(im.label_episodes_torch(s_in, lens, still)[1], grid)   # the schedule matters to the grid


def dataclass_replace(p, **kw):
    import dataclasses
    return dataclasses.replace(p, **kw)


def test_lens_all_zero_and_all_full():
    p = coverage_params(2, 9, 2)
    s = state_rows(3, 4, 2, 8, 3)
    labels, grid, _ = im.label_episodes_torch(s, torch.zeros(3, dtype=torch.int32), p)
    assert not labels.any() and bool((grid == bl.FRESH).all())
    full = torch.full((3,), 4, dtype=torch.int32)
    want = by_rows(s, full, p, None)
    labels, grid, _ = im.label_episodes_torch(s, full, p)
    assert torch.equal(labels, want[0]) and torch.equal(grid, want[1])


# ---- 3. the generic path ----------------------------------------------------------------------------------------------------------

def episode_dict(s, lens):
    T = s.shape[1]
    return {"s": s, "padded": (torch.arange(T).view(1, T) >= lens.view(-1, 1)).float().unsqueeze(2)}


@pytest.mark.parametrize("kind", ["coverage", "walk", "evade"])
def test_generic_path_equals_the_kernels_definition(kind):
    E, T, n = 5, 6, 3
    args = cs.make_env_args("flight_easy", n_agents=n, map_size=20, view_range=4)
    if kind == "coverage":
        expert = cs.CoverageAgents(args, batch=E, device="cpu", impl="torch")
    else:
        expert = cs.BeliefAgents(args, motion=mo.TargetMotion(mode=kind, speed=1.0, sense=6.0, every=2), batch=E, device="cpu", impl="torch")
    s, lens = state_rows(E, T, n, 4 * n + 6, 4), mixed_lens(E, T, 4)
    assert lens.min() == 0 and lens.max() == T
    batch = episode_dict(s, lens)
    assert torch.equal(im.episode_lens(batch), lens)
    want = im.label_episodes_torch(s, lens, im.expert_params(expert))
    got = im.label_episodes(expert, batch, return_state=True)      # a CPU batch: "auto" is the generic path
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if kind != "coverage":
        assert torch.equal(got[2], want[2])
        assert not expert.prev.any()
    assert bool((expert.grid == bl.FRESH).all())                   # left as a fresh episode would find it
    assert torch.equal(im.label_episodes(expert, batch, impl="rows"), want[0])


def test_generic_path_shadows_a_planner_step_by_step():
    E, T, n = 3, 5, 2
    args = cs.make_env_args("flight_easy", n_agents=n, map_size=20, view_range=4)
    s = state_rows(E, T, n, 4 * n + 6, 5)
    lens = torch.full((E,), T, dtype=torch.int32)
    shadow = cs.PlanAgents(args, base="coverage", depth=2, stride=2, batch=E, device="cpu", impl="torch")
    policy, want = shadow.policy(), []
    for t in range(T):
        want.append(policy(None, s[:, t].contiguous(), None, t).clone())
    labels = im.label_episodes(cs.PlanAgents(args, base="coverage", depth=2, stride=2, batch=E, device="cpu", impl="torch"), episode_dict(s, lens))
    assert torch.equal(labels, torch.stack(want, 1))
    short = torch.tensor([T, 2, 0], dtype=torch.int32)
    labels = im.label_episodes(shadow, episode_dict(s, short))
    assert torch.equal(labels[0], torch.stack(want, 1)[0]) and torch.equal(labels[1, :2], torch.stack(want, 1)[1, :2])
    assert not labels[1, 2:].any() and not labels[2].any()


# ---- 4. the loss's definition -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E, T, n, A, unavailable", [(3, 5, 3, 3, False), (3, 5, 3, 3, True), (5, 13, 3, 2, True), (5, 13, 3, 8, True), (4, 6, 5, 4, False)])
def test_bc_loss_torch_matches_the_float64_statement(E, T, n, A, unavailable):
    x = bc_inputs(E, T, n, A, unavailable)
    if E > 2:
        assert not x["mask"][1].any()   # a fully padded episode
    if unavailable:
        live = x["mask"].bool().unsqueeze(2).expand(E, T, n)
        gone = torch.gather(x["avail"], 3, x["labels"].unsqueeze(3)).squeeze(3) == 0
        assert bool((gone & live).any()) and bool(((x["avail"].sum(-1) < A) & ~gone & live).any())
    loss, stats, dlogits = bc_f64(x["logits"].numpy(), x["avail"].numpy(), x["labels"].numpy(), x["mask"].numpy())
    got_stats, got_grad = bc_twin(x, torch.float64)
    assert np.allclose(got_stats.numpy(), stats, rtol=1e-12, atol=1e-14)
    assert np.allclose(got_grad.numpy(), dlogits, rtol=1e-10, atol=1e-14)
    assert not got_grad[~x["mask"].bool()].any()   # padded rows: zeros
    assert 0 < stats[1] < 1 and stats[2] > 0
    s32, g32 = bc_twin(x, torch.float32)
    assert rel_err(g32, torch.from_numpy(dlogits)) < 1e-5 and abs(float(s32[1]) - stats[1]) < 1e-6


def test_bc_loss_argmax_ties_take_the_lowest_index_and_unavailable_labels_miss():
    logits = torch.tensor([[[[1.0, 1.0, 0.0]], [[0.0, 2.0, 2.0]], [[5.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]]]], dtype=torch.float64)   # [1, 4, 1, 3]
    avail = torch.ones_like(logits)
    avail[0, 2, 0, 0] = 0.0   # row 2: action 0 unavailable; the tie between 1 and 2 goes to 1
    mask = torch.ones(1, 4, dtype=torch.float64)
    for labels, hits in (([0, 1, 1, 0], 4), ([1, 2, 2, 1], 0), ([0, 1, 0, 0], 3)):
        u = torch.tensor(labels).view(1, 4, 1)
        z = logits.clone().requires_grad_(True)
        loss, stats = im.bc_loss_torch(z, avail, u, mask)
        assert abs(float(stats[1]) * 4 - hits) < 1e-12, labels
        loss.backward()
        want = bc_f64(logits.numpy(), avail.numpy(), u.numpy(), mask.numpy())
        assert np.allclose(stats.numpy(), want[1]) and np.allclose(z.grad.numpy(), want[2])
        if labels[2] == 0:   # a live row with an unavailable label: no loss, no gradient, a miss
            assert not z.grad[0, 2].any()
    out_of_range = torch.tensor([0, 1, 1, 7]).view(1, 4, 1)
    _, stats = im.bc_loss_torch(logits, avail, out_of_range, mask)
    assert abs(float(stats[1]) * 4 - 3) < 1e-12


# ---- 5. the learner -----------------------------------------------------------------------------------------------------------------

def test_learner_lowers_the_loss_and_its_checkpoint_is_the_reinforce_actor(tmp_path):
    args = bc_args(model_dir=str(tmp_path) + "/")
    learner = im.ImitationLearner(args, device="cpu", unroll="torch")
    twin_args = bc_args(model_dir=str(tmp_path) + "/")
    cs.get_reinforce_args(twin_args, seed=args.seed)
    reinforce = cs.ReinforceLearner(twin_args, device="cpu", unroll="torch")
    for (k, a), (_, b) in zip(learner.eval_rnn.state_dict().items(), reinforce.eval_rnn.state_dict().items()):
        assert torch.equal(a, b), k   # the same actor for the same seed
    batch = synthetic_batch(args, 16, 0)
    with pytest.raises(KeyError):
        learner.learn({k: v for k, v in batch.items() if k != "u_expert"})
    losses = [float(learner.learn(batch)) for _ in range(10)]
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    assert learner.last_stats.shape == (3,) and abs(float(learner.last_stats[0]) - losses[-1]) < 1e-6
    assert 0.0 <= float(learner.last_stats[1]) <= 1.0
    short = float(learner.learn(batch, max_episode_len=3))
    assert np.isfinite(short)
    path = learner.save_model(3)
    assert path == os.path.join(cs.learner.model_dir(types.SimpleNamespace(**dict(vars(args), alg="bc")), "bc"), "3_rnn_net_params.pkl")
    assert os.path.exists(path) and learner.model_dir == os.path.dirname(path)
    fresh = im.ImitationLearner(bc_args(seed=99, model_dir=str(tmp_path) + "/"), device="cpu", unroll="torch")
    fresh.load_model(path)
    reinforce.load_model(path)
    for k, v in learner.eval_rnn.state_dict().items():
        assert torch.equal(fresh.eval_rnn.state_dict()[k], v) and torch.equal(reinforce.eval_rnn.state_dict()[k], v), k
    as_reinforce = learner.save_model(5, alg="reinforce")
    assert as_reinforce == os.path.join(reinforce.model_dir, "5_rnn_net_params.pkl")
    args.alg = "reinforce"   # the acting rule FusedAgents reads: the directories keep their names
    assert im.ImitationLearner(args, device="cpu", unroll="torch").save_model(6) == os.path.join(os.path.dirname(path), "6_rnn_net_params.pkl")


# ---- 6. the ring ----------------------------------------------------------------------------------------------------------------------

def test_labelled_ring_stays_aligned_with_a_device_replay_buffer():
    args = bc_args(T=4)
    ring, dense = im.LabelledRing(args, 5, device="cpu"), cs.DeviceReplayBuffer(args, 5, device="cpu")
    assert ring.keys == cs.replay.KEYS + ("u_expert",) and tuple(ring.buffers) == ring.keys
    assert isinstance(ring, cs.replay._EpisodeRing)
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for k, E in enumerate((2, 2, 3, 1)):   # wraps
        batch = synthetic_batch(args, E, 10 + k)
        ring.store_episode(batch)
        dense.store_episode(batch)
        assert (ring.current_idx, ring.current_size) == (dense.current_idx, dense.current_size)
        n = ring.current_size
        for key in cs.replay.KEYS:
            assert torch.equal(ring.buffers[key][:n], dense.buffers[key][:n]), key
        a, b = ring.sample(4, ga), dense.sample(4, gb)
        for key in cs.replay.KEYS:
            assert torch.equal(a[key], b[key]), key
        assert a["u_expert"].shape == (4, 4, args.n_agents, 1)
    # the label travels with its episode: in every sampled slot u_expert is the label of that slot's observations
    a = ring.sample(8, ga)
    want = ((a["o"][..., 0] > -1 / 3).long() + (a["o"][..., 0] > 1 / 3).long()).unsqueeze(3).float() * (1 - a["padded"]).unsqueeze(3)
    assert torch.equal(a["u_expert"], want)
    with pytest.raises(ValueError):
        ring.store_episode(synthetic_batch(args, 6, 0))
    with pytest.raises(KeyError):
        ring.store_episode({k: v for k, v in synthetic_batch(args, 1, 0).items() if k != "u_expert"})


# ---- 7. the loop ------------------------------------------------------------------------------------------------------------------------

def test_distil_call_order_and_history(monkeypatch):
    args = bc_args(T=4)
    B, calls = 3, []

    class StubCollector:
        def __init__(self, env):
            self.k = 0

        def generate_episodes(self, policy=None, agents=None, evaluate=True, init=False, **kw):
            calls.append(("fly", "policy" if policy is not None else "agents", evaluate))
            if policy is not None:
                assert policy(None, torch.zeros(B, args.state_shape), None, 0).shape == (B, args.n_agents)
            batch = synthetic_batch(args, B, 20 + self.k)
            self.k += 1
            del batch["u_expert"]
            return batch, None, None, torch.tensor([3, 4, 5])

    class StubAgents:
        def __init__(self, net):
            self.net, self.synced = net, []

        def sync_weights(self):
            calls.append(("sync",))
            self.synced.append({k: v.clone() for k, v in self.net.state_dict().items()})

    monkeypatch.setattr(im, "EpisodeCollector", StubCollector)
    expert = cs.CoverageAgents(args, batch=B, device="cpu", impl="torch")
    learner = im.ImitationLearner(args, device="cpu", unroll="torch")
    real_learn, real_label, labelled = learner.learn, im.label_episodes, []

    def learn(batch):
        calls.append(("learn", int(batch["u"].shape[0])))
        return real_learn(batch)

    def label(expert, batch, impl="auto"):
        calls.append(("label", impl))
        labelled.append(real_label(expert, batch, impl))
        return labelled[-1]

    monkeypatch.setattr(learner, "learn", learn)
    monkeypatch.setattr(im, "label_episodes", label)
    agents = StubAgents(cs.AgentRNN(cs.rnn_input_shape(args), args))   # a net of its own: distil copies the student's into it
    ring = im.LabelledRing(args, 16, device="cpu")
    history = im.distil(None, expert, learner, agents, ring, iterations=3, updates=2, sample=5, generator=torch.Generator().manual_seed(0))
    per_iter = lambda fly, label: [fly] + label + [("learn", 5), ("learn", 5), ("sync",)]
    assert calls == per_iter(("fly", "policy", True), []) + 2 * per_iter(("fly", "agents", True), [("label", "auto")])
    assert [h["iteration"] for h in history] == [0, 1, 2] and [h["flown_by"] for h in history] == ["expert", "student", "student"]
    assert all(set(h) == {"iteration", "flown_by", "loss", "agreement", "targets_find"} for h in history)
    assert all(np.isfinite(h["loss"]) and 0 <= h["agreement"] <= 1 and h["targets_find"] == 4.0 for h in history)
    assert ring.current_size == 9
    assert torch.equal(ring.buffers["u_expert"][:3], ring.buffers["u"][:3])                       # iteration 0: the actions flown
    assert torch.equal(ring.buffers["u_expert"][3:6].squeeze(3).long(), labelled[0])               # iteration 1: the relabelling
    for k, v in learner.eval_rnn.state_dict().items():
        assert torch.equal(agents.synced[-1][k], v), k                                             # agents act with the student's weights
    history = im.distil(None, expert, learner, agents, ring, iterations=1, updates=0, sample=1)
    assert history[0]["loss"] is None and history[0]["agreement"] is None
    with pytest.raises(ValueError):
        im.distil(None, expert, learner, agents, ring, iterations=0, updates=1, sample=1)
