"""CPU tests of the swept-area accounting (sweep.py, include/coopsearch.h: cs_sweep_episodes): the boundary declares, exports
and registers it; the definition (sweep.sweep_episodes_torch) does what DESIGN.md section 18 says on hand cases checked against
plain-Python integer discs; the bonus is aligned with the steps and reaches the learner through Runner.train only when asked
for; and on the C oracle the coverage policy sweeps more of the map than the random policy on the same seeds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import sweep as sw
from cooperative_search_amd.replay import KEYS
from oracle import oracle as orc
from test_runner_cpu import FIXTURE, Recorder, make_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, VR = 50, 7   # flight_easy: map_size, view_range
NAN = float("nan")


@pytest.fixture()
def one_thread():
    """The definition's tensors are small: torch's thread pool only costs time on them."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(before)


def table(episodes, tail=45):
    """states float32 [E, T1, 4n + tail] of episodes given as rows of agents' (xn, yn); headings and the tail are never read."""
    return torch.tensor([[[v for xn, yn in row for v in (xn, yn, 1.0, 0.0)] + [0.5] * tail for row in ep] for ep in episodes],
                        dtype=torch.float32)


def counts_of(*c):
    return torch.tensor(c, dtype=torch.int32)


def points(states, n, side=SIDE):
    """The quantised positions of every row as Python ints: [E][T1][n] of (X, Y)."""
    E, T1, S = states.shape
    X, Y = bl.quantise_positions(states.reshape(E * T1, S), n, side)
    X, Y = X.view(E, T1, n).tolist(), Y.view(E, T1, n).tolist()
    return [[[(X[e][t][i], Y[e][t][i]) for i in range(n)] for t in range(T1)] for e in range(E)]


def disc(px, py, side=SIDE, view_range=VR):
    """The set of cells ix * side + iy whose centre lies within 16 view_range sub-units of (px, py), in plain Python integers."""
    R2 = (16 * view_range) ** 2
    return {ix * side + iy for ix in range(side) for iy in range(side) if (16 * ix + 8 - px) ** 2 + (16 * iy + 8 - py) ** 2 <= R2}


def by_hand(states, counts, n, side=SIDE, view_range=VR):
    """(first, new_cells, seen_cells) as nested Python lists, from integer discs and sets."""
    pts = points(states, n, side)
    E, T1 = len(pts), len(pts[0])
    first, new, seen = [[-1] * (side * side) for _ in range(E)], [[0] * T1 for _ in range(E)], [[0] * T1 for _ in range(E)]
    for e in range(E):
        for t in range(min(max(int(counts[e]), 0), T1)):
            swept = set().union(*(disc(x, y, side, view_range) for x, y in pts[e][t]))
            seen[e][t] = len(swept)
            for c in swept:
                if first[e][c] < 0:
                    first[e][c] = t
                    new[e][t] += 1
    return first, new, seen


def check_by_hand(states, counts, n, side=SIDE, view_range=VR):
    res = sw.sweep_episodes_torch(states, counts, n, side, view_range)
    first, new, seen = by_hand(states, counts, n, side, view_range)
    assert res.first.dtype == res.new_cells.dtype == res.seen_cells.dtype == torch.int32
    assert res.first.tolist() == first and res.new_cells.tolist() == new and res.seen_cells.tolist() == seen
    return res


# ---- 1. the boundary ----------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_sweep_episodes\s*\(\s*const\s+cs_sweep_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_sweep_episodes" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "cs_sweep_episodes") and L.cs_sweep_episodes.argtypes is not None
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    fields = re.search(r"typedef struct cs_sweep_params \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"int32_t\s+(\w+);", fields) == [k for k, _ in _lib.CsSweepParams._fields_]
    assert [k for k, _ in _lib.CsSweepParams._fields_] == ["n_agents", "side", "view_range", "state_width", "rows", "reserved"]
    schema = str(_lib.torch_ops().sweep_episodes.default._schema)
    assert schema == ("coopsearch::sweep_episodes(Tensor states, Tensor counts, Tensor(a!) first, Tensor(b!) new_cells, "
                      "Tensor(c!) seen_cells, int n_agents, int side, int view_range) -> ()")
    from cooperative_search_amd import build
    assert "sweep.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "sweep_episodes")
    for name in ("SweepResult", "sweep_episodes", "sweep_episodes_torch", "sweep_batch", "swept_curve", "sweep_efficiency",
                 "sweep_bonus", "with_sweep_bonus", "collect_sweep_data"):
        assert getattr(cs, name) is getattr(sw, name), name


@pytest.mark.parametrize("field, value, msg", [("n_agents", 0, "n_agents"), ("n_agents", 9, "n_agents"), ("side", 0, "side"),
                                               ("side", 65, "side"), ("view_range", -1, "view_range"), ("view_range", 65, "view_range"),
                                               ("state_width", 11, "state_width"), ("rows", 0, "rows"), ("reserved", 1, "reserved"),
                                               ("E", 0, "E must"), ("E", -3, "E must"),
                                               ("ptr", 0, "NULL"), ("ptr", 1, "NULL"), ("ptr", 2, "NULL"), ("ptr", 3, "NULL"),
                                               ("ptr", 4, "NULL"), ("params", None, "NULL")])
def test_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    p = _lib.CsSweepParams(3, SIDE, VR, 57, 201, 0)
    E, ptrs, ref = 4, [C.c_void_p(256 * (k + 1)) for k in range(5)], C.byref(p)
    if field == "ptr":
        ptrs[value] = None
    elif field == "params":
        ref = None
    elif field == "E":
        E = value
    else:
        setattr(p, field, value)
    assert L.cs_sweep_episodes(ref, ptrs[0], ptrs[1], E, ptrs[2], ptrs[3], ptrs[4], None) == -1   # CS_E_CONFIG
    err = L.cs_episodes_last_error().decode()
    assert err.startswith("cs_sweep_episodes") and msg in err


def test_op_and_hip_impl_refuse_cpu_tensors():
    states, counts = table([[[(0.0, 0.0)] * 3] * 4] * 2), counts_of(4, 4)
    outs = [torch.zeros(2, SIDE * SIDE, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)]
    with pytest.raises(RuntimeError, match="GPU"):   # a CPU tensor must be refused, not dereferenced
        _lib.torch_ops().sweep_episodes(states, counts, *outs, 3, SIDE, VR)
    with pytest.raises(RuntimeError, match="first must be"):
        _lib.torch_ops().sweep_episodes(states, counts, outs[0][:, :-1].contiguous(), outs[1], outs[2], 3, SIDE, VR)
    with pytest.raises(RuntimeError, match="side must be"):
        _lib.torch_ops().sweep_episodes(states, counts, *outs, 3, 65, VR)
    with pytest.raises(ValueError, match="not on a GPU"):
        cs.sweep_episodes(states, counts, 3, SIDE, VR)
    with pytest.raises(ValueError, match="impl must be"):
        cs.sweep_episodes(states, counts, 3, SIDE, VR, impl="cpu")
    res = cs.sweep_episodes(states, counts, 3, SIDE, VR, impl="torch")
    assert isinstance(res, cs.SweepResult) and res.first.shape == (2, SIDE * SIDE) and res.new_cells.shape == res.seen_cells.shape == (2, 4)
    for bad in (dict(n_agents=9), dict(side=65), dict(view_range=-1)):
        kw = dict(n_agents=3, side=SIDE, view_range=VR) | bad
        with pytest.raises(ValueError, match="sweep"):
            cs.sweep_episodes_torch(states, counts, **kw)
    with pytest.raises(ValueError, match="counts"):
        cs.sweep_episodes_torch(states, counts.to(torch.int64), 3, SIDE, VR)
    with pytest.raises(ValueError, match="states"):
        cs.sweep_episodes_torch(states[:, :, :11], counts, 3, SIDE, VR)


# ---- 2. the definition on hand cases ------------------------------------------------------------------------------------------

def test_the_quantisation_is_the_coverage_policys():
    states = table([[[(0.3, -0.2), (-1.0, 1.0)]]])
    assert points(states, 2)[0][0] == [(int(np.rint((np.float32(0.3) * np.float32(25) + np.float32(25)) * np.float32(16))),
                                        int(np.rint((np.float32(-0.2) * np.float32(25) + np.float32(25)) * np.float32(16)))),
                                       (0, 16 * SIDE)]
    X, Y, _ = bl.quantise(states[0], 2, SIDE)
    assert points(states, 2)[0][0] == list(zip(X[0].tolist(), Y[0].tolist()))


def test_one_stationary_agent_sweeps_its_disc_once():
    states = table([[[(0.1, -0.3)]] * 6])
    res = check_by_hand(states, counts_of(6), 1)
    (x, y), = points(states, 1)[0][0]
    cells = len(disc(x, y))
    assert 100 < cells < 200
    assert res.new_cells.tolist() == [[cells, 0, 0, 0, 0, 0]] and res.seen_cells.tolist() == [[cells] * 6]
    assert set(res.first[0].tolist()) == {-1, 0} and int((res.first[0] == 0).sum()) == cells


def test_an_agent_moved_by_one_cell_sweeps_a_crescent():
    states = table([[[(0.0, 0.0)], [(0.04, 0.0)]]])   # one cell along +x: 16 sub-units
    res = check_by_hand(states, counts_of(2), 1)
    (p0,), (p1,) = points(states, 1)[0]
    assert p0 == (400, 400) and p1 == (416, 400)
    d0, d1 = disc(*p0), disc(*p1)
    crescent = d1 - d0
    assert 0 < len(crescent) < len(d1) and res.new_cells.tolist() == [[len(d0), len(crescent)]]
    assert {c for c, f in enumerate(res.first[0].tolist()) if f == 0} == d0
    assert {c for c, f in enumerate(res.first[0].tolist()) if f == 1} == crescent
    assert all(c // SIDE > 25 for c in crescent)   # the grid index is ix * side + iy: the crescent lies towards +x


def test_two_overlapping_discs_count_their_union():
    states = table([[[(0.0, 0.0), (0.12, 0.08)]]])
    res = check_by_hand(states, counts_of(1), 2)
    p0, p1 = points(states, 2)[0][0]
    d0, d1 = disc(*p0), disc(*p1)
    assert d0 & d1 and int(res.seen_cells[0, 0]) == len(d0 | d1) < len(d0) + len(d1)


def test_agents_on_the_walls_and_in_the_corners():
    """Exactly 0 and exactly map_size on either axis: a quarter or half of a disc lies on the map, no index leaves it."""
    states = table([[[(-1.0, -1.0), (1.0, 1.0)], [(-1.0, 1.0), (1.0, -1.0)], [(0.0, -1.0), (1.0, 0.0)]]])
    res = check_by_hand(states, counts_of(3), 2)
    assert points(states, 2)[0][0] == [(0, 0), (16 * SIDE, 16 * SIDE)]
    quarter = len(disc(0, 0))
    assert res.seen_cells[0].tolist()[:2] == [2 * quarter, 2 * quarter] and 30 < quarter < 50
    assert int(res.first[0, 0]) == 0 and int(res.first[0, SIDE * SIDE - 1]) == 0 and int(res.first[0, SIDE - 1]) == 1


@pytest.mark.parametrize("side", [50, 7, 64, 1])
def test_view_range_zero_and_view_range_beyond_the_map(side):
    """view_range 0: a cell is swept only when an agent stands exactly on its centre (never for a get_state() row of an even
    map: X is a multiple of 8 there only by chance).  view_range 64 from anywhere on a map of at most 64 / sqrt(2) cells
    sweeps all of it at row 0."""
    states = table([[[(0.0, 0.0), (-1.0, -1.0)], [(0.3, 0.7), (1.0, 1.0)]]])
    res = check_by_hand(states, counts_of(2), 2, side, 0)
    on_centre = sum((x - 8) % 16 == 0 and (y - 8) % 16 == 0 and 0 <= x < 16 * side and 0 <= y < 16 * side
                    for x, y in points(states, 2, side)[0][0])
    assert int(res.seen_cells[0, 0]) == on_centre <= 2
    res = check_by_hand(states, counts_of(2), 2, side, 64)
    if side <= 45:
        assert res.new_cells.tolist() == [[side * side, 0]] and res.seen_cells.tolist() == [[side * side] * 2]
        assert bool((res.first == 0).all())


def test_rows_at_and_past_the_count_are_never_looked_at():
    ep = [[(0.0, 0.0)], [(0.2, 0.0)], [(0.4, 0.0)], [(0.6, 0.0)]]
    clean = table([ep] * 5)
    counts = counts_of(0, 1, 4, 7, -2)   # 7 and -2 are clamped to T1 = 4 and to 0
    dirty = clean.clone()
    for e, c in enumerate((0, 1, 4, 4, 0)):
        dirty[e, c:] = NAN
    dirty[1, 2:] = 1e30
    want = check_by_hand(clean, counts, 1)
    got = sw.sweep_episodes_torch(dirty, counts, 1, SIDE, VR)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert not bool(got.new_cells[0].any()) and not bool(got.seen_cells[0].any()) and bool((got.first[0] == -1).all())
    assert got.new_cells[1].tolist()[1:] == [0, 0, 0] and int(got.new_cells[1, 0]) > 0 and int(got.first[1].max()) == 0
    assert torch.equal(got.first[2], got.first[3]) and int(got.first[2].max()) == 3 and torch.equal(got.first[4], got.first[0])
    # a NaN inside a VALID row is a position like any other: it quantises to -2^15, far off the map
    inside = clean.clone()
    inside[2, 1, 0] = NAN
    assert int(check_by_hand(inside, counts, 1).seen_cells[2, 1]) == 0


def test_new_cells_count_the_first_rows_on_random_episodes(one_thread):
    g = torch.Generator().manual_seed(11)
    E, T1, n, side = 9, 14, 3, 23
    states = torch.rand(E, T1, 4 * n + 5, generator=g) * 2.2 - 1.1   # some positions off the map
    counts = torch.randint(0, T1 + 1, (E,), generator=g, dtype=torch.int32)
    counts[:3] = torch.tensor([0, 1, T1], dtype=torch.int32)
    for vr in (0, 1, 4, 30):
        res = sw.sweep_episodes_torch(states, counts, n, side, vr)
        t = torch.arange(T1).view(1, T1, 1)
        assert torch.equal(res.new_cells, (res.first.view(E, 1, -1) == t).sum(2).to(torch.int32)), vr
        assert torch.equal(res.new_cells.sum(1), (res.first >= 0).sum(1)), vr
        assert bool((res.new_cells <= res.seen_cells).all()) and bool((res.first < counts.view(E, 1).clamp(min=0)).all()), vr
        assert bool((res.seen_cells[torch.arange(T1).view(1, T1) >= counts.view(E, 1)] == 0).all()), vr
    check_by_hand(states[:3], counts[:3] + torch.tensor([5, 6, 0], dtype=torch.int32), n, side, 4)


def test_swept_curve_and_efficiency():
    res = cs.SweepResult(torch.zeros(2, 64, dtype=torch.int32), torch.tensor([[16, 8, 0, 0], [32, 0, 16, 8]], dtype=torch.int32),
                         torch.tensor([[16, 16, 0, 0], [32, 32, 32, 32]], dtype=torch.int32))
    curve = cs.swept_curve(res)
    assert curve.dtype == torch.float64 and curve.tolist() == [0.375, 0.4375, 0.5625, 0.625]   # an ended episode holds its final value
    assert cs.sweep_efficiency(res) == 80 / 160


# ---- 3. the bonus ---------------------------------------------------------------------------------------------------------------

def dense_batch(paths, steps, n_actions=3):
    """A dense episode batch (the reference's 11 keys, float32) that follows the collector's padding rules, of agents' paths
    [E][T + 1][n] of (xn, yn) and the real steps per episode; one target, rewards -1 per real step."""
    full = table(paths, tail=3)                                 # [E, T + 1, 4n + 3]
    E, T, n = full.shape[0], full.shape[1] - 1, len(paths[0][0])
    real = (torch.arange(T).view(1, T) < torch.tensor(steps).view(E, 1)).to(torch.float32).view(E, T, 1)
    ag = full[..., :4 * n].reshape(E, T + 1, n, 4)
    u = torch.zeros(E, T, n, 1)
    return {"o": ag[:, :T] * real.unsqueeze(-1), "o_next": ag[:, 1:] * real.unsqueeze(-1), "s": full[:, :T] * real, "s_next": full[:, 1:] * real,
            "u": u, "r": -real, "avail_u": real.unsqueeze(-1).expand(E, T, n, n_actions).contiguous(),
            "avail_u_next": real.unsqueeze(-1).expand(E, T, n, n_actions).contiguous(),
            "u_onehot": torch.nn.functional.one_hot(u.long().squeeze(-1), n_actions).to(torch.float32) * real.unsqueeze(-1),
            "padded": 1 - real, "terminated": 1 - real}


PATHS = [[[(0.0, 0.0), (-0.5, 0.5)], [(0.04, 0.0), (-0.5, 0.5)], [(0.04, 0.0), (-0.5, 0.54)], [(0.08, 0.0), (-0.5, 0.58)], [(0.9, 0.9), (0.9, 0.9)]],
         [[(0.5, 0.5), (0.5, 0.5)], [(0.5, 0.46), (0.5, 0.5)], [(0.5, 0.42), (0.5, 0.5)], [(0.5, 0.38), (0.5, 0.5)], [(0.5, 0.34), (0.5, 0.5)]]]
STEPS = [2, 4]
ARGS = cs.make_env_args("flight_easy", n_agents=2)


def test_the_bonus_pays_step_t_for_the_move_into_row_t_plus_one():
    batch = dense_batch(PATHS, STEPS)
    assert set(batch) == set(KEYS)
    bonus = cs.sweep_bonus(batch, ARGS, 0.25, impl="torch")
    assert bonus.dtype == torch.float32 and bonus.shape == (2, 4, 1)
    # by hand: the rows the episodes really have (steps + 1), discs as sets
    _, new, _ = by_hand(table(PATHS), [s + 1 for s in STEPS], 2)
    assert bonus.view(2, 4).tolist() == [[0.25 * v for v in row[1:]] for row in new]
    assert new[0][1] > 0 and new[0][2] > 0 and new[0][3:] == [0, 0]      # episode 0 ends after 2 steps: the padded steps earn 0
    assert all(v > 0 for v in new[1])                                    # (the far jump of its row 4 is never looked at)
    res = cs.sweep_batch(batch, ARGS, impl="torch")
    assert res.new_cells[:, 0].tolist() == [new[0][0], new[1][0]] and new[0][0] > 0   # row 0, the reset pose, is in no step's bonus
    # the map-once twin of the batch gives the same tensor
    twin = cs.compact_from_dense(batch)
    assert "s_full" in twin and torch.equal(cs.sweep_bonus(twin, ARGS, 0.25, impl="torch"), bonus)
    with pytest.raises(ValueError, match="not on a GPU"):
        cs.sweep_bonus(batch, ARGS, 0.25)


def test_with_sweep_bonus_copies_the_dict_and_leaves_the_batch_alone():
    batch = dense_batch(PATHS, STEPS)
    before = {k: v.clone() for k, v in batch.items()}
    out = cs.with_sweep_bonus(batch, ARGS, 0.5)   # a host batch goes to the definition
    assert out is not batch and out["r"] is not batch["r"]
    assert all(out[k] is batch[k] for k in batch if k != "r") and set(out) == set(batch)
    assert all(torch.equal(batch[k], before[k]) for k in batch)
    assert torch.equal(out["r"], before["r"] + cs.sweep_bonus(batch, ARGS, 0.5, impl="torch"))
    assert bool((out["r"] > before["r"]).any())


class SweepRecorder(Recorder):
    """test_runner_cpu's stubs with real (hand-made) episode batches and a learner that keeps what it is handed."""

    def __init__(self, args):
        super().__init__(args)
        self.made, self.learnt = [], []
        self.learner.learn = lambda batch, max_episode_len=None, train_step=0, *eps: self.learnt.append(batch)

    def episode(self, k):
        self.made.append(dense_batch(PATHS[:1] * k, STEPS[:1] * k))
        return self.made[-1]


@pytest.mark.parametrize("cfg", FIXTURE["configs"], ids=[c["name"] for c in FIXTURE["configs"]])
def test_runner_hands_the_learner_the_bonus_only_when_asked(cfg, tmp_path):
    args = make_args(cfg, str(tmp_path / "off"), n_agents=2, n_epoch=2, n_episodes=1)
    assert not hasattr(args, "sweep_bonus")
    rec = SweepRecorder(args)
    rec.runner().run(0)
    assert rec.learnt and all(any(b is m for m in rec.made) for b in rec.learnt)   # the very same objects
    args = make_args(cfg, str(tmp_path / "zero"), n_agents=2, n_epoch=2, n_episodes=1, sweep_bonus=0.0)
    rec = SweepRecorder(args)
    rec.runner().run(0)
    assert rec.learnt and all(any(b is m for m in rec.made) for b in rec.learnt)
    args = make_args(cfg, str(tmp_path / "on"), n_agents=2, n_epoch=2, n_episodes=1, sweep_bonus=0.125)
    rec = SweepRecorder(args)
    rec.runner().run(0)
    assert rec.learnt and len(rec.learnt) <= len(rec.made)
    for b in rec.learnt:
        src = [m for m in rec.made if m["s"] is b["s"]]
        assert len(src) == 1 and b is not src[0]
        assert torch.equal(src[0]["r"], dense_batch(PATHS[:1], STEPS[:1])["r"].expand_as(src[0]["r"]))   # the stored batch is untouched
        assert torch.equal(b["r"], src[0]["r"] + cs.sweep_bonus(src[0], args, 0.125, impl="torch"))
        assert bool((b["r"] != src[0]["r"]).any())


# ---- 4. closed loop on the C oracle -------------------------------------------------------------------------------------------

def oracle_tables(policy, B, T, n, seeds):
    """(states float32 [B, T + 1, S], counts int32 [B]) of `policy(state float32 [B, S], t) -> int [B, n]` on the C oracle:
    row 0 the reset pose, row t + 1 the state after step t; counts = real steps + 1."""
    ob = orc.OracleBatch(orc.make_config(variant="flight_easy", n_agents=n), B, seeds)
    ob.reset(init=True, threads=4)
    state = np.stack([ob.env(b).get_state() for b in range(B)]).astype(np.float32)
    rows, counts = [state], np.full(B, T + 1, dtype=np.int32)
    for t in range(T):
        _r, term, _w = ob.step(np.asarray(policy(torch.from_numpy(state), t), dtype=np.int32), freeze_done=True, threads=4)
        state = ob.state.copy()
        rows.append(state)
        counts = np.where((np.asarray(term) != 0) & (counts == T + 1), t + 2, counts).astype(np.int32)
    return torch.from_numpy(np.stack(rows, 1)), torch.from_numpy(counts)


def test_coverage_sweeps_more_of_the_map_than_random_on_the_oracle(one_thread):
    """flight_easy, 3 agents, 64 envs, 200 steps, reset(init=True): the coverage policy's swept curve lies strictly above the
    random policy's at row 60 on the same seeds, and the reset pose sweeps 156 cells in every env.  Both sides are measured here."""
    B, T, n = 64, 200, 3
    seeds = np.arange(B, dtype=np.uint32) + 1000
    ag = cs.CoverageAgents(cs.make_env_args("flight_easy", n_agents=n), batch=B, device="cpu", impl="torch")
    pol = ag.policy()
    rng = np.random.RandomState(0)
    res = {}
    for name, policy in (("coverage", lambda s, t: pol(None, s, None, t).numpy()), ("random", lambda s, t: rng.randint(0, 3, size=(B, n)))):
        states, counts = oracle_tables(policy, B, T, n, seeds)
        res[name] = cs.sweep_episodes(states, counts, n, SIDE, VR, impl="torch")
    cov, rnd = cs.swept_curve(res["coverage"]), cs.swept_curve(res["random"])
    print(f"share of the map swept by row 60 / 200: coverage {cov[60]:.3f} / {cov[200]:.3f}, random {rnd[60]:.3f} / {rnd[200]:.3f}; "
          f"efficiency coverage {cs.sweep_efficiency(res['coverage']):.3f}, random {cs.sweep_efficiency(res['random']):.3f}")
    assert float(cov[60]) > float(rnd[60])
    for r in res.values():
        assert r.new_cells[:, 0].tolist() == [156] * B and r.seen_cells[:, 0].tolist() == [156] * B
