"""GPU tests of the private-grid observations (csrc/localobs.h, localobs.py): both kernels bit for bit against
their definitions, the walk kernel against T launches of the existing step kernels, against what LocalGridAgents traced while flying
and against the rows path, the distillation loop end to end, and the stream rules.  Everything is torch.equal on integers or on float
bits: no tolerance, and nothing is asserted about what a policy finds."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import belief as be
from cooperative_search_amd import gridobs as go
from cooperative_search_amd import imitate as im
from cooperative_search_amd import localobs as lo
from cooperative_search_amd import motion as mo
from local_util import KEEP, SIDE, boundary_rows, far_rows, tie_rows, walk, wall_rows
from localobs_util import DECISION_SHAPES, MODELS, SEED, T, WALK_SHAPES, episodes, lens_for, params, ranges_for, same_bits, spoil_past

pytestmark = pytest.mark.gpu
DEV = "cuda"


def behind(shape, dtype):
    """A contiguous device tensor that starts one element behind a 16-byte boundary (the kernels' scalar paths)."""
    buf = torch.zeros(int(np.prod(shape)) + 1, dtype=dtype, device=DEV)
    view = buf[1:].view(*shape)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def mixed_grids(B, n, side, seed):
    """int32 [B, n, side * side]: agent i of env b holds kind (b + i) % 5 of: fresh, random in 0..CAP, all zero, a full-CAP map, and
    garbage below 0 and above CAP -- the grids of an env differ in kind."""
    g = torch.Generator().manual_seed(seed)
    cells = side * side
    kinds = [torch.full((cells,), 65536, dtype=torch.int32), None, torch.zeros(cells, dtype=torch.int32), torch.full((cells,), be.CAP, dtype=torch.int32), None]
    out = torch.empty(B, n, cells, dtype=torch.int32)
    for b in range(B):
        for i in range(n):
            k = (b + i) % 5
            if k == 1:
                out[b, i] = torch.randint(0, be.CAP + 1, (cells,), generator=g, dtype=torch.int32)
            elif k == 4:
                out[b, i] = torch.randint(-(1 << 31), (1 << 31) - 1, (cells,), generator=g, dtype=torch.int64).to(torch.int32)
            else:
                out[b, i] = kinds[k]
    return out


# ---- 1. the per-decision kernel against the definition ---------------------------------------------------------------------------

def decide(state, grids, n, side, vr, look=None, misalign=False):
    want = lo.local_grid_features_torch(state, grids, n, side, vr, look)
    if misalign:
        sd, gd, out = behind(state.shape, torch.float32), behind(grids.shape, torch.int32), behind(want.shape, torch.float32)
        sd.copy_(state)
        gd.copy_(grids)
    else:
        sd, gd, out = state.to(DEV), grids.to(DEV), torch.empty(want.shape, device=DEV)
    out.fill_(-7.0)
    keep_s, keep_g = sd.clone(), gd.clone()
    got = lo.local_grid_features_hip(sd, gd, n, side, vr, look, out=out)
    assert got is out and same_bits(got.cpu(), want), (tuple(state.shape), n, side, vr, look, misalign)
    assert torch.equal(gd, keep_g) and same_bits(sd, keep_s)   # read, never written
    return want


@pytest.mark.parametrize("B, n, side, vr", DECISION_SHAPES)
def test_decision_kernel_equals_the_definition_bit_for_bit(B, n, side, vr):
    states = walk(B, n, 8, SEED)
    for k, t in enumerate((0, 3, 7)):   # (row 3 sets one agent on a corner and another well outside the map)
        want = decide(states[t], mixed_grids(B, n, side, 10 * B + k), n, side, vr)
        assert bool(want.any())
    decide(states[1], mixed_grids(B, n, side, 3), n, side, vr, look=0)
    decide(states[1], mixed_grids(B, n, side, 4), n, side, vr, look=side)
    decide(states[2], mixed_grids(B, n, side, 5), n, side, vr, misalign=True)
    # the private grids ARE read privately: the same call on agent 0's grid for everybody gives other features
    grids = mixed_grids(B, n, side, 6)
    if n > 1:
        shared = grids[:, :1].expand(B, n, side * side).contiguous()
        assert not same_bits(lo.local_grid_features_hip(states[0].to(DEV), grids.to(DEV), n, side, vr),
                             lo.local_grid_features_hip(states[0].to(DEV), shared.to(DEV), n, side, vr))


def test_decision_kernel_on_odd_far_tie_and_wall_rows_and_at_the_edge_parameters():
    """Rows no env emits (NaN, infinities, huge values), positions 2^16 sub-units apart, two agents on one spot, probes clamped at the
    walls with lookahead = side; view_range 0 and 64."""
    n, B = 3, 5
    odd = walk(B, n, 1, 2)[0]
    odd[0, 0], odd[1, 1], odd[2, 2], odd[3, 3], odd[3, 4], odd[4, 5] = float("nan"), float("inf"), float("nan"), -1e30, 1e30, 7.5
    decide(odd, mixed_grids(B, n, SIDE, 1), n, SIDE, 7)
    decide(odd, mixed_grids(B, n, SIDE, 1), n, SIDE, 7, misalign=True)
    decide(far_rows(), mixed_grids(1, 2, SIDE, 2), 2, SIDE, 7)
    decide(tie_rows(), mixed_grids(1, 2, SIDE, 3), 2, SIDE, 7)
    decide(boundary_rows(), mixed_grids(2, 2, SIDE, 4), 2, SIDE, 7)
    walls = wall_rows(3)
    decide(walls, mixed_grids(walls.shape[0], 3, SIDE, 5), 3, SIDE, 7, look=SIDE)
    state = walk(3, 8, 1, 6)[0]
    state[0, :2] = 0.0   # agent 0 of env 0 on the centre of the map
    full = torch.full((3, 8, 64 * 64), be.CAP, dtype=torch.int32)   # the 2^31 probe sum
    for vr, look in ((64, 64), (64, 0), (0, 0), (0, 64)):
        decide(state, full, 8, 64, vr, look)
    decide(walk(2, 2, 1, 7)[0], mixed_grids(2, 2, 1, 7), 2, 1, 1, 1)   # side 1


# ---- 2. the walk kernel against its definition -------------------------------------------------------------------------------------

def run_kernel(s, lens, p, labels=True, prev_out=True, heard_out=True, misalign=False):
    """One cs_local_feature_episodes launch on CPU inputs -> CPU outputs (feat, labels, grids, prev, heard)."""
    E, steps, n, cells = s.shape[0], s.shape[1], p.n_agents, p.side * p.side
    if not misalign:
        sd, ld = s.to(DEV), lens.to(DEV)
        keep_s, keep_l = sd.clone(), ld.clone()
        out = lo.local_feature_episodes_hip(sd, ld, p, labels=labels, prev_out=prev_out, heard_out=heard_out)
        assert torch.equal(ld, keep_l) and same_bits(sd, keep_s)
        return tuple(None if x is None else x.cpu() for x in out)
    sd = behind(s.shape, torch.float32)
    sd.copy_(s)
    feat, lab, grids = behind((E, steps, n, 16), torch.float32), behind((E, steps, n), torch.int64), behind((E, n, cells), torch.int32)
    belief = p.expert == im.BELIEF
    prev, heard = (behind((E, 8, 2), torch.int32), behind((E, 8), torch.int32)) if belief else (None, None)
    grids.fill_(-12345)   # the workspace's content on entry does not matter
    _lib.torch_ops().local_feature_episodes(sd, lens.to(DEV), feat, lab, grids, prev, heard, p.expert, n, p.side, p.view_range, p.keep, p.regrow,
                                            p.lookahead, p.model.mode, p.model.sense16, p.every, p.moving, list(p.model.dx), list(p.model.dy),
                                            p.comm_range)
    return feat.cpu(), lab.cpu(), grids.cpu(), None if prev is None else prev.cpu(), None if heard is None else heard.cpu()


def same(got, want, what):
    assert same_bits(got[0], want[0]), ("feat", what)
    for k, name in ((1, "labels"), (2, "grids"), (3, "prev"), (4, "heard")):
        assert (got[k] is None and want[k] is None) or torch.equal(got[k], want[k]), (name, what)


@pytest.mark.parametrize("kind, mode, speed", MODELS)
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("E, n, side, vr", WALK_SHAPES)
def test_walk_kernel_equals_the_definition(E, n, side, vr, which, kind, mode, speed):
    """Every filter of MODELS (coverage; belief static, walking at 0.25, evading at 1.0 and 3.5; `every` 1 and 3 where the targets move)
    at the three ranges of the shape (unlimited, 0, the mixed one), on lens that mix 0, 1, a middle value and T with NaN behind them:
    feat, labels, grids, prev and heard; then the same launch without labels, without each optional output, and on tensors one word
    behind a 16-byte boundary."""
    s = episodes(E, n)
    comm = ranges_for(s, n, side)[which]
    for k, every in enumerate((1, 3) if speed > 0 else (1,)):
        p = params(kind, mode, speed, n, side, vr, comm, every)
        lens = lens_for(E, shift=which + 2 * k + len(kind))
        poisoned = spoil_past(s, lens)
        want = lo.local_feature_episodes_torch(poisoned, lens, p)
        what = (E, n, side, comm, kind, every)
        same(run_kernel(poisoned, lens, p), want, what)
        bare = run_kernel(poisoned, lens, p, labels=False, prev_out=False, heard_out=False)   # NULL labels: the choose step is skipped
        assert same_bits(bare[0], want[0]) and torch.equal(bare[2], want[2]) and bare[1] is None and bare[3] is None and bare[4] is None, what
        if k == 0:
            same(run_kernel(poisoned, lens, p, misalign=True), want, what)
            if p.expert == im.BELIEF:
                half = run_kernel(poisoned, lens, p, labels=False, heard_out=False)
                assert same_bits(half[0], want[0]) and torch.equal(half[3], want[3]) and half[4] is None, what
                half = run_kernel(poisoned, lens, p, prev_out=False)
                assert torch.equal(half[1], want[1]) and torch.equal(half[4], want[4]) and half[3] is None, what
        for e in range(E):
            tail = want[0][e, int(lens[e]):]
            assert same_bits(tail, torch.zeros_like(tail)) and not want[1][e, int(lens[e]):].any()
    assert bool(want[0].any()) or int(lens.max()) == 0


def test_walk_kernel_on_full_and_empty_lens_odd_widths_and_the_edge_parameters():
    E, n, side = 4, 3, 50
    for S in (4 * n, 4 * n + 9, 4 * n + 8):   # no tail, an odd width, a width that keeps every row 16-byte aligned
        s = episodes(E, n, 5, 11 + S, tail=S - 4 * n)
        for kind, mode, speed in (MODELS[0], MODELS[3]):
            p = params(kind, mode, speed, n, side, 7, 30)
            for lens in (torch.zeros(E, dtype=torch.int32), torch.full((E,), 5, dtype=torch.int32), lens_for(E, 5, 1)):
                same(run_kernel(s, lens, p), lo.local_feature_episodes_torch(s, lens, p), (S, kind, lens.tolist()))
            over = torch.tensor([7, -3, 5, 2], dtype=torch.int32)   # the kernel reads lens clamped to 0..T
            same(run_kernel(s, over, p), lo.local_feature_episodes_torch(s, over.clamp(0, 5), p), (S, kind, "clamped"))
    s, lens = episodes(E, n, 5, 3), lens_for(E, 5, 2)
    for look, vr in ((0, 7), (50, 0), (50, 7)):   # every probe on the agent; a radius that holds at most one cell; probes at the walls
        for kind, mode, speed in (MODELS[0], MODELS[2]):
            p = params(kind, mode, speed, n, side, vr, 30, lookahead=look)
            same(run_kernel(s, lens, p), lo.local_feature_episodes_torch(s, lens, p), (look, vr, kind))
    s8 = episodes(2, 8, 4, 4)
    p = params("belief", "evade", 3.5, 8, 64, 64, 20, lookahead=64)   # whole-map discs on the full accumulator
    same(run_kernel(s8, torch.tensor([4, 3], dtype=torch.int32), p), lo.local_feature_episodes_torch(s8, torch.tensor([4, 3], dtype=torch.int32), p), "64")


# ---- 3. the walk kernel against the existing step kernels ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["coverage", "evade"])
@pytest.mark.parametrize("E, n, side, vr", WALK_SHAPES)
def test_walk_kernel_equals_t_launches_of_the_step_kernel_and_the_decision_kernel(E, n, side, vr, kind):
    """Full-length episodes: features and labels equal T calls of the filter's choose_action (HIP) each followed by
    local_grid_features_hip, and the workspace ends as the filter's grids (prev and heard likewise)."""
    s = episodes(E, n).to(DEV)
    comm = ranges_for(s.cpu(), n, side)[2]
    env_like = type("Env", (), dict(n_agents=n, map_size=side, view_range=vr, detect_prob=0.9, batch=E, device=DEV))()
    if kind == "coverage":
        filt = cs.LocalCoverageAgents(env_like, comm)
    else:
        filt = cs.LocalBeliefAgents(env_like, comm, motion=mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=3))
    assert filt.impl == "hip"
    p = lo.local_expert_params(filt)
    feat, labels, grids, prev, heard = lo.local_feature_episodes_hip(s, torch.full((E,), T, dtype=torch.int32, device=DEV), p)
    policy = filt.policy()
    for t in range(T):
        row = s[:, t].contiguous()
        assert torch.equal(labels[:, t], policy(None, row, None, t)), t
        assert same_bits(feat[:, t], lo.local_grid_features_hip(row, filt.grids, n, side, vr)), t
    assert torch.equal(grids, filt.grids)
    if kind == "evade":
        assert torch.equal(prev, filt.prev) and torch.equal(heard, filt.heard)
    batch = {"s": s, "padded": torch.zeros(E, T, 1, device=DEV)}
    assert torch.equal(lo.local_label_episodes(filt, batch), labels) and torch.equal(lo.local_label_episodes(filt, batch, impl="hip"), labels)
    assert torch.equal(lo.local_label_episodes(filt, batch, impl="rows"), labels) and torch.equal(im.label_episodes(filt, batch), labels)
    assert same_bits(lo.local_feature_episodes(filt, batch), feat) and bool((filt.grids == 65536).all())   # the rows path ended on reset()


# ---- 4. the closed loop --------------------------------------------------------------------------------------------------------------

STEPS, ENVS = 40, 33


def flight(comm, tmp_path, every=1):
    args = cs.make_env_args("flight_easy", n_agents=3)
    args.time_limit = STEPS
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, every=every, seed=4)
    env = cs.MovingTargetEnv(args, batch=ENVS, seeds=np.arange(ENVS, dtype=np.uint32) + 40, target_motion=motion)
    cs.apply_env_info(args, env)
    im.get_bc_args(args, seed=3)
    args.model_dir = str(tmp_path) + "/"
    return args, env, motion


@pytest.mark.parametrize("kind", ["coverage", "evade"])
def test_what_local_grid_agents_traced_is_what_the_walk_kernel_computes(kind, tmp_path):
    """LocalGridAgents.policy() on MovingTargetEnv, 33 envs, 40 steps, exploring: its trace equals local_feature_episodes of the
    recorded episode on every live row, and the labels of that launch equal the rows path."""
    args, env, motion = flight(10, tmp_path, every=3)
    filt = cs.LocalCoverageAgents(env, 10) if kind == "coverage" else cs.LocalBeliefAgents(env, 10)
    agents = lo.LocalGridAgents(args, filt, seed=2)
    assert agents.batch == ENVS and agents.net.fc1.in_features == cs.rnn_input_shape(args) + 16
    trace = torch.full((STEPS, ENVS, 3, 16), -1.0, device=DEV)
    torch.cuda.synchronize()
    episode = cs.EpisodeCollector(env).generate_episodes(policy=agents.policy(epsilon=0.4, evaluate=False, trace=trace), init=True)[0]
    lens = im.episode_lens(episode)
    feat, lab = lo.local_feature_episodes(filt, episode, labels=True)
    live = (torch.arange(STEPS, device=DEV).view(1, STEPS) < lens.view(ENVS, 1)).view(ENVS, STEPS, 1, 1).expand_as(feat)
    traced = trace.transpose(0, 1)
    assert same_bits(torch.where(live, feat, torch.zeros_like(feat)), torch.where(live, traced, torch.zeros_like(traced)))
    assert not feat[~live].any() and int(lens.max()) == STEPS and bool(feat[live].any())
    fresh_filter = cs.LocalCoverageAgents(env, 10) if kind == "coverage" else cs.LocalBeliefAgents(env, 10)
    assert torch.equal(lab, im.label_episodes(fresh_filter, episode, impl="rows"))
    assert episode["u"].unique().numel() == 3   # (an untrained network explores with epsilon 0.4: the flight is not one circle)
    assert bool((feat[:, :, 0] != feat[:, :, 1]).any())   # the agents of an env do not observe one grid


@pytest.mark.parametrize("expert_kind", ["own", "other_range"])
def test_distil_local_grid_for_two_iterations(expert_kind, tmp_path):
    args, env, motion = flight(10, tmp_path)
    filt = cs.LocalBeliefAgents(env, 10)
    expert = filt if expert_kind == "own" else cs.LocalBeliefAgents(env, 35)   # the same class, other parameters: not the same decisions
    learner = go.GridImitationLearner(args, device=DEV)
    agents = lo.LocalGridAgents(args, filt, net=learner.eval_rnn, seed=1)
    ring = go.FeatureRing(args, 4 * ENVS, device=DEV)
    before = agents.packed.clone()
    history = lo.distil_local_grid(env, expert, filt, learner, agents, ring, iterations=2, updates=3, sample=16,
                                   generator=torch.Generator(DEV).manual_seed(2))
    assert [h["flown_by"] for h in history] == ["expert", "student"] and ring.current_size == 2 * ENVS
    assert all(set(h) == {"iteration", "flown_by", "loss", "agreement", "targets_find"} for h in history)
    assert all(np.isfinite(h["loss"]) and 0 <= h["agreement"] <= 1 and 0 <= h["targets_find"] <= args.target_num for h in history)
    first = {k: v[:ENVS] for k, v in ring.buffers.items()}
    second = {k: v[ENVS:2 * ENVS] for k, v in ring.buffers.items()}
    live = (1 - first["padded"]).unsqueeze(3)
    assert torch.equal(first["u_expert"] * live, first["u"] * live)   # iteration 0: the actions the expert flew
    for part in (first, second):
        assert same_bits(part["f"], lo.local_feature_episodes(cs.LocalBeliefAgents(env, 10), part)) and bool(part["f"].any())
    relabel = cs.LocalBeliefAgents(env, 10 if expert_kind == "own" else 35)
    assert torch.equal(second["u_expert"].squeeze(3).long(), im.label_episodes(relabel, second, impl="rows"))   # the rows path
    assert not torch.equal(second["u_expert"], second["u"])           # ... of the student's own flight
    agents.check_weights()
    assert not torch.equal(agents.packed, before)                     # agents act with the synced weights


# ---- 5. refusals and synchronisation -------------------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops = _lib.torch_ops()
    state = walk(B, n, 1, 0, tail=45)[0].to(DEV)
    grids = torch.full((B, n, side * side), 1234, dtype=torch.int32, device=DEV)
    feat = torch.full((B, n, 16), -7.0, device=DEV)
    bad = [dict(state=state.double()), dict(state=state.cpu()), dict(state=state[:, ::2]), dict(state=state[:, :11].contiguous()), dict(grids=grids.long()),
           dict(grids=grids.cpu()), dict(grids=grids[:, :, :-1].contiguous()), dict(grids=grids[:, 0].contiguous()), dict(grids=grids.transpose(0, 1).contiguous().transpose(0, 1)),
           dict(feat=feat.double()), dict(feat=feat.cpu()), dict(feat=feat[:, :2].contiguous()), dict(feat=feat.transpose(1, 2).contiguous().transpose(1, 2))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.local_grid_features(kw.get("state", state), kw.get("grids", grids), kw.get("feat", feat), n, side, 7, 7)
    for pos, value in ((0, 9), (1, 65), (2, 65), (3, side + 1)):
        a = [n, side, 7, 7]
        a[pos] = value
        with pytest.raises(RuntimeError, match="local_grid_features"):
            ops.local_grid_features(state, grids, feat, *a)
    assert bool((feat == -7.0).all()) and bool((grids == 1234).all())
    E, steps = 4, 3
    p = params("belief", "evade", 1.0, n, side, 7, 10)
    s, lens = episodes(E, n, steps, 1, tail=45).to(DEV), torch.full((E,), steps, dtype=torch.int32, device=DEV)
    f4 = torch.full((E, steps, n, 16), -7.0, device=DEV)
    labels = torch.full((E, steps, n), -7, dtype=torch.int64, device=DEV)
    prev, heard = torch.full((E, 8, 2), 99, dtype=torch.int32, device=DEV), torch.full((E, 8), 99, dtype=torch.int32, device=DEV)
    ints = (1, n, side, 7, KEEP, 8, 7, p.model.mode, p.model.sense16, 1, 1, list(p.model.dx), list(p.model.dy), 10)
    bad = [dict(s=s.double()), dict(s=s.cpu()), dict(s=s[:, :, ::2]), dict(lens=lens.long()), dict(lens=lens.cpu()), dict(lens=lens[:-1].contiguous()),
           dict(feat=f4.double()), dict(feat=f4.cpu()), dict(feat=f4[:, :, :2].contiguous()), dict(feat=f4.transpose(2, 3).contiguous().transpose(2, 3)),
           dict(labels=labels.int()), dict(labels=labels.cpu()), dict(labels=labels[:, :, :2].contiguous()), dict(grids=grids.long()), dict(grids=grids.cpu()),
           dict(grids=grids[:, :, :-1].contiguous()), dict(grids=grids[:, :2].contiguous()), dict(prev=prev.long()), dict(prev=prev.cpu()),
           dict(prev=prev[:, :3].contiguous()), dict(heard=heard.long()), dict(heard=heard.cpu()), dict(heard=heard[:, :3].contiguous())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.local_feature_episodes(kw.get("s", s), kw.get("lens", lens), kw.get("feat", f4), kw.get("labels", labels), kw.get("grids", grids),
                                       kw.get("prev", prev), kw.get("heard", heard), *ints)
    for pos, value in ((0, 2), (1, 9), (2, 65), (3, 65), (4, 65537), (5, 0), (6, side + 1), (7, 2), (8, 2049), (9, 0), (10, 2), (11, [0] * 15),
                       (12, [1025] + [0] * 15), (13, -2), (13, 129)):
        a = list(ints)
        a[pos] = value
        with pytest.raises(RuntimeError, match="local_feature_episodes"):
            ops.local_feature_episodes(s, lens, f4, labels, grids, prev, heard, *a)
    coverage = list(ints)
    coverage[0] = 0
    for kw in (dict(), dict(prev=None)):   # prev_out and heard_out are the belief filter's
        with pytest.raises(RuntimeError, match="belief filter"):
            ops.local_feature_episodes(s, lens, f4, labels, grids, kw.get("prev", prev), heard, *coverage)
    assert bool((f4 == -7.0).all()) and bool((labels == -7).all()) and bool((grids == 1234).all()) and bool((prev == 99).all()) and bool((heard == 99).all())
    with pytest.raises(ValueError, match="on s's device"):
        lo.local_feature_episodes_hip(s, lens.cpu(), p)
    with pytest.raises(ValueError, match="grids must be"):
        lo.local_grid_features_hip(state, grids.cpu(), n, side, 7)


def test_neither_call_synchronises_and_both_run_on_the_current_stream():
    E, n, side = 16, 3, 50
    s = episodes(E, n, 6, 2)
    filt = cs.LocalBeliefAgents(cs.make_env_args("flight_easy"), 30, motion=mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), batch=E, device=DEV)
    batch = {"s": s.to(DEV), "padded": torch.zeros(E, 6, 1, device=DEV)}
    batch["padded"][3, 4:] = 1.0
    state, grids = s[:, 0].contiguous(), mixed_grids(E, n, side, 1)
    sd, gd = state.to(DEV), grids.to(DEV)
    lo.local_feature_episodes(filt, batch)   # (the op library is loaded)
    lo.local_grid_features(sd, gd, n, side, 7)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            feat, labels = lo.local_feature_episodes(filt, batch, labels=True)
            only = lo.local_label_episodes(filt, batch)
            one = lo.local_grid_features(sd, gd, n, side, 7)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    stream.synchronize()
    want = lo.local_feature_episodes_torch(s, im.episode_lens(batch).cpu(), lo.local_expert_params(filt))
    assert same_bits(feat.cpu(), want[0]) and torch.equal(labels.cpu(), want[1]) and torch.equal(only, labels)
    assert same_bits(one.cpu(), lo.local_grid_features_torch(state, grids, n, side, 7))
