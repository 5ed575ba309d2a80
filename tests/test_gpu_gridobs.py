"""GPU tests of the grid observations (csrc/gridobs.h, gridobs.py): both kernels bit for bit against their
definitions, the episode kernel against the labeller and against what GridAgents traced while flying, the policy forward with
features against a float64 twin, the learner fused against torch, the distillation loop end to end, and the stream rules."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import belief as be
from cooperative_search_amd import gridobs as go
from cooperative_search_amd import imitate as im
from cooperative_search_amd import motion as mo
from gridobs_util import FEATURE_CASES, FORWARD_SEED, clear_fraction, forward_case, grids, rows, same_bits, twin_of, twin_step
from imitate_util import KEEP, belief_params, coverage_params, mixed_lens, state_rows
from test_gpu_imitate import SHAPES, env_rows, recorded, rows_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5   # the project's bound for cs_policy_forward against the float32 module (tests/test_gpu_policy.py)


def behind(shape, dtype):
    """A contiguous device tensor that starts one element behind a 16-byte boundary (the kernels' scalar paths)."""
    buf = torch.zeros(int(np.prod(shape)) + 1, dtype=dtype, device=DEV)
    view = buf[1:].view(*shape)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


# ---- 1. the per-decision kernel against the definition ---------------------------------------------------------------------------

@pytest.mark.parametrize("n, side, vr, look", FEATURE_CASES)
@pytest.mark.parametrize("B", [1, 3, 65])
def test_feature_kernel_equals_the_definition_bit_for_bit(B, n, side, vr, look):
    state = rows(B, n, 4 * n + 5, 7 * B + n, spoil=(B == 3))
    for kind in ("fresh", "coverage", "belief", "cap", "wild"):
        grid = grids(kind, state, n, side, vr, look, seed=B)
        want = go.grid_features_torch(state, grid, n, side, vr, look)
        sd, gd = state.to(DEV), grid.to(DEV)
        keep_s, keep_g = sd.clone(), gd.clone()
        got = go.grid_features_hip(sd, gd, n, side, vr, look)
        assert same_bits(got.cpu(), want), kind
        assert torch.equal(gd, keep_g) and same_bits(sd, keep_s)   # read, never written
    assert bool(want.any()) or vr == 0   # (a probe at view_range 0 counts a cell only if it IS that cell's centre: the next test)


def test_feature_kernel_at_view_range_zero_reads_the_one_cell_under_the_probe():
    side = 7
    state = torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.3, -0.2, 0.0, 1.0]])   # agent 0 on the centre of cell (3, 3), agent 1 between centres
    grid = (torch.arange(side * side, dtype=torch.int32) * 1000 + 300).view(1, -1)
    want = go.grid_features_torch(state, grid, 2, side, 0, 0)
    assert bool((want[0, 0] == float((24 * 1000 + 300) >> 8) * 2.0 ** -15).all()) and not want[0, 1].any()
    assert same_bits(go.grid_features_hip(state.to(DEV), grid.to(DEV), 2, side, 0, 0).cpu(), want)


def test_feature_kernel_on_unaligned_tensors_and_an_odd_state_width():
    B, n, side, vr = 5, 3, 50, 7
    state = rows(B, n, 4 * n + 45, 2)   # S = 57, odd
    grid = grids("belief", state, n, side, vr, vr)
    sd, gd, out = behind(state.shape, torch.float32), behind(grid.shape, torch.int32), behind((B, n, 16), torch.float32)
    sd.copy_(state)
    gd.copy_(grid)
    out.fill_(-7.0)
    go.grid_features_hip(sd, gd, n, side, vr, out=out)
    assert same_bits(out.cpu(), go.grid_features_torch(state, grid, n, side, vr))


# ---- 2. the episode kernel against its definition ---------------------------------------------------------------------------------

def run_kernel(s, lens, p, misalign=False, labels=True, outputs=True):
    """One cs_feature_episodes launch on CPU inputs -> CPU outputs (feat, labels, grid_out, prev_out)."""
    E, T, n, cells = s.shape[0], s.shape[1], p.n_agents, p.side * p.side
    if not misalign:
        sd, ld = s.to(DEV), lens.to(DEV)
        keep_s, keep_l = sd.clone(), ld.clone()
        out = go.feature_episodes_hip(sd, ld, p, labels=labels, grid_out=outputs, prev_out=outputs)
        assert torch.equal(ld, keep_l) and same_bits(sd, keep_s)
        return tuple(None if x is None else x.cpu() for x in out)
    sd = behind(s.shape, torch.float32)
    sd.copy_(s)
    feat, lab, grid = behind((E, T, n, 16), torch.float32), behind((E, T, n), torch.int64), behind((E, cells), torch.int32)
    prev = behind((E, 8, 2), torch.int32) if p.expert == im.BELIEF else None
    _lib.torch_ops().feature_episodes(sd, lens.to(DEV), feat, lab, grid, prev, p.expert, p.n_agents, p.side, p.view_range, p.keep, p.regrow,
                                      p.lookahead, p.model.mode, p.model.sense16, p.every, p.moving, list(p.model.dx), list(p.model.dy))
    return feat.cpu(), lab.cpu(), grid.cpu(), None if prev is None else prev.cpu()


def same(got, want):
    assert same_bits(got[0], want[0]), "feat"
    assert torch.equal(got[1], want[1]), "labels"
    assert torch.equal(got[2], want[2]), "grid_out"
    assert (got[3] is None and want[3] is None) or torch.equal(got[3], want[3]), "prev_out"


@pytest.mark.parametrize("E, T, n, side", SHAPES)
def test_coverage_episode_kernel_equals_the_definition(E, T, n, side):
    p = coverage_params(n, side, min(7, side))
    s, lens = rows_for(E, T, n, side, 1), mixed_lens(E, T, E + 8)
    want = go.feature_episodes_torch(s, lens, p)
    same(run_kernel(s, lens, p), want)
    same(run_kernel(s, lens, p, misalign=True), want)
    only = run_kernel(s, lens, p, labels=False, outputs=False)   # NULL labels: the choose step is skipped, the features are the same
    assert same_bits(only[0], want[0]) and only[1] is None and only[2] is None and only[3] is None
    assert bool(want[0].any()) or int(lens.max()) == 0


@pytest.mark.parametrize("E, T, n, side", SHAPES)
@pytest.mark.parametrize("mode", ["walk", "evade"])
def test_belief_episode_kernel_equals_the_definition(E, T, n, side, mode):
    s, lens = rows_for(E, T, n, side, 2), mixed_lens(E, T, E + 1)
    for speed, every, sense in ((1.0, 3, 10.0), (3.5, 1, 2.0 * side)):
        p = belief_params(n, side, min(7, side), mode, speed, sense, every)
        want = go.feature_episodes_torch(s, lens, p)
        same(run_kernel(s, lens, p), want)
    same(run_kernel(s, lens, p, misalign=True), want)
    only = run_kernel(s, lens, p, labels=False)   # NULL labels with grid_out and prev_out
    assert same_bits(only[0], want[0]) and only[1] is None and torch.equal(only[2], want[2]) and torch.equal(only[3], want[3])


@pytest.mark.parametrize("kind", ["coverage", "belief"])
def test_episode_kernel_on_spoilt_rows_and_every_lens(kind):
    E, T, n, side = 6, 7, 3, 50
    p = coverage_params(n, side, 7) if kind == "coverage" else belief_params(n, side, 7, "evade", 1.0, 10.0, 1)
    for S, spoil in ((4 * n, True), (4 * n + 9, True), (4 * n + 8, False)):
        s = state_rows(E, T, n, S, 3 + S, spoil=spoil)
        for lens in (mixed_lens(E, T, 5), torch.zeros(E, dtype=torch.int32), torch.full((E,), T, dtype=torch.int32)):
            same(run_kernel(s, lens, p), go.feature_episodes_torch(s, lens, p))
        lens = mixed_lens(E, T, 5)
        poisoned = s.clone()
        for e in range(E):
            poisoned[e, int(lens[e]):] = float("nan")   # rows past lens change nothing: feature +0.0, label 0
        got = run_kernel(poisoned, lens, p)
        same(got, go.feature_episodes_torch(s, lens, p))
        assert all(same_bits(got[0][e, int(lens[e]):], torch.zeros_like(got[0][e, int(lens[e]):])) for e in range(E))
    for look, vr in ((0, 7), (50, 0)):   # every probe on the agent; a radius that holds at most one cell
        q = coverage_params(n, side, vr, lookahead=look) if kind == "coverage" else belief_params(n, side, vr, "walk", 1.0, 0.0, 1, lookahead=look)
        same(run_kernel(s, lens, q), go.feature_episodes_torch(s, lens, q))


# ---- 3. the episode kernel against the labeller and against the acting class --------------------------------------------------------

@pytest.mark.parametrize("kind", ["coverage", "evade"])
def test_episode_kernel_equals_the_labeller_and_what_grid_agents_traced(kind):
    B, n, T = 33, 3, 120
    motion = None if kind == "coverage" else mo.TargetMotion(mode="evade", speed=0.5, sense=10.0, every=3, seed=3)
    # (a) on test_gpu_imitate's recorded batches: labels, grid and positions are cs_label_episodes'
    args, batch = recorded("flight_easy", B, motion)
    lens = im.episode_lens(batch)
    assert int(lens.min()) < T and int(lens.max()) == T
    filt = cs.CoverageAgents(args, batch=2 * B, device=DEV) if kind == "coverage" else cs.BeliefAgents(args, motion=motion, batch=2 * B, device=DEV)
    p = im.expert_params(filt)
    s = batch["s"].float().contiguous()
    feat, lab, grid, prev = go.feature_episodes_hip(s, lens, p)
    want = im.label_episodes_hip(s, lens, p)
    assert torch.equal(lab, want[0]) and torch.equal(grid, want[1]) and (prev is None and want[2] is None or torch.equal(prev, want[2]))
    assert same_bits(go.feature_episodes(filt, batch), feat) and bool(feat.any())
    # (b) a batch flown by GridAgents itself: what it observed at every live step is what the episode kernel computes afterwards
    args = cs.make_env_args("flight_easy", n_agents=n, target_num=1)
    args.time_limit = T
    seeds = np.arange(B, dtype=np.uint32) + 500
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds) if motion is None else cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion)
    cs.apply_env_info(args, env)
    im.get_bc_args(args, seed=5)
    filt = cs.CoverageAgents(env) if kind == "coverage" else cs.BeliefAgents(env)
    agents = go.GridAgents(args, filt, seed=2)
    trace = torch.full((T, B, n, 16), -1.0, device=DEV)
    episode = cs.EpisodeCollector(env).generate_episodes(policy=agents.policy(epsilon=0.4, evaluate=False, trace=trace), init=True)[0]
    lens = im.episode_lens(episode)
    feat, lab = go.feature_episodes(filt, episode, labels=True)
    live = (torch.arange(T, device=DEV).view(1, T) < lens.view(B, 1)).view(B, T, 1, 1).expand_as(feat)
    traced = trace.transpose(0, 1)
    assert same_bits(torch.where(live, feat, torch.zeros_like(feat)), torch.where(live, traced, torch.zeros_like(traced)))
    assert not feat[~live].any() and int(lens.max()) == T and bool(feat[live].any())
    assert torch.equal(lab, im.label_episodes(type(filt)(env), episode))
    assert episode["u"].unique().numel() == 3   # (an untrained network explores with epsilon 0.4: the flight is not one circle)


# ---- 4. the policy forward with features ---------------------------------------------------------------------------------------------

# The bound is max(TOL, K * the float32 torch module's error against the same float64 twin), DESIGN.md section 23's rule; every
# step starts all three from the kernel's own hidden state and last actions (test_gpu_policy.py keeps its two recurrences together
# the same way).  K = 2 x the worst kernel / twin ratio measured on an MI355X (1.90, at n = 3, B = 1, step 1, where the twin lands
# 2.7e-7 from float64); the figures are in the test's docstring and in DESIGN.md section 24.  Every measured error lies below TOL.
K = 3.8


def args_for(n):
    a = cs.make_env_args("flight_easy", n_agents=n)
    a.n_actions, a.obs_shape, a.rnn_hidden_dim, a.conv, a.last_action, a.reuse_network = 3, 4, 64, False, True, True
    return a


class CaseFeatures(go.GridAgents):
    """GridAgents whose features are the case's own (written into self.features before the call), not the filter's: the launch
    under test is the policy forward."""

    def observe(self, state, moved=False):
        return self.features


@pytest.mark.parametrize("n, B", [(3, 1), (3, 37), (8, 129)])
def test_grid_agents_forward_matches_the_float64_twin(n, B):
    """Measured on an MI355X over the three cases and six steps, largest absolute error of (q, hidden) against float64: kernel
    2.7e-7 to 8.7e-7, float32 module 2.3e-7 to 1.07e-6, ratio 0.64 to 1.90 (worst per case: 1.90, 1.07, 1.03).  K = 2 x 1.90."""
    a = args_for(n)
    net, feats, obs = forward_case(a, n, B, seed=FORWARD_SEED)
    filt = cs.CoverageAgents(a, batch=B, device=DEV)
    agents = CaseFeatures(a, filt, net=net)
    m64, m32 = twin_of(net, torch.float64), twin_of(net, torch.float32)
    state = torch.zeros(B, 4 * n, device=DEV)
    worst = 0.0
    for t in range(feats.shape[0]):
        h_in, last = agents.hidden.cpu(), agents.actions.cpu().clone()
        agents.features.copy_(feats[t])
        act = agents.choose_action(obs[t].to(DEV), state, want_q=True).cpu().clone()
        q64, h64 = twin_step(m64, feats[t], obs[t], last, h_in, n, 3)
        q32, h32 = twin_step(m32, feats[t], obs[t], last, h_in, n, 3)
        got = torch.cat([agents.q.cpu().view(B * n, 3).double(), agents.hidden.cpu().double()], 1)
        want, twin = torch.cat([q64, h64], 1), torch.cat([q32.double(), h32.double()], 1)
        err, twin_err = float((got - want).abs().max()), float((twin - want).abs().max())
        worst = max(worst, err / max(twin_err, 1e-30))
        print(f"grid forward n={n} B={B} t={t}: kernel {err:.3g} twin {twin_err:.3g} ratio {err / max(twin_err, 1e-30):.3g}")
        assert err <= max(TOL, K * twin_err), (t, err, twin_err)
        share, clear = clear_fraction(q64)
        assert share >= 0.9, (t, share)
        assert bool((act.view(-1) == q64.argmax(1))[clear].all())
    print(f"grid forward n={n} B={B}: worst ratio {worst:.3g}")


# ---- 5. the learner and the loop -----------------------------------------------------------------------------------------------------

def featured_batch(B=32, T=50, n=3, seed=7):
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = T
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 900)
    cs.apply_env_info(args, env)
    im.get_bc_args(args, seed=seed)
    filt = cs.CoverageAgents(env)
    episode = cs.EpisodeCollector(env).generate_episodes(policy=cs.random_policy(torch.Generator(DEV).manual_seed(1)), init=True)[0]
    episode["f"], labels = go.feature_episodes(filt, episode, labels=True)
    episode["u_expert"] = labels.unsqueeze(3).float()
    return args, episode


def test_fused_and_torch_grid_learners_agree_and_lower_the_loss():
    args, batch = featured_batch()
    fused, plain = go.GridImitationLearner(args, device=DEV, unroll="fused"), go.GridImitationLearner(args, device=DEV, unroll="torch")
    for (k, a), (_, b) in zip(fused.eval_rnn.state_dict().items(), plain.eval_rnn.state_dict().items()):
        assert torch.equal(a, b), k
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = fused.learn(batch)   # no host synchronisation
    finally:
        torch.cuda.set_sync_debug_mode(0)
    lf, lt = [float(first)], [float(plain.learn(batch))]
    for _ in range(19):
        lf.append(float(fused.learn(batch)))
        lt.append(float(plain.learn(batch)))
    rel = [abs(a - b) / abs(b) for a, b in zip(lf, lt)]
    print(f"grid bc learn fused vs torch: first {rel[0]:.3g}, worst of 20 {max(rel):.3g}; loss {lf[0]:.4f} -> {lf[9]:.4f} -> {lf[-1]:.4f}; "
          f"agreement {float(fused.last_stats[1]):.3f}")
    assert rel[0] <= 1e-4 and max(rel) <= 1e-3
    assert lf[9] < lf[0] and lt[9] < lt[0]


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("expert_kind", ["own", "forecast"])
def test_distil_grid_for_two_iterations(moving, expert_kind, tmp_path):
    B, n = 33, 3
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = 40
    seeds = np.arange(B, dtype=np.uint32) + 40
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, seed=4)
    env = cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion) if moving else cs.BatchedFlightEnv(args, batch=B, seeds=seeds)
    cs.apply_env_info(args, env)
    im.get_bc_args(args, seed=3)
    args.model_dir = str(tmp_path) + "/"
    if expert_kind == "own":   # labels and features from one launch
        expert = filt = cs.CoverageAgents(env)
    else:                      # a planner over a separate belief filter
        expert, filt = cs.ForecastAgents(env, motion=motion), cs.BeliefAgents(env, motion=motion)
    learner = go.GridImitationLearner(args, device=DEV)
    agents = go.GridAgents(args, filt, net=learner.eval_rnn, seed=1)
    ring = go.FeatureRing(args, 4 * B, device=DEV)
    before = agents.packed.clone()
    history = go.distil_grid(env, expert, filt, learner, agents, ring, iterations=2, updates=3, sample=16, generator=torch.Generator(DEV).manual_seed(2))
    assert [h["flown_by"] for h in history] == ["expert", "student"] and ring.current_size == 2 * B
    assert all(set(h) == {"iteration", "flown_by", "loss", "agreement", "targets_find"} for h in history)
    assert all(np.isfinite(h["loss"]) and 0 <= h["agreement"] <= 1 and 0 <= h["targets_find"] <= args.target_num for h in history)
    first = {k: v[:B] for k, v in ring.buffers.items()}
    second = {k: v[B:2 * B] for k, v in ring.buffers.items()}
    live = (1 - first["padded"]).unsqueeze(3)
    assert torch.equal(first["u_expert"] * live, first["u"] * live)                          # iteration 0: the actions the expert flew
    fresh_filter = type(filt)(env, motion=motion) if type(filt) is cs.BeliefAgents else type(filt)(env)
    for part in (first, second):
        assert same_bits(part["f"], go.feature_episodes(fresh_filter, part)) and bool(part["f"].any())
    relabel = type(expert)(env, motion=motion) if expert_kind == "forecast" else type(expert)(env)
    assert torch.equal(second["u_expert"].squeeze(3).long(), im.label_episodes(relabel, second, impl="rows"))
    assert not torch.equal(second["u_expert"], second["u"])                                  # ... of the student's own flight
    agents.check_weights()
    assert not torch.equal(agents.packed, before)                                            # agents act with the synced weights
    fresh = go.GridAgents(args, filt, net=learner.eval_rnn, seed=1)
    assert torch.equal(fresh.packed, agents.packed)


# ---- 6. refusals and synchronisation -------------------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    B, n, side = 4, 3, 50
    ops = _lib.torch_ops()
    state, grid = rows(B, n, 57, 0).to(DEV), torch.full((B, side * side), 1234, dtype=torch.int32, device=DEV)
    feat = torch.full((B, n, 16), -7.0, device=DEV)
    bad = [dict(state=state.double()), dict(state=state.cpu()), dict(state=state[:, ::2]), dict(state=state[:, :11].contiguous()), dict(grid=grid.long()),
           dict(grid=grid.cpu()), dict(grid=grid[:, :-1].contiguous()), dict(grid=grid.t().contiguous().t()), dict(feat=feat.double()), dict(feat=feat.cpu()),
           dict(feat=feat[:, :2].contiguous()), dict(feat=feat.transpose(1, 2).contiguous().transpose(1, 2))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.grid_features(kw.get("state", state), kw.get("grid", grid), kw.get("feat", feat), n, side, 7, 7)
    for pos, value in ((0, 9), (1, 65), (2, 65), (3, side + 1)):
        a = [n, side, 7, 7]
        a[pos] = value
        with pytest.raises(RuntimeError, match="grid_features"):
            ops.grid_features(state, grid, feat, *a)
    assert bool((feat == -7.0).all()) and bool((grid == 1234).all())
    E, T = 4, 3
    p = belief_params(n, side, 7, "evade", 1.0, 10.0, 1)
    s, lens = env_rows(E, T, n).to(DEV), torch.full((E,), T, dtype=torch.int32, device=DEV)
    f4 = torch.full((E, T, n, 16), -7.0, device=DEV)
    labels = torch.full((E, T, n), -7, dtype=torch.int64, device=DEV)
    g2, prev = torch.full((E, side * side), 1234, dtype=torch.int32, device=DEV), torch.full((E, 8, 2), 99, dtype=torch.int32, device=DEV)
    ints = (1, n, side, 7, KEEP, 8, 7, p.model.mode, p.model.sense16, 1, 1, list(p.model.dx), list(p.model.dy))
    bad = [dict(s=s.double()), dict(s=s.cpu()), dict(s=s[:, :, ::2]), dict(lens=lens.long()), dict(lens=lens.cpu()), dict(lens=lens[:-1].contiguous()),
           dict(feat=f4.double()), dict(feat=f4.cpu()), dict(feat=f4[:, :, :2].contiguous()), dict(feat=f4.transpose(2, 3).contiguous().transpose(2, 3)),
           dict(labels=labels.int()), dict(labels=labels.cpu()), dict(labels=labels[:, :, :2].contiguous()), dict(grid=g2.long()), dict(grid=g2.cpu()),
           dict(grid=g2[:, :-1].contiguous()), dict(prev=prev.long()), dict(prev=prev.cpu()), dict(prev=prev[:, :3].contiguous())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.feature_episodes(kw.get("s", s), kw.get("lens", lens), kw.get("feat", f4), kw.get("labels", labels), kw.get("grid", g2),
                                 kw.get("prev", prev), *ints)
    for pos, value in ((0, 2), (1, 9), (2, 65), (3, 65), (4, 65537), (5, 0), (6, side + 1), (7, 2), (8, 2049), (9, 0), (10, 2), (11, [0] * 15),
                       (12, [1025] + [0] * 15)):
        a = list(ints)
        a[pos] = value
        with pytest.raises(RuntimeError, match="feature_episodes"):
            ops.feature_episodes(s, lens, f4, labels, g2, prev, *a)
    assert bool((f4 == -7.0).all()) and bool((labels == -7).all()) and bool((g2 == 1234).all()) and bool((prev == 99).all())


def test_neither_call_synchronises_and_both_run_on_the_current_stream():
    E, T, n, side = 16, 6, 3, 50
    s = env_rows(E, T, n)
    filt = cs.BeliefAgents(cs.make_env_args("flight_easy"), motion=mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), batch=E, device=DEV)
    batch = {"s": s.to(DEV), "padded": torch.zeros(E, T, 1, device=DEV)}
    batch["padded"][3, 4:] = 1.0
    state = s[:, 0].contiguous()
    grid = grids("belief", state, n, side, 7, 7)
    sd, gd = state.to(DEV), grid.to(DEV)
    go.feature_episodes(filt, batch)   # (the op library is loaded)
    go.grid_features(sd, gd, n, side, 7)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(stream):
            feat, labels = go.feature_episodes(filt, batch, labels=True)
            one = go.grid_features(sd, gd, n, side, 7)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    stream.synchronize()
    want = go.feature_episodes_torch(s, im.episode_lens(batch).cpu(), im.expert_params(filt))
    assert same_bits(feat.cpu(), want[0]) and torch.equal(labels.cpu(), want[1])
    assert same_bits(one.cpu(), go.grid_features_torch(state, grid, n, side, 7))
