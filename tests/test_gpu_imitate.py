"""GPU tests of the imitation module (csrc/label.h, csrc/bc_loss.h, imitate.py): the one-launch labeller
against its definition and against the per-step kernels it replaces, the loss kernel against a float64 twin, the learner
fused against torch, and the distillation loop end to end."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import baseline as bl
from cooperative_search_amd import imitate as im
from cooperative_search_amd import motion as mo
from imitate_util import (BC_CASES, KEEP, bc_f64, bc_inputs, bc_twin, belief_params, coverage_params, mixed_lens, rel_err, state_rows)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1, 50), (3, 7, 3, 50), (65, 5, 5, 50), (7, 9, 8, 64), (5, 6, 2, 7)]   # (E, T, n, side)


def env_rows(E, T, n):
    """float32 [E, T, 4n + 45]: the get_state() rows of a flight_easy env flown T steps at random, on the CPU."""
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=E, seeds=np.arange(E, dtype=np.uint32) + 13 * n)
    g = torch.Generator().manual_seed(E + n)
    rows = []
    for _ in range(T):
        rows.append(env.get_state().cpu())
        env.step(torch.randint(0, 3, (E, n), generator=g).cuda())
    return torch.stack(rows, 1).contiguous()


def run_kernel(s, lens, p, misalign=False, outputs=True):
    """One cs_label_episodes launch on CPU inputs -> CPU outputs; misalign: s, labels, grid_out and prev_out each start one
    element behind a 16-byte boundary (the scalar paths), through the op itself."""
    E, T, n, cells = s.shape[0], s.shape[1], p.n_agents, p.side * p.side
    if not misalign:
        sd, ld = s.cuda(), lens.cuda()
        keep_s, keep_l = sd.clone(), ld.clone()
        out = im.label_episodes_hip(sd, ld, p, grid_out=outputs, prev_out=outputs)
        assert torch.equal(ld, keep_l) and torch.equal(sd.view(torch.int32), keep_s.view(torch.int32))   # bit-unchanged
        return tuple(None if x is None else x.cpu() for x in out)

    def behind(shape, dtype):
        buf = torch.zeros(int(np.prod(shape)) + 1, dtype=dtype, device=DEV)
        view = buf[1:].view(*shape)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view
    sd = behind(s.shape, torch.float32)
    sd.copy_(s)
    labels, grid = behind((E, T, n), torch.int64), behind((E, cells), torch.int32)
    prev = behind((E, 8, 2), torch.int32) if p.expert == im.BELIEF else None
    _lib.torch_ops().label_episodes(sd, lens.cuda(), labels, grid, prev, p.expert, p.n_agents, p.side, p.view_range, p.keep, p.regrow,
                                    p.lookahead, p.model.mode, p.model.sense16, p.every, p.moving, list(p.model.dx), list(p.model.dy))
    return labels.cpu(), grid.cpu(), None if prev is None else prev.cpu()


def same(got, want):
    assert torch.equal(got[0], want[0]), "labels"
    assert torch.equal(got[1], want[1]), "grid_out"
    assert (got[2] is None and want[2] is None) or torch.equal(got[2], want[2]), "prev_out"


def rows_for(E, T, n, side, seed):
    """Env rows where the env has this side, hand-made ones otherwise; S = 4n + 45 (odd: the scalar loads) or 4n + 4 (float4)."""
    if side == 50 and n <= 5:
        return env_rows(E, T, n)
    return state_rows(E, T, n, 4 * n + 4, seed)


# ---- 1. the labeller against its definition ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("E, T, n, side", SHAPES)
@pytest.mark.parametrize("regrow", [8, 16])
def test_coverage_labeller_equals_the_definition(E, T, n, side, regrow):
    p = coverage_params(n, side, min(7, side), regrow)
    s, lens = rows_for(E, T, n, side, 1), mixed_lens(E, T, E + regrow)
    want = im.label_episodes_torch(s, lens, p)
    same(run_kernel(s, lens, p), want)
    same(run_kernel(s, lens, p, misalign=True), want)
    assert int(want[0].max()) > 0 or E * T * n < 4


@pytest.mark.parametrize("E, T, n, side", SHAPES)
@pytest.mark.parametrize("mode", ["walk", "evade"])
def test_belief_labeller_equals_the_definition(E, T, n, side, mode):
    s, lens = rows_for(E, T, n, side, 2), mixed_lens(E, T, E + 1)
    for speed, every, sense in ((0.25, 1, 0.0), (1.0, 3, 10.0), (3.5, 1, 2.0 * side), (float(side), 3, 10.0)):
        p = belief_params(n, side, min(7, side), mode, speed, sense, every)
        want = im.label_episodes_torch(s, lens, p)
        same(run_kernel(s, lens, p), want)
    same(run_kernel(s, lens, p, misalign=True), want)


@pytest.mark.parametrize("expert", ["coverage", "belief"])
def test_labeller_on_spoilt_rows_wide_rows_and_every_lens(expert):
    E, T, n, side = 6, 7, 3, 50
    make = (lambda: coverage_params(n, side, 7)) if expert == "coverage" else (lambda: belief_params(n, side, 7, "evade", 1.0, 10.0, 1))
    p = make()
    for S, spoil in ((4 * n, True), (4 * n + 9, True), (4 * n + 8, False)):   # S = 4n exactly, S > 4n odd, S > 4n a multiple of 4
        s = state_rows(E, T, n, S, 3 + S, spoil=spoil)
        for lens in (mixed_lens(E, T, 5), torch.zeros(E, dtype=torch.int32), torch.full((E,), T, dtype=torch.int32)):
            want = im.label_episodes_torch(s, lens, p)
            same(run_kernel(s, lens, p), want)
        lens = mixed_lens(E, T, 5)
        poisoned = s.clone()
        for e in range(E):
            poisoned[e, int(lens[e]):] = float("nan")   # rows past lens change nothing and get label 0
        got = run_kernel(poisoned, lens, p)
        same(got, im.label_episodes_torch(s, lens, p))
        assert all(not got[0][e, int(lens[e]):].any() for e in range(E))
    labels, grid, prev = run_kernel(s, lens, p, outputs=False)   # NULL grid_out and prev_out
    assert grid is None and prev is None and torch.equal(labels, im.label_episodes_torch(s, lens, p)[0])


# ---- 2. the labeller against the per-step kernels, on recorded batches ----------------------------------------------------------

def recorded(variant, B, motion):
    """One batch flown by CoverageAgents ++ one flown at random, on a fresh env each; one target, so that some episodes end
    early (a win) and others run to the time limit."""
    args = cs.make_env_args(variant, n_agents=3, target_num=1)
    args.time_limit = 120
    parts = []
    for k, flown in enumerate(("coverage", "random")):
        seeds = np.arange(B, dtype=np.uint32) + 500 + 97 * k
        env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds) if motion is None else cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion)
        policy = cs.CoverageAgents(env).policy() if flown == "coverage" else cs.random_policy(torch.Generator(DEV).manual_seed(5))
        parts.append(cs.EpisodeCollector(env).generate_episodes(policy=policy, init=True)[0])
    return args, {k: torch.cat([parts[0][k], parts[1][k]]) for k in ("s", "padded")}


@pytest.mark.parametrize("variant, B", [("flight_easy", 33), ("flight", 9)])
@pytest.mark.parametrize("kind", ["coverage", "walk", "evade"])
def test_labeller_equals_the_per_step_kernels_on_recorded_batches(variant, B, kind):
    motion = {"coverage": None, "walk": mo.TargetMotion(mode="walk", speed=0.5, every=1, seed=3),
              "evade": mo.TargetMotion(mode="evade", speed=0.5, sense=10.0, every=3, seed=3)}[kind]
    args, batch = recorded(variant, B, motion)
    E, T = 2 * B, 120
    lens = im.episode_lens(batch)
    print(f"{variant} {kind}: lens min {int(lens.min())} max {int(lens.max())}, {int((lens < T).sum())} of {E} ended early")
    assert int(lens.min()) < T and int(lens.max()) == T   # both trip-count cases on real rows
    expert = cs.CoverageAgents(args, batch=E, device=DEV) if kind == "coverage" else cs.BeliefAgents(args, motion=motion, batch=E, device=DEV)
    one = im.label_episodes(expert, batch, return_state=True)
    rows = im.label_episodes(expert, batch, impl="rows", return_state=True)
    assert len(one) == len(rows) == (2 if kind == "coverage" else 3)
    for a, b in zip(one, rows):
        assert torch.equal(a, b)
    assert bool((expert.grid == bl.FRESH).all())
    assert torch.equal(one[0], im.label_episodes(expert, batch, impl="hip"))
    assert one[0].unique().numel() == 3


# ---- 3. the loss kernel ------------------------------------------------------------------------------------------------------------

# The bound of every case is max(1e-6, K * the float32 torch twin's error against the same float64 twin), tests/ppo_util.py's
# protocol.  K = 2 x the worst kernel / twin ratio measured on an MI355X over BC_CASES (4.13, on the statistics of A = 2,
# (32, 50, 5) with unavailable actions, where the twin happens to land 1.6e-8 from float64); the measured ranges are in DESIGN.md
# section 23 and in test_bc_loss_kernel_matches_the_float64_twin's docstring.  Every measured error lies below the 1e-6 floor.
K = 8.3


def kernel_loss(x):
    z = x["logits"].float().to(DEV).requires_grad_(True)
    mask = x["mask"].float().to(DEV)
    n = z.shape[2]
    loss, stats = im.BCLoss.apply(z, x["avail"].float().to(DEV), x["labels"].to(DEV), mask, 1 / (n * mask.sum()))
    loss.backward()
    return loss.detach().cpu(), stats.cpu(), z.grad.cpu()


@pytest.mark.parametrize("E, T, n, A, unavailable", BC_CASES)
def test_bc_loss_kernel_matches_the_float64_twin(E, T, n, A, unavailable):
    """Measured on an MI355X over the 18 BC_CASES, relative Frobenius errors against float64: dlogits kernel 4.6e-8 to 7.3e-8,
    twin 4.1e-8 to 9.3e-8, ratio 0.74 to 1.40; statistics (loss, entropy) kernel 4.7e-9 to 1.6e-7, twin 1.2e-8 to 1.5e-7, ratio
    0.10 to 4.13 (both are a few float32 roundings of a mean: the ratio is noise around 1).  K = 2 x 4.13."""
    x = bc_inputs(E, T, n, A, unavailable)
    loss64, stats64, d64 = bc_f64(x["logits"].numpy(), x["avail"].numpy(), x["labels"].numpy(), x["mask"].numpy())
    stats64, d64 = torch.from_numpy(stats64), torch.from_numpy(d64)
    stats32, d32 = bc_twin(x, torch.float32)
    loss, stats, d = kernel_loss(x)
    cont = lambda st: st[[0, 2]]   # the loss and the entropy; the agreement is a count
    err_d, twin_d = rel_err(d, d64), rel_err(d32, d64)
    err_s, twin_s = rel_err(cont(stats), cont(stats64)), rel_err(cont(stats32), cont(stats64))
    print(f"bc_loss A={A} E={E} T={T} n={n} unavailable={unavailable}: dlogits kernel {err_d:.3g} twin {twin_d:.3g} ratio "
          f"{err_d / max(twin_d, 1e-30):.3g}; stats kernel {err_s:.3g} twin {twin_s:.3g} ratio {err_s / max(twin_s, 1e-30):.3g}")
    assert err_d <= max(1e-6, K * twin_d)
    assert err_s <= max(1e-6, K * twin_s)
    live_rows = float(x["mask"].sum()) * n
    assert abs(float(stats[1]) * live_rows - float(stats64[1]) * live_rows) <= 1e-6 * live_rows   # the agreement: the same rows, counted
    assert abs(float(stats[1]) - float(stats64[1])) <= 1e-6
    assert float(loss) == float(stats[0])
    dead = (x["mask"] == 0).reshape(E, T, 1, 1).expand_as(d)
    assert not d[dead].any()
    loss2, stats2, d2 = kernel_loss(x)
    assert torch.equal(stats, stats2) and torch.equal(d, d2)   # reruns are bit-identical


def test_bc_loss_backward_equals_autograd_through_the_definition():
    x = bc_inputs(5, 13, 3, 3, True)
    z = x["logits"].float().to(DEV)
    av, u, m = x["avail"].float().to(DEV), x["labels"].to(DEV), x["mask"].float().to(DEV)
    za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    la, sa = im.BCLoss.apply(za, av, u, m, 1 / (3 * m.sum()))
    lb, sb = im.bc_loss_torch(zb, av, u, m)
    (2.5 * la).backward()
    (2.5 * lb).backward()
    assert rel_err(za.grad.cpu(), zb.grad.cpu().double()) < 1e-5 and rel_err(sa.cpu(), sb.cpu().double()) < 1e-5
    assert not sa.requires_grad


# ---- 4. the learner ----------------------------------------------------------------------------------------------------------------

def labelled_batch(B=32, T=50, n=3, seed=7):
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = T
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 900)
    cs.apply_env_info(args, env)
    im.get_bc_args(args, seed=seed)
    expert = cs.CoverageAgents(env)
    episode = cs.EpisodeCollector(env).generate_episodes(policy=cs.random_policy(torch.Generator(DEV).manual_seed(1)), init=True)[0]
    episode["u_expert"] = im.label_episodes(expert, episode).unsqueeze(3).float()
    return args, env, expert, episode


def test_fused_and_torch_learners_agree_and_lower_the_loss():
    args, env, expert, batch = labelled_batch()
    fused, plain = im.ImitationLearner(args, device=DEV, unroll="fused"), im.ImitationLearner(args, device=DEV, unroll="torch")
    for (k, a), (_, b) in zip(fused.eval_rnn.state_dict().items(), plain.eval_rnn.state_dict().items()):
        assert torch.equal(a, b), k
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first = fused.learn(batch)   # no host synchronisation
    finally:
        torch.cuda.set_sync_debug_mode(0)
    lf, lt = [float(first)], [float(plain.learn(batch))]
    sf, st = [fused.last_stats.cpu()], [plain.last_stats.cpu()]
    for _ in range(19):
        lf.append(float(fused.learn(batch)))
        lt.append(float(plain.learn(batch)))
        sf.append(fused.last_stats.cpu())
        st.append(plain.last_stats.cpu())
    rel = [abs(a - b) / abs(b) for a, b in zip(lf, lt)]
    print(f"bc learn fused vs torch: first {rel[0]:.3g}, worst of 20 {max(rel):.3g}; loss {lf[0]:.4f} -> {lf[9]:.4f} -> {lf[-1]:.4f}; "
          f"agreement {float(sf[0][1]):.3f} -> {float(sf[-1][1]):.3f}")
    assert rel[0] <= 1e-4 and max(rel) <= 1e-3
    assert lf[9] < lf[0] and lt[9] < lt[0]   # ten updates on one fixed batch lower the loss
    assert abs(float(sf[-1][1]) - float(st[-1][1])) <= 0.01 and abs(float(sf[-1][2]) - float(st[-1][2])) <= 1e-3 * float(st[-1][2])


@pytest.mark.parametrize("moving", [False, True])
def test_distil_for_two_iterations(moving, tmp_path):
    B, n = 32, 3
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = 40
    seeds = np.arange(B, dtype=np.uint32) + 40
    motion = mo.TargetMotion(mode="evade", speed=1.0, sense=10.0, seed=4)
    env = cs.MovingTargetEnv(args, batch=B, seeds=seeds, target_motion=motion) if moving else cs.BatchedFlightEnv(args, batch=B, seeds=seeds)
    cs.apply_env_info(args, env)
    im.get_bc_args(args, seed=3)
    args.model_dir = str(tmp_path) + "/"
    expert = cs.BeliefAgents(env) if moving else cs.CoverageAgents(env)
    learner = im.ImitationLearner(args, device=DEV)
    agents = cs.FusedAgents(args, B, net=learner.eval_rnn, seed=1)
    ring = im.LabelledRing(args, 4 * B, device=DEV)
    before = agents.packed.clone()
    history = im.distil(env, expert, learner, agents, ring, iterations=2, updates=3, sample=16, generator=torch.Generator(DEV).manual_seed(2))
    assert [h["flown_by"] for h in history] == ["expert", "student"] and ring.current_size == 2 * B
    assert all(np.isfinite(h["loss"]) and 0 <= h["agreement"] <= 1 and 0 <= h["targets_find"] <= args.target_num for h in history)
    first = {k: v[:B] for k, v in ring.buffers.items()}
    second = {k: v[B:2 * B] for k, v in ring.buffers.items()}
    assert torch.equal(first["u_expert"], first["u"])                                   # iteration 0: the actions the expert flew
    rows = im.label_episodes(type(expert)(env), second, impl="rows")
    assert torch.equal(second["u_expert"].squeeze(3).long(), rows)                      # iteration 1: the rows path's labels
    assert not torch.equal(second["u_expert"], second["u"])                             # ... of the student's own flight
    agents.check_weights()
    assert not torch.equal(agents.packed, before)                                       # agents act with the synced weights
    fresh = cs.FusedAgents(args, B, net=learner.eval_rnn, seed=1)
    assert torch.equal(fresh.packed, agents.packed)
    path = learner.save_model(1, alg="reinforce")
    cs.get_reinforce_args(args, seed=3)
    reinforce = cs.ReinforceLearner(args, device=DEV)
    reinforce.load_model(path)
    for k, v in learner.eval_rnn.state_dict().items():
        assert torch.equal(reinforce.eval_rnn.state_dict()[k], v), k


# ---- 5. refusals and synchronisation ------------------------------------------------------------------------------------------------

def test_wrong_tensors_are_refused_before_anything_is_launched():
    E, T, n, side = 4, 3, 3, 50
    ops, p = _lib.torch_ops(), belief_params(n, side, 7, "evade", 1.0, 10.0, 1)
    s, lens = env_rows(E, T, n).cuda(), torch.full((E,), T, dtype=torch.int32, device=DEV)
    labels = torch.full((E, T, n), -7, dtype=torch.int64, device=DEV)
    grid = torch.full((E, side * side), 1234, dtype=torch.int32, device=DEV)
    prev = torch.full((E, 8, 2), 99, dtype=torch.int32, device=DEV)
    ints = (1, n, side, 7, KEEP, 8, 7, p.model.mode, p.model.sense16, 1, 1, list(p.model.dx), list(p.model.dy))
    bad = [dict(s=s.double()), dict(s=s.cpu()), dict(s=s[:, :, ::2]), dict(s=s[:, :, :4 * n - 1].contiguous()), dict(lens=lens.long()), dict(lens=lens.cpu()),
           dict(lens=lens[:-1].contiguous()), dict(labels=labels.int()), dict(labels=labels.cpu()), dict(labels=labels[:, :, :2].contiguous()),
           dict(labels=labels.transpose(1, 2).contiguous().transpose(1, 2)), dict(grid=grid.long()), dict(grid=grid.cpu()),
           dict(grid=grid[:, :-1].contiguous()), dict(prev=prev.long()), dict(prev=prev.cpu()), dict(prev=prev[:, :3].contiguous())]
    for kw in bad:
        with pytest.raises(RuntimeError, match="coopsearch"):
            ops.label_episodes(kw.get("s", s), kw.get("lens", lens), kw.get("labels", labels), kw.get("grid", grid), kw.get("prev", prev), *ints)
    for pos, value in ((0, 2), (1, 9), (2, 65), (3, 65), (4, 65537), (5, 0), (6, side + 1), (7, 2), (8, 2049), (9, 0), (10, 2), (11, [0] * 15),
                       (12, [1025] + [0] * 15)):
        a = list(ints)
        a[pos] = value
        with pytest.raises(RuntimeError, match="label_episodes"):
            ops.label_episodes(s, lens, labels, grid, prev, *a)
    assert bool((labels == -7).all()) and bool((grid == 1234).all()) and bool((prev == 99).all())
    z, av, u, mk = torch.zeros(6, 3, device=DEV), torch.ones(6, 3, device=DEV), torch.zeros(6, dtype=torch.int64, device=DEV), torch.ones(2, device=DEV)
    inv, dz, stt, sc = torch.ones(1, device=DEV), torch.full((6, 3), 5.0, device=DEV), torch.zeros(3, device=DEV), torch.zeros(3, device=DEV)
    for kw in (dict(z=z.double()), dict(av=av[:5]), dict(u=u.int()), dict(mk=mk.cpu()), dict(inv=inv.double()), dict(dz=dz[:, :2]), dict(stt=stt[:2]),
               dict(sc=sc[:2])):
        a = dict(dict(z=z, av=av, u=u, mk=mk, inv=inv, dz=dz, stt=stt, sc=sc), **kw)
        with pytest.raises(RuntimeError, match="coopsearch|cs_bc_loss"):
            ops.bc_loss(a["z"], a["av"], a["u"], a["mk"], 6, 3, 3, a["inv"], a["dz"], a["stt"], a["sc"])
    assert bool((dz == 5.0).all())


def test_a_labelling_call_never_synchronises_and_runs_on_the_current_stream():
    E, T, n = 16, 6, 3
    s = env_rows(E, T, n)
    expert = cs.BeliefAgents(cs.make_env_args("flight_easy"), motion=mo.TargetMotion(mode="evade", speed=1.0, sense=10.0), batch=E, device=DEV)
    batch = {"s": s.cuda(), "padded": torch.zeros(E, T, 1, device=DEV)}
    batch["padded"][3, 4:] = 1.0
    im.label_episodes(expert, batch)   # (the op library is loaded)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            out = im.label_episodes(expert, batch, return_state=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    side.synchronize()
    same(tuple(x.cpu() for x in out), im.label_episodes_torch(s, im.episode_lens(batch).cpu(), im.expert_params(expert)))
