"""GPU tests of the PPO learner: cs_gae against a NumPy float32 statement of its evaluation order (bit for bit), float64 and
the returns kernel; cs_ppo_loss against float64 autograd of its torch twin; the fused learner against REINFORCE's recorded
gradient, against the torch unroll over 20 learn calls, and in the loops collect -> learn -> act and save -> resume."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import runner as rn
from cooperative_search_amd.learner import PPOLearner, PPOPolicyLoss, episode_returns, gae, get_ppo_args, ppo_logp
from ppo_util import (BETAS, CLIP, EPSILONS, LOSS_SHAPES, WIDTH_BETA, WIDTH_CASES, gae_case, gae_f32, gae_f64, loss_case, rel_err,
                      twin)
from test_gpu_learner_pg import acts_with, first_step_q, no_sync, replay, to_dev
from test_gpu_resume import flat
from test_learner_ppo_cpu import check_reinforce_identity
from test_learner_pg_cpu import load_pg_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"

# cs_ppo_loss against float64: its error may be K times the error of float32 autograd of the torch twin on the same case
# (floor 1e-6).  K = twice the worst kernel / twin ratio measured on an MI355X.  Measured over the 20 cases below: the kernel
# 4.3e-8 to 3.0e-7 from float64, the twin 5.8e-8 to 3.1e-7, ratio 0.44 to 3.24 for dlogits (worst: E, T, n = 3, 5, 3, epsilon 0,
# no entropy term) and 0.45 to 3.14 for the stats.  Every one of these errors lies under the floor, so the floor is the bar
# that binds at these sizes; K speaks for cases whose float32 error is larger.
K = 6.5


# ---- cs_gae -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E,T", [(E, T) for E in (1, 7, 257) for T in (1, 2, 9)] + [(32, 200)])
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
def test_gae_kernel_matches_float32_order_float64_and_the_returns_kernel(E, T, lam):
    r, term, pad, v, vn = gae_case(E, T, seed=E * 1000 + T)
    dev = lambda x: torch.from_numpy(x).to(DEV)
    got = [x.cpu().numpy() for x in gae(dev(r), dev(term), dev(pad), dev(v), dev(vn), 0.99, lam)]
    again = [x.cpu().numpy() for x in gae(dev(r), dev(term), dev(pad), dev(v), dev(vn), 0.99, lam)]
    want32, want64 = gae_f32(r, term, pad, v, vn, 0.99, lam), gae_f64(r, term, pad, v, vn, 0.99, lam)
    for g, a, w32, w64 in zip(got, again, want32, want64):
        assert g.shape == (E, T)
        assert np.array_equal(g.view(np.uint32), a.view(np.uint32))   # no atomics: reruns are bit-identical
        assert np.array_equal(g.view(np.uint32), w32.view(np.uint32)), float(np.abs(g - w32).max())
        assert float(np.abs(g - w64).max()) <= 1e-5 * max(1.0, float(np.abs(w64).max()))
        assert np.all(g[pad == 1] == 0)
    if lam == 1.0:   # no critic: the advantages are REINFORCE's returns, from the kernel pinned to the reference
        zero = torch.zeros(E, T, device=DEV)
        adv, ret = gae(dev(r), dev(term), dev(pad), zero, zero, 0.99, 1.0)
        want = episode_returns(dev(r), dev(term), dev(pad), None, 0.99)
        assert torch.equal(adv.view(torch.int32), want.view(torch.int32))
        assert torch.equal(ret, want)


# ---- cs_ppo_loss --------------------------------------------------------------------------------------------------------------

def kernel_loss(x, epsilon, beta, eps_on_device=False):
    """PPOPolicyLoss on the case's float32 tensors, without a host synchronisation -> (loss, stats [4], dlogits, logp of the
    no-grad mode) on the CPU."""
    c = lambda k: x[k].float().to(DEV)
    logits = c("logits").requires_grad_(True)
    eps = torch.tensor([epsilon], device=DEV) if eps_on_device else epsilon
    avail, u, old_logp, adv, mask = c("avail"), x["u"].to(DEV), c("old_logp"), c("adv"), c("mask")

    def run():
        inv_count = 1 / (logits.shape[2] * mask.sum())
        loss, stats = PPOPolicyLoss.apply(logits, avail, u, old_logp, adv, mask, CLIP, beta, eps, inv_count)
        loss.backward()
        return loss.detach(), stats, logits.grad, ppo_logp(logits, avail, u, mask, eps)
    return tuple(t.cpu() for t in no_sync(run))


@pytest.mark.parametrize("E,T,n", LOSS_SHAPES)
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("beta", BETAS)
def test_ppo_loss_kernel_matches_float64_autograd(E, T, n, epsilon, beta):
    check_ppo_loss_kernel(E, T, n, epsilon, beta, 3)


@pytest.mark.parametrize("A,E,T,n,epsilon", WIDTH_CASES)
def test_ppo_loss_kernel_matches_float64_autograd_at_every_width(A, E, T, n, epsilon):
    """k_ppo_loss<A> for the widths ppo_launch instantiates besides 3 (2, 4, 5 and 8 of 2 .. 8), under the bar of the test above,
    unchanged: max(1e-6, K * twin error), K = 6.5, both errors against the float64 twin.  With A = 2 the rows of the (5, 13, 3)
    shape that lose an action keep a single one: p = 1, entropy 0, log p = 0.
    Measured on an MI355X over the 16 cases: dlogits kernel 9.3e-8 to 3.7e-7 from float64, twin 6.6e-8 to 3.6e-7, ratio 0.74 to
    2.96 (worst: A = 8, E, T, n = 3, 5, 3, epsilon 0); stats kernel 2.3e-8 to 2.0e-7, twin 1.6e-8 to 2.2e-7, ratio 0.53 to 4.16
    (worst: A = 8, E, T, n = 5, 13, 3, epsilon 0.3, kernel 1.0e-7 against a twin of 2.5e-8).  Every error lies under the 1e-6
    floor, which binds here as it does for A = 3; per width the worst dlogits error is 2.6e-7 (A = 2), 3.7e-7 (4), 2.7e-7 (5),
    2.7e-7 (8)."""
    check_ppo_loss_kernel(E, T, n, epsilon, WIDTH_BETA, A)


def check_ppo_loss_kernel(E, T, n, epsilon, beta, A):
    x = loss_case(E, T, n, epsilon, beta, A)   # asserts the conditions on the case from the float64 yardstick
    loss64, stats64, d64, count64 = x["want"]
    loss32, stats32, d32, _ = twin(x, torch.float32, epsilon, beta)
    loss, stats, d, logp = kernel_loss(x, epsilon, beta, eps_on_device=epsilon > 0)
    vec = lambda l, s: torch.cat([s[:2].double(), s[3:].double(), l.reshape(1).double()])   # policy loss, entropy, KL, loss
    err_d, twin_d = rel_err(d, d64), rel_err(d32, d64)
    err_s, twin_s = rel_err(vec(loss, stats), vec(loss64, stats64)), rel_err(vec(loss32, stats32), vec(loss64, stats64))
    print(f"ppo_loss A={A} E={E} T={T} n={n} eps={epsilon} beta={beta}: dlogits kernel {err_d:.3g} twin {twin_d:.3g} ratio "
          f"{err_d / max(twin_d, 1e-30):.3g}; stats kernel {err_s:.3g} twin {twin_s:.3g} ratio {err_s / max(twin_s, 1e-30):.3g}")
    assert err_d <= max(1e-6, K * twin_d)
    assert err_s <= max(1e-6, K * twin_s)
    live_rows = float(x["mask"].sum()) * n
    assert int(round(float(stats[2]) * live_rows)) == count64   # the clip fraction: the same rows, counted
    assert abs(float(stats[2]) - count64 / live_rows) <= 1e-6
    dead = (x["mask"] == 0).reshape(E, T, 1, 1).expand_as(d)
    assert bool((d[dead] == 0).all()) and bool((logp[dead[..., 0]] == 0).all())   # rows with mask 0: exactly zero
    # reruns are bit-identical, from a scalar epsilon as from a device one; the no-grad mode writes the full mode's logp
    loss2, stats2, d2, logp2 = kernel_loss(x, epsilon, beta)
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32)) and torch.equal(stats.view(torch.int32), stats2.view(torch.int32))
    assert torch.equal(loss, loss2) and torch.equal(logp.view(torch.int32), logp2.view(torch.int32))
    ops = cs.lib.torch_ops()
    c = lambda k, *shape: x[k].float().to(DEV).reshape(*shape).contiguous()
    R = E * T * n
    full_logp, scratch = torch.empty(R, device=DEV), torch.empty(4 * ((R + 255) // 256), device=DEV)
    ops.ppo_loss(c("logits", R, A), c("avail", R, A), x["u"].to(DEV).reshape(R), c("old_logp", R), c("adv", E * T), c("mask", E * T),
                 R, n, A, CLIP, beta, epsilon, None, (1 / (n * c("mask", E * T).sum())).reshape(1), torch.empty(R, A, device=DEV),
                 full_logp, torch.empty(4, device=DEV), scratch)
    assert torch.equal(full_logp.cpu().view(torch.int32), logp.reshape(R).view(torch.int32))
    live = (x["mask"] > 0).reshape(E, T, 1).expand(E, T, n)
    from cooperative_search_amd.learner import action_prob, log_pi_taken   # float64 log pi(u) of the yardstick's policy
    want_logp = log_pi_taken(action_prob(x["logits"], x["avail"], epsilon), x["u"], live.double())
    assert float((logp.double() - want_logp)[live].abs().max()) <= 1e-5


def test_ppo_kernels_refuse_bad_arguments():
    ops = cs.lib.torch_ops()
    z, zl = torch.zeros(4, 5, device=DEV), torch.zeros(12, dtype=torch.int64, device=DEV)
    out = lambda: torch.empty(4, 5, device=DEV)
    with pytest.raises(RuntimeError, match="v_next"):
        ops.gae(z, z, z, z, z[:, :4].contiguous(), 4, 5, 0.99, 0.95, out(), out())
    with pytest.raises(RuntimeError, match="float32"):
        ops.gae(z, z, z, z.double(), z, 4, 5, 0.99, 0.95, out(), out())
    lg, m = torch.zeros(12, 3, device=DEV), torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError, match="avail"):
        ops.ppo_loss(lg, lg[:, :2].contiguous(), zl, None, None, m, 12, 3, 3, 0.2, 0.0, 0.0, None, None, None, torch.empty(12, device=DEV),
                     None, None)
    with pytest.raises(RuntimeError, match="u must be"):
        ops.ppo_loss(lg, lg, zl.int(), None, None, m, 12, 3, 3, 0.2, 0.0, 0.0, None, None, None, torch.empty(12, device=DEV), None, None)
    with pytest.raises(RuntimeError, match="scratch"):   # the full mode needs every output
        ops.ppo_loss(lg, lg, zl, torch.zeros(12, device=DEV), m, m, 12, 3, 3, 0.2, 0.0, 0.0, None, m[:1].clone(),
                     torch.empty(12, 3, device=DEV), None, torch.empty(4, device=DEV), None)
    L = cs.lib.load()
    p = C.c_void_p(z.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.cs_gae(p, p, p, p, p, 4, 0, 0.99, 0.95, p, p, stream)   # T = 0: refused before any launch
    assert rc != 0 and L.cs_learn_last_error().decode().startswith("cs_gae: bad argument")
    rc = L.cs_gae(p, None, p, p, p, 4, 5, 0.99, 0.95, p, p, stream)
    assert rc != 0 and b"cs_gae" in L.cs_learn_last_error()
    rc = L.cs_ppo_loss(p, None, p, None, None, p, 12, 3, 3, 0.2, 0.0, 0.0, None, None, None, p, None, None, 0, stream)
    assert rc != 0 and L.cs_learn_last_error().decode().startswith("cs_ppo_loss: bad argument")
    rc = L.cs_ppo_loss(p, p, p, p, p, p, 12, 3, 3, 0.2, 0.0, 0.0, None, p, p, None, p, p, 0, stream)   # no room for the partials
    assert rc != 0 and b"scratch" in L.cs_learn_last_error()


# ---- the fused learner --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx():
    return load_pg_fixture()


def test_reduced_fused_ppo_is_reinforce(fx):
    check_reinforce_identity(fx, DEV, "fused", to_batch=to_dev, run=no_sync)


def ppo_fields(args, seed, **over):
    get_ppo_args(args, seed=seed)
    args.alg = "ppo"
    for k, v in over.items():
        setattr(args, k, v)
    return args


def collected(env_name, n, episodes, compact=False):
    """(args, 20 batches): episodes of a random policy, as test_fused_and_torch_learners_agree_over_20_steps collects them; or
    (compact) 20 samples of map-once episodes of a fresh acting network."""
    if not compact:
        args, rb, g = replay(env_name, n, episodes=64 if env_name == "flight_easy" else 8, seed=11, alg="reinforce")
        return args, [rb.sample(episodes, generator=g) for _ in range(20)]
    args = cs.make_env_args(env_name, n_agents=n)
    args.time_limit = 40
    env = cs.BatchedFlightEnv(args, batch=8)
    cs.apply_env_info(args, env)
    ppo_fields(args, 11)
    ring = cs.CompactReplayBuffer(args, 8)
    torch.manual_seed(21)
    cs.EpisodeCollector(env).generate_episodes(agents=cs.FusedAgents(args, 8, seed=9), evaluate=False, into=ring, compact=True)
    g = torch.Generator(DEV).manual_seed(11)
    return args, [ring.sample(episodes, generator=g) for _ in range(20)]


@pytest.mark.parametrize("env_name,n,E,compact,steps", [("flight_easy", 3, 32, False, 100), ("flight_easy", 5, 32, False, 100),
                                                         ("flight", 3, 4, False, 40), ("flight", 3, 4, True, None)])
def test_fused_and_torch_ppo_agree_over_20_learn_calls(env_name, n, E, compact, steps):
    """Two epochs per call.  The advantages are left as they are (ppo_norm_adv off): at ratio 1 the policy loss is minus their
    mean, which standardising makes zero by construction -- there would be no relative error to speak of.  `steps`: learn on
    the first that many steps of every episode (max_episode_len; the map-once episodes are 40 steps long): the torch twin's
    step loop costs 20 calls x 3 passes x T, and no kernel takes another path at a larger T.
    Measured: the value losses are equal (the critic's path is the same torch code in both); policy loss and entropy agree
    to 1.9e-7 over the 20 calls -- the centred advantage magnifies nothing here, so the plain bars hold."""
    args, batches = collected(env_name, n, E, compact)
    ppo_fields(args, 11, ppo_epochs=2, ppo_norm_adv=False)
    fused, ref = PPOLearner(args, device=DEV, unroll="fused"), PPOLearner(args, device=DEV, unroll="torch")
    lf = torch.stack([no_sync(lambda: fused.learn(b, steps, epsilon=0.3)) for b in batches]).cpu()   # [20, 2, 5]
    lt = torch.stack([ref.learn(b, steps, epsilon=0.3) for b in batches]).cpu()
    assert torch.isfinite(lf).all() and torch.isfinite(lt).all()
    rel = (lf - lt).abs() / lt.abs()
    print(f"ppo 20 calls {env_name} n={n} E={E} compact={compact}: call 0 epoch 0 policy {float(rel[0, 0, 0]):.3g} value "
          f"{float(rel[0, 0, 4]):.3g}; worst policy {float(rel[..., 0].max()):.3g} value {float(rel[..., 4].max()):.3g} entropy "
          f"{float(rel[..., 1].max()):.3g}")
    # from the same parameters (call 0, epoch 0) 1e-4; over the 20 calls the existing bar of the QMIX / DOP / REINFORCE tests
    assert float(rel[0, 0, 0]) <= 1e-4 and float(rel[0, 0, 4]) <= 1e-4, (lf[0], lt[0])
    assert float(rel[..., 4].max()) <= 1e-3, (lf[..., 4], lt[..., 4])
    assert float(rel[..., 0].max()) <= 1e-3, (lf[..., 0], lt[..., 0])
    assert float(rel[..., 1].max()) <= 1e-3
    assert torch.equal(lf[:, 0, 2], torch.zeros(20)) and torch.equal(lf[:, 0, 3], torch.zeros(20))   # epoch 0: ratio exactly 1


def test_one_learn_call_lowers_the_surrogate():
    """Four epochs on one fixed batch of 32 collected episodes: the policy loss of the last epoch lies below that of epoch 0
    (which is ~0: standardised advantages at ratio 1).  On the CPU (unroll='torch', the recorded batch of the learner
    fixtures, seeds 1 to 3) the drop is ~1e-3 after three steps, four orders above float32's noise in that mean."""
    args, rb, g = replay("flight_easy", 3, episodes=64, seed=11, alg="reinforce")
    ppo_fields(args, 1, ppo_epochs=4)
    learner, batch = PPOLearner(args, device=DEV), rb.sample(32, generator=g)
    stats = no_sync(lambda: learner.learn(batch, epsilon=0.0)).cpu()
    print("ppo surrogate over 4 epochs:", stats[:, 0].tolist())
    assert stats.shape == (4, 5) and bool(torch.isfinite(stats).all())
    assert float(stats[3, 0]) < float(stats[0, 0]) - 1e-4


def test_ppo_collect_learn_act():
    """PPO on-policy: a softmax FusedAgents collects -> learn on the returned episode dict -> sync_weights -> act."""
    B, n = 64, 3
    args = cs.make_env_args("flight_easy", n_agents=n)
    env = cs.BatchedFlightEnv(args, batch=B)
    cs.apply_env_info(args, env)
    ppo_fields(args, 5)
    learner = PPOLearner(args, device=DEV)
    agents = cs.FusedAgents(args, B, net=learner.eval_rnn, seed=1)
    assert agents.softmax
    col = cs.EpisodeCollector(env)
    q0, _ = first_step_q(env, agents, B, n)
    stats, actions = [], []
    for _ in range(3):
        episode, _, _, _ = col.generate_episodes(agents=agents, epsilon=args.epsilon, evaluate=False)
        assert episode is not None and episode["o"].shape[:2] == (B, args.episode_limit)
        actions.append(episode["u"][:, 0].clone())
        stats.append(no_sync(lambda: learner.learn(episode, epsilon=args.epsilon)))
        agents.sync_weights()
    agents.check_weights()
    q1, obs = first_step_q(env, agents, B, n)
    q_ref = acts_with(learner.eval_rnn, agents, obs, B, n)
    assert all(bool(torch.isfinite(x).all()) for x in stats)
    assert torch.isfinite(q1).all() and not torch.equal(q0, q1)
    assert float((q1.reshape(B * n, -1) - q_ref).abs().max()) <= 1e-4
    assert len(torch.unique(actions[0])) > 1   # sampled from the softmax, not the argmax of one fresh network


def test_a_resumed_ppo_run_equals_the_uninterrupted_one(tmp_path):
    """Runner(alg='ppo') at B = 8: three epochs, save_state, two more -- against a fresh Runner (other env seeds) that loads
    the state and runs the same two.  ppo_minibatches = 2: the permutation draws come from the device generator that the
    state carries.  Parameters, optimizer states and result lists are equal bit for bit."""
    def make(root, seed0):
        args = cs.make_env_args("flight_easy", n_agents=3)
        env = cs.BatchedFlightEnv(args, batch=8, seeds=np.arange(8, dtype=np.uint32) + seed0)
        cs.apply_env_info(args, env)
        ppo_fields(args, 17, ppo_minibatches=2, ppo_epochs=2, evaluate_cycle=2, save_cycle=4, evaluate_epoch=8)
        args.model_dir, args.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
        return rn.Runner(env, args)

    def outcome(r):
        out = {}
        flat("learner", rn.learner_state(r.learner), out)
        return out, (list(r.win_rates), list(r.episode_rewards), list(r.targets_find)), (r.epoch, r.train_steps)

    first = make(str(tmp_path / "a"), 101)
    assert isinstance(first.learner, PPOLearner) and first.buffer is None and first.agents.softmax
    first.run(0, n_epoch=3)
    path = str(tmp_path / "state.pt")
    first.save_state(path)
    first.run(0, n_epoch=5)
    second = make(str(tmp_path / "b"), 40000)
    second.load_state(path)
    assert (second.epoch, second.train_steps) == (3, 3)
    second.run(0, n_epoch=5)
    (want, want_res, want_counts), (got, got_res, got_counts) = outcome(first), outcome(second)
    assert want_counts == got_counts == (5, 5)
    assert sorted(want) == sorted(got)
    for k in want:
        assert torch.equal(want[k], got[k]), k
    assert want_res == got_res and len(want_res[0]) == 3
    saved = sorted(os.listdir(second.model_path))   # the checkpoint of train step 4, written after the resume
    assert len(saved) == 2 and saved[0].endswith("_critic_net_params.pkl") and saved[1].endswith("_rnn_net_params.pkl")
