"""CPU tests of the PPO learner (cooperative-search_amd/learner.py, csrc/ppo.h): the C ABI and the op layer carry cs_gae and
cs_ppo_loss; gae_torch against a NumPy float32 statement of the kernel's evaluation order, a float64 evaluation and REINFORCE's
returns; the torch-unroll learner against REINFORCE's gradient on the reference's recorded batch (which pins it to the
reference's own learn steps); ppo_policy_loss_torch, the yardstick of the GPU tests, in float32 against itself in float64;
checkpoints, learner state and the driver."""
import os
import types

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import runner as rn
from cooperative_search_amd.learner import PPOLearner, ReinforceLearner, ValueCritic, gae_torch, get_ppo_args, returns_torch
from learn_util import record
from ppo_util import (BETAS, EPSILONS, LOSS_SHAPES, WIDTH_BETA, WIDTH_CASES, gae_case, gae_f32, gae_f64, loss_case, ppo_args, rel_err,
                      twin)
from test_learner_pg_cpu import load_pg_fixture, pg_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_registered():
    hdr = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    assert "int cs_gae(" in hdr and "int cs_ppo_loss(" in hdr and "#define CS_ABI_VERSION 7 " in hdr
    L = _lib.load()
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    for name in ("cs_gae", "cs_ppo_loss"):
        assert name in _lib.EXPORTS and getattr(L, name).argtypes is not None, name
    assert len(L.cs_gae.argtypes) == 12 and len(L.cs_ppo_loss.argtypes) == 20
    ops = _lib.torch_ops()
    assert hasattr(ops, "gae") and hasattr(ops, "ppo_loss")
    z = torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="GPU"):   # no device here: CPU tensors are refused, not dereferenced
        ops.gae(z, z, z, z, z, 3, 4, 0.99, 0.95, torch.zeros(3, 4), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ppo_loss(torch.zeros(12, 3), torch.zeros(12, 3), torch.zeros(12, dtype=torch.int64), None, None, torch.zeros(4), 12, 3,
                     3, 0.2, 0.0, 0.0, None, None, None, torch.zeros(12), None, None)
    # host-side argument checks: no launch, the error names the entry point
    assert L.cs_gae(None, None, None, None, None, 0, 0, 0.99, 0.95, None, None, None) != 0
    assert L.cs_learn_last_error().startswith(b"cs_gae: bad argument")
    assert L.cs_ppo_loss(*[None] * 6, 0, 3, 3, 0.2, 0.0, 0.0, *[None] * 6, 0, None) != 0
    assert L.cs_learn_last_error().startswith(b"cs_ppo_loss: bad argument")


@pytest.mark.parametrize("E,T", [(1, 1), (7, 2), (7, 9), (32, 200)])
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
def test_gae_torch_matches_the_float32_order_and_float64(E, T, lam):
    r, term, pad, v, vn = gae_case(E, T, seed=E * 1000 + T)
    t = torch.from_numpy
    adv, ret = (x.numpy() for x in gae_torch(t(r), t(term), t(pad), t(v), t(vn), 0.99, lam))
    for got, want32, want64 in zip((adv, ret), gae_f32(r, term, pad, v, vn, 0.99, lam), gae_f64(r, term, pad, v, vn, 0.99, lam)):
        assert np.array_equal(got.view(np.uint32), want32.view(np.uint32)), float(np.abs(got - want32).max())
        assert float(np.abs(got - want64).max()) <= 1e-5 * max(1.0, float(np.abs(want64).max()))
        assert np.all(got[pad == 1] == 0)


@pytest.mark.parametrize("E,T", [(1, 1), (7, 9), (32, 200)])
def test_gae_without_a_critic_is_the_reinforce_return(E, T):
    r, term, pad, _, _ = gae_case(E, T, seed=E + T)
    t = torch.from_numpy
    zero = torch.zeros(E, T)
    adv, ret = gae_torch(t(r), t(term), t(pad), zero, zero, 0.99, 1.0)
    want = returns_torch(t(r), t(term), t(pad), 0.99).numpy()
    assert np.array_equal(adv.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ret.numpy(), want)


@pytest.fixture(scope="module")
def fx():
    return load_pg_fixture()


def identity_args(meta, **over):
    """PPO reduced to REINFORCE: one epoch on the whole batch, no entropy bonus, raw advantages, lambda = 1 (the critic's last
    layer is zeroed by the caller, so V = 0 and the advantage is the return)."""
    env = vars(pg_args(meta, "reinforce"))
    fields = dict(ppo_epochs=1, ppo_minibatches=1, ppo_entropy=0.0, ppo_norm_adv=False, gae_lambda=1.0, lr_actor=env["lr_actor"])
    fields.update(over)
    return ppo_args(env, fields.pop("seed", env["seed"]), **fields)


def zero_value_head(learner):
    with torch.no_grad():
        learner.critic.fc3.weight.zero_()
        learner.critic.fc3.bias.zero_()


def check_actor_grads(learner, want, bar):
    """check_grads of test_learner_pg_cpu for the actor: |dg| <= bar * max(|g|, 1e-3 |g_all|) per tensor."""
    g_all = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in want.values())))
    have = {"rnn." + k: p.grad for k, p in learner.eval_rnn.named_parameters()}
    assert set(k for k, g in have.items() if g is not None) == set(want)
    for k, w in want.items():
        d = float(np.linalg.norm((have[k].detach().cpu().double().numpy() - w).ravel()))
        assert d <= bar * max(float(np.linalg.norm(w.ravel())), 1e-3 * g_all), (k, d)


def check_reinforce_identity(fx, device, unroll, to_batch=lambda b: b, run=lambda fn: fn()):
    """The actor's gradient of the reduced PPO against ReinforceLearner's on the same batch and seed and against the
    reference's recorded REINFORCE gradient, both at 1e-4; epoch 0's ratio is 1: nothing clipped, no KL."""
    meta, batch, init, steps = fx
    ppo = PPOLearner(identity_args(meta), device=device, unroll=unroll)
    pg = ReinforceLearner(pg_args(meta, "reinforce"), device=device, unroll=unroll)
    for (k, p), q in zip(ppo.eval_rnn.named_parameters(), pg.eval_rnn.parameters()):
        assert torch.equal(p, q), k   # the same initial actor
        assert np.array_equal(p.detach().cpu().numpy(), init["rnn." + k]), k
    zero_value_head(ppo)
    b = to_batch({k: v.copy() for k, v in batch.items()})
    stats = run(lambda: ppo.learn(b, epsilon=meta["epsilon"]))
    pg.learn(to_batch({k: v.copy() for k, v in batch.items()}), epsilon=meta["epsilon"])
    assert float(ppo.last_actor_grad_norm) < ppo.args.grad_norm_clip   # the clip left the gradient as it was
    check_actor_grads(ppo, {"rnn." + k: p.grad.detach().cpu().double().numpy() for k, p in pg.eval_rnn.named_parameters()}, 1e-4)
    check_actor_grads(ppo, record(steps["reinforce"][0], "grad"), 1e-4)
    stats = stats.cpu()
    assert stats.shape == (1, 5) and bool(torch.isfinite(stats).all())
    assert float(stats[0, 2]) == 0.0 and abs(float(stats[0, 3])) <= 1e-6
    return stats


def test_reduced_ppo_is_reinforce(fx):
    check_reinforce_identity(fx, "cpu", "torch")


@pytest.mark.parametrize("E,T,n", LOSS_SHAPES)
@pytest.mark.parametrize("epsilon", EPSILONS)
@pytest.mark.parametrize("beta", BETAS)
def test_loss_twin_in_float32_matches_float64(E, T, n, epsilon, beta):
    """The GPU tests' yardstick is sound: float32 autograd of ppo_policy_loss_torch against float64, at float32's precision
    (1e-5 relative: sums of up to ~1000 terms of ~6e-8 each, amplified by the 1 / p of the taken action)."""
    check_loss_twin(E, T, n, epsilon, beta, 3)


@pytest.mark.parametrize("A,E,T,n,epsilon", WIDTH_CASES)
def test_loss_twin_in_float32_matches_float64_at_every_width(A, E, T, n, epsilon):
    """The cases of the GPU test of the other row widths (ppo_util.WIDTH_CASES, each with its committed seed): loss_case's
    conditions hold for every one of them, and the yardstick is sound at that width too.  With A = 2 and unavailable actions
    some live rows keep a single action: probability 1 and no entropy whatever the logits, so the row's gradient is zero up to
    float64's rounding of the softmax's backward (a few 1e-18 against entries of 1e-2)."""
    x = check_loss_twin(E, T, n, epsilon, WIDTH_BETA, A)
    assert tuple(x["logits"].shape) == (E, T, n, A) and int(x["u"].max()) == A - 1 and int(x["u"].min()) == 0
    live = (x["mask"] > 0).reshape(E, T, 1).expand(E, T, n)
    single = (x["avail"].sum(-1) == 1) & live
    assert bool(single.any()) == (A == 2 and x["unavailable"])
    if bool(single.any()):
        assert float(x["want"][2][single].abs().max()) <= 1e-15 and float(x["want"][2].abs().max()) >= 1e-3


def check_loss_twin(E, T, n, epsilon, beta, A):
    x = loss_case(E, T, n, epsilon, beta, A)
    loss64, stats64, d64, count64 = x["want"]
    loss32, stats32, d32, count32 = twin(x, torch.float32, epsilon, beta)
    assert bool(torch.isfinite(d64).all()) and float(d64.norm()) > 0
    assert rel_err(d32, d64) <= 1e-5
    assert rel_err(torch.cat([stats32, loss32.reshape(1)]), torch.cat([stats64, loss64.reshape(1)])) <= 1e-5
    assert count32 == count64
    dead = (x["mask"] == 0).reshape(E, T, 1, 1).expand_as(d64)
    assert bool((d64[dead] == 0).all()) and bool((d32[dead] == 0).all())   # padded rows: exactly zero
    return x


def small_ppo(tmp_path, fx, **over):
    return PPOLearner(identity_args(fx[0], model_dir=str(tmp_path) + "/", **over), device="cpu", unroll="torch")


def test_checkpoints_and_learner_state_round_trip(fx, tmp_path):
    meta, batch = fx[0], fx[1]
    lr = small_ppo(tmp_path, fx, ppo_epochs=2, ppo_minibatches=2, ppo_norm_adv=True, ppo_entropy=0.01)
    lr.learn({k: v.copy() for k, v in batch.items()}, epsilon=0.0)
    lr.save_model(7)
    assert sorted(os.listdir(lr.model_dir)) == ["7_critic_net_params.pkl", "7_rnn_net_params.pkl"]
    assert lr.model_dir.endswith("_ppo_3a{}t(AM{}TM{})".format(
        meta["target_num"], meta["agent_mode"], meta["target_mode"]))
    # the actor's file is REINFORCE's: the reference's loader (and Runner.replay) read it
    pg = ReinforceLearner(pg_args(meta, "reinforce", seed=1), device="cpu", unroll="torch")
    pg.load_model(os.path.join(lr.model_dir, "7_rnn_net_params.pkl"))
    assert all(torch.equal(p, q) for p, q in zip(pg.eval_rnn.parameters(), lr.eval_rnn.parameters()))
    other = small_ppo(tmp_path, fx, seed=meta["reinforce"]["args"]["seed"] + 1)
    other.load_model(os.path.join(lr.model_dir, "7_rnn_net_params.pkl"), os.path.join(lr.model_dir, "7_critic_net_params.pkl"))
    for net in ("eval_rnn", "critic"):
        assert all(torch.equal(p, q) for p, q in zip(getattr(other, net).parameters(), getattr(lr, net).parameters())), net

    sd = rn.learner_state(lr)
    assert sorted(sd["modules"]) == ["critic", "eval_rnn"] and sorted(sd["optimizers"]) == ["critic_optimizer", "rnn_optimizer"]
    path = os.path.join(str(tmp_path), "state.pt")
    torch.save(sd, path)
    third = small_ppo(tmp_path, fx, seed=3, ppo_epochs=2, ppo_minibatches=2, ppo_norm_adv=True, ppo_entropy=0.01)
    rn.load_learner_state(third, torch.load(path, map_location="cpu", weights_only=True))
    # the same state -> the same next step, bit for bit (parameters, both Adam states, the permutation draw)
    outs = []
    for learner in (lr, third):
        torch.manual_seed(99)
        outs.append(learner.learn({k: v.copy() for k, v in batch.items()}, epsilon=0.0))
    assert torch.equal(outs[0], outs[1]) and outs[0].shape == (2, 5)
    for net in ("eval_rnn", "critic"):
        assert all(torch.equal(p, q) for p, q in zip(getattr(third, net).parameters(), getattr(lr, net).parameters())), net
    with pytest.raises(ValueError, match="learner state"):
        rn.load_learner_state(ReinforceLearner(pg_args(meta, "reinforce"), device="cpu", unroll="torch"), sd)


def test_args_and_critic():
    a = get_ppo_args(types.SimpleNamespace(), seed=5)
    want = dict(off_policy=False, rnn_hidden_dim=64, critic_dim=128, lr_actor=5e-4, lr_critic=1e-3, gae_lambda=0.95, ppo_clip=0.2,
                ppo_epochs=4, ppo_minibatches=1, ppo_entropy=0.01, ppo_norm_adv=True, epsilon=0, anneal_epsilon=0, min_epsilon=0,
                epsilon_anneal_scale="epoch", grad_norm_clip=10, n_episodes=1, evaluate_cycle=200, save_cycle=500, gamma=0.99,
                optimizer="Adam", seed=5)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    assert get_ppo_args(types.SimpleNamespace(gamma=0.9, optimizer="RMS")).gamma == 0.9
    critic = ValueCritic(57, a)
    assert [tuple(p.shape) for p in critic.parameters()] == [(128, 57), (128,), (128, 128), (128,), (1, 128), (1,)]
    assert critic(torch.zeros(2, 5, 57)).shape == (2, 5, 1)
    assert cs.PPOLearner is PPOLearner and cs.get_ppo_args is get_ppo_args


def test_runner_accepts_ppo(tmp_path):
    """The driver with alg = 'ppo' and its parts passed in (the stubs of test_runner_cpu): on-policy epochs, one learn call
    each with env 0's epsilon, the acting network repacked after each, both checkpoint files named for resume."""
    from test_runner_cpu import FIXTURE, Recorder, SAVE_FILES, make_args
    assert rn.LEARNERS["ppo"] is PPOLearner and rn._RESUME["ppo"] == ("rnn", "critic")
    SAVE_FILES.setdefault("ppo", ("rnn", "critic"))
    cfg = dict(FIXTURE["configs"][0], alg="reinforce")
    args = make_args(cfg, str(tmp_path), n_epoch=3, evaluate_cycle=2, save_cycle=1)
    get_ppo_args(args)
    args.alg = "ppo"
    args.n_epoch, args.evaluate_cycle, args.save_cycle = 3, 2, 1
    rec = Recorder(args)
    r = rec.runner()
    r.run(0)
    assert [ev for ev in rec.trace if ev[0] == "learn"] == [["learn", k, True, 1] for k in range(3)]
    assert rec.agents.syncs == 3 and r.buffer is None
    assert r.model_path.endswith("_ppo_3a{}t(AM{}TM{})".format(args.target_num, args.agent_mode, args.target_mode))
    saved = sorted(os.listdir(r.model_path))
    assert saved and all(f.endswith(("_rnn_net_params.pkl", "_critic_net_params.pkl")) for f in saved)
    args.load_model = True
    rec2 = Recorder(args)
    rec2.runner()
    newest = max(int(f.split("_")[0]) for f in saved)
    assert rec2.loaded == [[f"{newest}_rnn_net_params.pkl", f"{newest}_critic_net_params.pkl"]]
    with pytest.raises(ValueError, match="ppo"):
        rn.Runner(types.SimpleNamespace(batch=1, device="cpu"), make_args(cfg, str(tmp_path), alg="coma"))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_learn_call_lowers_the_surrogate_on_the_recorded_batch(fx, seed):
    """Four epochs with the default settings on the recorded batch: epoch 0's policy loss is ~0 (standardised advantages at
    ratio 1) and three steps later it lies ~1e-3 lower, whatever the seed -- the margin the GPU test of the same name rests on."""
    meta, batch = fx[0], fx[1]
    lr = PPOLearner(ppo_args(vars(pg_args(meta, "reinforce")), seed), device="cpu", unroll="torch")
    stats = lr.learn({k: v.copy() for k, v in batch.items()}, epsilon=0.0)
    assert abs(float(stats[0, 0])) <= 1e-6 and float(stats[3, 0]) < -3e-4
    assert bool((stats[1:, 4] < stats[:-1, 4]).all())   # the critic's loss falls too
