"""CPU tests of the DOP and REINFORCE learners (cooperative-search_amd/learner.py) against the reference's own learn steps,
recorded by tests/golden/gen_learn_pg.py: the torch unroll (the reference's per-transition loops and its O(T^2) lambda-return,
over the same modules) reproduces the reference's initial parameters, gradients, pre-clip norms, Adam step, soft update,
returns and checkpoint files; the C ABI and the torch op layer carry cs_episode_returns."""
import json
import os
import types

import numpy as np
import pytest
import torch

from cooperative_search_amd import _lib
from cooperative_search_amd.learner import (DOPLearner, ReinforceLearner, get_dop_args, get_reinforce_args, returns_torch,
                                            td_lambda_torch)
from learn_util import GOLDEN, rebuild_batch, record


def load_pg_fixture():
    """(meta, the 11-key batch, initial parameters {"<module>.<name>": array}, {"dop": [step records], "reinforce": [...]})."""
    z = np.load(os.path.join(GOLDEN, "learn_pg_easy3.npz"))
    meta = json.loads(str(z["meta"]))
    batch = rebuild_batch(np.load(os.path.join(GOLDEN, meta["batch"])), meta["dop"]["args"]["n_actions"])
    init = {k[len("init_"):]: z[k] for k in z.files if k.startswith("init_")}
    steps = {alg: [dict(np.load(os.path.join(GOLDEN, f"learn_pg_easy3_{alg}_step{k}.npz"))) for k in range(meta["steps"])]
             for alg in ("dop", "reinforce")}
    return meta, batch, init, steps


def pg_args(meta, alg, **over):
    """The learner's namespace: the env fields and get_*_args values the fixture was recorded with."""
    a = dict(meta[alg]["args"])
    a.update(env=meta["env"], n_agents=meta["n_agents"], agent_mode=meta["agent_mode"], target_num=meta["target_num"],
             target_mode=meta["target_mode"], map_size=50)
    a.update(over)
    return types.SimpleNamespace(**a)


def make(alg, meta, device="cpu", unroll="torch", **over):
    cls = DOPLearner if alg == "dop" else ReinforceLearner
    return cls(pg_args(meta, alg, **over), device=device, unroll=unroll)


def named_params(learner, which="eval"):
    """{"<module>.<name>": parameter}: eval = actor / critic / mixer (DOP) or rnn (REINFORCE); target = critic / mixer."""
    if isinstance(learner, ReinforceLearner):
        mods = {"rnn": learner.eval_rnn} if which == "eval" else {}
    elif which == "eval":
        mods = {"actor": learner.actor, "critic": learner.eval_critic, "mixer": learner.eval_mixer_net}
    else:
        mods = {"critic": learner.target_critic, "mixer": learner.target_mixer_net}
    return {f"{m}.{k}": p for m, net in mods.items() for k, p in net.named_parameters()}


def groups(learner):
    """The parameter names of each gradient-clip call: DOP clips critic + mixer, then the actor; REINFORCE does not clip."""
    if isinstance(learner, ReinforceLearner):
        return [(None, [k for k in named_params(learner)])]
    names = named_params(learner)
    return [("last_critic_grad_norm", [k for k in names if not k.startswith("actor.")]),
            ("last_actor_grad_norm", [k for k in names if k.startswith("actor.")])]


def load_params(learner, ev, tg):
    dev = next(iter(named_params(learner).values())).device
    with torch.no_grad():
        for which, vals in (("eval", ev), ("target", tg)):
            for k, p in named_params(learner, which).items():
                p.copy_(torch.from_numpy(vals[k]).to(dev))


def start_state(learner, init, steps, k):
    """The parameters before learn call k: the initial ones, or those after call k-1 (Adam restarts: call 1 is a first step
    from the recorded state, as in test_learner_cpu)."""
    if k == 0:
        tg = {key[len("target_"):]: v for key, v in init.items() if key.startswith("target_")}
        load_params(learner, init, tg)
    else:
        load_params(learner, record(steps[k - 1], "eval"), record(steps[k - 1], "target"))


def norms_of(rec):
    return {"last_critic_grad_norm": float(rec["critic_grad_norm"]), "last_actor_grad_norm": float(rec["actor_grad_norm"])} \
        if "critic_grad_norm" in rec else {}


def check_grads(learner, want, norms, bar):
    """check_grads of test_learner_cpu per clip group: |dg| <= bar * max(|g|, 1e-3 |g_group|) per tensor; tensors without a
    recorded gradient have none here either; each pre-clip norm within bar relative."""
    have = {k: p.grad for k, p in named_params(learner).items()}
    assert set(k for k, g in have.items() if g is not None) == set(want), "parameters with a gradient differ"
    for norm_attr, names in groups(learner):
        g_all = float(np.sqrt(sum(float((want[k].astype(np.float64) ** 2).sum()) for k in names if k in want)))
        for k in names:
            if k not in want:
                continue
            g = have[k].detach().cpu().double().numpy()
            d = float(np.linalg.norm((g - want[k]).ravel()))
            floor = max(float(np.linalg.norm(want[k].ravel())), 1e-3 * g_all)
            assert d <= bar * floor, (k, d, floor)
        if norm_attr is not None:
            assert abs(float(getattr(learner, norm_attr)) - norms[norm_attr]) <= bar * norms[norm_attr], norm_attr


def lr_of(meta, alg, name):
    a = meta[alg]["args"]
    if alg == "reinforce":
        return a["lr_actor"]
    return a["lr"] if name.startswith("actor.") else a["critic_lr"]


def check_step(learner, alg, fx, bar, epsilon, to_batch=lambda b: b, run=lambda fn: fn()):
    """One learn step from the recorded initial state against the reference's first step: gradients and norms at `bar`, the
    Adam step, the soft update of the critic and mixer (DOP), and no target for the actor.  to_batch: the batch's conversion
    before the call; run: what the call runs under."""
    meta, batch, init, steps = fx
    tau = meta["dop"]["args"]["tau"]
    before = {k: p.detach().cpu().clone() for k, p in named_params(learner, "target").items()}
    b = to_batch({k: v.copy() for k, v in batch.items()})
    run(lambda: learner.learn(b, epsilon=epsilon))
    rec = steps[alg][0]
    grads = record(rec, "grad")
    check_grads(learner, grads, norms_of(rec), bar)
    want_eval = record(rec, "eval")
    for k, p in named_params(learner).items():
        have, w = p.detach().cpu().double().numpy(), want_eval[k].astype(np.float64)
        if k not in grads:
            assert np.array_equal(have, w), k   # no gradient: the parameter never moves
            continue
        g = np.abs(grads[k])
        big = g >= 1e-3 * g.max()
        # Adam's first step is ~lr * sign(g): where the gradient is at noise level its sign may flip
        assert np.abs(have - w)[big].max(initial=0.0) <= 1e-6, k
        assert np.abs(have - w)[~big].max(initial=0.0) <= 2 * lr_of(meta, alg, k), k
    want_target = record(rec, "target")
    assert set(named_params(learner, "target")) == set(want_target)   # critic and mixer only: the actor has no target
    for k, p in named_params(learner, "target").items():
        e = named_params(learner)[k].detach().cpu().double()
        want = tau * e + (1 - tau) * before[k].double()
        assert float((p.detach().cpu().double() - want).abs().max()) <= 1e-6, k
        assert float((p.detach().cpu().double() - torch.from_numpy(want_target[k]).double()).abs().max()) <= 1e-6, k


@pytest.fixture(scope="module")
def fx():
    return load_pg_fixture()


@pytest.mark.parametrize("alg", ["dop", "reinforce"])
def test_initial_parameters_are_the_references(fx, alg):
    meta, _, init, _ = fx
    lr = make(alg, meta)
    for k, p in named_params(lr).items():
        assert np.array_equal(p.detach().numpy(), init[k]), k
    for k, p in named_params(lr, "target").items():
        assert np.array_equal(p.detach().numpy(), init["target_" + k]), k
    if alg == "dop":
        names = {id(p): k for k, p in named_params(lr).items()}
        assert meta["dop"]["c_params"] == [names[id(p)] for p in lr.c_params]   # the order clip_grad_norm_ sums in
        assert meta["dop"]["actor_params"] == [names[id(p)] for p in lr.actor_params]


@pytest.mark.parametrize("alg", ["dop", "reinforce"])
@pytest.mark.parametrize("k", [0, 1])
def test_gradients_match_the_reference(fx, alg, k):
    meta, batch, init, steps = fx
    lr = make(alg, meta)
    start_state(lr, init, steps[alg], k)
    lr.learn({key: v.copy() for key, v in batch.items()}, epsilon=meta["epsilon"])
    check_grads(lr, record(steps[alg][k], "grad"), norms_of(steps[alg][k]), 1e-6)


@pytest.mark.parametrize("alg", ["dop", "reinforce"])
def test_one_learn_step_matches_the_reference(fx, alg):
    check_step(make(alg, fx[0]), alg, fx, 1e-6, fx[0]["epsilon"])


def test_returns_match_the_reference(fx):
    """The torch path's lambda-return (the O(T^2) n-step table) and REINFORCE return against the reference's, and the
    target mixer's q_total_target that feeds the lambda-return."""
    meta, batch, init, steps = fx
    b = {k: torch.from_numpy(v) for k, v in batch.items()}
    rec = steps["dop"][0]
    lam = rec["lambda_return"]
    assert all(np.array_equal(lam[..., 0], lam[..., j]) for j in range(lam.shape[-1]))   # the reference's repeat over agents
    a = meta["dop"]["args"]
    got = td_lambda_torch(b["r"], b["terminated"], b["padded"], torch.from_numpy(rec["q_total_target"]), a["gamma"], a["td_lambda"])
    assert float(np.abs(got.numpy() - lam[..., 0]).max()) <= 1e-6
    ret = steps["reinforce"][0]["returns"]
    got = returns_torch(b["r"], b["terminated"], b["padded"], meta["reinforce"]["args"]["gamma"])
    assert float(np.abs(got.numpy() - ret[..., 0]).max()) <= 1e-6

    lr = make("dop", meta)
    seen = []
    inner = lr.td_lambda_target
    lr.td_lambda_target = lambda bb, q: seen.append(q.detach().clone()) or inner(bb, q)
    lr.learn({key: v.copy() for key, v in batch.items()}, epsilon=meta["epsilon"])
    assert float((seen[0] - torch.from_numpy(rec["q_total_target"])).abs().max()) <= 1e-6


@pytest.mark.parametrize("alg", ["dop", "reinforce"])
def test_checkpoints_use_the_reference_names_and_round_trip(fx, alg, tmp_path):
    meta, batch = fx[0], fx[1]
    m = meta[alg]
    lr = make(alg, meta, model_dir=str(tmp_path) + "/")
    lr.learn({key: v.copy() for key, v in batch.items()}, epsilon=meta["epsilon"])
    lr.save_model(7)
    assert lr.model_dir == str(tmp_path) + "/" + m["model_dir"][len(m["args"]["model_dir"]):]
    assert sorted(os.listdir(lr.model_dir)) == sorted(f.format(num=7) for f in m["files"])
    paths = {f.split("_")[1]: os.path.join(lr.model_dir, f.format(num=7)) for f in m["files"]}   # actor / critic / mixer / rnn
    for mod, path in paths.items():
        sd = torch.load(path, map_location="cpu", weights_only=True)
        assert {k: list(v.shape) for k, v in sd.items()} == m["state_dicts"][mod], mod
    # the actor of DOP and REINFORCE's network are the checkpoints the reference ships (trained_easy3_* fixtures)
    shipped = np.load(os.path.join(GOLDEN, f"trained_easy3_{alg}.npz"))
    sd = torch.load(paths["actor" if alg == "dop" else "rnn"], map_location="cpu", weights_only=True)
    w = {k[2:]: shipped[k] for k in shipped.files if k.startswith("w_")}
    assert list(sd) == list(w) and all(list(sd[k].shape) == list(w[k].shape) for k in w)

    other = make(alg, meta, seed=m["args"]["seed"] + 1)
    if alg == "dop":
        other.load_model(paths["actor"], paths["critic"], paths["mixer"])
    else:
        other.load_model(paths["rnn"])
    for k, p in named_params(lr).items():
        assert torch.equal(named_params(other)[k], p), k
    for k, p in named_params(other, "target").items():   # targets copied from the loaded eval networks
        assert torch.equal(named_params(other)[k], p), k


@pytest.mark.parametrize("alg", ["dop", "reinforce"])
def test_args_are_the_references(fx, alg):
    want = fx[0][alg]["get_args"]
    fn = get_dop_args if alg == "dop" else get_reinforce_args
    a = fn(types.SimpleNamespace(), seed=5)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    assert a.seed == 5


def test_returns_op_is_registered_and_refuses_cpu_tensors():
    ops = _lib.torch_ops()
    assert hasattr(ops, "episode_returns")
    E, T = 3, 4
    z = torch.zeros(E, T)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.episode_returns(z, z, z, None, E, T, 0.99, 0.8, torch.zeros(E, T))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.episode_returns(z, z, z, z, E, T, 0.99, 0.8, torch.zeros(E, T))
    L = _lib.load()
    assert "cs_episode_returns" in _lib.EXPORTS and hasattr(L, "cs_episode_returns")
    # host-side argument checks: no launch, the error names the entry point
    rc = L.cs_episode_returns(None, None, None, None, 0, 0, 0.99, 0.8, None, None)
    assert rc != 0 and b"cs_episode_returns" in L.cs_learn_last_error()
