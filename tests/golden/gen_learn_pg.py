#!/usr/bin/env python3
"""Fixture of the reference's DOP and REINFORCE learners (policy/dop.py:89-130, policy/reinforce.py:63-99) for
tests/test_learner_pg_cpu.py and tests/test_gpu_learner_pg.py.

Runs ONLY in the build container (needs /root/reference) and contains no reference code: it imports the reference's own
`DOP`, `Reinforce` (policy/), `get_dop_args` and `get_reinforce_args` (common/arguments.py) at run time.

    1. The batch of tests/golden/learn_easy3.npz (flight_easy, 3 agents, 8 episodes, one of them won and zero-padded), rebuilt
       with learn_util.rebuild_batch.
    2. The reference `DOP(args)` and `Reinforce(args)` with cuda = False, a fixed args.seed, Adam and the get_*_args values;
       the initial parameters of every module, targets included.
    3. K = 2 calls of `learn` per algorithm on a copy of that batch (learn converts the batch in place) with epsilon = 0.3, so
       that the epsilon mix of the action probabilities is exercised.  After each: every parameter's .grad (absent when None),
       the eval and target parameters, and for DOP both pre-clip norms (critic + mixer, then actor: the values clip_grad_norm_
       returned, captured by wrapping it).  The first call also records DOP's q_total_target and lambda-return (the argument
       and result of _td_lambda_target) and REINFORCE's _get_returns, captured by wrapping those methods.

Stored (each file < 1 MB):
    learn_pg_easy3.npz                   init_<module>.<name> of both algorithms (modules actor, critic, mixer, target_critic,
                                         target_mixer; rnn); meta (JSON: args, the fields get_*_args set, state_dict keys
                                         and shapes, clip order, file names, epsilon)
    learn_pg_easy3_dop_step<k>.npz       grad_ / eval_ / target_<module>.<name>, critic_grad_norm, actor_grad_norm;
                                         step 0 also q_total_target [E][T][1], lambda_return [E][T][n]
    learn_pg_easy3_reinforce_step<k>.npz grad_ / eval_rnn.<name>; step 0 also returns [E][T][n]

    python tests/golden/gen_learn_pg.py
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import REF, import_reference  # noqa: E402
from learn_util import GOLDEN, rebuild_batch  # noqa: E402

K, SEED, EPSILON = 2, 20240611, 0.3


def ref_modules():
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        from common.arguments import get_dop_args, get_reinforce_args
        from policy.dop import DOP
        from policy.reinforce import Reinforce
    finally:
        os.chdir(cwd)
    return get_dop_args, get_reinforce_args, DOP, Reinforce


def fields_set_by(fn):
    """The fields a get_*_args function sets, on a namespace that keeps the caller's seed (show = True)."""
    a = argparse.Namespace(show=True, load_model=False, seed_idx=4)
    before = set(vars(a))
    fn(a)
    return {k: v for k, v in vars(a).items() if k not in before}


def sd(mods, pre):
    return {f"{pre}_{m}.{k}": v.detach().numpy().copy() for m, net in mods.items() for k, v in net.state_dict().items()}


def grads(mods):
    return {f"grad_{m}.{k}": p.grad.detach().numpy().copy() for m, net in mods.items() for k, p in net.named_parameters()
            if p.grad is not None}


def main():
    import torch
    import_reference()
    get_dop_args, get_reinforce_args, DOP, Reinforce = ref_modules()
    z = np.load(os.path.join(GOLDEN, "learn_easy3.npz"))
    qmeta = json.loads(str(z["meta"]))
    qa = qmeta["args"]
    batch = rebuild_batch(z, qa["n_actions"])
    T = batch["o"].shape[1]

    def base_args(alg):
        a = argparse.Namespace(env=qmeta["env"], map_size=50, target_num=qmeta["target_num"], target_mode=qmeta["target_mode"],
                               agent_mode=qmeta["agent_mode"], n_agents=qmeta["n_agents"], view_range=7, alg=alg,
                               last_action=True, reuse_network=True, gamma=0.99, optimizer="Adam", model_dir="./model/",
                               load_model=False, cuda=False, show=True, seed_idx=4, seed=SEED, conv=False,
                               n_actions=qa["n_actions"], state_shape=qa["state_shape"], obs_shape=qa["obs_shape"],
                               episode_limit=qa["episode_limit"])
        return a

    norms = []
    clip = torch.nn.utils.clip_grad_norm_

    def recording_clip(*a, **kw):
        v = clip(*a, **kw)
        norms.append(float(v))
        return v

    meta = dict(env=qmeta["env"], n_agents=qmeta["n_agents"], agent_mode=qmeta["agent_mode"], target_num=qmeta["target_num"],
                target_mode=qmeta["target_mode"], batch="learn_easy3.npz", steps=K, epsilon=EPSILON, lengths=qmeta["lengths"])
    init, records = {}, {}
    torch.nn.utils.clip_grad_norm_ = recording_clip
    try:
        # ---- DOP
        args = get_dop_args(base_args("dop"))
        assert args.seed == SEED
        with contextlib.redirect_stdout(io.StringIO()):
            d = DOP(args)
        evals = {"actor": d.actor, "critic": d.eval_critic, "mixer": d.eval_mixer_net}
        targets = {"critic": d.target_critic, "mixer": d.target_mixer_net}
        init.update(sd(evals, "init"))
        init.update(sd({"target_critic": d.target_critic, "target_mixer": d.target_mixer_net}, "init"))
        captured = {}
        td = d._td_lambda_target

        def recording_td(b, mel, q_targets):
            out = td(b, mel, q_targets)
            captured.setdefault("q_total_target", q_targets.detach().numpy().copy())
            captured.setdefault("lambda_return", out.detach().numpy().copy())
            return out

        d._td_lambda_target = recording_td
        names = {id(p): f"{m}.{k}" for m, net in evals.items() for k, p in net.named_parameters()}
        steps = []
        for k in range(K):
            b = {key: v.copy() for key, v in batch.items()}
            n0 = len(norms)
            with contextlib.redirect_stdout(io.StringIO()):
                d.learn(b, T, k, EPSILON)
            assert len(norms) == n0 + 2
            rec = grads(evals)
            rec.update(sd(evals, "eval"))
            rec.update(sd(targets, "target"))
            rec["critic_grad_norm"], rec["actor_grad_norm"] = np.float64(norms[n0]), np.float64(norms[n0 + 1])
            if k == 0:
                rec.update(captured)
            steps.append(rec)
        records["dop"] = steps
        meta["dop"] = dict(
            args={k: getattr(args, k) for k in ("seed", "lr", "critic_lr", "td_lambda", "tau", "gamma", "grad_norm_clip",
                                                "optimizer", "rnn_hidden_dim", "offpg_hidden_dim", "qmix_hidden_dim",
                                                "two_hyper_layers", "hyper_hidden_dim", "last_action", "reuse_network",
                                                "n_actions", "state_shape", "obs_shape", "episode_limit", "model_dir", "alg",
                                                "conv")},
            get_args=fields_set_by(get_dop_args), model_dir=d.model_dir,
            files=["{num}_actor_net_params.pkl", "{num}_critic_net_params.pkl", "{num}_mixer_net_params.pkl"],
            state_dicts={m: {k: list(v.shape) for k, v in net.state_dict().items()} for m, net in evals.items()},
            c_params=[names[id(p)] for p in d.c_params], actor_params=[names[id(p)] for p in d.actor_params],
            grad_norms=[[s["critic_grad_norm"].item(), s["actor_grad_norm"].item()] for s in steps])

        # ---- REINFORCE
        args = get_reinforce_args(base_args("reinforce"))
        assert args.seed == SEED
        with contextlib.redirect_stdout(io.StringIO()):
            rf = Reinforce(args)
        evals = {"rnn": rf.eval_rnn}
        init.update(sd(evals, "init"))
        captured = {}
        gr = rf._get_returns

        def recording_returns(*a):
            out = gr(*a)
            captured.setdefault("returns", out.detach().numpy().copy())
            return out

        rf._get_returns = recording_returns
        steps = []
        for k in range(K):
            b = {key: v.copy() for key, v in batch.items()}
            n0 = len(norms)
            with contextlib.redirect_stdout(io.StringIO()):
                rf.learn(b, T, k, EPSILON)
            assert len(norms) == n0   # no gradient clipping (reinforce.py:97)
            rec = grads(evals)
            rec.update(sd(evals, "eval"))
            if k == 0:
                rec.update(captured)
            steps.append(rec)
        records["reinforce"] = steps
        meta["reinforce"] = dict(
            args={k: getattr(args, k) for k in ("seed", "lr_actor", "gamma", "optimizer", "rnn_hidden_dim", "last_action",
                                                "reuse_network", "n_actions", "state_shape", "obs_shape", "episode_limit",
                                                "model_dir", "alg", "conv")},
            get_args=fields_set_by(get_reinforce_args), model_dir=rf.model_dir, files=["{num}_rnn_net_params.pkl"],
            state_dicts={"rnn": {k: list(v.shape) for k, v in rf.eval_rnn.state_dict().items()}})
    finally:
        torch.nn.utils.clip_grad_norm_ = clip

    out = dict(init)
    out["meta"] = np.array(json.dumps(meta))
    files = {"learn_pg_easy3.npz": out}
    for alg, steps in records.items():
        for k, rec in enumerate(steps):
            files[f"learn_pg_easy3_{alg}_step{k}.npz"] = rec
    for fn, content in files.items():
        np.savez_compressed(os.path.join(HERE, fn), **content)
        size = os.path.getsize(os.path.join(HERE, fn))
        assert size < 1 << 20, (fn, size)
        print(f"{fn}: {size / 1024:.0f} KiB")
    print("DOP pre-clip norms", meta["dop"]["grad_norms"])


if __name__ == "__main__":
    main()
