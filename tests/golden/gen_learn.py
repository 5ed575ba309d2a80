#!/usr/bin/env python3
"""Fixture of the reference's QMIX learner (policy/qmix.py:85-130) for tests/test_learner_cpu.py and tests/test_gpu_learner.py.

Runs ONLY in the build container (needs /root/reference) and contains no reference code: it imports the reference's own
`RolloutWorker` (common/rollout.py), `get_mixer_args` (common/arguments.py) and `QMIX` (policy/qmix.py) at run time.

    1. E episodes of flight_easy, 3 agents, AM0 from `RolloutWorker.generate_episode`, driven by seeded uniform random actions
       (a stub Agents object replays a pre-drawn action table, like gen_golden.capture_episode).  Episode seeds are searched in
       order until the batch holds time-limit episodes and one WON episode, whose tail is zero-padded.
    2. The reference `QMIX(args)` with cuda = False, a fixed args.seed and the get_mixer_args values; its initial parameters.
    3. K = 2 calls of `learn` on that batch; after each: every eval parameter's .grad (the clipped gradient of that step; absent
       when None), the pre-clip norm (the value clip_grad_norm_ returned, captured by wrapping it), the eval and target parameters.

Stored compactly (each file < 1 MB):
    learn_easy3.npz          the batch as o_full / s_full [E][T+1][...] (obs and state of every step and the one after the last),
                             u int8 [E][T][n], r / term [E][T], lengths [E]; init_<module>.<name>; meta (JSON: args, seeds,
                             state_dict keys and shapes, file names)
    learn_easy3_step<k>.npz  grad_<module>.<name>, eval_<module>.<name>, target_<module>.<name>, grad_norm
tests/learn_util.py rebuilds the 11 batch keys exactly (checked here against the reference's own arrays).

    python tests/golden/gen_learn.py
"""
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
from gen_golden import REF, import_reference, make_args  # noqa: E402
from learn_util import KEYS, rebuild_batch  # noqa: E402

E, K, N_AGENTS, SEED = 8, 2, 3, 20240519


def ref_modules():
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        from common.rollout import RolloutWorker
        from common.arguments import get_mixer_args
        from policy.qmix import QMIX
    finally:
        os.chdir(cwd)
    return RolloutWorker, get_mixer_args, QMIX


def collect(RolloutWorker, Easy, circle):
    n = N_AGENTS
    args = make_args("flight_easy", n, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        env = Easy(args, circle)
    info = env.get_env_info()
    args.n_actions, args.state_shape, args.obs_shape = info["n_actions"], info["state_shape"], info["obs_shape"]
    args.episode_limit = info["episode_limit"]
    args.epsilon, args.anneal_epsilon, args.min_epsilon, args.epsilon_anneal_scale = 0.0, 0.0, 0.0, "step"
    args.alg, args.evaluate_epoch = "scripted", 20

    class StubPolicy:
        def init_hidden(self, k):
            pass

    class StubAgents:
        def __init__(self, actions):
            self.policy, self.actions, self.calls = StubPolicy(), actions, 0

        def choose_action(self, obs, last_action, agent_num, avail_actions, epsilon, evaluate=False):
            t, self.calls = self.calls // n, self.calls + 1
            return int(self.actions[t][agent_num])

    won, limit = [], []
    seed = 0
    while len(won) < 1 or len(limit) < E - 1:
        actions = np.random.RandomState(10_000 + seed).randint(0, 3, size=(args.episode_limit, n))
        with contextlib.redirect_stdout(io.StringIO()):
            worker = RolloutWorker(env, StubAgents(actions), args)
        np.random.seed(seed)
        episode, _, win_tag, _ = worker.generate_episode(1, evaluate=True)
        steps = int((np.asarray(episode["padded"])[0, :, 0] == 0).sum())
        if win_tag and steps < args.episode_limit and len(won) < 1:
            won.append((seed, episode))
        elif not win_tag and steps == args.episode_limit and len(limit) < E - 1:
            limit.append((seed, episode))
        seed += 1
    chosen = limit[:3] + won + limit[3:]   # the won episode in the middle of the batch
    batch = {k: np.concatenate([np.asarray(ep[k]) for _, ep in chosen], 0) for k in KEYS}
    return args, [s for s, _ in chosen], batch


def compact(batch):
    T = batch["o"].shape[1]
    lengths = (batch["padded"][:, :, 0] == 0).sum(1).astype(np.int32)
    o_full = np.concatenate([batch["o"], np.zeros_like(batch["o"][:, :1])], 1)
    s_full = np.concatenate([batch["s"], np.zeros_like(batch["s"][:, :1])], 1)
    for e, L in enumerate(lengths):
        o_full[e, L] = batch["o_next"][e, L - 1]
        s_full[e, L] = batch["s_next"][e, L - 1]
    return dict(o_full=o_full.astype(np.float32), s_full=s_full.astype(np.float32),
                u=batch["u"][..., 0].astype(np.int8), r=batch["r"][..., 0].astype(np.float32),
                term=batch["terminated"][..., 0].astype(np.uint8), lengths=lengths, T=np.int32(T))


def main():
    import torch
    Easy, _, load_targets = import_reference()
    RolloutWorker, get_mixer_args, QMIX = ref_modules()
    circle = load_targets(os.path.join(REF, "flight_targets.txt"))
    args, seeds, batch = collect(RolloutWorker, Easy, circle)
    stored = compact(batch)
    rebuilt = rebuild_batch(stored, args.n_actions)
    for k in KEYS:   # the compact form loses nothing the learner reads (after its float32 / long conversion)
        want = batch[k].astype(np.int64 if k == "u" else np.float32)
        assert rebuilt[k].shape == want.shape and np.array_equal(rebuilt[k], want), k

    args.alg, args.last_action, args.reuse_network, args.gamma, args.optimizer = "qmix", True, True, 0.99, "Adam"
    args.model_dir, args.load_model, args.cuda, args.show, args.seed_idx, args.seed = "./model/", False, False, True, 4, SEED
    get_mixer_args(args)   # show = True: keeps args.seed
    assert args.seed == SEED
    with contextlib.redirect_stdout(io.StringIO()):
        q = QMIX(args)
    modules = {"rnn": q.eval_rnn, "qmix": q.eval_qmix_net}
    targets = {"rnn": q.target_rnn, "qmix": q.target_qmix_net}
    sd = lambda mods, pre: {f"{pre}_{m}.{k}": v.detach().numpy().copy() for m, net in mods.items() for k, v in net.state_dict().items()}
    init = sd(modules, "init")
    assert all(np.array_equal(v, sd(targets, "init")[k]) for k, v in init.items())   # target <- eval (qmix.py:63-64)

    norms = []
    clip = torch.nn.utils.clip_grad_norm_

    def recording_clip(*a, **kw):
        v = clip(*a, **kw)
        norms.append(float(v))
        return v

    torch.nn.utils.clip_grad_norm_ = recording_clip
    names = {id(p): f"{m}.{k}" for m, net in modules.items() for k, p in net.named_parameters()}
    steps = []
    try:
        for k in range(K):
            b = {key: v.copy() for key, v in batch.items()}
            with contextlib.redirect_stdout(io.StringIO()):
                q.learn(b, batch["o"].shape[1], k)
            rec = {f"grad_{names[id(p)]}": p.grad.detach().numpy().copy() for p in q.eval_parameters if p.grad is not None}
            rec.update(sd(modules, "eval"))
            rec.update(sd(targets, "target"))
            rec["grad_norm"] = np.float64(norms[-1])
            steps.append(rec)
    finally:
        torch.nn.utils.clip_grad_norm_ = clip

    meta = dict(env="flight_easy", n_agents=N_AGENTS, agent_mode=0, target_num=15, target_mode=0, episodes=E, steps=K,
                episode_seeds=seeds, action_seed_base=10_000, lengths=[int(x) for x in stored["lengths"]],
                args={k: getattr(args, k) for k in ("seed", "lr", "tau", "gamma", "grad_norm_clip", "optimizer", "rnn_hidden_dim",
                                                    "qmix_hidden_dim", "two_hyper_layers", "hyper_hidden_dim", "last_action",
                                                    "reuse_network", "n_actions", "state_shape", "obs_shape", "episode_limit",
                                                    "model_dir", "alg", "conv")},
                model_dir=q.model_dir, files=["{num}_qmix_net_params.pkl", "{num}_rnn_net_params.pkl"],
                state_dicts={m: {k: list(v.shape) for k, v in net.state_dict().items()} for m, net in modules.items()},
                eval_parameters=[names[id(p)] for p in q.eval_parameters])
    out = dict(stored)
    out.update(init)
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "learn_easy3.npz"), **out)
    for k, rec in enumerate(steps):
        np.savez_compressed(os.path.join(HERE, f"learn_easy3_step{k}.npz"), **rec)
    for fn in ["learn_easy3.npz"] + [f"learn_easy3_step{k}.npz" for k in range(K)]:
        size = os.path.getsize(os.path.join(HERE, fn))
        assert size < 1 << 20, (fn, size)
        print(f"{fn}: {size / 1024:.0f} KiB")
    print("episodes", seeds, "lengths", meta["lengths"], "pre-clip norms", norms)


if __name__ == "__main__":
    main()
