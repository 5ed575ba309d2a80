#!/usr/bin/env python3
"""Fixture of the reference's training driver (runner.py:41-84, agent/agent.py:112-136) for tests/test_runner_cpu.py.

Runs ONLY in the build container (needs the reference tree) and contains no reference code: it imports the reference's own
`Runner` (runner.py) and `Agents` (agent/agent.py) at run time and drives `Runner.run` with recording stubs in place of the
rollout worker, the replay buffer and the learner (`Agents.policy`); matplotlib is stubbed in sys.modules as gen_golden.py
stubs cv2 and pynvml.  The reference's own get_model_idx (policy/qmix.py:197-207) numbers the checkpoints: the stub learner
creates the files the real one would, so the numbering runs over real directory listings.

Recorded per configuration, in order:
    ["evaluate"]                         one evaluation (the worker's generate_episode(0, evaluate=True) call)
    ["generate_episode", idx]            one exploring episode (episode_num = idx)
    ["store", k]                         k episodes stored in the ring
    ["sample", size]                     buffer.sample(size)
    ["learn", train_step, eps, k]        policy.learn with train_step, whether an epsilon was passed, k episodes
    ["save", idx]                        policy.save_model(idx)
plus the model / result directory names (relative to the run root), the files in them, and the saved result arrays.

    python tests/golden/gen_runner.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import REF  # noqa: E402

T = 4   # episode_limit of the stub episodes

# (name, alg, fields): the off-policy configurations fill the ring past batch_size (2 episodes per epoch, batch_size 5)
CONFIGS = [
    ("qmix_off_policy", "qmix", dict(off_policy=True, n_epoch=7, evaluate_cycle=3, save_cycle=2, train_steps=2, n_episodes=2,
                                     batch_size=5, buffer_size=30, evaluate_epoch=4)),
    ("dop_off_policy", "dop", dict(off_policy=True, n_epoch=7, evaluate_cycle=3, save_cycle=2, train_steps=2, n_episodes=2,
                                   batch_size=5, buffer_size=30, evaluate_epoch=4)),
    ("reinforce_on_policy", "reinforce", dict(off_policy=False, n_epoch=7, evaluate_cycle=3, save_cycle=2, train_steps=1,
                                              n_episodes=2, batch_size=5, buffer_size=30, evaluate_epoch=4)),
]
SAVE_FILES = {"qmix": ("qmix", "rnn"), "dop": ("actor", "mixer", "critic"), "reinforce": ("rnn",)}
EVAL_REWARD, EVAL_TARGETS = 3.0, 2.0


def make_run_args(alg, fields, root):
    return types.SimpleNamespace(env="flight_easy", map_size=50, target_num=15, target_mode=0, agent_mode=0, n_agents=3,
                                 view_range=7, alg=alg, seed=1234, show=False, load_model=False, cuda=False, search_env=True,
                                 n_actions=3, state_shape=57, obs_shape=4, episode_limit=T, epsilon=0.5, anneal_epsilon=0.1,
                                 min_epsilon=0.05, model_dir=os.path.join(root, "model") + "/",
                                 result_dir=os.path.join(root, "result") + "/", **fields)


def episode(k):
    return {key: np.zeros((k, T, 1)) for key in ("o", "u", "s", "r", "o_next", "s_next", "avail_u", "avail_u_next",
                                                    "u_onehot", "padded", "terminated")}


def run_reference(alg, fields):
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        import runner as ref_runner
        import agent.agent as ref_agent
        from policy.qmix import QMIX
    finally:
        os.chdir(cwd)
    trace = []

    class Worker:
        def __init__(self, env, agents, args):
            self.epsilon = args.epsilon

        def generate_episode(self, episode_num=None, evaluate=False):
            if evaluate:
                if episode_num == 0:
                    trace.append(["evaluate"])
                return None, EVAL_REWARD, False, EVAL_TARGETS
            trace.append(["generate_episode", episode_num])
            return episode(1), 0.0, False, 0.0

    class Buffer:
        def __init__(self, args, size):
            self.current_size = 0

        def store_episode(self, batch):
            k = int(batch["o"].shape[0])
            trace.append(["store", k])
            self.current_size += k

        def sample(self, size):
            trace.append(["sample", int(size)])
            return episode(size)

    class Policy:
        get_model_idx = QMIX.get_model_idx   # the reference's numbering rule, over the stub's files

        def __init__(self, args):
            self.args = args
            self.model_dir = args.model_dir + args.env + "_Seed" + str(args.seed) + "_" + args.alg + \
                "_{}a{}t(AM{}TM{})".format(args.n_agents, args.target_num, args.agent_mode, args.target_mode)

        def learn(self, batch, max_episode_len, train_step, epsilon=None):
            trace.append(["learn", int(train_step), epsilon is not None, int(batch["o"].shape[0])])

        def save_model(self, idx):
            trace.append(["save", int(idx)])
            os.makedirs(self.model_dir, exist_ok=True)
            for part in SAVE_FILES[self.args.alg]:
                open(os.path.join(self.model_dir, f"{idx}_{part}_net_params.pkl"), "w").close()

    ref_runner.RolloutWorker = Worker
    ref_runner.ReplayBuffer = Buffer
    for name in ("QMIX", "DOP", "Reinforce"):
        setattr(ref_agent, name, Policy)
    with tempfile.TemporaryDirectory() as root:
        args = make_run_args(alg, fields, root)
        with contextlib.redirect_stdout(io.StringIO()):
            r = ref_runner.Runner(None, args)
            r.run(0)
        return dict(trace=trace, **listing(root, r.model_path, r.result_path))


def listing(root, model_path, result_path):
    res = {}
    for key, path in (("model", model_path), ("result", result_path)):
        res[key + "_dir"] = os.path.relpath(path, root)
        res[key + "_files"] = sorted(os.listdir(path))
    for f in res["result_files"]:
        if f.endswith(".npy"):
            res[f] = np.load(os.path.join(result_path, f)).tolist()
    return res


def main():
    mpl = types.ModuleType("matplotlib")
    plt = types.ModuleType("matplotlib.pyplot")
    for name in ("figure", "axis", "cla", "subplot", "plot", "xlabel", "ylabel", "savefig", "close"):
        setattr(plt, name, lambda *a, **k: None)
    mpl.pyplot = plt
    mpl.use = lambda *a, **k: None
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, plt
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    sys.path.insert(0, REF)
    out = {"episode_limit": T, "eval": [EVAL_REWARD, EVAL_TARGETS], "configs": []}
    for name, alg, fields in CONFIGS:
        rec = run_reference(alg, fields)
        out["configs"].append(dict(name=name, alg=alg, fields=fields, **rec))
    path = os.path.join(HERE, "runner_schedule.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
