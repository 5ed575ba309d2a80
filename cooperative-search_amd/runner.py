"""The training driver: the reference's `Runner.run` (runner.py:41-84, with agent/agent.py:112-136 for train / save) over the
device-resident pieces -- `EpisodeCollector` (rows f1 / f4), `DeviceReplayBuffer` (f2), `FusedAgents` (f3) and the learners.

One epoch is: evaluate (every `evaluate_cycle` epochs, epoch 0 included) -> collect `n_episodes` batches of B episodes with
exploration -> off-policy: store them in the ring and make `train_steps` learn calls on samples of min(current_size,
batch_size); on-policy: one learn call on the batches concatenated along the episode axis -> after EVERY learn call the acting
network follows the learner through `FusedAgents.sync_weights()` (the pack kernel, on the device).  Checkpoints are written
where the reference's Agents.train writes them (train_step > 0 and train_step % save_cycle == 0), numbered by its
get_model_idx rule.  Between evaluation and save points an epoch never synchronises with the host: the ring slots are made on
the device, the repack is one launch, and epsilon reaches the learner as a device scalar.

Batched semantics: one epoch stores B * n_episodes episodes but makes `train_steps` learn calls, as the
reference's makes them on its n_episodes; an evaluation covers ceil(evaluate_epoch / B) batches, i.e. at least evaluate_epoch
episodes.  DOP and REINFORCE take the epsilon of env 0 (`schedule.values[0]`): the reference has one RolloutWorker and one
epsilon, a batch of B envs carries B of them (collector.EpsilonSchedule), and env 0 anneals exactly as that one worker would.
"""
import errno
import math
import os

import numpy as np
import torch

from .agents import FusedAgents
from .collector import EpisodeCollector, EpsilonSchedule
from .learner import DOPLearner, PPOLearner, QMixLearner, ReinforceLearner
from .replay import CompactReplayBuffer, DeviceReplayBuffer
from .sweep import with_sweep_bonus

# fields the reference's get_mixer_args / get_common_args set and this package's get_*_args leave to the caller
# (common/arguments.py:43-46, :84-104)
RUN_DEFAULTS = dict(n_epoch=500000, n_episodes=1, train_steps=1, evaluate_cycle=200, save_cycle=500, evaluate_epoch=20,
                    model_dir="./model/", result_dir="./result/", load_model=False, compact_episodes=False)
LEARNERS = {"qmix": QMixLearner, "dop": DOPLearner, "reinforce": ReinforceLearner, "ppo": PPOLearner}
# the checkpoint file whose presence get_model_idx() - 1 must show when resuming (the reference learners' __init__)
_RESUME = {"qmix": ("rnn", "qmix"), "dop": ("actor", "critic", "mixer"), "reinforce": ("rnn",), "ppo": ("rnn", "critic")}


def run_name(args):
    """<env>_Seed<seed>_<alg>_<n>a<targets>t(AM<agent_mode>TM<target_mode>): runner.py:31-38's directory name."""
    return (args.env + "_Seed" + str(args.seed) + "_" + args.alg +
            "_{}a{}t(AM{}TM{})".format(args.n_agents, args.target_num, args.agent_mode, args.target_mode))


def get_model_idx(model_dir):
    """The reference learners' get_model_idx (policy/qmix.py:197-207): 1 + the largest leading integer of the file names in
    model_dir; 0 (creating the directory) when it is missing."""
    if not os.path.exists(model_dir):
        os.makedirs(model_dir)
        return 0
    idx = 0
    for name in os.listdir(model_dir):
        lead = name.split("_")[0]
        if lead.isdigit():   # (the run's state file, STATE_FILE, lives here too: it is no checkpoint)
            idx = max(idx, int(lead))
    return idx + 1


STATE_FILE = "state.pt"   # <model_path>/state.pt: Runner.save_state's file for args.state_cycle / args.load_state
STATE_FORMAT = 1


def learner_state(learner):
    """Every network of a learner (targets included) and every optimizer, by attribute name."""
    return {"modules": {k: v.state_dict() for k, v in vars(learner).items() if isinstance(v, torch.nn.Module)},
            "optimizers": {k: v.state_dict() for k, v in vars(learner).items() if isinstance(v, torch.optim.Optimizer)}}


def check_learner_state(learner, sd):
    """ValueError unless `sd` names this learner's networks and optimizers, with every tensor of a network in its shape."""
    have = learner_state(learner)
    for kind in ("modules", "optimizers"):
        if sorted(sd[kind]) != sorted(have[kind]):
            raise ValueError(f"learner state: {kind} {sorted(sd[kind])} do not match this learner's {sorted(have[kind])}")
    for name, msd in sd["modules"].items():
        mine = have["modules"][name]
        if sorted(msd) != sorted(mine) or any(tuple(msd[k].shape) != tuple(mine[k].shape) for k in mine):
            raise ValueError(f"learner state: the tensors of {name} do not match this learner's")
    for name, osd in sd["optimizers"].items():
        if [len(g["params"]) for g in osd["param_groups"]] != [len(g["params"]) for g in have["optimizers"][name]["param_groups"]]:
            raise ValueError(f"learner state: the parameter groups of {name} do not match this learner's")


def load_learner_state(learner, sd):
    check_learner_state(learner, sd)
    for kind in ("modules", "optimizers"):
        for k, v in sd[kind].items():
            getattr(learner, k).load_state_dict(v)


def apply_run_defaults(args):
    """RUN_DEFAULTS for the fields `args` does not carry (existing values are kept)."""
    for k, v in RUN_DEFAULTS.items():
        if not hasattr(args, k):
            setattr(args, k, v)
    return args


class Runner:
    """Runner(env, args): `env` a BatchedFlightEnv; `args` the reference's namespace after get_mixer_args / get_dop_args /
    get_reinforce_args / get_ppo_args and apply_env_info; args.alg selects the learner.  The parts (learner, agents, schedule, collector,
    buffer) are built here unless passed in.  args.compact_episodes (flight only; default False): episodes are collected,
    stored and learnt from in the map-once format (replay.COMPACT_KEYS) -- a CompactReplayBuffer and
    generate_episodes(compact=True); the schedule of calls is the same.  args.conv_impl (absent: "torch") goes to the learner.
    Exact resume: `save_state` / `load_state` carry everything that changes during `run`;
    args.state_cycle (absent or 0: never) writes <model_path>/state.pt every that many epochs, args.load_state=True loads it
    here.  args.sweep_bonus (absent or 0: off, and the learner is handed the very batch object it was before): the reward the
    learner sees is r + sweep_bonus * (cells the step sweeps for the first time) (sweep.with_sweep_bonus);
    evaluation, episode_rewards, the ring and save_state never see it.  `epoch` and `train_steps` count what this run has done;
    `run` goes on from them."""

    def __init__(self, env, args, learner=None, agents=None, schedule=None, collector=None, buffer=None):
        alg = getattr(args, "alg", None)
        if alg in ("vdn", "random"):
            raise ValueError(f"Runner: alg {alg!r} is not trained here (VDN and random have no device learner)")
        if alg not in LEARNERS:
            raise ValueError(f"Runner: no such algorithm {alg!r} (qmix, dop, reinforce or ppo)")
        self.env, self.args = env, apply_run_defaults(args)
        device = getattr(env, "device", "cuda")
        if learner is None:   # args.conv_impl (absent: "torch"): the learners' conv front end, learner.check_conv_impl
            learner = LEARNERS[alg](args, device, conv_impl=getattr(args, "conv_impl", "torch"))
        self.learner = learner
        self.model_path = args.model_dir + run_name(args)
        if args.load_model:   # policy/*.py __init__: the newest checkpoint of the learner's own directory
            idx = get_model_idx(self.model_path) - 1
            files = [os.path.join(self.model_path, f"{idx}_{part}_net_params.pkl") for part in _RESUME[alg]]
            if not os.path.exists(files[0]):
                raise Exception("No model!")
            self.learner.load_model(*files)
        if agents is None:   # the learner's acting network itself (agent.py:58-61): its parameters ARE the learner's
            acting = self.learner.actor if alg == "dop" else self.learner.eval_rnn
            agents = FusedAgents(args, env.batch, device, net=acting, seed=args.seed)
        self.agents = agents
        self.schedule = schedule if schedule is not None else EpsilonSchedule(args, env.batch, device)
        self.collector = collector if collector is not None else EpisodeCollector(env, self.schedule)
        self.buffer = None
        if args.off_policy:
            ring = CompactReplayBuffer if args.compact_episodes else DeviceReplayBuffer
            self.buffer = buffer if buffer is not None else ring(args, args.buffer_size, device)
        # generate_episodes' format switch; nothing is passed for the dense format, so a collector without it keeps working
        self._collect_kw = dict(compact=True) if args.compact_episodes else {}
        self.win_rates, self.targets_find, self.episode_rewards = [], [], []
        self.result_path = args.result_dir + run_name(args)
        os.makedirs(self.result_path, exist_ok=True)   # runner.py:33-39
        os.makedirs(self.model_path, exist_ok=True)
        self.epoch, self.train_steps = 0, 0
        self.state_path = os.path.join(self.model_path, STATE_FILE)
        if getattr(args, "load_state", False):
            if not os.path.exists(self.state_path):
                raise Exception("No state!")
            self.load_state(self.state_path)

    def run(self, num, n_epoch=None):
        """runner.py:41-84 up to epoch n_epoch (default args.n_epoch), starting at self.epoch (0 unless a state was loaded or an
        earlier call ran); results are saved after every evaluation and at the end."""
        a = self.args
        n_epoch = a.n_epoch if n_epoch is None else int(n_epoch)
        state_cycle = int(getattr(a, "state_cycle", 0) or 0)
        for epoch in range(self.epoch, n_epoch):
            if epoch % a.evaluate_cycle == 0:
                win_rate, episode_reward, targets_find = self.evaluate()
                self.win_rates.append(win_rate)
                self.targets_find.append(targets_find)
                self.episode_rewards.append(episode_reward)
                self.save_results(num)
            self.train_steps = self.train_epoch(self.train_steps)
            self.epoch = epoch + 1
            if state_cycle and self.epoch % state_cycle == 0:
                self.save_state(self.state_path)
        self.save_results(num)

    def _rng_device(self):
        dev = torch.device(getattr(self.env, "device", "cpu"))
        return dev if dev.type == "cuda" else None

    def save_state(self, path, with_buffer=True):
        """Everything that changes during `run`, in one file: the env snapshot, every learner network (targets included) and
        optimizer, the ring (its filled part; with_buffer=False: an empty ring), every env's epsilon, the acting agents' noise
        counter / hidden state / last actions, torch's CPU and device generator states, epoch, train_steps and the result lists.
        Written through a temporary file and a rename: a reader sees the old file or the new one.  Synchronises."""
        dev = self._rng_device()
        state = {"format": STATE_FORMAT, "alg": self.args.alg, "epoch": int(self.epoch), "train_steps": int(self.train_steps),
                 "env": self.env.snapshot().cpu().state_dict(),
                 "learner": learner_state(self.learner),
                 "buffer": None if self.buffer is None else self.buffer.state_dict(with_buffer=with_buffer),
                 "schedule": self.schedule.state_dict(), "agents": self.agents.state_dict(),
                 "rng": {"cpu": torch.get_rng_state(), "device": None if dev is None else torch.cuda.get_rng_state(dev)},
                 "results": {"win_rates": [float(v) for v in self.win_rates], "targets_find": [float(v) for v in self.targets_find],
                             "episode_rewards": [float(v) for v in self.episode_rewards]}}
        tmp = path + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, path)

    def load_state(self, path):
        """The inverse of save_state, into this Runner's parts (built for the same args and batch): afterwards `run` continues
        exactly as the saved run would have.  The env's seeds do not matter: every env takes its record.  A file that does not
        fit (other alg, batch, team, ring or network shapes) raises ValueError before anything is changed."""
        from .snapshot import EnvSnapshot, env_meta
        state = torch.load(path, map_location="cpu", weights_only=True)
        if state.get("format") != STATE_FORMAT or state.get("alg") != self.args.alg:
            raise ValueError(f"{path}: state of format {state.get('format')!r} for alg {state.get('alg')!r}; this Runner reads "
                             f"format {STATE_FORMAT} and trains {self.args.alg!r}")
        snap = EnvSnapshot.from_state_dict(state["env"])
        if len(snap) != self.env.batch:
            raise ValueError(f"{path}: {len(snap)} env records for a batch of {self.env.batch}")
        if (state["buffer"] is None) != (self.buffer is None):
            raise ValueError(f"{path}: the saved run and this one disagree on having a replay ring")
        # every part is validated before any part is touched: a refused file leaves this Runner as it was
        snap.check(env_meta(self.env))
        check_learner_state(self.learner, state["learner"])
        if self.buffer is not None:
            self.buffer.check_state_dict(state["buffer"])
        self.schedule.check_state_dict(state["schedule"])
        self.agents.check_state_dict(state["agents"])
        self.env.restore(snap)
        load_learner_state(self.learner, state["learner"])
        if self.buffer is not None:
            self.buffer.load_state_dict(state["buffer"])
        self.schedule.load_state_dict(state["schedule"])
        self.agents.load_state_dict(state["agents"])
        self.agents.sync_weights()   # the acting blob follows the loaded network
        self.epoch, self.train_steps = int(state["epoch"]), int(state["train_steps"])
        res = state["results"]
        self.win_rates, self.targets_find = list(res["win_rates"]), list(res["targets_find"])
        self.episode_rewards = list(res["episode_rewards"])
        torch.set_rng_state(state["rng"]["cpu"])
        dev = self._rng_device()
        if dev is not None and state["rng"]["device"] is not None:
            torch.cuda.set_rng_state(state["rng"]["device"], dev)

    def train_epoch(self, train_steps):
        """Collect, store, learn, repack: one epoch without its evaluation.  Returns the updated learn-call count."""
        a = self.args
        if a.off_policy:
            for idx in range(a.n_episodes):
                self.collector.generate_episodes(agents=self.agents, evaluate=False, episode_num=idx, into=self.buffer,
                                                 **self._collect_kw)
            for _ in range(a.train_steps):
                self.train(self.buffer.sample(min(self.buffer.current_size, a.batch_size)), train_steps)
                train_steps += 1
        else:
            eps = [self.collector.generate_episodes(agents=self.agents, evaluate=False, episode_num=idx, **self._collect_kw)[0]
                   for idx in range(a.n_episodes)]
            batch = eps[0] if len(eps) == 1 else {k: torch.cat([e[k] for e in eps], 0) for k in eps[0]}
            self.train(batch, train_steps)
            train_steps += 1
        return train_steps

    def train(self, batch, train_step):
        """agent.py:112-136: one learn call (QMIX without epsilon, DOP, REINFORCE and PPO with env 0's), the acting network repacked,
        a checkpoint when train_step > 0 and train_step % save_cycle == 0.  With args.sweep_bonus the batch passes through
        sweep.with_sweep_bonus first."""
        beta = float(getattr(self.args, "sweep_bonus", 0) or 0)
        if beta:   # the exploration bonus (sweep.py): a copy of the dict with r + bonus; the batch and the ring stay as they are
            batch = with_sweep_bonus(batch, self.args, beta)
        if self.args.alg == "qmix":
            self.learner.learn(batch, None, train_step)
        else:
            self.learner.learn(batch, None, train_step, self.schedule.values[0])
        self.agents.sync_weights()
        if train_step > 0 and train_step % self.args.save_cycle == 0:
            self.agents.check_weights()   # the host waits here anyway
            self.learner.save_model(get_model_idx(self.model_path))

    def evaluate(self):
        """runner.py:86-96 -> (win_rate, episode_reward, targets_find): the greedy policy over ceil(evaluate_epoch / B) batches."""
        self.agents.check_weights()
        batches = max(1, math.ceil(self.args.evaluate_epoch / self.env.batch))
        return self.collector.evaluate(self.agents.policy(0.0, True), batches)

    def load_checkpoint(self, num):
        """runner.py:118-134 / :142-154: checkpoint `num` of this run's model directory into the learner (the files of
        _RESUME[alg]; a missing one is the FileNotFoundError torch.load raises there), then the acting network follows."""
        files = [os.path.join(self.model_path, f"{num}_{part}_net_params.pkl") for part in _RESUME[self.args.alg]]
        for f in files:
            if not os.path.exists(f):
                raise FileNotFoundError(errno.ENOENT, os.strerror(errno.ENOENT), f)
        self.learner.load_model(*files)
        self.agents.sync_weights()
        self.agents.check_weights()

    def replay(self, num, episodes=None, size=256, path=None):
        """runner.py:118-137 with pictures: load checkpoint `num`, run ONE greedy batch from reset(init=True)
        (generate_replay's reset, rollout.py:145) and draw its first `episodes` envs (default min(batch, 16)) as `size` x `size`
        frames on the device (render.render_episodes: one launch for every step of every episode).  Writes
        <result_path>/replay_<num>.gif (`path` overrides; the array as .npy where PIL is missing), prints the reference's line
        for env 0 and returns (frames uint8 [K, T + 1, W, W, 3], targets_find [B], episode_reward [B], steps [B]) as device
        tensors."""
        from . import render as _render
        self.load_checkpoint(num)
        batch, episode_reward, _win, targets_find = self.collector.generate_episodes(agents=self.agents, evaluate=True, init=True,
                                                                                     **self._collect_kw)
        states, maps, counts = _render.episode_tables(batch, self.args)
        K = min(int(states.shape[0]), 16 if episodes is None else max(1, int(episodes)))
        spec = _render.RenderSpec.for_env(self.args, size)
        frames = _render.render_episodes(states[:K].contiguous(), None if maps is None else maps[:K].contiguous(),
                                         counts[:K].contiguous(), spec)
        written = _render.write_frames(frames, path if path is not None else os.path.join(self.result_path, f"replay_{num}.gif"))
        print("targets_find: ", int(targets_find[0]), " reward: ", int(episode_reward[0]))   # runner.py:137
        print("replay saved:", written)
        return frames, targets_find, episode_reward, counts.to(torch.int64) - 1

    def collect_experiment_data(self, num, replay_times):
        """runner.py:139-172: load checkpoint `num`, run at least `replay_times` greedy episodes from reset(init=True) --
        ceil(replay_times / B) batches -- and save the percentage of targets found by every step as
        <result_path>/average_res_<num>.npy.  Prints the reference's two lines; returns (curve, stats)."""
        self.load_checkpoint(num)
        batches = max(1, math.ceil(int(replay_times) / self.env.batch))
        res, stats = self.collector.collect_experiment_data(self.agents.policy(0.0, True), batches, num=num,
                                                            result_path=self.result_path, return_stats=True)
        print(stats["targets_find"], stats["episode_reward"], stats["steps"])
        idx = [i for i in (10, 20, 40, 60, 80, 100, 150, 199) if i < len(res)]
        print(np.asarray(res)[idx])
        print("process data saved!")
        return res, stats

    def save_results(self, num):
        """runner.py:98-116: targets_find_<num>.npy (search envs) and episode_rewards_<num>.npy; plt_<num>.png when matplotlib
        is available."""
        a = self.args
        self._plot(num)
        if getattr(a, "search_env", True):
            np.save(os.path.join(self.result_path, "targets_find_{}".format(num)), self.targets_find)
        np.save(os.path.join(self.result_path, "episode_rewards_{}".format(num)), self.episode_rewards)

    def _plot(self, num):
        try:
            import matplotlib
            matplotlib.use("Agg", force=False)
            import matplotlib.pyplot as plt
        except Exception:   # noqa: BLE001  (no matplotlib, or no usable backend: the picture is optional)
            return
        a = self.args
        plt.figure()
        plt.axis([0, a.n_epoch, 0, 100])
        plt.cla()
        if getattr(a, "search_env", True):
            plt.subplot(2, 1, 1)
            plt.plot(range(len(self.targets_find)), self.targets_find)
            plt.xlabel("epoch*{}".format(a.evaluate_cycle))
            plt.ylabel("targets_find")
            plt.subplot(2, 1, 2)
        plt.plot(range(len(self.episode_rewards)), self.episode_rewards)
        plt.xlabel("epoch*{}".format(a.evaluate_cycle))
        plt.ylabel("episode_rewards")
        plt.savefig(os.path.join(self.result_path, "plt_{}.png".format(num)), format="png")
        plt.close()
