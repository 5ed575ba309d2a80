"""CPU tests of env snapshot / restore and of Runner.save_state / load_state: the record size, the ops' registration and their
tensor checks, EnvSnapshot's host side, and -- with recording fakes in place of the runner's parts -- that a run split by a
state file makes the calls of the unsplit run."""
import ctypes as C
import math
import os
import types

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import runner as rn
from cooperative_search_amd import snapshot as sn
from cooperative_search_amd.env import _cfg_from_args
from cooperative_search_amd.replay import KEYS
from cooperative_search_amd.targets import default_circle_dict

T = 5
# 16 + 16 header words, targets double [16][2], agents double [8][4], 624 MT19937 words (include/coopsearch.h)
RECORD_BASE = 4 * 16 + 4 * 16 + 8 * 16 * 2 + 8 * 8 * 4 + 4 * 624


def config(variant, n=3, batch=4):
    args = cs.make_env_args(variant, n_agents=n)
    return _cfg_from_args(args, default_circle_dict(), batch, 1 if variant == "flight" else 0), args


def cfg_tensor(cfg):
    return torch.frombuffer(bytearray(bytes(cfg)), dtype=torch.uint8)


# ---- the C ABI and the ops ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant, n", [("flight_easy", 3), ("flight_easy", 8), ("flight", 3)])
def test_snapshot_bytes_is_the_documented_formula(variant, n):
    L = _lib.load()
    cfg, args = config(variant, n)
    want = RECORD_BASE + (4 * args.map_size ** 2 if variant == "flight" else 0)
    assert RECORD_BASE == 3136 and want % 16 == 0
    assert L.cs_snapshot_bytes(C.byref(cfg)) == want
    assert int(_lib.torch_ops().snapshot_bytes(cfg_tensor(cfg))) == want
    meta = dict(variant=variant, n_agents=n, n_targets=args.target_num, map_size=args.map_size, version=sn.FORMAT_VERSION)
    assert sn.record_bytes(meta) == want
    cfg.n_agents = 9   # a config cs_state_layout refuses has no record size
    assert L.cs_snapshot_bytes(C.byref(cfg)) == 0


def test_the_entry_points_are_exported_and_registered_without_new_ctypes_twins():
    L = _lib.load()
    for name in ("cs_snapshot_bytes", "cs_snapshot", "cs_restore"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    ops = _lib.torch_ops()
    for name in ("snapshot_bytes", "env_snapshot", "env_restore"):
        assert hasattr(ops, name) and not hasattr(_lib.CtypesOps, name)
    assert sn.FORMAT_VERSION == 1


def test_argument_errors_return_before_any_launch():
    """No GPU here: the fake pointers are never dereferenced."""
    L = _lib.load()
    cfg, _ = config("flight_easy")
    state, recs = C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    assert L.cs_snapshot(C.byref(cfg), state, None, 5, recs, None) == -2          # more records than envs, no index array
    assert L.cs_snapshot(C.byref(cfg), state, None, 2, C.c_void_p((1 << 21) + 8), None) == -2   # records not 16-byte aligned
    assert L.cs_snapshot(C.byref(cfg), state, None, -1, recs, None) == -2
    assert L.cs_restore(C.byref(cfg), state, recs, 2, None, None, 3, None, None, None, None) == -2   # identity src past the records
    assert L.cs_restore(C.byref(cfg), state, recs, 8, None, None, 5, None, None, None, None) == -2   # identity dst past the batch
    assert L.cs_restore(C.byref(cfg), state, C.c_void_p((1 << 21) + 4), 4, None, None, 4, None, None, None, None) == -2
    assert L.cs_restore(C.byref(cfg), None, recs, 4, None, None, 4, None, None, None, None) == -2
    assert L.cs_last_error() == b"null state"


def test_the_ops_refuse_cpu_tensors_like_env_init():
    ops = _lib.torch_ops()
    cfg, _ = config("flight_easy")
    ct = cfg_tensor(cfg)
    state = torch.zeros(int(ops.state_bytes(ct)), dtype=torch.uint8)
    recs = torch.zeros(4, RECORD_BASE, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="coopsearch"):
        ops.env_init(ct, state)
    with pytest.raises(RuntimeError, match="coopsearch"):
        ops.env_snapshot(ct, state, None, recs)
    with pytest.raises(RuntimeError, match="coopsearch"):
        ops.env_restore(ct, state, recs, None, None, None, None, None)


# ---- EnvSnapshot -------------------------------------------------------------------------------------------------------------

META = dict(variant="flight_easy", n_agents=3, n_targets=15, map_size=50, version=sn.FORMAT_VERSION)


def test_envsnapshot_survives_torch_save(tmp_path):
    recs = torch.arange(2 * RECORD_BASE, dtype=torch.int64).remainder(251).to(torch.uint8).view(2, RECORD_BASE)
    snap = sn.EnvSnapshot(recs, META)
    assert len(snap) == 2 and snap.cpu().records.device.type == "cpu" and snap.to("cpu").meta == META
    path = str(tmp_path / "snap.pt")
    torch.save(snap.state_dict(), path)
    back = sn.EnvSnapshot.from_state_dict(torch.load(path, weights_only=True))
    assert back.meta == META and torch.equal(back.records, recs) and back.records.dtype == torch.uint8
    with pytest.raises(ValueError, match="records"):
        sn.EnvSnapshot(recs[:, :-16], META)
    with pytest.raises(ValueError, match="records"):
        sn.EnvSnapshot(recs, dict(META, variant="flight"))   # a flight record carries its map


@pytest.mark.parametrize("field, other", [("variant", "flight"), ("n_agents", 5), ("n_targets", 12), ("map_size", 40), ("version", 2)])
def test_envsnapshot_refuses_each_mismatching_meta_field(field, other):
    snap = sn.EnvSnapshot(torch.zeros(1, RECORD_BASE, dtype=torch.uint8), META)
    snap.check(META)
    with pytest.raises(ValueError, match=field):
        snap.check(dict(META, **{field: other}))
    # restore() makes this check on the host before anything is launched: a stub env without a device is enough to see it
    env = types.SimpleNamespace(variant="flight_easy", n_agents=3, target_num=15, map_size=50, batch=1, device=torch.device("cpu"))
    if field == "version":   # an env always speaks the current format: the stranger is the snapshot
        snap = sn.EnvSnapshot(snap.records, dict(META, version=other))
    else:
        setattr(env, {"n_targets": "target_num"}.get(field, field), other)
    assert (sn.env_meta(env)[field] != snap.meta[field])
    with pytest.raises(ValueError, match=field):
        sn.restore(env, snap)


# ---- Runner: a run split by a state file ----------------------------------------------------------------------------------------

class Parts:
    """Recording fakes of the runner's parts.  Each carries a counter that its events show and its state_dict holds, so a trace
    continues correctly only if the state travelled."""

    def __init__(self, args, batch=2):
        self.trace, self.args, self.batch = [], args, batch
        rec = self

        class Env:
            device = torch.device("cpu")
            episodes = 0
            variant, n_agents, target_num, map_size = "flight_easy", 3, 15, 50   # what META says: load_state compares them

            def __init__(self):
                self.batch = batch

            def snapshot(self):
                recs = torch.zeros(batch, RECORD_BASE, dtype=torch.uint8)
                recs[:, 0] = self.episodes
                return sn.EnvSnapshot(recs, META)

            def restore(self, snap):
                rec.trace.append(["restore", len(snap)])
                self.episodes = int(snap.records[0, 0])

        class Buffer:
            current_size = 0

            def sample(self, size):
                rec.trace.append(["sample", int(size)])
                return {key: torch.zeros(size, T, 1) for key in KEYS}

            def state_dict(self, with_buffer=True):
                return {"current_size": self.current_size if with_buffer else 0}

            def check_state_dict(self, sd):
                assert set(sd) == {"current_size"}

            def load_state_dict(self, sd):
                self.current_size = sd["current_size"]

        class Collector:
            def generate_episodes(self, agents=None, evaluate=True, episode_num=None, into=None, **kw):
                rec.env.episodes += 1
                rec.agents.calls += T
                rec.trace.append(["generate_episode", episode_num, rec.env.episodes, rec.agents.calls])
                if into is not None:
                    into.current_size += batch
                    return None, None, None, None
                return {key: torch.zeros(batch, T, 1) for key in KEYS}, None, None, None

            def evaluate(self, policy, batches=1):
                assert batches == math.ceil(args.evaluate_epoch / batch)
                rec.env.episodes += batches
                rec.trace.append(["evaluate", rec.env.episodes])
                return 0.0, float(rec.env.episodes), 1.5

        class Learner:
            """A network and an optimizer, as the real learners hold them: the runner finds both by type.  The bias counts the
            learn calls, the optimizer's momentum buffer is state only the file can carry."""

            def __init__(self):
                self.net = torch.nn.Linear(1, 1)
                torch.nn.init.zeros_(self.net.weight)
                torch.nn.init.zeros_(self.net.bias)
                self.opt = torch.optim.SGD(self.net.parameters(), lr=1.0, momentum=0.5)

            @property
            def updates(self):
                return int(round(float(self.net.bias.detach())))

            def learn(self, batch, max_episode_len=None, train_step=0, *epsilon):
                self.opt.zero_grad()
                self.net.weight.grad = torch.ones_like(self.net.weight)   # weight = -(sum of momentum terms): needs the buffer
                self.net.bias.grad = torch.zeros_like(self.net.bias)
                self.opt.step()
                with torch.no_grad():
                    self.net.bias += 1
                rec.trace.append(["learn", int(train_step), self.updates, int(batch["o"].shape[0]),
                                  [float(e) for e in epsilon], float(self.net.weight.detach())])

            def save_model(self, idx):
                rec.trace.append(["save", int(idx)])
                open(os.path.join(args.model_dir + rn.run_name(args), f"{idx}_rnn_net_params.pkl"), "w").close()

        class Agents:
            calls = 0
            syncs = 0

            def sync_weights(self):
                self.syncs += 1

            def check_weights(self):
                pass

            def policy(self, epsilon=0.0, evaluate=True):
                return None

            def state_dict(self):
                return {"calls": self.calls}

            def check_state_dict(self, sd):
                assert set(sd) == {"calls"}

            def load_state_dict(self, sd):
                self.calls = sd["calls"]

        class Schedule:
            def __init__(self):
                self.values = torch.full((batch,), 0.5, dtype=torch.float64)

            def state_dict(self):
                return {"values": self.values}

            def check_state_dict(self, sd):
                if sd["values"].shape != self.values.shape:
                    raise ValueError("schedule state of another batch")

            def load_state_dict(self, sd):
                self.values = sd["values"].clone()

        self.env, self.buffer, self.collector, self.learner = Env(), Buffer(), Collector(), Learner()
        self.agents, self.schedule = Agents(), Schedule()

    def runner(self):
        return rn.Runner(self.env, self.args, learner=self.learner, agents=self.agents, schedule=self.schedule,
                         collector=self.collector, buffer=self.buffer)


def make_args(alg, root, **over):
    a = cs.make_env_args("flight_easy", n_agents=3)
    a.n_actions, a.state_shape, a.obs_shape, a.episode_limit = 3, 57, 4, T
    a.alg, a.seed = alg, 1234
    {"qmix": cs.get_mixer_args, "dop": cs.get_dop_args, "reinforce": cs.get_reinforce_args}[alg](a)
    a.n_episodes, a.train_steps, a.batch_size, a.evaluate_cycle, a.save_cycle, a.evaluate_epoch = 2, 2, 3, 3, 4, 4
    a.model_dir, a.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_a_split_run_makes_the_calls_of_the_whole_one(alg, tmp_path):
    whole = Parts(make_args(alg, str(tmp_path / "w")))
    rw = whole.runner()
    assert (rw.epoch, rw.train_steps) == (0, 0)
    rw.run(0, n_epoch=6)
    steps = 6 * (2 if alg != "reinforce" else 1)
    assert (rw.epoch, rw.train_steps) == (6, steps)

    first = Parts(make_args(alg, str(tmp_path / "s")))
    r1 = first.runner()
    r1.run(0, n_epoch=3)
    assert (r1.epoch, r1.train_steps) == (3, steps // 2)
    path = str(tmp_path / "state.pt")
    first.schedule.values -= 0.125   # something only the state file can carry over
    whole_eps = whole.schedule.values
    r1.save_state(path)
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    second = Parts(make_args(alg, str(tmp_path / "s")))
    r2 = second.runner()
    r2.load_state(path)
    assert (r2.epoch, r2.train_steps) == (3, steps // 2) and second.agents.syncs == 1
    assert second.trace == [["restore", 2]]
    assert torch.equal(second.schedule.values, whole_eps - 0.125)
    assert r2.episode_rewards == r1.episode_rewards and len(r2.episode_rewards) == 1
    second.trace.clear()
    r2.run(0, n_epoch=6)
    assert (r2.epoch, r2.train_steps) == (6, steps)

    def plain(trace):   # epsilon differs by the 0.125 planted above: compare its presence, not its value
        return [ev[:4] + [len(ev[4]), ev[5]] if ev[0] == "learn" else ev for ev in trace]
    assert plain(first.trace + second.trace) == plain(whole.trace)
    assert r2.episode_rewards == rw.episode_rewards and r2.targets_find == rw.targets_find and r2.win_rates == rw.win_rates
    assert second.agents.syncs - 1 + first.agents.syncs == whole.agents.syncs
    # a run that has reached n_epoch does nothing more
    second.trace.clear()
    r2.run(0, n_epoch=6)
    assert second.trace == []


def test_state_cycle_writes_the_file_atomically_and_load_state_picks_it_up(tmp_path, monkeypatch):
    args = make_args("qmix", str(tmp_path), state_cycle=2)
    parts = Parts(args)
    r = parts.runner()
    seen = []
    real_replace = os.replace

    def replace(src, dst):
        seen.append((os.path.basename(src), os.path.basename(dst), os.path.exists(src)))
        real_replace(src, dst)
    monkeypatch.setattr(os, "replace", replace)
    r.run(0, n_epoch=5)
    assert seen == [("state.pt.tmp", "state.pt", True)] * 2   # after epochs 2 and 4, each through a temporary file
    assert r.state_path == os.path.join(r.model_path, "state.pt") and os.path.exists(r.state_path)
    assert not os.path.exists(r.state_path + ".tmp")
    assert torch.load(r.state_path, weights_only=True)["epoch"] == 4
    assert rn.get_model_idx(r.model_path) == 1 + max(ev[1] for ev in parts.trace if ev[0] == "save")   # the state file is no checkpoint
    # args.load_state: the constructor loads it
    again = Parts(make_args("qmix", str(tmp_path), load_state=True))
    r2 = again.runner()
    assert (r2.epoch, r2.train_steps) == (4, 8) and again.trace == [["restore", 2]]
    assert again.learner.updates == 8 and again.buffer.current_size == 16 and again.agents.calls == parts.agents.calls - 2 * T
    with pytest.raises(Exception, match="No state!"):
        Parts(make_args("qmix", str(tmp_path / "elsewhere"), load_state=True)).runner()


def test_without_state_cycle_no_state_file_appears(tmp_path):
    args = make_args("qmix", str(tmp_path))
    assert not hasattr(args, "state_cycle") and not hasattr(args, "load_state")
    r = Parts(args).runner()
    r.run(0, n_epoch=4)
    assert "state.pt" not in os.listdir(r.model_path)
    assert all(f.split("_")[0].isdigit() for f in os.listdir(r.model_path))
    r.args.state_cycle = 0
    r.run(0, n_epoch=6)
    assert "state.pt" not in os.listdir(r.model_path)


def test_save_state_without_the_ring_and_the_wrong_algorithm(tmp_path):
    parts = Parts(make_args("qmix", str(tmp_path / "a")))
    r = parts.runner()
    r.run(0, n_epoch=2)
    path = str(tmp_path / "s.pt")
    r.save_state(path, with_buffer=False)
    assert torch.load(path, weights_only=True)["buffer"] == {"current_size": 0}
    other = Parts(make_args("dop", str(tmp_path / "b")))
    with pytest.raises(ValueError, match="alg"):
        other.runner().load_state(path)


def test_a_refused_state_file_leaves_the_runner_as_it_was(tmp_path):
    parts = Parts(make_args("qmix", str(tmp_path / "a")))
    r = parts.runner()
    r.run(0, n_epoch=2)
    path = str(tmp_path / "s.pt")
    r.save_state(path)
    for what in ("schedule", "learner", "env"):
        other = Parts(make_args("qmix", str(tmp_path / what)))
        if what == "schedule":
            other.schedule.values = torch.zeros(5, dtype=torch.float64)       # a schedule of another batch: checked after the env
        elif what == "learner":
            other.learner.net = torch.nn.Linear(2, 1)                          # a network of another shape
            torch.nn.init.zeros_(other.learner.net.bias)
        else:
            other.env.n_agents = 5                                             # an env of another team size
        r2 = other.runner()
        with pytest.raises(ValueError):
            r2.load_state(path)
        assert other.trace == [] and other.env.episodes == 0 and other.learner.updates == 0 and other.buffer.current_size == 0
        assert (r2.epoch, r2.train_steps) == (0, 0) and other.agents.syncs == 0 and other.agents.calls == 0


def test_the_real_parts_round_trip_their_state():
    """EpsilonSchedule and the rings, on the host: what save_state stores of them comes back, the filled part only."""
    a = make_args("qmix", "/nonexistent")
    a.episode_limit = T
    sched = cs.EpsilonSchedule(a, 4, "cpu")
    sched.values[2] = 0.25
    other = cs.EpsilonSchedule(a, 4, "cpu")
    other.load_state_dict(sched.state_dict())
    assert torch.equal(other.values, sched.values) and other.values.data_ptr() != sched.values.data_ptr()
    with pytest.raises(ValueError):
        cs.EpsilonSchedule(a, 5, "cpu").load_state_dict(sched.state_dict())
    ring = cs.DeviceReplayBuffer(a, 6, "cpu")
    for k, v in ring.buffers.items():
        v.copy_(torch.arange(v.numel(), dtype=torch.float32).view(v.shape))
    ring._get_storage_idx(4)
    sd = ring.state_dict()
    assert all(v.shape[0] == 4 for v in sd["buffers"].values()) and (sd["current_idx"], sd["current_size"]) == (4, 4)
    back = cs.DeviceReplayBuffer(a, 6, "cpu")
    back.load_state_dict(sd)
    assert (back.current_idx, back.current_size) == (4, 4)
    for k in KEYS:
        assert torch.equal(back.buffers[k][:4], ring.buffers[k][:4]), k
    assert ring.state_dict(with_buffer=False)["current_size"] == 0
    with pytest.raises(ValueError):
        cs.DeviceReplayBuffer(a, 3, "cpu").load_state_dict(sd)
