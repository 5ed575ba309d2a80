"""HBM-resident episode replay buffer: the storage between collector and learner.

Counterpart of /root/reference/common/replay_buffer.py:5-101, which keeps `[size, episode_limit, ...]` float64 arrays
in host memory.  Here the ring lives on the device as float32 (a 3000-episode flight buffer with its 2504-wide obs is
~36 GB: sized for 288 GB of HBM, not for host RAM), whole batches of episodes are stored with one indexed copy per
key, and sampling never leaves the GPU.  The FIFO index rule (`_get_storage_idx`, :84-101), `can_sample`, uniform
sampling with replacement (`sample`, :63-68) and `sample_latest` (:70-82) follow the reference exactly; the index
arithmetic is plain host integers, as there.

`CompactReplayBuffer` is the same ring over the map-once format of a flight episode (`COMPACT_KEYS`):
every probability map once instead of 2n times.
"""
import numpy as np
import torch

KEYS = ("o", "u", "s", "r", "o_next", "s_next", "avail_u", "avail_u_next", "u_onehot", "padded", "terminated")
# the map-once format of a flight episode batch: map [E, T+1, cells] and s_full [E, T+1, S] hold the env's probability map
# and get_state() before step t (row T: after the last step), zero past the episode's last real step; u, r, padded,
# terminated are the dense keys of the same names
COMPACT_KEYS = ("map", "s_full", "u", "r", "padded", "terminated")


def expand_compact(batch, n_agents, n_actions, wide=True):
    """The reference's 11 keys of a compact episode batch: the DEFINITION of the format, in stock torch ops (the learners and
    the collector never materialise `o` / `o_next`).  With real = 1 - padded:
        o[e, t]      = (map[e, t] for every agent ++ s_full[e, t, :4n].view(n, 4)) * real[e, t]
        o_next[e, t] = the same from row t + 1, * real[e, t]
        s = s_full[:, :T] * real,  s_next = s_full[:, 1:] * real,  avail_u = avail_u_next = real,  u_onehot = onehot(u) * real
    (an agent's own 4 observation floats are state[4i..4i+3]: the kernels write one float4 to both places).
    wide=False leaves out o and o_next, the only keys that repeat the map."""
    m, sf, u, padded = batch["map"], batch["s_full"], batch["u"], batch["padded"]
    E, T, n, A = int(u.shape[0]), int(u.shape[1]), int(n_agents), int(n_actions)
    real = 1 - padded            # [E, T, 1]
    real4 = real.unsqueeze(-1)   # [E, T, 1, 1]
    out = {"u": u, "r": batch["r"], "padded": padded, "terminated": batch["terminated"],
           "s": sf[:, :T] * real, "s_next": sf[:, 1:] * real}
    out["avail_u"] = real4.expand(E, T, n, A).contiguous()
    out["avail_u_next"] = out["avail_u"].clone()
    out["u_onehot"] = torch.nn.functional.one_hot(u.long().squeeze(-1), A).to(sf.dtype) * real4
    if wide:
        full = torch.cat([m.unsqueeze(2).expand(E, T + 1, n, m.shape[-1]), sf[..., :4 * n].reshape(E, T + 1, n, 4)], 3)
        out["o"], out["o_next"] = full[:, :T] * real4, full[:, 1:] * real4
    return out


def compact_from_dense(batch):
    """The inverse of expand_compact for batches that follow the collector's padding rules (collector.assemble_episodes_torch):
    row 0 of map / s_full is o[:, 0] / s[:, 0], row t + 1 is o_next[:, t] / s_next[:, t] -- zero once step t is padded."""
    o, o_next = batch["o"], batch["o_next"]
    cells = int(o.shape[-1]) - 4
    out = {"map": torch.cat([o[:, :1, 0, :cells], o_next[:, :, 0, :cells]], 1),
           "s_full": torch.cat([batch["s"][:, :1], batch["s_next"]], 1)}
    out.update({k: batch[k] for k in ("u", "r", "padded", "terminated")})
    return out


class _EpisodeRing:
    """The FIFO ring over `keys` / `buffers`: the index rule, sampling and the indexed store, shared by the dense and the
    map-once buffer (same index sequences, same generator use)."""
    keys = KEYS

    def _get_storage_idx(self, inc=None):
        """Ring positions for the next `inc` episodes.  Same sequence as the reference's three-case rule
        (replay_buffer.py:84-101), written as modular arithmetic: writing starts at the cursor (or at 0 when the cursor
        sits exactly at `size`, which the reference leaves un-wrapped after an exact fill), wraps modulo `size`, and the
        cursor ends one past the last written slot -- again left at `size` rather than 0 after an exact fill."""
        inc = inc or 1
        if inc > self.size:
            # the reference's index arithmetic breaks here too (it raises on the assignment); duplicated slots would
            # make several episodes race for one ring entry
            raise ValueError(f"cannot store {inc} episodes at once in a buffer of {self.size}")
        start = 0 if self.current_idx >= self.size else self.current_idx
        idx = (start + np.arange(inc)) % self.size
        end = start + inc
        self.current_idx = end if end <= self.size else end - self.size
        self.current_size = min(self.size, self.current_size + inc)
        return idx

    def store_episode(self, episode_batch):
        """episode_batch: dict of [k, T, ...] tensors (EpisodeCollector.generate_episodes) or ndarrays."""
        k = int(episode_batch[self.keys[0]].shape[0])
        idx = torch.as_tensor(self._get_storage_idx(inc=k), device=self.device)
        for key in self.keys:
            src = torch.as_tensor(episode_batch[key], device=self.device).to(self.buffers[key].dtype)
            self.buffers[key].index_copy_(0, idx, src)

    def can_sample(self, batch_size):
        return self.current_size >= batch_size

    def state_dict(self, with_buffer=True):
        """The cursor and the FILLED part of every buffer, on the host (with_buffer=False: an empty ring, cursor at 0)."""
        if not with_buffer:
            return {"current_idx": 0, "current_size": 0, "buffers": {k: v[:0].cpu() for k, v in self.buffers.items()}}
        return {"current_idx": int(self.current_idx), "current_size": int(self.current_size),
                "buffers": {k: v[:self.current_size].cpu() for k, v in self.buffers.items()}}

    def check_state_dict(self, sd):
        n = int(sd["current_size"])
        if tuple(sd["buffers"]) != tuple(self.keys) or n > self.size:
            raise ValueError(f"ring state with keys {tuple(sd['buffers'])} and {n} episodes for a ring of {self.keys}, size {self.size}")
        for k, v in sd["buffers"].items():
            if tuple(v.shape) != (n,) + tuple(self.buffers[k].shape[1:]):
                raise ValueError(f"ring state: {k} is {tuple(v.shape)}, the ring's episodes are {tuple(self.buffers[k].shape[1:])}")

    def load_state_dict(self, sd):
        self.check_state_dict(sd)
        n = int(sd["current_size"])
        for k, v in sd["buffers"].items():
            self.buffers[k][:n].copy_(v)
        self.current_idx, self.current_size = int(sd["current_idx"]), n

    def sample(self, batch_size, generator=None):
        """Uniform with replacement over the filled part (replay_buffer.py:63-68), drawn on the device."""
        idx = torch.randint(0, self.current_size, (batch_size,), device=self.device, generator=generator)
        return {k: v.index_select(0, idx) for k, v in self.buffers.items()}

    def latest_indices(self, batch_size):
        """The `batch_size` most recently stored slots, oldest first (replay_buffer.py:70-79)."""
        assert self.can_sample(batch_size)
        return [(self.current_idx - batch_size + k) % self.current_size for k in range(batch_size)]

    def sample_latest(self, batch_size):
        idx = torch.as_tensor(self.latest_indices(batch_size), device=self.device)
        return {k: v.index_select(0, idx) for k, v in self.buffers.items()}


class DeviceReplayBuffer(_EpisodeRing):
    def __init__(self, args, buffer_size, device="cuda", dtype=torch.float32):
        self.args = args
        self.n_actions, self.n_agents = args.n_actions, args.n_agents
        self.state_shape, self.obs_shape = args.state_shape, args.obs_shape
        self.size, self.episode_limit = int(buffer_size), args.episode_limit
        self.current_idx = 0
        self.current_size = 0
        obs = self.obs_shape + (args.map_size ** 2 if getattr(args, "conv", False) else 0)  # replay_buffer.py:18-21
        S, T, n, A = self.size, self.episode_limit, self.n_agents, self.n_actions
        shapes = {"o": (S, T, n, obs), "u": (S, T, n, 1), "s": (S, T, self.state_shape), "r": (S, T, 1),
                  "o_next": (S, T, n, obs), "s_next": (S, T, self.state_shape), "avail_u": (S, T, n, A),
                  "avail_u_next": (S, T, n, A), "u_onehot": (S, T, n, A), "padded": (S, T, 1), "terminated": (S, T, 1)}
        self.device = torch.device(device)
        self.buffers = {k: torch.empty(shapes[k], dtype=dtype, device=self.device) for k in KEYS}


class CompactReplayBuffer(_EpisodeRing):
    """The ring over COMPACT_KEYS, flight only: 2 060 628 bytes per 3-agent episode instead of 12 136 800 (T = 200, 15
    targets).  Slots, cursor, sampling and generator use are DeviceReplayBuffer's; `sample` returns compact batches, which
    the learners take as they are (expand_compact gives the 11 dense keys of one)."""
    keys = COMPACT_KEYS

    def __init__(self, args, buffer_size, device="cuda", dtype=torch.float32):
        if not getattr(args, "conv", False):
            raise ValueError(f"CompactReplayBuffer is for the flight variant: an observation of "
                             f"{getattr(args, 'env', 'flight_easy')!r} carries no map (use DeviceReplayBuffer)")
        self.args = args
        self.n_actions, self.n_agents = args.n_actions, args.n_agents
        self.state_shape, self.obs_shape = args.state_shape, args.obs_shape
        self.size, self.episode_limit = int(buffer_size), args.episode_limit
        self.current_idx = 0
        self.current_size = 0
        S, T, n = self.size, self.episode_limit, self.n_agents
        shapes = {"map": (S, T + 1, args.map_size ** 2), "s_full": (S, T + 1, self.state_shape), "u": (S, T, n, 1),
                  "r": (S, T, 1), "padded": (S, T, 1), "terminated": (S, T, 1)}
        self.device = torch.device(device)
        self.buffers = {k: torch.empty(shapes[k], dtype=dtype, device=self.device) for k in COMPACT_KEYS}
