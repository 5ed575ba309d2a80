"""Env snapshot / restore: an env's logical state as one record per env (include/coopsearch.h: cs_snapshot, cs_restore).

The state blob is not copyable field by field -- the MT19937 row's form depends on the kernel that ran last, words 624..655
mirror words 0..31, the hit tape is accepted by threshold and word count alone, and the map sweep's pending bits are leftovers
of the last launch -- so capture and restore live behind the ABI.  A record is per env: it goes to an
env of any batch size or shard whose variant, n_agents, n_targets and map_size are the record's.  Everything a `cs_config`
holds besides those four (time_limit, detect_prob, view_range, velocity, forces, agent_mode, target file) belongs to the
RESTORING env.

The calls go through torch.ops.coopsearch (csrc/torch_ops.cpp) whatever the env's binding is; there is no ctypes twin.
"""
import torch

from . import _lib

FORMAT_VERSION = 1   # CS_SNAPSHOT_VERSION
META_FIELDS = ("variant", "n_agents", "n_targets", "map_size", "version")


def env_meta(env):
    """What a record of `env` is bound to."""
    return dict(variant=str(env.variant), n_agents=int(env.n_agents), n_targets=int(env.target_num), map_size=int(env.map_size),
                version=FORMAT_VERSION)


def record_bytes(meta):
    """cs_snapshot_bytes as a formula: 16 + 16 header words, 16 x 2 + 8 x 4 doubles, 624 MT19937 words [+ the float map]."""
    return 4 * (16 + 16) + 8 * (32 + 32) + 4 * 624 + (4 * meta["map_size"] ** 2 if meta["variant"] == "flight" else 0)


class EnvSnapshot:
    """`records` uint8 [count, bytes] (one record per env, on any device) and `meta` (variant, n_agents, n_targets, map_size,
    version)."""

    def __init__(self, records, meta):
        meta = {k: meta[k] for k in META_FIELDS}
        if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] != record_bytes(meta):
            raise ValueError(f"EnvSnapshot: records must be uint8 [count, {record_bytes(meta)}] for {meta}")
        self.records, self.meta = records, meta

    def __len__(self):
        return int(self.records.shape[0])

    def to(self, device):
        return EnvSnapshot(self.records.to(device), self.meta)

    def cpu(self):
        return self.to("cpu")

    def check(self, meta):
        """ValueError naming the first field of `meta` (an env's `env_meta`) that this snapshot does not share."""
        for k in META_FIELDS:
            if self.meta[k] != meta[k]:
                raise ValueError(f"EnvSnapshot: {k} is {self.meta[k]!r}, the env's is {meta[k]!r}")

    def state_dict(self):
        """Plain tensors and builtins: what torch.save takes."""
        return {"records": self.records, "meta": dict(self.meta)}

    @classmethod
    def from_state_dict(cls, sd):
        return cls(sd["records"], sd["meta"])


def _index(idx, env, name):
    if idx is None:
        return None
    idx = torch.as_tensor(idx, device=env.device)
    if idx.dtype != torch.int64:
        idx = idx.to(torch.int64)
    if idx.dim() != 1:
        raise ValueError(f"{name} must be a 1-D index")
    return idx.contiguous()


def snapshot(env, envs=None):
    """Records of the envs `envs` (int64 indices; None: all, in order) of a BatchedFlightEnv.  The env is only read; nothing
    synchronises when `envs` is None or a device tensor."""
    ops = _lib.torch_ops_for("env snapshots need")
    meta = env_meta(env)
    idx = _index(envs, env, "envs")
    count = env.batch if idx is None else int(idx.numel())
    records = torch.empty(count, int(ops.snapshot_bytes(env._cfg_t)), dtype=torch.uint8, device=env.device)
    if count:
        ops.env_snapshot(env._cfg_t, env._blob, idx, records)
    return EnvSnapshot(records, meta)


def restore(env, snap, src=None, dst=None, status=None):
    """Env dst[i] takes record src[i] of `snap` (None: i; src may repeat -- a fork; dst entries must be distinct).  A `meta`
    mismatch raises ValueError before anything is launched.  The live get_obs() / get_state() buffers are refreshed and the next
    step() refreshes the hit tapes.  `status` (int32 [4] on the env's device) receives cs_restore's verdict on the indices and
    record headers: {0, -1, -1, 0}, or {1, kind, entry, value} for the first refused entry, whose env stays untouched."""
    ops = _lib.torch_ops_for("env snapshots need")
    snap.check(env_meta(env))
    src, dst = _index(src, env, "src"), _index(dst, env, "dst")
    if src is not None and dst is not None and src.numel() != dst.numel():
        raise ValueError("restore: src and dst must have the same length")
    count = src.numel() if src is not None else (dst.numel() if dst is not None else len(snap))
    if (src is None and count > len(snap)) or (dst is None and count > env.batch):
        raise ValueError(f"restore: {count} entries for {len(snap)} records and a batch of {env.batch}")
    records = snap.records if snap.records.device == env.device else snap.records.to(env.device)
    ops.env_restore(env._cfg_t, env._blob, records.contiguous(), src, dst, status, env._obs, env._state)
    from .env import STEP_ADVANCE_EVERY
    env._steps_since_advance = STEP_ADVANCE_EVERY
