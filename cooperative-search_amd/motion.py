"""Moving targets: the target-motion kernel's definition, its launch, and the env that moves its targets
(include/coopsearch.h: cs_move_targets).

The reference's targets never move: tgt is written by reset() and only read afterwards, so swept ground never goes stale and the
task saturates.  This module is the opt-in scenario in which unfound targets move -- a seeded random walk over 16 headings, or an
evasion of the nearest agent inside a sensing radius.

`move_targets_torch` is the DEFINITION, in stock torch ops on any device: fp64, every operation rounded once, no sqrt, no division
and no transcendental; the kernel (csrc/motion.h) equals it bit for bit.  Per env b (global index g = env_offset + b) and target
slot j:

  moves     iff j < n_targets, bit j of CS_H_FOUND is clear and the env is live on entry -- the predicate by which cs_step with
            CS_FREEZE_DONE leaves an env alone: win bit of CS_H_FLAGS clear and CS_H_TIME_STEP < time_limit.  Every other double
            of tgt keeps its bits.
  heading   one of 16: CX[k], CY[k] = cos, sin(2 pi k / 16), the hex-float literals below (csrc/motion.h repeats them).
  walk      k = key >> 28, in uint32 arithmetic:
              fmix(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
              key = seed; for w in (g & 0xffffffff, g >> 32, CS_H_EPISODES, CS_H_TIME_STEP // persist, j): key = fmix(key ^ w) + 0x9E3779B9
            A pure function of the env's logical state and its global index: snapshots and resume need nothing new, a sharded
            batch equals the whole batch, and one state forked into several env indices diffuses differently in each.
  evade     d2_i = (x - ax_i)^2 + (y - ay_i)^2 for the agents i < n_agents.  If some d2_i <= sense * sense: the smallest such d2
            (lowest i on ties) gives (dx, dy) = (x - ax, y - ay), and k is the lowest index that maximises dx CX[k] + dy CY[k];
            otherwise k is the walk heading.
  move      x' = min(max(x + speed CX[k], 0), map_size), y' likewise with CY (two selects: a NaN stays a NaN).
  speed 0   nothing moves: the input comes back bit for bit (and cs_move_targets launches nothing).

`MovingTargetEnv` moves the targets at the START of every `every`-th step, before the agents, so s[t + 1] is the true state after
step t and a policy acts without knowing the coming move.
"""
import dataclasses
import functools
import math

import torch

from . import _lib
from .env import BatchedFlightEnv

HEADINGS = 16
# cos and sin of 2 pi k / 16, k = 0..15, evaluated once in Python doubles (math.cos / math.sin) and frozen as literals:
# csrc/motion.h holds the same ones (tests/test_motion_cpu.py compares the two)
CX = tuple(float.fromhex(v) for v in (
    "0x1.0000000000000p+0", "0x1.d906bcf328d46p-1", "0x1.6a09e667f3bcdp-1", "0x1.87de2a6aea964p-2",
    "0x1.1a62633145c07p-54", "-0x1.87de2a6aea962p-2", "-0x1.6a09e667f3bccp-1", "-0x1.d906bcf328d46p-1",
    "-0x1.0000000000000p+0", "-0x1.d906bcf328d47p-1", "-0x1.6a09e667f3bcep-1", "-0x1.87de2a6aea96dp-2",
    "-0x1.a79394c9e8a0ap-53", "0x1.87de2a6aea967p-2", "0x1.6a09e667f3bcbp-1", "0x1.d906bcf328d44p-1"))
CY = tuple(float.fromhex(v) for v in (
    "0x0.0p+0", "0x1.87de2a6aea963p-2", "0x1.6a09e667f3bccp-1", "0x1.d906bcf328d46p-1",
    "0x1.0000000000000p+0", "0x1.d906bcf328d46p-1", "0x1.6a09e667f3bcdp-1", "0x1.87de2a6aea965p-2",
    "0x1.1a62633145c07p-53", "-0x1.87de2a6aea961p-2", "-0x1.6a09e667f3bccp-1", "-0x1.d906bcf328d44p-1",
    "-0x1.0000000000000p+0", "-0x1.d906bcf328d45p-1", "-0x1.6a09e667f3bcep-1", "-0x1.87de2a6aea96ep-2"))
MODES = {"walk": 0, "evade": 1}   # CS_MOTION_WALK, CS_MOTION_EVADE
MAX_PERSIST = 65536
MAX_ENV_OFFSET = 1 << 62
_M32 = 0xFFFFFFFF


@dataclasses.dataclass(frozen=True)
class TargetMotion:
    """How targets move.  mode "walk" | "evade"; speed: cells per move (finite, 0..map_size); every: env steps between moves
    (>= 1); persist: time steps for which a walk heading is kept (1..65536); sense: evade only, the radius inside which a target
    sees an agent (finite, 0..2 map_size); seed: uint32 seed of the heading keys.  The bounds that depend on the map are
    checked by `check(map_size)`, the rest at construction."""
    mode: str = "walk"
    speed: float = 0.0
    every: int = 1
    persist: int = 1
    sense: float = 0.0
    seed: int = 0

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"TargetMotion: mode must be 'walk' or 'evade', got {self.mode!r}")
        for name in ("speed", "sense"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"TargetMotion: {name} must be a finite number >= 0, got {v!r}")
            object.__setattr__(self, name, float(v))
        for name, lo, hi in (("every", 1, None), ("persist", 1, MAX_PERSIST), ("seed", 0, _M32)):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or v < lo or (hi is not None and v > hi):
                raise ValueError(f"TargetMotion: {name} must be a whole number {lo}..{'' if hi is None else hi}, got {v!r}")
            object.__setattr__(self, name, int(v))

    def check(self, map_size):
        """The map-dependent bounds: speed <= map_size, sense <= 2 map_size.  Returns self."""
        if self.speed > map_size:
            raise ValueError(f"TargetMotion: speed must be 0..map_size = {map_size}, got {self.speed!r}")
        if self.sense > 2 * map_size:
            raise ValueError(f"TargetMotion: sense must be 0..2 map_size = {2 * map_size}, got {self.sense!r}")
        return self

    @classmethod
    def from_args(cls, args):
        """The spec an args namespace asks for: target_speed, target_motion (the mode), target_move_every, target_persist,
        target_sense, target_motion_seed; absent fields take the defaults."""
        return cls(mode=getattr(args, "target_motion", "walk"), speed=getattr(args, "target_speed", 0.0),
                   every=getattr(args, "target_move_every", 1), persist=getattr(args, "target_persist", 1),
                   sense=getattr(args, "target_sense", 0.0), seed=getattr(args, "target_motion_seed", 0))


def _team(env):
    """(n_agents, n_targets, map_size, time_limit) of an env or an args namespace."""
    m = env.target_num
    if int(env.map_size) != env.map_size:
        raise ValueError(f"motion: map_size must be a whole number of cells, got {env.map_size!r}")
    n, m, side, limit = int(env.n_agents), int(m), int(env.map_size), int(env.time_limit)
    if not 1 <= n <= _lib.MAX_AGENTS or not 1 <= m <= _lib.MAX_TARGETS:
        raise ValueError(f"motion: n_agents must be 1..{_lib.MAX_AGENTS} and target_num 1..{_lib.MAX_TARGETS}")
    return n, m, side, limit


def _check_offset(env_offset):
    env_offset = int(env_offset)
    if not 0 <= env_offset <= MAX_ENV_OFFSET:
        raise ValueError(f"motion: env_offset must be 0..2^62, got {env_offset}")
    return env_offset


def _fmix(x):
    """MurmurHash3's 32-bit finaliser on int64 tensors that hold uint32 values (the products are split so that nothing passes
    2^63)."""
    def mul(v, c):
        return (v * (c & 0xFFFF) + (((v * (c >> 16)) & 0xFFFF) << 16)) & _M32
    x = x ^ (x >> 16)
    x = mul(x, 0x85EBCA6B)
    x = x ^ (x >> 13)
    x = mul(x, 0xC2B2AE35)
    return x ^ (x >> 16)


def walk_headings(hdr, motion, env_offset=0):
    """int64 [B, 16]: the walk heading k of every target slot (module docstring), whether or not the target moves."""
    B, dev, i64 = int(hdr.shape[0]), hdr.device, torch.int64
    h = hdr.to(i64)
    g = _check_offset(env_offset) + torch.arange(B, dtype=i64, device=dev)
    j = torch.arange(16, dtype=i64, device=dev).view(1, 16)
    words = ((g & _M32).view(B, 1), ((g >> 32) & _M32).view(B, 1), (h[:, _lib.H_EPISODES] & _M32).view(B, 1),
             ((h[:, _lib.H_TIME_STEP] & _M32) // motion.persist).view(B, 1), j)
    key = torch.full((B, 16), motion.seed, dtype=i64, device=dev)
    for w in words:
        key = (_fmix(key ^ w) + 0x9E3779B9) & _M32
    return key >> 28


def moving_mask(hdr, n_targets, time_limit):
    """bool [B, 16]: the target slots that move (module docstring)."""
    h = hdr.to(torch.int64)
    j = torch.arange(16, dtype=torch.int64, device=hdr.device).view(1, 16)
    live = ((h[:, _lib.H_FLAGS] & 1) == 0) & (h[:, _lib.H_TIME_STEP] < time_limit)
    unfound = (((h[:, _lib.H_FOUND] & _M32).view(-1, 1) >> j) & 1) == 0
    return live.view(-1, 1) & unfound & (j < n_targets)


def move_targets_torch(tgt, agent, hdr, motion, env, env_offset=0):
    """The definition (module docstring): tgt float64 [B, 16, 2], agent float64 [B, 8, 4], hdr int32 [B, 16] -- the arrays of
    `BatchedFlightEnv.raw()` -- -> the moved tgt, a new tensor (the inputs are not written).  `env`: an env or an args namespace
    (n_agents, target_num, map_size, time_limit are read).  Stock EAGER torch ops on the tensors' device."""
    n, m, side, limit = _team(env)
    motion.check(side)
    B = int(tgt.shape[0]) if torch.is_tensor(tgt) and tgt.dim() == 3 else -1
    for name, t, dt, shape in (("tgt", tgt, torch.float64, (B, 16, 2)), ("agent", agent, torch.float64, (B, 8, 4)),
                               ("hdr", hdr, torch.int32, (B, _lib.H_WORDS))):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or B < 1 or t.device != tgt.device:
            raise ValueError(f"motion: {name} must be {dt} [B, {shape[1]}{', ' + str(shape[2]) if len(shape) > 2 else ''}] "
                             "with B >= 1, all on one device")
    if motion.speed == 0.0:
        return tgt.clone()
    dev, f64 = tgt.device, torch.float64
    x, y = tgt[:, :, 0], tgt[:, :, 1]
    k = walk_headings(hdr, motion, env_offset)
    cx, cy = torch.tensor(CX, dtype=f64, device=dev), torch.tensor(CY, dtype=f64, device=dev)
    if motion.mode == "evade":
        sense2 = motion.sense * motion.sense
        best = torch.full_like(x, math.inf)
        bdx, bdy = torch.zeros_like(x), torch.zeros_like(x)
        seen = torch.zeros_like(x, dtype=torch.bool)
        for i in range(n):   # the nearest agent inside the radius, lowest index on ties
            dx, dy = x - agent[:, i, 0].view(B, 1), y - agent[:, i, 1].view(B, 1)
            d2 = dx * dx + dy * dy
            take = (d2 <= sense2) & (d2 < best)
            best, bdx, bdy = torch.where(take, d2, best), torch.where(take, dx, bdx), torch.where(take, dy, bdy)
            seen = seen | take
        top = bdx * CX[0] + bdy * CY[0]
        kev = torch.zeros_like(k)
        for q in range(1, HEADINGS):   # the heading that leads away fastest, lowest index on ties
            s = bdx * CX[q] + bdy * CY[q]
            take = s > top
            top, kev = torch.where(take, s, top), torch.where(take, torch.full_like(kev, q), kev)
        k = torch.where(seen, kev, k)

    def clamp(v):
        v = torch.where(v < 0.0, torch.zeros_like(v), v)
        return torch.where(v > float(side), torch.full_like(v, float(side)), v)

    nx, ny = clamp(x + motion.speed * cx[k]), clamp(y + motion.speed * cy[k])
    moves = moving_mask(hdr, m, limit)
    return torch.stack((torch.where(moves, nx, x), torch.where(moves, ny, y)), dim=2)


def split_runs(phase, T, every):
    """How a call of T steps that starts at step `phase` is cut at the multiples of `every`: a list of (start, stop, move) with
    the runs start..stop-1 covering 0..T-1 once, in order, maximal with no move inside; move: a move precedes the run's first
    step, i.e. its global step phase + start is a multiple of `every`."""
    phase, T, every = int(phase), int(T), int(every)
    if phase < 0 or T < 0 or every < 1:
        raise ValueError("split_runs: phase >= 0, T >= 0 and every >= 1")
    runs, start = [], 0
    while start < T:
        stop = min(T, start + every - (phase + start) % every)
        runs.append((start, stop, (phase + start) % every == 0))
        start = stop
    return runs


# the op layer, _lib.torch_ops(), with this module's words for a failure to load it; a module attribute, so that a test can wrap it
_ops = functools.partial(_lib.torch_ops_for, "the target-motion kernel needs")


def move_targets(env, motion, env_offset=None):
    """One move of env's targets in place in its state blob: the kernel, one launch on the current stream, no synchronisation
    (none at all when speed is 0).  get_obs() / get_state() lag until the next step() or refresh()."""
    off = env.env_offset if env_offset is None else env_offset
    _ops().move_targets(env._cfg_t, env._blob, MODES[motion.mode], motion.persist, motion.seed, motion.speed, motion.sense,
                        _check_offset(off))


class MovingTargetEnv(BatchedFlightEnv):
    """A `BatchedFlightEnv` (either variant, same arguments) whose unfound targets move: `target_motion`, a `TargetMotion`
    (default: `TargetMotion.from_args(args)`).  Targets move at the START of a step, before the agents: a move precedes the
    object's step s iff s % every == 0, where s = `motion_phase` counts the steps executed through this object since the last
    reset() without a mask (settable: a resumed env continues where the snapshot was taken).  `rollout`, `rollout_policy` and
    `collect_flight` cut their T steps at those multiples (`split_runs`) and make the parent's call per run on slices of the
    tables, so one call equals T step() calls.  With speed 0 every method is the parent's and no motion launch is ever made.
    The B = 1 adapters and the inside of the fused rollout kernels know nothing of moving targets."""

    def __init__(self, args, *a, target_motion=None, **kw):
        motion = TargetMotion.from_args(args) if target_motion is None else target_motion
        if not isinstance(motion, TargetMotion):
            raise TypeError("MovingTargetEnv: target_motion must be a TargetMotion")
        self.motion = motion.check(int(args.map_size))
        self.motion_phase = 0
        super().__init__(args, *a, **kw)   # ends with reset(init=True): step 0 comes next
        _check_offset(self.env_offset + self.batch)

    @property
    def moving(self):
        return self.motion.speed > 0.0

    def move_targets(self):
        """One move now, whatever the phase (the live get_obs() / get_state() lag until the next step() or refresh())."""
        if self.moving:
            move_targets(self, self.motion)

    def reset(self, init=False, mask=None):
        super().reset(init=init, mask=mask)
        if mask is None:
            self.motion_phase = 0

    # ---------------------------------------------------------------------------------------------------------- plumbing
    def _validate_actions(self, a):
        """CS_CHECK_ACTIONS over a whole action table BEFORE the first move, so that a bad action in a later run still leaves
        the envs untouched: the parent's IndexError, worded as its check words it.  Synchronises, as that check does."""
        bad = ((a < 0) | (a > 2)).reshape(-1).nonzero()
        if bad.numel():
            i = int(bad[0])
            per_step, n = self.batch * self.n_agents, self.n_agents
            raise IndexError(f"list index out of range: action {int(a.reshape(-1)[i])} of step {i // per_step}, env "
                             f"{(i % per_step) // n}, agent {i % n} is not in 0..2 (dyaw[act], flight_env_easy.py:262; the "
                             "batched path takes no negative indices)")

    def _tables(self, who, spec, out):
        """The whole call's tables ({key: (shape, dtype)}), allocated once or validated: contiguous, T-major."""
        out = dict(out) if out else {}
        for k, (shape, dt) in spec.items():
            if out.get(k) is None:
                out[k] = torch.empty(shape, dtype=dt, device=self.device)
            elif out[k].numel() * out[k].element_size() != torch.Size(shape).numel() * dt.itemsize or not out[k].is_contiguous() \
                    or out[k].dim() < 1 or out[k].shape[0] != shape[0]:
                raise ValueError(f"{who}(out=): bad destination for {k!r}")
        return out

    def _runs(self, T, call):
        """call(start, stop, last) for every run of a T-step call, the move first where one is due."""
        runs = split_runs(self.motion_phase, T, self.motion.every)
        saved = self.check_actions
        self.check_actions = False   # (rollout has validated the whole table; the closed loops choose their own actions)
        try:
            for start, stop, move in runs:
                if move:
                    self.move_targets()
                call(start, stop, stop == T)
                self.motion_phase += stop - start
        finally:
            self.check_actions = saved

    # ------------------------------------------------------------------------------------------------------ the step calls
    def step(self, actions, out=None):
        if not self.moving:
            return super().step(actions, out=out)
        if self.motion_phase % self.motion.every == 0:
            if self.check_actions:
                self._validate_actions(self._actions(actions, (self.batch,)))
            self.move_targets()
        res = super().step(actions, out=out)
        self.motion_phase += 1
        return res

    def rollout(self, actions, emit=True, out=None, update_views=True):
        T = int(actions.shape[0])
        if not self.moving or T < 1:
            return super().rollout(actions, emit=emit, out=out, update_views=update_views)
        a = self._actions(actions, (T, self.batch))
        B, n = self.batch, self.n_agents
        if out is not None:
            emit = out.get("obs") is not None and out.get("state") is not None
        spec = dict(reward=((T, B), torch.float32), terminated=((T, B), torch.uint8), win=((T, B), torch.uint8))
        if emit:
            spec.update(obs=((T, B, n, self.obs_width), torch.float32), state=((T, B, self.state_shape), torch.float32))
        out = self._tables("rollout", spec, out)
        if self.check_actions:
            self._validate_actions(a)
        parent = super().rollout

        def call(start, stop, last):
            parent(a[start:stop], out={k: (out.get(k)[start:stop] if k in spec else None) for k in ("reward", "terminated", "win", "obs", "state")},
                   update_views=update_views and last)
        self._runs(T, call)
        out.setdefault("obs", None)
        out.setdefault("state", None)
        out["terminated"], out["win"] = (out[k].view(torch.uint8).view(torch.bool) for k in ("terminated", "win"))
        return out

    def _closed_loop_spec(self, T, extra):
        B, n = self.batch, self.n_agents
        spec = dict(reward=((T, B), torch.float32), terminated=((T, B), torch.uint8), win=((T, B), torch.uint8),
                    actions=((T, B, n), torch.int64))
        spec.update(extra)
        return spec

    def rollout_policy(self, agents, T, epsilon=0.0, evaluate=True, emit=True, out=None, update_views=True, eps_env=None,
                       anneal=0.0, min_epsilon=0.0, per_step=False, eps_trace=None):
        T = int(T)
        kw = dict(eps_env=eps_env, anneal=anneal, min_epsilon=min_epsilon, per_step=per_step)
        if not self.moving or T < 1:
            return super().rollout_policy(agents, T, epsilon, evaluate, emit=emit, out=out, update_views=update_views,
                                          eps_trace=eps_trace, **kw)
        B, n = self.batch, self.n_agents
        extra = {}
        if emit or (out and out.get("obs") is not None):
            extra = dict(obs=((T, B, n, self.obs_width), torch.float32), state=((T, B, self.state_shape), torch.float32))
        spec = self._closed_loop_spec(T, extra)
        out = self._tables("rollout_policy", spec, out)
        if eps_trace is not None and (eps_trace.numel() != T * B or not eps_trace.is_contiguous()):
            raise ValueError(f"rollout_policy: eps_trace must be a contiguous float64 device tensor of {T * B} elements")
        trace = None if eps_trace is None else eps_trace.view(T, B)
        parent = super().rollout_policy

        def call(start, stop, last):
            parent(agents, stop - start, epsilon, evaluate, emit=False, out={k: out[k][start:stop] for k in spec},
                   update_views=update_views and last, eps_trace=None if trace is None else trace[start:stop], **kw)
        self._runs(T, call)
        out["terminated"], out["win"] = (out[k].view(torch.uint8).view(torch.bool) for k in ("terminated", "win"))
        return out

    def collect_flight(self, agents, T, epsilon=0.0, evaluate=True, out=None, update_views=True, eps_env=None, anneal=0.0,
                       min_epsilon=0.0, per_step=False, eps_trace=None):
        T = int(T)
        kw = dict(eps_env=eps_env, anneal=anneal, min_epsilon=min_epsilon, per_step=per_step)
        if not self.moving or T < 1 or not self.flight:
            return super().collect_flight(agents, T, epsilon, evaluate, out=out, update_views=update_views, eps_trace=eps_trace, **kw)
        B = self.batch
        spec = self._closed_loop_spec(T, dict(map=((T + 1, B, self.cells), torch.float32),
                                              state=((T + 1, B, self.state_shape), torch.float32)))
        out = self._tables("collect_flight", spec, out)
        if eps_trace is not None and (eps_trace.numel() != T * B or not eps_trace.is_contiguous()):
            raise ValueError(f"collect_flight: eps_trace must be a contiguous float64 device tensor of {T * B} elements")
        trace = None if eps_trace is None else eps_trace.view(T, B)
        state_tab = out["state"].view(T + 1, B, self.state_shape)
        entry = torch.empty(B, self.state_shape, dtype=torch.float32, device=self.device)
        parent = super().collect_flight
        phase0, every = self.motion_phase, self.motion.every

        def call(start, stop, last):
            # a run's entry row is the state its call finds: AFTER the run's move.  The table's row `start` is the state after
            # step start - 1, before the move (row 0: the state on entry of the whole call), so it is kept and put back
            moved = (phase0 + start) % every == 0
            if moved:
                entry.copy_(state_tab[start])
            sub = {k: out[k][start:stop] for k in ("actions", "reward", "terminated", "win")}
            sub.update(map=out["map"][start:stop + 1], state=out["state"][start:stop + 1])
            parent(agents, stop - start, epsilon, evaluate, out=sub, update_views=update_views and last,
                   eps_trace=None if trace is None else trace[start:stop], **kw)
            if moved:
                state_tab[start].copy_(entry)
        if phase0 % every == 0:   # row 0 as the call finds the envs, before the first move
            self._ops.env_emit(self._cfg_t, self._blob, None, state_tab[0])
        self._runs(T, call)
        out["terminated"], out["win"] = (out[k].view(torch.uint8).view(torch.bool) for k in ("terminated", "win"))
        return out


def make_env(args, *a, **kw):
    """A `MovingTargetEnv` when args.target_speed > 0, a plain `BatchedFlightEnv` otherwise (same arguments)."""
    if float(getattr(args, "target_speed", 0) or 0) > 0:
        return MovingTargetEnv(args, *a, **kw)
    kw.pop("target_motion", None)
    return BatchedFlightEnv(args, *a, **kw)
