"""Swept-area accounting of recorded episodes, and the exploration bonus it gives (include/coopsearch.h: cs_sweep_episodes).

The found-fraction curve and the episode reward say where the 15 targets of one layout happen to lie; they do not say how a team
searches.  This module measures that: how much of the map the sensors have swept by row t of an episode, and how much of a
row's sweeping lands on ground already seen.  Its per-step increment -- the number of cells a step sweeps for the first time --
is the count-based exploration bonus of `sweep_bonus` / `args.sweep_bonus` (runner.Runner.train).

`sweep_episodes_torch` is the DEFINITION, in stock torch ops; the kernel (csrc/sweep.h) reproduces its three outputs element
for element.  DESIGN.md section 18 has the text; in short, per episode:

  rows      states float32 [E, T1, S]: row 0 is the reset pose, row t + 1 the state after step t (render.episode_tables).  Only
            the first 4n floats of a row are read: agent i = (xn, yn, cos, sin) at 4i.  Row t is valid if t < clamp(counts[e],
            0, T1); what the other rows hold, NaN included, changes nothing.
  quantise  baseline.quantise's positions, unchanged: X = rint((xn * half + half) * 16) clamped to +-2^15, float32, every
            operation rounded once; everything after is integer.
  sweep     cell ix * side + iy (centre 16 ix + 8, 16 iy + 8) is swept at row t if dx^2 + dy^2 <= (16 view_range)^2 for any
            agent at that row -- the sweep test of the coverage policy.
  first     int32 [E, side * side]: the first valid row at which the cell is swept, -1 if never.
  new_cells int32 [E, T1]: the number of cells with first == t;  seen_cells int32 [E, T1]: the number of cells swept at row t
            (the union of the n discs).  Both are 0 at and past the count.
"""
import collections

import torch

from . import _lib
from . import baseline as _bl
from . import render as _render

SweepResult = collections.namedtuple("SweepResult", ["first", "new_cells", "seen_cells"])


def _check_params(n, side, view_range):
    _bl._check_team("sweep", n, side, view_range)


def _check(states, counts, n, side, view_range):
    _check_params(n, side, view_range)
    if not torch.is_tensor(states) or states.dim() != 3 or states.dtype != torch.float32 or min(states.shape[:2]) < 1 \
            or states.shape[2] < 4 * n:
        raise ValueError(f"sweep: states must be float32 [E, T1, S] with E >= 1, T1 >= 1 and S >= 4 n_agents = {4 * n}")
    if not torch.is_tensor(counts) or counts.dtype != torch.int32 or tuple(counts.shape) != (states.shape[0],) \
            or counts.device != states.device:
        raise ValueError(f"sweep: counts must be int32 [{states.shape[0]}] on the states' device")


def sweep_episodes_torch(states, counts, n_agents, side, view_range):
    """The definition (module docstring): states float32 [E, T1, S >= 4n], counts int32 [E] -> SweepResult(first int32
    [E, side * side], new_cells int32 [E, T1], seen_cells int32 [E, T1]).  Stock EAGER torch ops on the tensors' device (the
    quantisation must not be contracted into a fused multiply-add: see baseline.coverage_actions_torch)."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    _check(states, counts, n, side, view_range)
    dev = states.device
    E, T1, S = (int(v) for v in states.shape)
    R2 = (16 * view_range) ** 2
    X, Y = _bl.quantise_positions(states.reshape(E * T1, S), n, side)
    X, Y = X.view(E, T1, n), Y.view(E, T1, n)
    centre = _bl.cell_centres(side, dev)
    valid = torch.arange(T1, dtype=torch.int64, device=dev).view(1, T1) < counts.to(torch.int64).clamp(0, T1).view(E, 1)   # [E, T1]
    first = torch.full((E, side * side), -1, dtype=torch.int32, device=dev)
    new_cells = torch.zeros(E, T1, dtype=torch.int32, device=dev)
    seen_cells = torch.zeros(E, T1, dtype=torch.int32, device=dev)
    for t in range(T1):
        seen = _bl.swept(centre, X[:, t], Y[:, t], R2) & valid[:, t].view(E, 1)
        fresh = seen & (first < 0)
        first = torch.where(fresh, torch.full_like(first, t), first)
        new_cells[:, t] = fresh.sum(1)
        seen_cells[:, t] = seen.sum(1)
    return SweepResult(first, new_cells, seen_cells)


def _impl_for(tensor, impl):
    """impl None: the kernel for device tensors, the definition for host tensors (as render.render_episodes chooses)."""
    if impl is None:
        return "hip" if tensor.is_cuda else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError("impl must be 'hip' (the kernel of csrc/sweep.h) or 'torch' (the definition)")
    return impl


def sweep_episodes(states, counts, n_agents, side, view_range, impl="hip"):
    """SweepResult of E recorded episodes.  impl = "hip": the kernel, one launch on the current stream, no synchronisation
    (the op checks dtypes, shapes and contiguity); "torch": the definition, on the tensors' device."""
    impl = _impl_for(states, impl)
    if impl == "torch":
        return sweep_episodes_torch(states, counts, n_agents, side, view_range)
    if not torch.is_tensor(states) or not states.is_cuda:
        raise ValueError("sweep_episodes(impl='hip') runs a HIP kernel and the states are not on a GPU: there is no CPU "
                         "fallback (impl='torch' runs the definition anywhere)")
    n, side, view_range = int(n_agents), int(side), int(view_range)
    _check_params(n, side, view_range)
    if states.dim() != 3:
        raise ValueError("sweep: states must be float32 [E, T1, S]")
    E, T1 = int(states.shape[0]), int(states.shape[1])
    dev = states.device
    out = SweepResult(torch.empty(E, side * side, dtype=torch.int32, device=dev), torch.empty(E, T1, dtype=torch.int32, device=dev),
                      torch.empty(E, T1, dtype=torch.int32, device=dev))
    _lib.torch_ops_for("the sweep kernel needs").sweep_episodes(states, counts, out.first, out.new_cells, out.seen_cells, n, side,
                                                                view_range)
    return out


def _team(args):
    """(n_agents, side, view_range) of an env or an args namespace."""
    if int(args.view_range) != args.view_range or int(args.map_size) != args.map_size:
        raise ValueError(f"sweep: view_range and map_size must be whole numbers of cells, got {args.view_range!r} and {args.map_size!r}")
    return int(args.n_agents), int(args.map_size), int(args.view_range)


def sweep_batch(batch, args, impl="hip"):
    """SweepResult of an episode batch of either format (the reference's 11 keys, or replay.COMPACT_KEYS) through
    render.episode_tables; `args`: an env or an args namespace (n_agents, map_size, view_range are read)."""
    n, side, view_range = _team(args)
    states, _maps, counts = _render.episode_tables(batch, args, with_maps=False)
    return sweep_episodes(states, counts, n, side, view_range, impl=impl)


def swept_curve(result):
    """float64 [T1]: the share of the map swept by row t, the mean over episodes of cumsum(new_cells) / side^2.  Rows after an
    episode's end hold its final value (new_cells is 0 there)."""
    cells = int(result.first.shape[1])
    return (result.new_cells.to(torch.float64).cumsum(1) / cells).mean(0)


def sweep_efficiency(result):
    """Newly swept cells per swept cell over the whole batch: sum(new_cells) / sum(seen_cells) (1: no sweeping ever lands on
    ground already seen).  A Python float; synchronises."""
    seen = int(result.seen_cells.sum())
    return float(int(result.new_cells.sum())) / seen if seen else 0.0


def sweep_bonus(batch, args, beta, impl="hip"):
    """The exploration bonus of an episode batch, float32 [E, T, 1]: beta * new_cells[:, 1:].  r[e, t] pays for the move into
    row t + 1; row 0, the reset pose, earns nothing; a padded step gets 0 (its row lies at or past the count)."""
    new_cells = sweep_batch(batch, args, impl=impl).new_cells
    return (new_cells[:, 1:].to(torch.float32) * float(beta)).unsqueeze(-1)


def with_sweep_bonus(batch, args, beta, impl=None):
    """A shallow copy of the batch dict whose "r" is r + sweep_bonus: the stored batch (a ring's own tensors) is never
    modified.  impl None: the kernel where the batch lives on a GPU, the definition for a host batch."""
    out = dict(batch)
    out["r"] = batch["r"] + sweep_bonus(batch, args, beta, impl=_impl_for(batch["r"], impl)).to(batch["r"].dtype)
    return out


def collect_sweep_data(collector, policy, batches=1, init=True, impl="hip"):
    """`batches` calls of collector.generate_episodes(policy=..., init=init), swept: {"curve": float64 [T + 1], percent of the
    map swept by row t, "efficiency": sum(new_cells) / sum(seen_cells), "targets_find", "steps": means over the episodes,
    "episodes"}.  One process: no reduction across ranks."""
    env = collector.env
    curve, new, seen, found, steps, episodes = None, 0, 0, 0.0, 0.0, 0
    for _ in range(int(batches)):
        episode, _reward, _win, targets_find = collector.generate_episodes(policy=policy, init=init)
        res = sweep_batch(episode, env, impl=impl)
        E = int(res.first.shape[0])
        part = swept_curve(res) * E
        curve = part if curve is None else curve + part
        new, seen = new + int(res.new_cells.sum()), seen + int(res.seen_cells.sum())
        found += float(targets_find.to(torch.float64).sum())
        steps += float((1 - episode["padded"].to(torch.float64)).sum())
        episodes += E
    return {"curve": (100.0 * curve / episodes).cpu().numpy(), "efficiency": float(new) / seen if seen else 0.0,
            "targets_find": found / episodes, "steps": steps / episodes, "episodes": episodes}
