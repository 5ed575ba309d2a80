"""The planner scored on the density predicted along its horizon (include/coopsearch.h: cs_belief_forecast and
cs_plan_forecast_actions).

`PlanAgents` scores a plan of D segments of S steps on the density of NOW.  Moving targets leave that density within a few steps:
against evaders at speed 1.0 the planner over the density filter finds fewer targets than the filter alone (DESIGN.md section
21).  The cure is to run the filter's prediction step forward along the plan and to score segment d on the density at the time
the segment ends.

Two DEFINITIONS, in stock eager torch ops on any device, all integer; the kernels (csrc/forecast.h) reproduce them element for
element:

  forecast_torch               F_{-1} = clamp(grid, 0, CAP), CAP = 2^19; F_d = belief.predict_torch applied moves[d] times to
                               F_{d-1}, every time with prev = pos; a level with moves[d] == 0 is a copy of the level before.
                               stack = (F_0 .. F_{L-1}), int32 [B, L, side * side].
  plan_forecast_actions_torch  plan.plan_actions_torch on a working copy W = clamp(stack, 0, CAP) of `depth` levels: the gain of
                               a node of level d is summed over W[:, d]; the disc test, the exclusion of the ancestors' discs,
                               the Q8 weights and the lowest-s tie rule are unchanged; after an agent has chosen, the union of
                               its sequence's D discs is zeroed in EVERY level.  plan.py's bounds hold per level: a gain is at
                               most 2^31, the D gains of one sequence are taken over disjoint cells, a score is at most 2^39.
                               On a stack of identical levels it IS plan.plan_actions_torch on that level.

`ForecastAgents.choose_action(state, moved, t)` lets its `BeliefAgents` advance the grid (whose `prev` then holds the positions of
`state`, the positions the next target move is made against), counts the target moves that fall into each segment,
moves[d] = #{u in [t + d S, t + (d + 1) S) : u % every == 0} (a move precedes step u iff u % every == 0), forecasts and plans.

Not modelled: the agents are held at their current positions for the whole horizon, so evaders are forecast to flee where the
team IS, not where a sequence would take it; and, as in plan.py, the walk's `persist`, detection between segment ends and a joint
allocation of the team.
"""
import torch

from . import _lib
from . import baseline as bl
from . import belief as be
from . import plan as pl

CAP = pl.CAP
MAX_LEVELS = pl.MAX_DEPTH   # CS: cs_forecast_params.moves[5]


def _check_forecast(grid, pos, n, side, model, moves):
    if not 1 <= n <= _lib.MAX_AGENTS or not 1 <= side <= bl.MAX_MAP:
        raise ValueError(f"forecast: n_agents must be 1..{_lib.MAX_AGENTS} and side 1..{bl.MAX_MAP}")
    if not isinstance(model, be.BeliefModel):
        raise TypeError("forecast: model must be a BeliefModel")
    if not 1 <= len(moves) <= MAX_LEVELS or any(not 0 <= m <= pl.MAX_STRIDE for m in moves):
        raise ValueError(f"forecast: moves must hold 1..{MAX_LEVELS} integers in 0..{pl.MAX_STRIDE}")
    if not torch.is_tensor(grid) or not torch.is_tensor(pos):
        raise TypeError("forecast: grid and pos must be tensors")
    if grid.dim() != 2 or grid.dtype != torch.int32 or grid.shape[0] < 1 or grid.shape[1] != side * side:
        raise ValueError(f"forecast: grid must be int32 [B, {side * side}] with B >= 1")
    if pos.dtype != torch.int32 or tuple(pos.shape) != (grid.shape[0], _lib.MAX_AGENTS, 2) or pos.device != grid.device:
        raise ValueError(f"forecast: pos must be int32 [{grid.shape[0]}, {_lib.MAX_AGENTS}, 2] on the grid's device")


def forecast_torch(grid, pos, n_agents, side, model, moves):
    """The definition (module docstring): grid int32 [B, side * side] (read only), pos int32 [B, 8, 2] (BeliefAgents.prev's
    layout, read clamped to +-2^15), model a `BeliefModel`, moves a sequence of L ints -> stack int32 [B, L, side * side]."""
    n, side, moves = int(n_agents), int(side), tuple(int(m) for m in moves)
    _check_forecast(grid, pos, n, side, model, moves)
    F = grid.to(torch.int64).clamp(0, CAP)
    levels = []
    for m in moves:
        for _ in range(m):
            F = be.predict_torch(F, pos, n, side, model)
        levels.append(F.to(torch.int32))
    return torch.stack(levels, 1)


def _check_stack(state, stack, side, depth):
    if not torch.is_tensor(state) or not torch.is_tensor(stack):
        raise TypeError("forecast: state and stack must be tensors")
    if stack.dtype != torch.int32 or tuple(stack.shape) != (state.shape[0], depth, side * side) or stack.device != state.device:
        raise ValueError(f"forecast: stack must be int32 [{state.shape[0]}, depth = {depth}, {side * side}] on the state's device")


def plan_forecast_actions_torch(state, stack, n_agents, side, view_range, depth, stride, discount, return_plans=False):
    """The definition (module docstring): state float32 [B, S >= 4n], stack int32 [B, depth, side * side] (read only) -> actions
    int64 [B, n]; with return_plans also the winning sequence index and its score, int64 [B, n] each."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    depth, stride, discount = int(depth), int(stride), int(discount)
    pl._check_params(n, side, view_range, depth, stride, discount)
    _check_stack(state, stack, side, depth)
    pl._check_tensors(state, stack[:, 0], n, side)
    rows = max(1, pl._CHUNK // (3 ** depth * side * side))   # envs are independent: a large batch goes block by block
    parts = [pl._plan_rows(state[b:b + rows], stack[b:b + rows], n, side, view_range, depth, stride, discount)
             for b in range(0, int(state.shape[0]), rows)]
    actions, plans, scores = (torch.cat(t) for t in zip(*parts))
    return (actions, plans, scores) if return_plans else actions


def segment_moves(t, depth, stride, every, speed):
    """moves[d] = #{u in [t + d S, t + (d + 1) S) : u % every == 0} if speed > 0, else 0: the target moves inside segment d of a
    plan made at step t (MovingTargetEnv moves the targets at the start of step u iff u % every == 0)."""
    if not speed > 0:
        return (0,) * depth
    return tuple(sum(1 for u in range(t + d * stride, t + (d + 1) * stride) if u % every == 0) for d in range(depth))


class ForecastAgents(pl.PlanAgents):
    """The planner over a `BeliefAgents`' grid, scored on the forecast, for a batch of envs.  env_or_args, motion, depth, stride,
    discount, batch, device and impl as PlanAgents'; base: None (a `BeliefAgents` is built, with `motion`) or a `BeliefAgents` of
    the same impl, batch and device -- a coverage base has no motion model and is refused.  impl = "hip": three launches per
    `choose_action` on the current stream (cs_belief_actions, cs_belief_forecast, cs_plan_forecast_actions), no synchronisation;
    "torch": the definitions, on the same device.

    `choose_action(state, moved, t)`: t is the step `state` belongs to (module docstring).  When no target move falls into the
    horizon (static targets, speed 0) no forecast is launched and the call IS PlanAgents(base="belief")'s.  `policy()` resets at
    t == 0 and passes t.  `base`, `grid`, `plans`, `scores` and `reset()` are PlanAgents'; `stack` holds the last forecast, int32
    [B, depth, side * side].  Not modelled: see the module docstring."""

    def __init__(self, env_or_args, motion=None, depth=4, stride=3, discount=230, batch=None, device=None, impl="hip", base=None):
        if base is None:
            base = "belief"
        elif not isinstance(base, be.BeliefAgents):
            raise ValueError("ForecastAgents: base must be a BeliefAgents (a coverage base has no motion model to forecast with)")
        super().__init__(env_or_args, base=base, motion=motion, depth=depth, stride=stride, discount=discount, batch=batch, device=device,
                         impl=impl)
        self.stack = torch.zeros(self.batch, self.depth, self.side * self.side, dtype=torch.int32, device=self.device)

    def choose_action(self, state, moved=0, t=0):
        """get_state() rows float32 [B, S] of step t -> actions int64 [B, n]; the base's grid moves on by one step."""
        moves = segment_moves(int(t), self.depth, self.stride, self.motion.every, self.motion.speed)
        if not any(moves):
            return super().choose_action(state, moved)
        base = self.base
        base.choose_action(state, moved)
        if self.impl == "torch":
            self.stack.copy_(forecast_torch(base.grid, base.prev, self.n_agents, self.side, base.model, moves))
            actions, plans, scores = plan_forecast_actions_torch(state, self.stack, self.n_agents, self.side, self.view_range, self.depth,
                                                                 self.stride, self.discount, return_plans=True)
            self.plans.copy_(plans)
            self.scores.copy_(scores)
            return actions
        actions = torch.empty(self.batch, self.n_agents, dtype=torch.int64, device=self.device)
        ops = _lib.torch_ops_for(pl.NEEDS)
        ops.belief_forecast(base.grid, base.prev, self.stack, self.n_agents, self.side, base.model.mode, base.model.sense16,
                            list(base.model.dx), list(base.model.dy), list(moves))
        ops.plan_forecast_actions(state, self.stack, actions, self.plans, self.scores, self.n_agents, self.side, self.view_range,
                                  self.depth, self.stride, self.discount)
        return actions

    def policy(self):
        motion = self.motion

        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state, be.targets_moved(motion, t), t)
        return policy
