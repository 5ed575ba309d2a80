"""The forecast planner on private grids under a communication range (include/coopsearch.h: cs_local_belief_forecast and
cs_local_plan_forecast_actions).

`ForecastAgents` forecasts ONE density per env with the positions of ALL agents and lets every agent see every earlier claim: a
centralised planner.  `LocalPlanAgents` over a `LocalBeliefAgents` keeps a grid per agent and hears claims only inside `comm_range`,
but scores its plan on the density of NOW, which evaders have left by the time a segment ends (DESIGN.md sections 21, 28).  Here
agent i forecasts the grid it actually owns with the team-mates it actually hears, and plans on that forecast.

Two DEFINITIONS, in stock eager torch ops on any device, all integer after the one float32 quantisation; the kernels
(csrc/local_forecast.h) reproduce them bit for bit.  Everything is forecast.py's, local_belief.py's, local.py's, plan.py's and
baseline.py's: `forecast_torch`, `plan_forecast_actions_torch`, `segment_moves`, `heard_masks`, `heard_prev`, `links`,
`sequence_points`, `quantise`, `cell_centres` and `disc_mask` are imported, not restated.

  local_forecast_torch               stacks[:, i] = forecast_torch on grids[:, i] with the agents of heard[i] held in place at their
                                     prev positions: heard[i] is read as local_belief.py reads it (bits at and above n dropped, the
                                     own bit set) and the list is in index order (`heard_prev`).  After a `LocalBeliefAgents` call
                                     prev holds the current positions and heard the links of this call: agent i forecasts with the
                                     team-mates it hears now, frozen where they are, and knows nothing of the others -- exactly the
                                     list its filter will predict with at the next call.  In walk mode the mask plays no part.
  local_plan_forecast_actions_torch  local_plan.local_plan_actions_torch with W_i = clamp(stacks[:, i], 0, CAP) of `depth` levels:
                                     agent i's search is plan_forecast_actions_torch with n_agents = 1 on its four floats (segment d
                                     scored on level d); its claim is the `depth` discs around `sequence_points` of its choice; the
                                     claims of the linked agents j < i are zeroed in EVERY level of W_i, those of the others are not
                                     heard.

Six identities pin them (tests/test_local_forecast_cpu.py):
  A  all-heard masks, equal grids G: every stacks[:, i] is forecast_torch(G, prev); unlimited range, equal stacks: actions, plans
     and scores are plan_forecast_actions_torch's.
  B  own-bits-only masks: stacks[:, i] is forecast_torch with n_agents = 1 on agent i's position; range 0: row i is the lone planner's.
  C  prefix: the outputs of agents 0 .. k-1 do not depend on agents k .. n-1.
  D  the mask equals parking every unheard agent at (-2^15, -2^15).
  E  a stack of identical levels gives local_plan_actions_torch on that level.
  F  in walk mode the mask changes nothing.

Not modelled: as forecast.py, the agents are held at their current positions for the whole horizon; and the forecasts of two agents
DISAGREE where their masks differ -- agent i's evaders flee only those it hears -- so a claim heard from j was chosen on j's
forecast and is zeroed in i's.
"""
import torch

from . import _lib
from . import belief as be
from . import forecast as fc
from . import local_belief as lb
from . import local_plan as lp
from .baseline import _check_state_grid, cell_centres, disc_mask, quantise
from .forecast import forecast_torch, plan_forecast_actions_torch, segment_moves
from .local import _check_comm, links
from .local_belief import heard_masks, heard_prev
from .plan import CAP, _check_params, sequence_points

NEEDS = "the local forecast kernels need"   # _lib.torch_ops_for's words


def local_forecast_torch(grids, prev, heard, n_agents, side, model, moves):
    """The definition (module docstring): grids int32 [B, n, side * side], prev int32 [B, 8, 2] (read clamped to +-2^15), heard int32
    [B, 8] (all three read only), model a `BeliefModel`, moves a sequence of L ints -> stacks int32 [B, n, L, side * side]."""
    n, side, moves = int(n_agents), int(side), tuple(int(m) for m in moves)
    if not all(torch.is_tensor(t) for t in (grids, prev, heard)):
        raise TypeError("local forecast: grids, prev and heard must be tensors")
    if n < 1 or grids.dim() != 3 or grids.shape[1] != n:
        raise ValueError(f"local forecast: grids must be int32 [B, n_agents = {n} >= 1, {side * side}] with B >= 1")
    for i in range(n):   # forecast.py's checks, row by row
        fc._check_forecast(grids[:, i], prev, n, side, model, moves)
    B = grids.shape[0]
    if heard.dtype != torch.int32 or tuple(heard.shape) != (B, _lib.MAX_AGENTS) or heard.device != grids.device:
        raise ValueError(f"local forecast: heard must be int32 [{B}, {_lib.MAX_AGENTS}] on the grids' device")
    known = heard_masks(heard, n)
    return torch.stack([forecast_torch(grids[:, i], heard_prev(prev, known[:, i], n), n, side, model, moves) for i in range(n)], 1)


def local_plan_forecast_actions_torch(state, stacks, n_agents, side, view_range, depth, stride, discount, comm_range, return_plans=False):
    """The definition (module docstring): state float32 [B, S >= 4n], stacks int32 [B, n, depth, side * side] (read only), comm_range
    -1 or 0..128 -> actions int64 [B, n]; with return_plans also the winning sequence index and its score, int64 [B, n] each."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    depth, stride, discount, comm_range = int(depth), int(stride), int(discount), int(comm_range)
    _check_params(n, side, view_range, depth, stride, discount)
    _check_comm(comm_range)
    if not torch.is_tensor(state) or not torch.is_tensor(stacks):
        raise TypeError("local forecast plan: state and stacks must be tensors")
    _check_state_grid("local forecast plan", state, stacks, n, (n, depth, side * side), name="stacks")
    B = int(state.shape[0])
    X, Y, h = quantise(state, n, side)
    adj = links(X, Y, comm_range)
    centre, R2 = cell_centres(side, state.device), (16 * view_range) ** 2
    zero = torch.zeros((), dtype=torch.int32, device=state.device)
    out, claims = [], []
    for i in range(n):
        W = stacks[:, i].clamp(0, CAP)   # [B, depth, cells]
        for j in range(i):   # the claims agent i has heard, in every level
            W = torch.where((claims[j] & adj[:, i, j].view(B, 1)).unsqueeze(1), zero, W)
        one = plan_forecast_actions_torch(state[:, 4 * i:4 * i + 4].contiguous(), W, 1, side, view_range, depth, stride, discount,
                                          return_plans=True)
        out.append(one)
        px, py = sequence_points(X[:, i], Y[:, i], h[:, i], one[1][:, 0], side, depth, stride)
        claims.append(disc_mask(centre, px, py, R2).any(1))
    actions, plans, scores = (torch.cat(t, 1) for t in zip(*out))
    return (actions, plans, scores) if return_plans else actions


class LocalForecastAgents(lp.LocalPlanAgents):
    """The forecast planner over a `LocalBeliefAgents`' n private grids, for a batch of envs: a `LocalPlanAgents` over a belief base.
    env_or_args, comm_range, motion, depth, stride, discount, batch, device and impl as LocalPlanAgents'; base: None (a
    `LocalBeliefAgents` is built, with `motion`) or a `LocalBeliefAgents` of the same impl, batch, device and comm_range -- a coverage
    base has no motion model and is refused.  impl = "hip": three launches per `choose_action` on the current stream
    (cs_local_belief_actions, cs_local_belief_forecast, cs_local_plan_forecast_actions), no synchronisation; "torch": the definitions,
    on the same device.

    `choose_action(state, moved, t)`: t is the step `state` belongs to; moves = forecast.segment_moves(t, depth, stride, motion.every,
    motion.speed).  When no target move falls into the horizon (static targets, speed 0) nothing new is launched and the call IS
    LocalPlanAgents(base="belief")'s.  `policy()` resets at t == 0 and passes t.  `base`, `grids`, `plans`, `scores` and `reset()` are
    LocalPlanAgents'; `stacks` holds the last forecast, int32 [B, n, depth, side * side]: B * n * depth * side^2 * 4 bytes, 491 MB at
    4096 envs, 3 agents, depth 4 and side 50.  Not modelled: see the module docstring."""

    def __init__(self, env_or_args, comm_range, motion=None, depth=4, stride=3, discount=230, batch=None, device=None, impl="hip",
                 base=None):
        if base is None:
            base = "belief"
        elif not isinstance(base, lb.LocalBeliefAgents):
            raise ValueError("LocalForecastAgents: base must be a LocalBeliefAgents (a coverage base has no motion model to forecast "
                             "with)")
        super().__init__(env_or_args, comm_range, base=base, motion=motion, depth=depth, stride=stride, discount=discount, batch=batch,
                         device=device, impl=impl)
        self.stacks = torch.zeros(self.batch, self.n_agents, self.depth, self.side * self.side, dtype=torch.int32, device=self.device)

    def choose_action(self, state, moved=0, t=0):
        """get_state() rows float32 [B, S] of step t -> actions int64 [B, n]; the base's n grids move on by one step."""
        moves = segment_moves(int(t), self.depth, self.stride, self.motion.every, self.motion.speed)
        if not any(moves):
            return super().choose_action(state, moved)
        base = self.base
        base.choose_action(state, moved)
        if self.impl == "torch":
            self.stacks.copy_(local_forecast_torch(base.grids, base.prev, base.heard, self.n_agents, self.side, base.model, moves))
            actions, plans, scores = local_plan_forecast_actions_torch(state, self.stacks, self.n_agents, self.side, self.view_range,
                                                                       self.depth, self.stride, self.discount, self.comm_range,
                                                                       return_plans=True)
            self.plans.copy_(plans)
            self.scores.copy_(scores)
            return actions
        actions = torch.empty(self.batch, self.n_agents, dtype=torch.int64, device=self.device)
        ops = _lib.torch_ops_for(NEEDS)
        ops.local_belief_forecast(base.grids, base.prev, base.heard, self.stacks, self.n_agents, self.side, base.model.mode,
                                  base.model.sense16, list(base.model.dx), list(base.model.dy), list(moves))
        ops.local_plan_forecast_actions(state, self.stacks, actions, self.plans, self.scores, self.n_agents, self.side, self.view_range,
                                        self.depth, self.stride, self.discount, self.comm_range)
        return actions

    def policy(self):
        motion = self.motion

        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state, be.targets_moved(motion, t), t)
        return policy
