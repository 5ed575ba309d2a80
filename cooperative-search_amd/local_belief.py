"""The target-density filter under a limited communication range (include/coopsearch.h: cs_local_belief_actions).

`BeliefAgents` keeps ONE density per env and predicts it with the positions of ALL agents: a centralised filter.  `LocalCoverageAgents`
decentralised the coverage sweep, on static targets, where a greedy sweep is saturated and the range costs nothing.  Here agent i
keeps a density of its own, predicts it with the team-mates it actually HEARD at the previous call, and fuses it with the agents
it hears now: the hand-written yardstick for a decentralised learner on moving targets.

`local_belief_actions_torch` is the DEFINITION, in stock eager torch ops on any device; the kernel (csrc/local_belief.h) reproduces
grids, prev, heard and the actions bit for bit.  Everything is integer after the one float32 quantisation, and everything is
baseline.py's, local.py's and belief.py's: `quantise`, `cell_centres`, `disc_mask`, `greedy_choose`, `links`, `predict_torch`
(and through it `heading_tables`), `BeliefModel` and CAP are imported, not restated.  Per env the policy keeps

  grids   int32 [n, side * side]: agent i's private density, Q16, row-major [ix * side + iy]; a cell is read as clamp(cell, 0, CAP),
          CAP = 2^19; `reset()` fills it with 65536.
  prev    int32 [8, 2]: the quantised positions at the previous call, read clamped to +-2^15, as in BeliefAgents.
  heard   int32 [8]: the link mask of the previous call: bit j of heard[i] says that agent i heard agent j then.  It is read as
          (heard[i] & ((1 << n) - 1)) | (1 << i): garbage above bit n - 1 and a missing own bit do not matter.  `reset()` zeroes it:
          in the first call of an episode every agent knows of itself alone.
  Slots >= n of prev and heard are never read and keep their content.

and one call does, with belief.py's host integers (a `BeliefModel`, `moved`) and local.py's `comm_range`:

  quantise  X, Y, h as coverage_actions_torch does; links: adj = local.links(X, Y, comm_range) (strict, symmetric, 64-bit, own bit set).
  predict   only if moved; otherwise D'_i = clamp(D_i, 0, CAP).  Agent i runs belief.py's prediction step on its OWN grid, and in
            the evade test it knows only the agents j in its heard mask of the previous call (itself included), at their prev
            positions: at that call it knew where they were, and nothing of the others.  The list of agents handed to
            `predict_torch` for grid i is the heard ones in index order (`heard_prev`); nearest agent, lowest-index tie, evade
            heading, weights, bilinear split, clamped destinations, >> 12 per piece and min(sum, CAP) are predict_torch's own.
            In walk mode the mask plays no part.
  sweep     S_i = (D'_i keep) >> 16 inside agent i's own current disc (R = 16 view_range), D'_i elsewhere.
  merge     M_i = the cell-wise minimum of S_j over the j with adj(i, j), written back to grids[:, i].  ONE hop per call, from the
            post-sweep grids, as in local.py; the minimum starts at CAP + 1, above every cell.
  store     prev[i] = (X_i, Y_i) and heard[i] = the bits of adj[i, :], for i < n.
  choose    baseline.greedy_choose(M, ..., adj): agent i decides on M_i less the footprints claimed by linked agents before it.

Why the minimum is the merge, and what it costs.  (v keep) >> 16 <= v since keep <= 65536: where two agents' predictions AGREE,
the only difference between their grids is who has looked, and the minimum is "somebody has looked here" -- exactly the shared
filter's sweep.  Where they DISAGREE, because they predicted with different team-mates, the minimum takes the lower estimate and
loses mass: an evader shoved into a cell in C's grid (C knew of the agent that shoved it) is kept at the diffused, lower value of
A's grid once A and C meet.  The filter already only ever loses mass (to the floors, the cap and the sweep), so the merge errs the
way the filter errs: toward "already searched".  It is a stated heuristic, not a Bayes fusion of two posteriors.

Four identities pin the definition (tests/test_local_belief_cpu.py):
  A  unlimited range, equal grids: every grids[:, i] is the grid belief_actions_torch leaves, actions and prev are equal.
  B  range 0: grids[:, i] and action i are belief_actions_torch's with n_agents = 1 on agent i's four floats.
  C  moved = 0 and cells in 1..65536: local_coverage_actions_torch(..., regrow=16), since (65536 - G) >> 16 is 0 for G >= 1.
  D  the mask equals moving every unheard agent to (-2^15, -2^15): farther than the largest sense16 from every cell centre.
"""
import torch

from . import _lib
from . import motion as mo
from .baseline import FRESH, GridAgents, _check_state_grid, cell_centres, disc_mask, greedy_choose, quantise
from .belief import CAP, BeliefModel, _check_params, predict_torch, targets_moved
from .local import MAX_COMM, _check_comm, links


def _check_tensors(state, grids, prev, heard, n, side):
    _check_state_grid("local belief", state, grids, n, (n, side * side), name="grids")
    B = state.shape[0]
    if prev.dtype != torch.int32 or tuple(prev.shape) != (B, _lib.MAX_AGENTS, 2) or prev.device != state.device:
        raise ValueError(f"local belief: prev must be int32 [{B}, {_lib.MAX_AGENTS}, 2] on the state's device")
    if heard.dtype != torch.int32 or tuple(heard.shape) != (B, _lib.MAX_AGENTS) or heard.device != state.device:
        raise ValueError(f"local belief: heard must be int32 [{B}, {_lib.MAX_AGENTS}] on the state's device")


def heard_masks(heard, n_agents):
    """heard int32 [B, 8] -> bool [B, n, n]: [b, i, j] says that agent i heard agent j, read as the module docstring says (bits at
    and above n dropped, the own bit set)."""
    n = int(n_agents)
    idx = torch.arange(n, dtype=torch.int64, device=heard.device)
    bits = (heard[:, :n].to(torch.int64) & ((1 << n) - 1)) | (1 << idx)
    return ((bits.unsqueeze(-1) >> idx) & 1).bool()


def heard_prev(prev, mask, n_agents):
    """The agents one filter knows of: prev int32 [B, 8, 2], mask bool [B, n] (at least one bit per row) -> int32 [B, 8, 2] whose
    first n slots hold the masked-in agents IN INDEX ORDER, the last of them repeated to fill the n slots.  A repeated agent changes
    nothing in predict_torch's evade test (it is never nearer than itself), and the order keeps the lowest-index tie rule."""
    n = int(n_agents)
    idx = torch.arange(n, dtype=torch.int64, device=prev.device).expand(mask.shape[0], n)
    order = torch.where(mask, idx, idx + n).argsort(1)
    pick = order.gather(1, torch.minimum(idx, mask.sum(1, keepdim=True) - 1))
    out = prev.clone()
    out[:, :n] = prev[:, :n].gather(1, pick.unsqueeze(-1).expand(-1, -1, 2))
    return out


def local_belief_actions_torch(state, grids, prev, heard, n_agents, side, view_range, keep, model, moved, comm_range, lookahead=None,
                               return_scores=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grids int32 [B, n, side * side], prev int32 [B, 8, 2] and
    heard int32 [B, 8] (all three updated in place), model a `BeliefModel`, moved 0 / 1, comm_range -1 or 0..128 -> actions int64
    [B, n]; with return_scores also the scores each agent chose from, int64 [B, n, 3].  Stock EAGER torch ops on the tensors' device
    (see baseline.coverage_actions_torch on why eager)."""
    n, side, view_range, keep, moved, comm_range = int(n_agents), int(side), int(view_range), int(keep), int(moved), int(comm_range)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check_params(n, side, view_range, keep, lookahead, moved)
    _check_comm(comm_range)
    if not isinstance(model, BeliefModel):
        raise TypeError("local belief: model must be a BeliefModel")
    _check_tensors(state, grids, prev, heard, n, side)
    B, cells = int(state.shape[0]), side * side
    X, Y, h = quantise(state, n, side)
    adj = links(X, Y, comm_range)
    D = grids.to(torch.int64).clamp(0, CAP)   # [B, n, cells]
    if moved:   # agent i's filter, on the agents it heard at the previous call (the n filters of an env as B * n rows)
        known = heard_masks(heard, n)
        seen = torch.stack([heard_prev(prev, known[:, i], n) for i in range(n)], 1)
        D = predict_torch(D.reshape(B * n, cells), seen.reshape(B * n, _lib.MAX_AGENTS, 2), n, side, model).view(B, n, cells)
    centre, R2 = cell_centres(side, state.device), (16 * view_range) ** 2
    own = torch.stack([disc_mask(centre, X[:, i], Y[:, i], R2) for i in range(n)], 1)
    S = torch.where(own, (D * keep) >> 16, D)
    far = torch.full_like(S, CAP + 1)   # above every cell: an agent that is not heard does not enter the minimum
    M = torch.stack([torch.where(adj[:, i, :, None], S, far).min(1).values for i in range(n)], 1)
    grids.copy_(M.to(torch.int32))
    prev[:, :n, 0] = X.to(torch.int32)
    prev[:, :n, 1] = Y.to(torch.int32)
    bit = 1 << torch.arange(n, dtype=torch.int64, device=state.device)
    heard[:, :n] = (adj.to(torch.int64) * bit).sum(-1).to(torch.int32)
    actions, scores = greedy_choose(M, X, Y, h, side, view_range, lookahead, adj)
    return (actions, scores) if return_scores else actions


class LocalBeliefAgents(GridAgents):
    """The density filter under a communication range, for a batch of envs: BeliefAgents' arguments, and comm_range in whole cells,
    0..128, None = unlimited.

    `.grids` is int32 [B, n, side * side]: agent i's private density; `.prev` int32 [B, 8, 2] the stored positions; `.heard` int32
    [B, 8] the link masks of the previous call.  `policy()` resets them when t == 0 and tells the filter whether the targets moved:
    `belief.targets_moved(motion, t)`.  With comm_range None it flies BeliefAgents' episodes; with 0, n lone filters'."""
    KERNEL, NEEDS = "local_belief.h", "the local belief kernel needs"

    def __init__(self, env_or_args, comm_range, motion=None, batch=None, device=None, lookahead=None, impl="hip"):
        super().__init__(env_or_args, batch, device, lookahead, impl)
        _check_params(self.n_agents, self.side, self.view_range, self.keep, self.lookahead, 0)
        if comm_range is not None and (int(comm_range) != comm_range or comm_range < 0):
            raise ValueError(f"LocalBeliefAgents: comm_range must be a whole number of cells, 0..{MAX_COMM}, or None (unlimited), "
                             f"got {comm_range!r}")
        self.comm_range = -1 if comm_range is None else int(comm_range)
        _check_comm(self.comm_range)
        if motion is None:
            motion = getattr(env_or_args, "motion", None)
            if not isinstance(motion, mo.TargetMotion):
                motion = mo.TargetMotion.from_args(env_or_args)
        if not isinstance(motion, mo.TargetMotion):
            raise TypeError("LocalBeliefAgents: motion must be a TargetMotion")
        self.motion = motion
        self.model = BeliefModel.from_motion(motion, self.side)
        self.grids = torch.full((self.batch, self.n_agents, self.side * self.side), FRESH, dtype=torch.int32, device=self.device)
        self.prev = torch.zeros(self.batch, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=self.device)
        self.heard = torch.zeros(self.batch, _lib.MAX_AGENTS, dtype=torch.int32, device=self.device)

    def reset(self):
        """Fresh private densities; the stored positions and link masks are cleared: nobody has heard anybody."""
        self.grids.fill_(FRESH)
        self.prev.zero_()
        self.heard.zero_()

    def choose_action(self, state, moved):
        """get_state() rows float32 [B, S] -> actions int64 [B, n]; moved: did the targets move in the step that led here?  The n
        grids, the stored positions and the link masks move on by one step."""
        moved = 1 if moved else 0
        if self.impl == "torch":
            return local_belief_actions_torch(state, self.grids, self.prev, self.heard, self.n_agents, self.side, self.view_range,
                                              self.keep, self.model, moved, self.comm_range, self.lookahead)
        ops, actions = self._launch(state)
        ops.local_belief_actions(state, self.grids, self.prev, self.heard, actions, self.n_agents, self.side, self.view_range, self.keep,
                                 self.lookahead, self.model.mode, moved, self.model.sense16, list(self.model.dx), list(self.model.dy),
                                 self.comm_range)
        return actions

    def policy(self):
        motion = self.motion

        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state, targets_moved(motion, t))
        return policy
