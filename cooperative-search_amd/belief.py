"""A policy for moving targets: the target-density filter (include/coopsearch.h: cs_belief_actions).

`CoverageAgents` sweeps a belief grid that knows nothing of motion: what puts belief back into a swept cell is a constant leak,
the same everywhere.  Against evading targets it still sweeps nearly the whole map and finds fewer and fewer of them (DESIGN.md
section 19): they are driven ahead of the sweep into ground already swept.  Search theory's answer is a density filter: a
PREDICTION step pushes the expected density of unfound targets through the targets' own motion model -- a 16-heading diffusion
for the walk, a shove away from the nearest agent inside `sense` for the evasion -- and a MEASUREMENT step is the sweep the
coverage policy already has.  Mass piles up where the team has driven the evaders, and a policy that steers toward mass follows.

`belief_actions_torch` is the DEFINITION, in stock eager torch ops on any device; the kernel (csrc/belief.h) reproduces the grid,
the stored positions and the actions element for element.  Everything is integer after the one float32 quantisation of
baseline.quantise.  Per env the policy keeps

  grid      D, int32 [side * side], row-major [ix * side + iy], Q16: 65536 = one cell's worth of "nobody has looked"; `reset()`
            fills it.  A cell is read as clamp(cell, 0, CAP), CAP = 2^19: a whole map sums to at most 2^12 * 2^19 = 2^31, so
            every accumulator and every score fits uint32.
  prev      int32 [8, 2]: the quantised (X, Y) of the agents at the previous call, read clamped to +-2^15.  MovingTargetEnv
            moves the targets at the START of a step, against the agent positions of the state the policy saw one call
            earlier.  Slots i >= n_agents are never read and keep their content.

and one call does, with the host integers of a `BeliefModel` (mode, sense16, dx[16], dy[16]) and `moved` (0 / 1):

  quantise  X, Y, h per agent exactly as baseline.coverage_actions_torch does.
  predict   only if moved; otherwise D' = clamp(D, 0, CAP).  Every source cell (ix, iy) holds d = clamp(D, 0, CAP).  It EVADES
            iff mode is evade and some agent i < n has ex^2 + ey^2 <= sense16^2, ex = 16 ix + 8 - PX_i, ey = 16 iy + 8 - PY_i,
            (PX, PY) = prev; the smallest distance wins, the lowest i on ties, and the evade heading is the lowest k that
            maximises ex CQ[k] + ey SQ[k] (a cell under an agent: all scores 0, heading 0, as move_targets_torch does).  An
            evading cell sends all its mass along that heading (weight m = 16), every other cell one sixteenth along each of
            the 16 headings (m = 1 for every k).  Heading k: ux = 16 ix + dx[k], i0 = ux >> 4, fx = ux & 15 (the shift floors,
            the mask is two's complement), likewise uy, j0, fy; the four pieces go to (i0, j0), (i0 + 1, j0), (i0, j0 + 1),
            (i0 + 1, j0 + 1) with weights wx wy from (16 - fx, fx) and (16 - fy, fy); every destination index is clamped to
            0..side - 1 (targets clamp at the walls: mass stays in the wall cell); piece = (d m wx wy) >> 12, floored per
            piece (the product is at most 2^31).  D'[dest] = min(sum of its pieces, CAP).  Mass is only ever lost, to the
            floors and to the cap.
  sweep     a cell whose centre lies within R = 16 view_range of any CURRENT agent: D'' = (D' keep) >> 16.  D'' is written back
            to grid, and prev[i] = (X_i, Y_i) for i < n.
  choose    baseline's step on W = D'': three look-ahead points per agent, score = the sum of W over the footprint, the lowest
            action with the largest score wins, its footprint is zeroed in W, agents in index order.

Two choices are deliberate: the filter ignores `persist` (every walk move is a fresh uniform heading), and it models the evasion
at cell-centre resolution.  The model is a parameter of the policy, not read from the env: a walk model may be flown against
evading targets.
"""
import dataclasses

import torch

from . import _lib
from . import baseline as bl
from . import motion as mo

CAP = 1 << 19          # a cell is read as clamp(cell, 0, CAP)
FRESH = bl.FRESH
HEADINGS = mo.HEADINGS
MAX_SENSE16 = 2048     # 16 * 2 * CS_MAX_MAP
MAX_STEP16 = 1024      # 16 * CS_MAX_MAP
POS_LIM = 1 << 15


def heading_tables():
    """(CQ, SQ): rint(16384 CX[k]) and rint(16384 CY[k]) of motion's 16 headings, as Python ints (csrc/belief.h holds them as
    literals)."""
    return [int(round(16384.0 * v)) for v in mo.CX], [int(round(16384.0 * v)) for v in mo.CY]


@dataclasses.dataclass(frozen=True)
class BeliefModel:
    """The motion model of the prediction step as the integers the kernel takes.  mode: 0 walk, 1 evade (CS_MOTION_*); sense16 =
    rint(16 sense), 0..2048; dx[k] = rint(16 speed CX[k]), dy[k] likewise with CY, each -1024..1024 (Python doubles,
    round-half-even)."""
    mode: int = 0
    sense16: int = 0
    dx: tuple = (0,) * HEADINGS
    dy: tuple = (0,) * HEADINGS

    def __post_init__(self):
        object.__setattr__(self, "dx", tuple(int(v) for v in self.dx))
        object.__setattr__(self, "dy", tuple(int(v) for v in self.dy))
        if self.mode not in (0, 1) or not 0 <= self.sense16 <= MAX_SENSE16:
            raise ValueError(f"belief: mode must be 0 (walk) or 1 (evade) and sense16 0..{MAX_SENSE16}")
        if len(self.dx) != HEADINGS or len(self.dy) != HEADINGS or any(abs(v) > MAX_STEP16 for v in self.dx + self.dy):
            raise ValueError(f"belief: dx and dy must hold {HEADINGS} integers in -{MAX_STEP16}..{MAX_STEP16}")

    @classmethod
    def from_motion(cls, motion, map_size):
        """The model of a `TargetMotion` on a map of map_size cells per side."""
        motion.check(int(map_size))
        return cls(mode=mo.MODES[motion.mode], sense16=int(round(16.0 * motion.sense)),
                   dx=tuple(int(round(16.0 * motion.speed * v)) for v in mo.CX),
                   dy=tuple(int(round(16.0 * motion.speed * v)) for v in mo.CY))


def _check_params(n, side, view_range, keep, lookahead, moved):
    bl._check_team("belief", n, side, view_range)
    if not 0 <= keep <= FRESH or not 0 <= lookahead <= side or moved not in (0, 1):
        raise ValueError("belief: keep must be 0..65536, lookahead 0..side and moved 0 or 1")


def _check_tensors(state, grid, prev, n, side):
    bl._check_state_grid("belief", state, grid, n, (side * side,))
    if prev.dtype != torch.int32 or tuple(prev.shape) != (state.shape[0], _lib.MAX_AGENTS, 2) or prev.device != state.device:
        raise ValueError(f"belief: prev must be int32 [{state.shape[0]}, {_lib.MAX_AGENTS}, 2] on the state's device")


def predict_torch(D, prev, n_agents, side, model):
    """The prediction step alone: D int64 [B, side * side] with cells in 0..CAP, prev int32 [B, 8, 2] -> D', a new tensor."""
    i64, dev, B, n, cells = torch.int64, D.device, int(D.shape[0]), int(n_agents), side * side
    cell = torch.arange(side, dtype=i64, device=dev)
    one = torch.ones(B, cells, dtype=i64, device=dev)
    evades = torch.zeros(B, cells, dtype=torch.bool, device=dev)
    kev = torch.zeros(B, cells, dtype=i64, device=dev)
    if model.mode == 1:
        P = prev.to(i64).clamp(-POS_LIM, POS_LIM)
        centre = (16 * cell + 8).view(1, side)
        best = torch.full((B, cells), 1 << 62, dtype=i64, device=dev)
        bex, bey = torch.zeros_like(best), torch.zeros_like(best)
        for i in range(n):   # the nearest agent inside the radius, lowest index on ties
            ex = (centre - P[:, i, 0].view(B, 1)).view(B, side, 1).expand(B, side, side).reshape(B, cells)
            ey = (centre - P[:, i, 1].view(B, 1)).view(B, 1, side).expand(B, side, side).reshape(B, cells)
            d2 = ex * ex + ey * ey
            take = (d2 <= model.sense16 * model.sense16) & (d2 < best)
            best, bex, bey = torch.where(take, d2, best), torch.where(take, ex, bex), torch.where(take, ey, bey)
            evades = evades | take
        cq, sq = heading_tables()
        top = bex * cq[0] + bey * sq[0]
        for k in range(1, HEADINGS):   # the heading that leads away fastest, lowest index on ties
            s = bex * cq[k] + bey * sq[k]
            take = s > top
            top, kev = torch.where(take, s, top), torch.where(take, torch.full_like(kev, k), kev)
    out = torch.zeros(B, cells, dtype=i64, device=dev)
    for k in range(HEADINGS):
        m = torch.where(evades, torch.where(kev == k, 16 * one, 0 * one), one)
        ux, uy = 16 * cell + model.dx[k], 16 * cell + model.dy[k]
        i0, fx, j0, fy = ux >> 4, ux & 15, uy >> 4, uy & 15
        for di, wx in ((0, 16 - fx), (1, fx)):
            for dj, wy in ((0, 16 - fy), (1, fy)):
                dest = ((i0 + di).clamp(0, side - 1).view(side, 1) * side + (j0 + dj).clamp(0, side - 1).view(1, side)).reshape(cells)
                w = (wx.view(side, 1) * wy.view(1, side)).reshape(1, cells)
                out.index_add_(1, dest, (D * m * w) >> 12)
    return out.clamp(max=CAP)


def belief_actions_torch(state, grid, prev, n_agents, side, view_range, keep, model, moved, lookahead=None, return_scores=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grid int32 [B, side * side] and prev int32 [B, 8, 2] (both
    updated in place), model a `BeliefModel`, moved 0 / 1 -> actions int64 [B, n]; with return_scores also the scores each agent
    chose from, int64 [B, n, 3].  Stock EAGER torch ops on the tensors' device (see baseline.coverage_actions_torch on why eager)."""
    n, side, view_range, keep, moved = int(n_agents), int(side), int(view_range), int(keep), int(moved)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check_params(n, side, view_range, keep, lookahead, moved)
    if not isinstance(model, BeliefModel):
        raise TypeError("belief: model must be a BeliefModel")
    _check_tensors(state, grid, prev, n, side)
    X, Y, h = bl.quantise(state, n, side)
    D = grid.to(torch.int64).clamp(0, CAP)
    if moved:
        D = predict_torch(D, prev, n, side, model)
    D = torch.where(bl.swept(bl.cell_centres(side, state.device), X, Y, (16 * view_range) ** 2), (D * keep) >> 16, D)
    grid.copy_(D.to(torch.int32))
    prev[:, :n, 0] = X.to(torch.int32)
    prev[:, :n, 1] = Y.to(torch.int32)
    actions, scores = bl.greedy_choose(D, X, Y, h, side, view_range, lookahead)
    return (actions, scores) if return_scores else actions


def targets_moved(motion, t):
    """Did the targets of `motion` move in the step that led to the state of step t?  (MovingTargetEnv moves them at the start of
    step u iff u % every == 0.)"""
    return t > 0 and motion.speed > 0 and (t - 1) % motion.every == 0


class BeliefAgents(bl.GridAgents):
    """The density-filter policy for a batch of envs: baseline.GridAgents' arguments (a MovingTargetEnv serves as env), and motion:
    the `TargetMotion` the filter predicts with (default: the env's `.motion`, else `TargetMotion.from_args`) -- a parameter of the
    policy, not read from the env at decision time.  `.grid` is the density, int32 [B, side * side], `.prev` the stored positions,
    int32 [B, 8, 2].

    `policy()` also serves collect_sweep_data; it resets at t == 0 and tells the filter whether the targets moved in the step that
    led to `state`: `targets_moved(motion, t)`."""
    KERNEL, NEEDS = "belief.h", "the belief kernel needs"

    def __init__(self, env_or_args, motion=None, batch=None, device=None, lookahead=None, impl="hip"):
        super().__init__(env_or_args, batch, device, lookahead, impl)
        _check_params(self.n_agents, self.side, self.view_range, self.keep, self.lookahead, 0)
        if motion is None:
            motion = getattr(env_or_args, "motion", None)
            if not isinstance(motion, mo.TargetMotion):
                motion = mo.TargetMotion.from_args(env_or_args)
        if not isinstance(motion, mo.TargetMotion):
            raise TypeError("BeliefAgents: motion must be a TargetMotion")
        self.motion = motion
        self.model = BeliefModel.from_motion(motion, self.side)
        self.grid = torch.full((self.batch, self.side * self.side), FRESH, dtype=torch.int32, device=self.device)
        self.prev = torch.zeros(self.batch, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=self.device)

    def reset(self):
        """A fresh density: one cell's worth everywhere; the stored positions are cleared."""
        self.grid.fill_(FRESH)
        self.prev.zero_()

    def choose_action(self, state, moved):
        """get_state() rows float32 [B, S] -> actions int64 [B, n]; moved: did the targets move in the step that led here?  The
        grid and the stored positions move on by one step."""
        moved = 1 if moved else 0
        if self.impl == "torch":
            return belief_actions_torch(state, self.grid, self.prev, self.n_agents, self.side, self.view_range, self.keep, self.model,
                                        moved, self.lookahead)
        ops, actions = self._launch(state)
        ops.belief_actions(state, self.grid, self.prev, actions, self.n_agents, self.side, self.view_range, self.keep, self.lookahead,
                           self.model.mode, moved, self.model.sense16, list(self.model.dx), list(self.model.dy))
        return actions

    def policy(self):
        motion = self.motion

        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state, targets_moved(motion, t))
        return policy
