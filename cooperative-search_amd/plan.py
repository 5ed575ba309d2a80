"""A receding-horizon planner over the grid of a base policy (include/coopsearch.h: cs_plan_actions).

`CoverageAgents` and `BeliefAgents` decide myopically: three look-ahead points, all `lookahead` cells ahead along h, h + 10 and
h - 10 degrees, whose footprints overlap almost entirely.  Mass abeam of an agent or behind it scores 0 on all three, and the tie
rule flies the agent straight on -- into a wall, where it parks.  The classical non-myopic step of search planning is to enumerate
short turn sequences, score each by the mass it NEWLY sweeps along its path, and hand them out to the team greedily.

`plan_actions_torch` is the DEFINITION, in stock eager torch ops on any device; the kernel (csrc/plan.h) reproduces its actions,
plans and scores element for element.  Everything is integer after the one float32 quantisation of baseline.quantise.  `grid` is
the density a base policy left after its sweep (baseline's G or belief's D), int32 [side * side], row-major [ix * side + iy]; it is
only read, every cell as clamp(cell, 0, CAP), CAP = 2^19, which covers both ranges: a whole map sums to at most 2^31.  Per env the
agents decide in index order on a working copy W of the clamped grid:

  quantise   X, Y, h = baseline.quantise(state, n, side).
  sequences  s = 0 .. 3^D - 1, read as D base-3 digits, the most significant one the first segment.  Digit a means "hold action a
             for S steps"; one step is h = (h + {0, +1, 35}[a]) % 36, then x = clamp(x + ((16 CT[h]) >> 14), 0, 16 side), y
             likewise with ST (baseline.trig_tables; >> floors).  The point after segment d is P_d.  Sequences that share a prefix
             share their points: a tree of 3 + 9 + ... + 3^D <= 363 nodes.
  gain       of a node: the sum of W over the cells whose centre (16 ix + 8, 16 iy + 8) lies within R = 16 view_range of the
             node's point (<= on squared integers) and within R of NO ancestor node's point.  The agent's own position is no
             ancestor: the base policy swept that disc already.  Every gain is at most 2^31.
  score      of a sequence: sum over d of gain_d w_d, w_0 = 256, w_d = (w_{d-1} discount) >> 8 (Q8).  The gains of one sequence
             are taken over disjoint cells, so a score is at most 2^39.
  choice     the lowest s with the largest score; the action is its first digit; W is zeroed on the union of that sequence's D
             discs before the next agent decides.

Not modelled: the walk's `persist`, detection along the path BETWEEN segment ends (a sequence is credited with D discs, not with
the D S discs it flies through), and the teammates' later segments (an agent sees what earlier agents claimed, never what later
ones will).
"""
import torch

from . import _lib
from . import baseline as bl
from . import belief as be
from . import motion as mo

CAP = 1 << 19          # a cell is read as clamp(cell, 0, CAP)
MAX_DEPTH = 5          # CS_PLAN_MAX_DEPTH: 3^5 = 243 sequences, 363 nodes
MAX_STRIDE = 8
TURN = (0, 1, bl.HEADINGS - 1)
NEEDS = "the plan kernel needs"   # _lib.torch_ops_for's words, forecast.py's too
_CHUNK = 1 << 24       # the definition works on at most this many (env, sequence, cell) triples at a time (envs are independent)


def step_tables():
    """(SX, SY): (16 CT[h]) >> 14 and (16 ST[h]) >> 14, one step of one cell along heading h in sub-units, as Python ints."""
    ct, st = bl.trig_tables()
    return [(16 * v) >> 14 for v in ct], [(16 * v) >> 14 for v in st]


def weights(depth, discount):
    """w_0 .. w_{D-1} (Q8)."""
    w = [256]
    for _ in range(1, depth):
        w.append((w[-1] * discount) >> 8)
    return w


def sequence_points(X, Y, h, plans, side, depth, stride):
    """The segment end points of one sequence per row: quantised poses X, Y, h and sequence indices `plans`, int64 [B] each ->
    (px, py) int64 [B, depth], P_0 .. P_{D-1} of the module docstring (local_plan.py claims the discs around them)."""
    sx, sy = (torch.tensor(t, dtype=torch.int64, device=X.device) for t in step_tables())
    turn = torch.tensor(TURN, dtype=torch.int64, device=X.device)
    lim, px, py = 16 * side, [], []
    for d in range(depth):
        t = turn[(plans // 3 ** (depth - 1 - d)) % 3]
        for _ in range(stride):
            h = (h + t) % bl.HEADINGS
            X = torch.clamp(X + sx[h], 0, lim)
            Y = torch.clamp(Y + sy[h], 0, lim)
        px.append(X)
        py.append(Y)
    return torch.stack(px, 1), torch.stack(py, 1)


def _check_params(n, side, view_range, depth, stride, discount):
    bl._check_team("plan", n, side, view_range)
    if not 1 <= depth <= MAX_DEPTH or not 1 <= stride <= MAX_STRIDE or not 0 <= discount <= 256:
        raise ValueError(f"plan: depth must be 1..{MAX_DEPTH}, stride 1..{MAX_STRIDE} and discount 0..256")


def _check_tensors(state, grid, n, side):
    if not torch.is_tensor(state) or not torch.is_tensor(grid):
        raise TypeError("plan: state and grid must be tensors")
    bl._check_state_grid("plan", state, grid, n, (side * side,))


def _plan_rows(state, levels, n, side, view_range, depth, stride, discount):
    """The definition on a block of envs: (actions, plans, scores), int64 [B, n].  levels: int32 [B, L, side * side]; L = 1: the
    grid, every segment is scored on it; L = depth: segment d is scored on level d (forecast.plan_forecast_actions_torch)."""
    i64, dev = torch.int64, state.device
    B, R2, lim, cells = int(state.shape[0]), (16 * view_range) ** 2, 16 * side, side * side
    X, Y, h = bl.quantise(state, n, side)
    centre = bl.cell_centres(side, dev)
    sx, sy = (torch.tensor(t, dtype=i64, device=dev) for t in step_tables())
    turn = torch.tensor(TURN, dtype=i64, device=dev)
    w = weights(depth, discount)

    W = levels.to(i64).clamp(0, CAP)
    last = W.shape[1] - 1
    zero = torch.zeros((), dtype=i64, device=dev)
    actions = torch.empty(B, n, dtype=i64, device=dev)
    plans, scores = torch.empty_like(actions), torch.empty_like(actions)
    for i in range(n):
        x, y, hh = X[:, i:i + 1], Y[:, i:i + 1], h[:, i:i + 1]                       # [B, 1]: the root, no node itself
        covered = torch.zeros(B, 1, cells, dtype=torch.bool, device=dev)
        score = torch.zeros(B, 1, dtype=i64, device=dev)
        for d in range(depth):   # level d: 3^(d + 1) nodes, node j the child (j % 3) of node j // 3 of level d - 1
            x, y, hh = (t.repeat_interleave(3, dim=1) for t in (x, y, hh))
            t = turn.repeat(x.shape[1] // 3).unsqueeze(0)
            for _ in range(stride):
                hh = (hh + t) % bl.HEADINGS
                x = torch.clamp(x + sx[hh], 0, lim)
                y = torch.clamp(y + sy[hh], 0, lim)
            covered = covered.repeat_interleave(3, dim=1)
            disc = bl.disc_mask(centre, x, y, R2)
            gain = torch.where(disc & ~covered, W[:, min(d, last)].unsqueeze(1), zero).sum(-1)     # [B, 3^(d + 1)]
            score = score.repeat_interleave(3, dim=1) + gain * w[d]
            covered = covered | disc
        top = score.max(dim=1, keepdim=True).values
        s = torch.arange(score.shape[1], dtype=i64, device=dev)
        best = torch.where(score == top, s, torch.full_like(s, score.shape[1])).min(dim=1).values   # the lowest s of the largest
        plans[:, i] = best
        scores[:, i] = top[:, 0]
        actions[:, i] = best // (3 ** (depth - 1))
        chosen = covered.gather(1, best.view(B, 1, 1).expand(B, 1, cells))[:, 0]
        W = torch.where(chosen.unsqueeze(1), zero, W)   # in every level
    return actions, plans, scores


def plan_actions_torch(state, grid, n_agents, side, view_range, depth, stride, discount, return_plans=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grid int32 [B, side * side] (read only) -> actions int64
    [B, n]; with return_plans also the winning sequence index and its score, int64 [B, n] each.  Stock EAGER torch ops on the
    tensors' device (see baseline.coverage_actions_torch on why eager)."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    depth, stride, discount = int(depth), int(stride), int(discount)
    _check_params(n, side, view_range, depth, stride, discount)
    _check_tensors(state, grid, n, side)
    rows = max(1, _CHUNK // (3 ** depth * side * side))   # envs are independent: a large batch goes block by block
    parts = [_plan_rows(state[b:b + rows], grid[b:b + rows].unsqueeze(1), n, side, view_range, depth, stride, discount)
             for b in range(0, int(state.shape[0]), rows)]
    actions, plans, scores = (torch.cat(t) for t in zip(*parts))
    return (actions, plans, scores) if return_plans else actions


class PlanAgents:
    """The planner over a base policy's grid, for a batch of envs.  env_or_args: a BatchedFlightEnv / MovingTargetEnv or an args
    namespace, as the base reads it; base: "coverage" (a `CoverageAgents` is built), "belief" (a `BeliefAgents`, with `motion`) or
    an instance of either, of the same impl, batch and device; depth, stride, discount (Q8): the sequences of the module
    docstring.  impl = "hip": the kernels, one launch of the base's and one of cs_plan_actions per `choose_action` on the current
    stream, no synchronisation; "torch": the definitions, on the same device.

    `choose_action(state, moved)` lets the base advance its grid (regrow and sweep, or predict and sweep), discards the base's own
    actions and plans on the grid it left.  `policy()` is a `policy(obs, state, last, t)` callable with BeliefAgents' rule: it
    resets at t == 0 and moved = t > 0 and speed > 0 and (t - 1) % every == 0 (a coverage base ignores moved).  `plans` and
    `scores` hold the last decision's winning sequences and their scores, int64 [B, n]."""

    def __init__(self, env_or_args, base="coverage", motion=None, depth=4, stride=3, discount=230, batch=None, device=None, impl="hip"):
        src = env_or_args
        if impl not in ("hip", "torch"):
            raise ValueError("impl must be 'hip' (the kernel of csrc/plan.h) or 'torch' (the definition)")
        if isinstance(base, (bl.CoverageAgents, be.BeliefAgents)):
            if base.impl != impl:
                raise ValueError(f"PlanAgents: the base runs impl={base.impl!r}, the planner impl={impl!r}")
            if batch is not None and int(batch) != base.batch:
                raise ValueError(f"PlanAgents: batch {batch} is not the base's ({base.batch})")
            if device is not None and torch.device(device).type != base.device.type:
                raise ValueError(f"PlanAgents: device {device} is not the base's ({base.device})")
        elif base == "coverage":
            base = bl.CoverageAgents(src, batch=batch, device=device, impl=impl)
        elif base == "belief":
            base = be.BeliefAgents(src, motion=motion, batch=batch, device=device, impl=impl)
        else:
            raise ValueError("PlanAgents: base must be 'coverage', 'belief' or a CoverageAgents / BeliefAgents instance")
        self.base, self.impl = base, impl
        self.batch, self.device = base.batch, base.device
        if impl == "hip" and self.device.type != "cuda":
            raise ValueError(f"PlanAgents(impl='hip') runs a HIP kernel and {self.device} is not a GPU: there is no CPU "
                             "fallback (impl='torch' runs the definition anywhere)")
        self.n_agents, self.side, self.view_range = base.n_agents, base.side, base.view_range
        self.depth, self.stride, self.discount = int(depth), int(stride), int(discount)
        _check_params(self.n_agents, self.side, self.view_range, self.depth, self.stride, self.discount)
        if motion is None:
            motion = getattr(base, "motion", None) or getattr(src, "motion", None)
            if not isinstance(motion, mo.TargetMotion):
                motion = mo.TargetMotion.from_args(src)
        if not isinstance(motion, mo.TargetMotion):
            raise TypeError("PlanAgents: motion must be a TargetMotion")
        self.motion = motion
        self.plans = torch.zeros(self.batch, self.n_agents, dtype=torch.int64, device=self.device)
        self.scores = torch.zeros_like(self.plans)

    @property
    def grid(self):
        return self.base.grid

    def reset(self):
        self.base.reset()

    def choose_action(self, state, moved=0):
        """get_state() rows float32 [B, S] -> actions int64 [B, n]; the base's grid moves on by one step."""
        if isinstance(self.base, be.BeliefAgents):
            self.base.choose_action(state, moved)
        else:
            self.base.choose_action(state)
        if self.impl == "torch":
            actions, plans, scores = plan_actions_torch(state, self.base.grid, self.n_agents, self.side, self.view_range, self.depth,
                                                        self.stride, self.discount, return_plans=True)
            self.plans.copy_(plans)
            self.scores.copy_(scores)
            return actions
        actions = torch.empty(self.batch, self.n_agents, dtype=torch.int64, device=self.device)
        _lib.torch_ops_for(NEEDS).plan_actions(state, self.base.grid, actions, self.plans, self.scores, self.n_agents, self.side,
                                               self.view_range, self.depth, self.stride, self.discount)
        return actions

    def policy(self):
        motion = self.motion

        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state, be.targets_moved(motion, t))
        return policy
