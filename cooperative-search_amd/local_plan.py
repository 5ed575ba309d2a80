"""The receding-horizon planner on private grids under a communication range (include/coopsearch.h: cs_local_plan_actions; DESIGN.md
section 28).

`PlanAgents` plans on ONE grid per env and lets every agent see the claims of every agent that decided before it, however far apart
they fly: a centralised planner.  `LocalCoverageAgents` and `LocalBeliefAgents` keep a grid per agent and talk only inside
`comm_range`, but decide greedily, and park at walls as the greedy filters do.  Here agent i plans on the grid it actually owns and
hears only the claims of the team-mates it is linked to: the planner a decentralised learner can be held against, and cloned from.

`local_plan_actions_torch` is the DEFINITION, in stock eager torch ops on any device; the kernel (csrc/local_plan.h) reproduces its
actions, plans and scores bit for bit.  Everything is integer after the one float32 quantisation, and everything is baseline.py's,
local.py's and plan.py's: `quantise`, `cell_centres`, `disc_mask`, `links`, `_check_comm`, CAP, `plan_actions_torch` (and through it
`step_tables`, `weights`, TURN, the node tree, the gains less the ancestors' discs, the score and the tie rule) and
`sequence_points` are imported, not restated.  `grids` is int32 [B, n, side * side], agent i's private grid, row-major
[ix * side + iy]; it is only read.  Per env:

  links    adj = local.links(X, Y, comm_range): strict, symmetric, 64-bit, -1 unlimited, the diagonal set.
  order    the agents decide in index order.
  grid     agent i plans on W_i = clamp(grids[:, i], 0, CAP), zeroed on the union of the `depth` discs of the winning sequence of
           every j < i with adj[:, i, j]: the claims of the linked team-mates that decided before it, and no others (local.py's
           choose rule).
  search   plan.py's module docstring on W_i, for one agent: `plan_actions_torch` with n_agents = 1 on agent i's four floats.  The
           choice is the lowest s of the largest score, the action its first digit; its claim is the discs around
           `sequence_points` of the choice.

Four identities pin it (tests/test_local_plan_cpu.py):
  A  unlimited range, equal grids G: actions, plans and scores are plan_actions_torch(state, G, ...)'s.  W_i is then G less the discs
     of all j < i, which is plan.py's W when agent i decides.
  B  range 0: row i is plan_actions_torch with n_agents = 1 on agent i's four floats and grid i.
  C  prefix: the outputs of agents 0 .. k-1 do not depend on agents k .. n-1.
  D  a hand case: A - B - C in a line, A-B and B-C linked, A-C not; C's gain lacks B's disc and keeps A's.
"""
import torch

from . import _lib
from . import belief as be
from . import local as lc
from . import local_belief as lb
from . import motion as mo
from .baseline import _check_state_grid, cell_centres, disc_mask, quantise
from .local import _check_comm, links
from .plan import CAP, MAX_DEPTH, TURN, _check_params, plan_actions_torch, sequence_points, step_tables, weights  # noqa: F401

NEEDS = "the local plan kernel needs"   # _lib.torch_ops_for's words


def local_plan_actions_torch(state, grids, n_agents, side, view_range, depth, stride, discount, comm_range, return_plans=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grids int32 [B, n, side * side] (read only), comm_range -1 or
    0..128 -> actions int64 [B, n]; with return_plans also the winning sequence index and its score, int64 [B, n] each.  Stock EAGER
    torch ops on the tensors' device (see baseline.coverage_actions_torch on why eager)."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    depth, stride, discount, comm_range = int(depth), int(stride), int(discount), int(comm_range)
    _check_params(n, side, view_range, depth, stride, discount)
    _check_comm(comm_range)
    if not torch.is_tensor(state) or not torch.is_tensor(grids):
        raise TypeError("local plan: state and grids must be tensors")
    _check_state_grid("local plan", state, grids, n, (n, side * side), name="grids")
    B = int(state.shape[0])
    X, Y, h = quantise(state, n, side)
    adj = links(X, Y, comm_range)
    centre, R2 = cell_centres(side, state.device), (16 * view_range) ** 2
    zero = torch.zeros((), dtype=torch.int32, device=state.device)
    out, claims = [], []
    for i in range(n):
        W = grids[:, i].clamp(0, CAP)
        for j in range(i):   # the claims agent i has heard
            W = torch.where(claims[j] & adj[:, i, j].view(B, 1), zero, W)
        one = plan_actions_torch(state[:, 4 * i:4 * i + 4].contiguous(), W, 1, side, view_range, depth, stride, discount, return_plans=True)
        out.append(one)
        px, py = sequence_points(X[:, i], Y[:, i], h[:, i], one[1][:, 0], side, depth, stride)
        claims.append(disc_mask(centre, px, py, R2).any(1))
    actions, plans, scores = (torch.cat(t, 1) for t in zip(*out))
    return (actions, plans, scores) if return_plans else actions


class LocalPlanAgents:
    """The planner over a decentralised base policy's n private grids, for a batch of envs.  env_or_args: a BatchedFlightEnv /
    MovingTargetEnv or an args namespace, as the base reads it; comm_range in whole cells, 0..128, None = unlimited; base: "coverage"
    (a `LocalCoverageAgents` is built), "belief" (a `LocalBeliefAgents`, with `motion`) or an instance of either, of the same impl,
    batch, device and comm_range; depth, stride, discount (Q8): the sequences of plan.py's module docstring.  impl = "hip": the
    kernels, one launch of the base's and one of cs_local_plan_actions per `choose_action` on the current stream, no
    synchronisation; "torch": the definitions, on the same device.

    `choose_action(state, moved)` lets the base advance its n grids (regrow, sweep and merge, or predict, sweep and merge), discards
    the base's own actions and plans on the grids it left.  `policy()` is a `policy(obs, state, last, t)` callable with PlanAgents'
    rule: it resets at t == 0 and moved = belief.targets_moved(motion, t) (a coverage base ignores moved).  `grids` is the base's;
    `plans` and `scores` hold the last decision's winning sequences and their scores, int64 [B, n].  With comm_range None it flies
    PlanAgents' episodes; with 0, n lone planners'."""

    def __init__(self, env_or_args, comm_range, base="coverage", motion=None, depth=4, stride=3, discount=230, batch=None, device=None,
                 impl="hip"):
        src = env_or_args
        if impl not in ("hip", "torch"):
            raise ValueError("impl must be 'hip' (the kernel of csrc/local_plan.h) or 'torch' (the definition)")
        if comm_range is not None and (int(comm_range) != comm_range or comm_range < 0):
            raise ValueError(f"LocalPlanAgents: comm_range must be a whole number of cells, 0..{lc.MAX_COMM}, or None (unlimited), "
                             f"got {comm_range!r}")
        self.comm_range = -1 if comm_range is None else int(comm_range)
        _check_comm(self.comm_range)
        if isinstance(base, (lc.LocalCoverageAgents, lb.LocalBeliefAgents)):
            if base.impl != impl:
                raise ValueError(f"LocalPlanAgents: the base runs impl={base.impl!r}, the planner impl={impl!r}")
            if batch is not None and int(batch) != base.batch:
                raise ValueError(f"LocalPlanAgents: batch {batch} is not the base's ({base.batch})")
            if device is not None and torch.device(device).type != base.device.type:
                raise ValueError(f"LocalPlanAgents: device {device} is not the base's ({base.device})")
            if base.comm_range != self.comm_range:
                raise ValueError(f"LocalPlanAgents: comm_range {comm_range} is not the base's "
                                 f"({None if base.comm_range < 0 else base.comm_range})")
        elif base == "coverage":
            base = lc.LocalCoverageAgents(src, comm_range, batch=batch, device=device, impl=impl)
        elif base == "belief":
            base = lb.LocalBeliefAgents(src, comm_range, motion=motion, batch=batch, device=device, impl=impl)
        else:
            raise ValueError("LocalPlanAgents: base must be 'coverage', 'belief' or a LocalCoverageAgents / LocalBeliefAgents instance")
        self.base, self.impl = base, impl
        self.batch, self.device = base.batch, base.device
        if impl == "hip" and self.device.type != "cuda":
            raise ValueError(f"LocalPlanAgents(impl='hip') runs a HIP kernel and {self.device} is not a GPU: there is no CPU "
                             "fallback (impl='torch' runs the definition anywhere)")
        self.n_agents, self.side, self.view_range = base.n_agents, base.side, base.view_range
        self.depth, self.stride, self.discount = int(depth), int(stride), int(discount)
        _check_params(self.n_agents, self.side, self.view_range, self.depth, self.stride, self.discount)
        if motion is None:
            motion = getattr(base, "motion", None) or getattr(src, "motion", None)
            if not isinstance(motion, mo.TargetMotion):
                motion = mo.TargetMotion.from_args(src)
        if not isinstance(motion, mo.TargetMotion):
            raise TypeError("LocalPlanAgents: motion must be a TargetMotion")
        self.motion = motion
        self.plans = torch.zeros(self.batch, self.n_agents, dtype=torch.int64, device=self.device)
        self.scores = torch.zeros_like(self.plans)

    @property
    def grids(self):
        return self.base.grids

    def reset(self):
        self.base.reset()

    def choose_action(self, state, moved=0):
        """get_state() rows float32 [B, S] -> actions int64 [B, n]; the base's n grids move on by one step."""
        if isinstance(self.base, lb.LocalBeliefAgents):
            self.base.choose_action(state, moved)
        else:
            self.base.choose_action(state)
        if self.impl == "torch":
            actions, plans, scores = local_plan_actions_torch(state, self.base.grids, self.n_agents, self.side, self.view_range, self.depth,
                                                              self.stride, self.discount, self.comm_range, return_plans=True)
            self.plans.copy_(plans)
            self.scores.copy_(scores)
            return actions
        actions = torch.empty(self.batch, self.n_agents, dtype=torch.int64, device=self.device)
        _lib.torch_ops_for(NEEDS).local_plan_actions(state, self.base.grids, actions, self.plans, self.scores, self.n_agents, self.side,
                                                     self.view_range, self.depth, self.stride, self.discount, self.comm_range)
        return actions

    def policy(self):
        motion = self.motion

        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state, be.targets_moved(motion, t))
        return policy
