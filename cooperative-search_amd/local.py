"""Coverage search under a limited communication range (include/coopsearch.h: cs_local_coverage_actions).

`CoverageAgents` decides from one grid per env: every agent knows at once what every team-mate has swept, however far apart they
fly.  That is a centralised controller.  Here agent i keeps a grid of its own and hears only the team-mates within `comm_range`
cells of it: the hand-written baseline a decentralised learner should be held against, and the answer to "what does the team lose
when agents can only talk within r cells" (DESIGN.md section 25 has the numbers).

`local_coverage_actions_torch` is the DEFINITION, in stock torch ops; the kernel (csrc/local.h) reproduces its grids and its actions
bit for bit.  Everything is baseline.py's -- `quantise`, the trig tables, `keep_of`, FRESH, the regrowth, the sweep test, the
look-ahead footprints, the tie rule and the action coding -- but for the links:

  links   adj(i, j), i != j, holds iff comm_range < 0 (unlimited) or (X_i - X_j)^2 + (Y_i - Y_j)^2 < (16 comm_range)^2 in sub-units
          of 1/16 cell.  Strict, so comm_range 0 links nobody, not even two agents on one spot; adj(i, i) holds; it is symmetric;
          64-bit (clamped positions differ by up to 2^16 per axis).  comm_range is in whole cells: -1, or 0..128.
  regrow  every agent's grid: G += (65536 - G) >> regrow.
  sweep   agent i multiplies by keep >> 16 only the cells within 16 view_range of ITS OWN position: S_i.
  merge   M_i = min over the j with adj(i, j) of S_j, cell by cell, from the post-sweep grids; M_i is written back to grids[:, i].
          ONE hop per call: what C told B in this call reaches A, who hears B and not C, in the next.  News travels along a chain of
          linked agents one hop per decision.
  choose  agents decide in index order; agent i scores the three look-ahead footprints on W_i = M_i with the chosen footprint
          zeroed for every j < i with adj(i, j): it hears the claims of the linked team-mates that decided before it, and no others.
"""
import torch

from .baseline import (FRESH, GridAgents, _check_params, _check_state_grid, cell_centres, disc_mask, greedy_choose, keep_of, quantise,
                       trig_tables)

MAX_COMM = 128   # LOC_MAX_COMM of csrc/local.h, in cells (a 64-cell map's diagonal is under 91)


def _check_comm(comm_range):
    if not -1 <= comm_range <= MAX_COMM:
        raise ValueError(f"local coverage: comm_range must be -1 (unlimited) or 0..{MAX_COMM} cells, got {comm_range!r}")


def links(X, Y, comm_range):
    """Quantised positions int64 [B, n] -> adj, bool [B, n, n] (module docstring: strict, symmetric, the diagonal set)."""
    n = X.shape[1]
    eye = torch.eye(n, dtype=torch.bool, device=X.device).unsqueeze(0)
    if comm_range < 0:
        return eye | torch.ones(X.shape[0], n, n, dtype=torch.bool, device=X.device)
    dx, dy = X[:, :, None] - X[:, None, :], Y[:, :, None] - Y[:, None, :]   # int64: a square reaches 2^32
    return (dx * dx + dy * dy < (16 * comm_range) ** 2) | eye


def local_coverage_actions_torch(state, grids, n_agents, side, view_range, keep, comm_range, regrow=8, lookahead=None,
                                 return_scores=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grids int32 [B, n, side * side] (agent i's private grid,
    row-major [ix * side + iy], Q16, updated in place; a cell outside 0..65536 is read as the nearer bound) -> actions int64 [B, n];
    with return_scores also the scores each agent chose from, int64 [B, n, 3].  Eager torch only, as coverage_actions_torch.

    The merge is one hop per call and reads the post-sweep grids S, never an already merged one: news travels along a chain of
    linked agents one hop per decision.

    Two identities pin the policy from both sides:
      unlimited range  if all n grids start equal (G), every M_i equals the grid coverage_actions_torch leaves and the actions are
                       equal.  S_j is regrown G, multiplied by keep >> 16 inside j's disc only; (v * keep) >> 16 <= v since keep <=
                       65536, so the minimum over ALL j of S_j at a cell is the multiplied value where any agent sees the cell and
                       the regrown value elsewhere: coverage's sweep of the n discs.  The n grids are then equal again, so the
                       identity holds call after call.  With every pair linked, W_i is that grid with the footprints of all j < i
                       zeroed, which is coverage's W when agent i decides.
      range 0          nobody is linked: M_i = S_i, the regrowth and the one-disc sweep of coverage_actions_torch with n_agents = 1
                       on agent i's four floats, and W_i = M_i, since agent i hears no claim, as a lone agent has none to hear.
    """
    n, side, view_range, keep, regrow, comm_range = int(n_agents), int(side), int(view_range), int(keep), int(regrow), int(comm_range)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check_params(n, side, view_range, keep, regrow, lookahead)
    _check_comm(comm_range)
    _check_state_grid("local coverage", state, grids, n, (n, side * side), name="grids")
    X, Y, h = quantise(state, n, side)
    adj = links(X, Y, comm_range)
    centre, R2 = cell_centres(side, state.device), (16 * view_range) ** 2
    G = grids.to(torch.int64).clamp(0, FRESH)   # [B, n, cells]
    G = G + ((FRESH - G) >> regrow)
    own = torch.stack([disc_mask(centre, X[:, i], Y[:, i], R2) for i in range(n)], 1)
    S = torch.where(own, (G * keep) >> 16, G)
    far = torch.full_like(S, FRESH + 1)   # above every cell: an agent that is not heard does not enter the minimum
    M = torch.stack([torch.where(adj[:, i, :, None], S, far).min(1).values for i in range(n)], 1)
    grids.copy_(M.to(torch.int32))
    actions, scores = greedy_choose(M, X, Y, h, side, view_range, lookahead, adj)
    return (actions, scores) if return_scores else actions


class LocalCoverageAgents(GridAgents):
    """The coverage baseline under a communication range, for a batch of envs: CoverageAgents' arguments, and comm_range in whole
    cells, 0..128, None = unlimited.

    `.grids` is int32 [B, n, side * side]: agent i's private grid; `policy()` resets them when t == 0.  With comm_range None it
    flies CoverageAgents' episodes; with 0, n lone agents'."""
    KERNEL, NEEDS = "local.h", "the coverage kernel needs"

    def __init__(self, env_or_args, comm_range, batch=None, device=None, lookahead=None, regrow=8, impl="hip"):
        super().__init__(env_or_args, batch, device, lookahead, impl)
        self.regrow = int(regrow)
        _check_params(self.n_agents, self.side, self.view_range, self.keep, self.regrow, self.lookahead)
        if comm_range is not None and (int(comm_range) != comm_range or comm_range < 0):
            raise ValueError(f"LocalCoverageAgents: comm_range must be a whole number of cells, 0..{MAX_COMM}, or None (unlimited), "
                             f"got {comm_range!r}")
        self.comm_range = -1 if comm_range is None else int(comm_range)
        _check_comm(self.comm_range)
        self.grids = torch.full((self.batch, self.n_agents, self.side * self.side), FRESH, dtype=torch.int32, device=self.device)

    def reset(self):
        """Fresh private grids: nobody has looked anywhere, and nobody has been told anything."""
        self.grids.fill_(FRESH)

    def choose_action(self, state):
        """get_state() rows float32 [B, S] -> actions int64 [B, n]; the n grids move on by one step."""
        if self.impl == "torch":
            return local_coverage_actions_torch(state, self.grids, self.n_agents, self.side, self.view_range, self.keep, self.comm_range,
                                                self.regrow, self.lookahead)
        ops, actions = self._launch(state)
        ops.local_coverage_actions(state, self.grids, actions, self.n_agents, self.side, self.view_range, self.keep, self.regrow,
                                   self.lookahead, self.comm_range)
        return actions
