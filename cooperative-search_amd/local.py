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

from .baseline import FRESH, HEADINGS, _check_params, _ops, keep_of, quantise, trig_tables

MAX_COMM = 128   # LOC_MAX_COMM of csrc/local.h, in cells (a 64-cell map's diagonal is under 91)


def _check_comm(comm_range):
    if not -1 <= comm_range <= MAX_COMM:
        raise ValueError(f"local coverage: comm_range must be -1 (unlimited) or 0..{MAX_COMM} cells, got {comm_range!r}")


def _check_tensors(state, grids, n, side):
    if state.dim() != 2 or state.dtype != torch.float32 or state.shape[0] < 1 or state.shape[1] < 4 * n:
        raise ValueError(f"local coverage: state must be float32 [B, S] with B >= 1 and S >= 4 n_agents = {4 * n}")
    if grids.dtype != torch.int32 or tuple(grids.shape) != (state.shape[0], n, side * side) or grids.device != state.device:
        raise ValueError(f"local coverage: grids must be int32 [{state.shape[0]}, {n}, {side * side}] on the state's device")


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
    _check_tensors(state, grids, n, side)
    i64, dev = torch.int64, state.device
    B, R2 = int(state.shape[0]), (16 * view_range) ** 2
    X, Y, h = quantise(state, n, side)
    adj = links(X, Y, comm_range)
    centre = (16 * torch.arange(side, dtype=i64, device=dev) + 8).view(1, side)

    def within(px, py):   # [B] points -> [B, cells], cell ix * side + iy
        dx, dy = centre - px.view(B, 1), centre - py.view(B, 1)
        return ((dx * dx).view(B, side, 1) + (dy * dy).view(B, 1, side) <= R2).view(B, side * side)

    G = grids.to(i64).clamp(0, FRESH)   # [B, n, cells]
    G = G + ((FRESH - G) >> regrow)
    own = torch.stack([within(X[:, i], Y[:, i]) for i in range(n)], 1)
    S = torch.where(own, (G * keep) >> 16, G)
    far = torch.full_like(S, FRESH + 1)   # above every cell: an agent that is not heard does not enter the minimum
    M = torch.stack([torch.where(adj[:, i, :, None], S, far).min(1).values for i in range(n)], 1)
    grids.copy_(M.to(torch.int32))
    ct, st = trig_tables()
    offx = torch.tensor([(lookahead * 16 * v) >> 14 for v in ct], dtype=i64, device=dev)   # (Python's >> floors)
    offy = torch.tensor([(lookahead * 16 * v) >> 14 for v in st], dtype=i64, device=dev)
    zero = torch.zeros(B, side * side, dtype=i64, device=dev)
    actions = torch.empty(B, n, dtype=i64, device=dev)
    scores = torch.empty(B, n, 3, dtype=i64, device=dev)
    claims = []
    for i in range(n):
        W = M[:, i]
        for j in range(i):   # the claims agent i has heard
            W = torch.where(claims[j] & adj[:, i, j].view(B, 1), zero, W)
        foot, score = [], []
        for turn in (0, 1, HEADINGS - 1):
            hp = (h[:, i] + turn) % HEADINGS
            px = torch.clamp(X[:, i] + offx[hp], 0, 16 * side)
            py = torch.clamp(Y[:, i] + offy[hp], 0, 16 * side)
            foot.append(within(px, py))
            score.append(torch.where(foot[-1], W, zero).sum(1))
        best = (score[1] > score[0]).to(i64)
        best = torch.where(score[2] > torch.maximum(score[0], score[1]), torch.full_like(best, 2), best)
        actions[:, i] = best
        scores[:, i] = torch.stack(score, 1)
        claims.append(torch.where((best == 0).view(B, 1), foot[0], torch.where((best == 1).view(B, 1), foot[1], foot[2])))
    return (actions, scores) if return_scores else actions


class LocalCoverageAgents:
    """The coverage baseline under a communication range, for a batch of envs.  env_or_args, batch, device, lookahead, regrow and
    impl are CoverageAgents'; comm_range is in whole cells, 0..128, None = unlimited.  impl = "hip": the kernel of csrc/local.h, one
    launch per `choose_action` on the current stream, no synchronisation; "torch": the definition, on the same device.

    `.grids` is int32 [B, n, side * side]: agent i's private grid.  `policy()` is a `policy(obs, state, last, t)` callable for
    EpisodeCollector.generate_episodes(policy=...), collector.evaluate and collector.collect_experiment_data; it resets the grids
    when t == 0.  With comm_range None it flies CoverageAgents' episodes; with 0, n lone agents'."""

    def __init__(self, env_or_args, comm_range, batch=None, device=None, lookahead=None, regrow=8, impl="hip"):
        src = env_or_args
        if impl not in ("hip", "torch"):
            raise ValueError("impl must be 'hip' (the kernel of csrc/local.h) or 'torch' (the definition)")
        batch = getattr(src, "batch", None) if batch is None else batch
        if batch is None or int(batch) < 1:
            raise ValueError("LocalCoverageAgents: batch must be given (>= 1) with an args namespace")
        self.batch = int(batch)
        self.device = torch.device(device if device is not None else getattr(src, "device", "cuda"))
        if impl == "hip" and self.device.type != "cuda":
            raise ValueError(f"LocalCoverageAgents(impl='hip') runs a HIP kernel and {self.device} is not a GPU: there is no CPU "
                             "fallback (impl='torch' runs the definition anywhere)")
        self.impl = impl
        self.n_agents, self.side = int(src.n_agents), int(src.map_size)
        if int(src.view_range) != src.view_range:
            raise ValueError(f"LocalCoverageAgents: view_range must be a whole number of cells, got {src.view_range!r}")
        self.view_range = int(src.view_range)
        self.keep = keep_of(src.detect_prob)
        self.regrow = int(regrow)
        self.lookahead = min(self.view_range, self.side) if lookahead is None else int(lookahead)
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
        if not torch.is_tensor(state) or state.dim() != 2 or int(state.shape[0]) != self.batch:
            raise ValueError(f"LocalCoverageAgents: state must be a [{self.batch}, S] tensor")
        actions = torch.empty(self.batch, self.n_agents, dtype=torch.int64, device=self.device)
        _ops().local_coverage_actions(state, self.grids, actions, self.n_agents, self.side, self.view_range, self.keep, self.regrow,
                                      self.lookahead, self.comm_range)
        return actions

    def policy(self):
        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state)
        return policy
