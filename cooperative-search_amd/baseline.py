"""A policy to compare the learners with: the greedy coverage baseline (include/coopsearch.h: cs_coverage_actions).

The reference ships no hand-written policy (policy/trandition.py is a stub with a Random subclass), so a trained QMIX or PPO
team can only be held against `collector.random_policy`.  This is the classical answer to cooperative search, a greedy sweep
of a shared belief map: it needs no training and no checkpoint, and as a kernel it runs at env speed.

`coverage_actions_torch` is the DEFINITION, in stock torch ops; the kernel (csrc/coverage.h) reproduces its actions and its
grid element for element.  DESIGN.md section 17 has the text; in short, per env and call:

  state     only the first 4n floats of a get_state() row are read: agent i = (xn, yn, cos, sin) at 4i.  Targets, found flags
            and flight's map are never looked at, so the same code serves flight_easy and flight.
  grid      G, int32 [side * side], row-major [ix * side + iy], Q16: 65536 = "nobody has looked here"; `reset()` fills it.
            A cell outside 0..65536 is read as the nearer bound.
  quantise  half = map_size / 2 (float32): X = rint((xn * half + half) * 16), Y likewise (sub-units of 1/16 cell), c =
            rint(cos * 16384), s likewise -- float32, every operation rounded once, round-half-even; everything after is
            integer.  The heading index h is the lowest k of 0..35 that maximises c * CT[k] + s * ST[k], CT / ST =
            rint(16384 cos / sin(k pi / 18)).
  regrow    every cell: G += (65536 - G) >> regrow  (without it a team parks against a wall once all it can reach is 0)
  sweep     a cell (centre 16 ix + 8, 16 iy + 8) within R = 16 view_range of any agent: G = (G * keep) >> 16, keep =
            rint((1 - detect_prob) * 65536).  G is written back in this state.
  choose    W = G; agents decide in index order.  Action a turns the heading by {0, +1, -1}[a] (the env's coding: 1 is
            + pi / 18); the look-ahead point is P = clamp(X + ((16 lookahead * CT[h']) >> 14), 0, 16 side), the same for Y
            with ST (>> floors); score_a = the sum of W over the cells within R of P; the agent takes the lowest a with
            the largest score and W is zeroed on that footprint, so that teammates spread out.

Rows that no env emits are made harmless rather than undefined: a quantised position is clamped to +-2^15 sub-units and a
heading component to +-2^14 (NaN goes to the lower bound).  Neither changes anything for rows that get_state() produces.

Drawing a coverage episode (render.py):

    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy"), batch=4)
    episode, *_ = cs.EpisodeCollector(env).generate_episodes(policy=cs.CoverageAgents(env).policy(), init=True)
    cs.write_frames(cs.render_episodes(*cs.episode_tables(episode), cs.RenderSpec.for_env(env)), "coverage.gif")
"""
import math

import torch

from . import _lib

FRESH = 65536          # a cell nobody has looked at (Q16)
HEADINGS = 36          # the env turns by pi / 18
POS_LIM = float(1 << 15)
TRIG_LIM = float(1 << 14)
MAX_MAP = 64           # CS_MAX_MAP


def trig_tables():
    """(CT, ST): rint(16384 cos(k pi / 18)) and rint(16384 sin(k pi / 18)) for k = 0..35 as Python ints, computed in double
    (no product is within 0.06 of a tie, so every correctly rounded libm gives the same table; csrc/coverage.h holds it as literals)."""
    ct = [int(round(16384.0 * math.cos(k * math.pi / 18))) for k in range(HEADINGS)]
    st = [int(round(16384.0 * math.sin(k * math.pi / 18))) for k in range(HEADINGS)]
    return ct, st


def keep_of(detect_prob):
    """rint((1 - detect_prob) * 65536) in double."""
    keep = int(round((1.0 - float(detect_prob)) * 65536.0))
    if not 0 <= keep <= FRESH:
        raise ValueError(f"detect_prob must be in 0..1, got {detect_prob!r}")
    return keep


def _quant(v, lim):
    """rint(v) as int64 in [-lim, lim]; NaN gives -lim."""
    r = torch.round(v)
    hi, lo = torch.full_like(r, lim), torch.full_like(r, -lim)
    return torch.where(r >= -lim, torch.where(r <= lim, r, hi), lo).to(torch.int64)


def quantise_positions(state, n_agents, side):
    """The position part of `quantise`: state rows float32 [B, S] -> (X, Y), int64 [B, n], in sub-units of 1/16 cell."""
    B, n = int(state.shape[0]), int(n_agents)
    ag = state[:, :4 * n].reshape(B, n, 4)
    half = float(side) / 2.0
    return _quant((ag[..., 0] * half + half) * 16.0, POS_LIM), _quant((ag[..., 1] * half + half) * 16.0, POS_LIM)


def quantise(state, n_agents, side):
    """The first 4n floats of state rows float32 [B, S] -> (X, Y, h), int64 [B, n]: positions in sub-units, heading index."""
    B, n = int(state.shape[0]), int(n_agents)
    ag = state[:, :4 * n].reshape(B, n, 4)
    X, Y = quantise_positions(state, n, side)
    c, s = _quant(ag[..., 2] * 16384.0, TRIG_LIM), _quant(ag[..., 3] * 16384.0, TRIG_LIM)
    ct, st = (torch.tensor(t, dtype=torch.int64, device=state.device) for t in trig_tables())
    dot = c[..., None] * ct + s[..., None] * st                                           # [B, n, 36]
    k = torch.arange(HEADINGS, dtype=torch.int64, device=state.device)
    h = torch.where(dot == dot.max(-1, keepdim=True).values, k, torch.full_like(k, HEADINGS)).min(-1).values
    return X, Y, h


def _check_team(prefix, n, side, view_range):
    if not 1 <= n <= _lib.MAX_AGENTS or not 1 <= side <= MAX_MAP or not 0 <= view_range <= MAX_MAP:
        raise ValueError(f"{prefix}: n_agents must be 1..{_lib.MAX_AGENTS}, side 1..{MAX_MAP} and view_range 0..{MAX_MAP}")


def _check_params(n, side, view_range, keep, regrow, lookahead):
    _check_team("coverage", n, side, view_range)
    if not 0 <= keep <= FRESH or not 1 <= regrow <= 16 or not 0 <= lookahead <= side:
        raise ValueError("coverage: keep must be 0..65536, regrow 1..16 and lookahead 0..side")


def _check_state_grid(prefix, state, grid, n, shape, name="grid"):
    """state float32 [B, S >= 4n] and `grid` int32 [B, *shape] on the state's device."""
    if state.dim() != 2 or state.dtype != torch.float32 or state.shape[0] < 1 or state.shape[1] < 4 * n:
        raise ValueError(f"{prefix}: state must be float32 [B, S] with B >= 1 and S >= 4 n_agents = {4 * n}")
    want = (state.shape[0], *shape)
    if grid.dtype != torch.int32 or tuple(grid.shape) != want or grid.device != state.device:
        raise ValueError(f"{prefix}: {name} must be int32 {list(want)} on the state's device")


def cell_centres(side, device):
    """int64 [side]: 16 i + 8, the centre of row (or column) i in sub-units of 1/16 cell."""
    return 16 * torch.arange(side, dtype=torch.int64, device=device) + 8


def disc_mask(centre, px, py, R2):
    """Points int64 [B] or [B, N] -> bool [B, cells] or [B, N, cells], cell ix * side + iy: the cells whose centre (`centre`:
    `cell_centres`) lies within R of the point, R2 = R^2 (<= on squared integers)."""
    dx, dy = centre - px.unsqueeze(-1), centre - py.unsqueeze(-1)
    return ((dx * dx).unsqueeze(-1) + (dy * dy).unsqueeze(-2) <= R2).flatten(-2)


def swept(centre, X, Y, R2):
    """bool [B, cells]: the cells within R of any of the agents X, Y int64 [B, n] (the sweep test)."""
    seen = disc_mask(centre, X[:, 0], Y[:, 0], R2)
    for i in range(1, X.shape[1]):
        seen = seen | disc_mask(centre, X[:, i], Y[:, i], R2)
    return seen


def greedy_choose(M, X, Y, h, side, view_range, lookahead, adj=None):
    """The choose stage of the coverage, belief and local policies -> (actions int64 [B, n], scores int64 [B, n, 3]).  M int64: the
    swept grid, [B, cells] for one grid per env or [B, n, cells] for one per agent; X, Y, h: `quantise`'s.  Agents decide in index
    order: agent i scores its three look-ahead footprints on its grid with the footprints zeroed that the agents j < i chose and i
    heard of -- all of them, or with adj (bool [B, n, n]) those with adj[:, i, j]; the lowest action with the largest score wins."""
    i64, dev = torch.int64, M.device
    B, n = int(X.shape[0]), int(X.shape[1])
    R2, centre = (16 * view_range) ** 2, cell_centres(side, dev)
    ct, st = trig_tables()
    offx = torch.tensor([(lookahead * 16 * v) >> 14 for v in ct], dtype=i64, device=dev)   # (Python's >> floors)
    offy = torch.tensor([(lookahead * 16 * v) >> 14 for v in st], dtype=i64, device=dev)
    zero = torch.zeros(B, side * side, dtype=i64, device=dev)
    actions = torch.empty(B, n, dtype=i64, device=dev)
    scores = torch.empty(B, n, 3, dtype=i64, device=dev)
    claims = []
    for i in range(n):
        W = M if M.dim() == 2 else M[:, i]
        for j in range(i):   # the claims agent i has heard
            W = torch.where(claims[j] if adj is None else claims[j] & adj[:, i, j].view(B, 1), zero, W)
        foot, score = [], []
        for turn in (0, 1, HEADINGS - 1):
            hp = (h[:, i] + turn) % HEADINGS
            px = torch.clamp(X[:, i] + offx[hp], 0, 16 * side)
            py = torch.clamp(Y[:, i] + offy[hp], 0, 16 * side)
            foot.append(disc_mask(centre, px, py, R2))
            score.append(torch.where(foot[-1], W, zero).sum(1))
        best = (score[1] > score[0]).to(i64)
        best = torch.where(score[2] > torch.maximum(score[0], score[1]), torch.full_like(best, 2), best)
        actions[:, i] = best
        scores[:, i] = torch.stack(score, 1)
        claims.append(torch.where((best == 0).view(B, 1), foot[0], torch.where((best == 1).view(B, 1), foot[1], foot[2])))
    return actions, scores


def coverage_actions_torch(state, grid, n_agents, side, view_range, keep, regrow=8, lookahead=None, return_scores=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grid int32 [B, side * side] (updated in place) -> actions
    int64 [B, n]; with return_scores also the scores each agent chose from, int64 [B, n, 3].  Stock torch ops on the tensors'
    device: the CPU, or a GPU for a comparison on the same device.  The quantisation relies on EAGER torch, where the multiply
    and the add of `xn * half + half` are two kernels and each rounds once; do not run this under torch.compile, which may
    contract them into one fused multiply-add."""
    n, side, view_range, keep, regrow = int(n_agents), int(side), int(view_range), int(keep), int(regrow)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check_params(n, side, view_range, keep, regrow, lookahead)
    _check_state_grid("coverage", state, grid, n, (side * side,))
    X, Y, h = quantise(state, n, side)
    G = grid.to(torch.int64).clamp(0, FRESH)   # a cell outside 0..65536 is read as the nearer bound
    G = G + ((FRESH - G) >> regrow)
    G = torch.where(swept(cell_centres(side, state.device), X, Y, (16 * view_range) ** 2), (G * keep) >> 16, G)
    grid.copy_(G.to(torch.int32))
    actions, scores = greedy_choose(G, X, Y, h, side, view_range, lookahead)
    return (actions, scores) if return_scores else actions


class GridAgents:
    """What CoverageAgents, BeliefAgents and LocalCoverageAgents share.  env_or_args: a BatchedFlightEnv or an args namespace
    (map_size, n_agents, view_range, detect_prob are read); batch / device default to the env's (device: "cuda" for a namespace);
    lookahead: how far ahead an agent looks, in cells (default view_range, at most map_size).  impl = "hip": the kernel of
    csrc/<KERNEL>, one launch per `choose_action` on the current stream, no synchronisation; "torch": the definition, on the same
    device.

    `policy()` is a `policy(obs, state, last, t)` callable for EpisodeCollector.generate_episodes(policy=...),
    collector.evaluate and collector.collect_experiment_data; it resets when t == 0."""
    KERNEL = None   # the header under csrc/ that holds the subclass's kernel
    NEEDS = None    # what to say when the op layer cannot be loaded (_lib.torch_ops_for)

    def __init__(self, env_or_args, batch, device, lookahead, impl):
        src, name = env_or_args, type(self).__name__
        if impl not in ("hip", "torch"):
            raise ValueError(f"impl must be 'hip' (the kernel of csrc/{self.KERNEL}) or 'torch' (the definition)")
        batch = getattr(src, "batch", None) if batch is None else batch
        if batch is None or int(batch) < 1:
            raise ValueError(f"{name}: batch must be given (>= 1) with an args namespace")
        self.batch = int(batch)
        self.device = torch.device(device if device is not None else getattr(src, "device", "cuda"))
        if impl == "hip" and self.device.type != "cuda":
            raise ValueError(f"{name}(impl='hip') runs a HIP kernel and {self.device} is not a GPU: there is no CPU "
                             "fallback (impl='torch' runs the definition anywhere)")
        self.impl = impl
        self.n_agents, self.side = int(src.n_agents), int(src.map_size)
        if int(src.view_range) != src.view_range:
            raise ValueError(f"{name}: view_range must be a whole number of cells, got {src.view_range!r}")
        self.view_range = int(src.view_range)
        self.keep = keep_of(src.detect_prob)
        self.lookahead = min(self.view_range, self.side) if lookahead is None else int(lookahead)

    def _launch(self, state):
        """For impl "hip": (the op layer, a fresh actions tensor int64 [B, n]) once `state` is a [batch, S] tensor."""
        if not torch.is_tensor(state) or state.dim() != 2 or int(state.shape[0]) != self.batch:
            raise ValueError(f"{type(self).__name__}: state must be a [{self.batch}, S] tensor")
        return _lib.torch_ops_for(self.NEEDS), torch.empty(self.batch, self.n_agents, dtype=torch.int64, device=self.device)

    def policy(self):
        def policy(obs, state, last, t):
            if t == 0:
                self.reset()
            return self.choose_action(state)
        return policy


class CoverageAgents(GridAgents):
    """The coverage baseline for a batch of envs: GridAgents' arguments, and regrow: the regrowth shift.  `.grid` is the belief
    grid, int32 [B, side * side]; `reset()` fills it."""
    KERNEL, NEEDS = "coverage.h", "the coverage kernel needs"

    def __init__(self, env_or_args, batch=None, device=None, lookahead=None, regrow=8, impl="hip"):
        super().__init__(env_or_args, batch, device, lookahead, impl)
        self.regrow = int(regrow)
        _check_params(self.n_agents, self.side, self.view_range, self.keep, self.regrow, self.lookahead)
        self.grid = torch.full((self.batch, self.side * self.side), FRESH, dtype=torch.int32, device=self.device)

    def reset(self):
        """A fresh belief grid: nobody has looked anywhere."""
        self.grid.fill_(FRESH)

    def choose_action(self, state):
        """get_state() rows float32 [B, S] -> actions int64 [B, n]; the grid moves on by one step."""
        if self.impl == "torch":
            return coverage_actions_torch(state, self.grid, self.n_agents, self.side, self.view_range, self.keep, self.regrow,
                                          self.lookahead)
        ops, actions = self._launch(state)
        ops.coverage_actions(state, self.grid, actions, self.n_agents, self.side, self.view_range, self.keep, self.regrow, self.lookahead)
        return actions
