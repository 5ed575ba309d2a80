"""Grid observations: sixteen floats per agent that summarise a search policy's grid, and a student that reads them
(include/coopsearch.h: cs_grid_features, cs_feature_episodes).

Section 23 distilled the training-free search policies into the agent network and found that a planner on a density grid cannot
be cloned from (x, y, cos, sin): the observation does not carry the grid.  This module gives the network a summary of it.  A
FILTER -- a `CoverageAgents` or a `BeliefAgents` -- keeps the grid; after its call on a state, sixteen probes per agent read it.

`grid_features_torch` is the DEFINITION, in stock eager torch ops on any device; the kernels (csrc/gridobs.h) reproduce it bit
for bit.  Everything is integer after the one float32 quantisation of baseline.quantise:

  X, Y, h   baseline.quantise(state, n, side): positions in sub-units of 1/16 cell, heading index 0..35.
  D         clamp(grid, 0, belief.CAP) as int64.  The grid is read and never written.
  probe k   k = 8 ring + b, ring 0..1, b 0..7: hp = (h + REL[b]) % 36, REL = (0, 1, 35, 4, 32, 9, 27, 18) in steps of pi / 18;
            d16 = DIST[ring] * 16 * lookahead, DIST = (1, 3); px = clamp(X + ((d16 * CT[hp]) >> 14), 0, 16 side), py likewise
            with ST (>> floors; (CT, ST) = baseline.trig_tables()).  Ring 0, b = 0..2 are the three look-ahead points the
            policies score: their sums are agent 0's scores.
  sum_k     the sum of D over the cells whose centre lies within R = 16 view_range of the probe:
            (16 ix + 8 - px)^2 + (16 iy + 8 - py)^2 <= R^2.  At most 2^12 * 2^19 = 2^31.
  f_k       float32(sum_k >> 8) * 2^-15: sum_k >> 8 <= 2^23 is exact in float32 and the scale is a power of two.  A fresh map
            under a view_range-7 disc about a cell centre (149 cells) reads 149 / 128 = 1.164.

No team-mate claims are modelled: every agent reads the same grid.

  grid_features_torch / grid_features        the definition / the kernel path of one decision.
  feature_episodes_torch / feature_episodes  the same for a recorded batch: imitate.label_episodes_torch's loop with the probes
                                             taken after every step; one cs_feature_episodes launch, labels optional.
  GridAgents                                 FusedAgents whose input rows are [16 features | obs | last | id]: a filter launch, a
                                             feature launch and a policy launch per decision.
  GridImitationLearner, FeatureRing          ImitationLearner and LabelledRing with batch["f"].
  distil_grid                                imitate.distil with the features recomputed from every recorded batch.
"""
import torch

from . import _lib
from . import baseline as bl
from . import belief as be
from . import imitate as im
from . import learner as ln
from .agents import AgentRNN, FusedAgents, rnn_input_shape
from .collector import EpisodeCollector

REL = (0, 1, 35, 4, 32, 9, 27, 18)   # probe bearings relative to the heading, in steps of pi / 18
DIST = (1, 3)                        # ring distances in look-aheads
PROBES = 16                          # per agent: NFEAT of csrc/policy.hip, the width cs_policy_forward takes in front of obs
SCALE = 2.0 ** -15


NEEDS = "the grid-observation kernels need"   # _lib.torch_ops_for's words


def _check(state, grid, n, side, view_range, lookahead):
    if not 1 <= n <= _lib.MAX_AGENTS or not 1 <= side <= bl.MAX_MAP or not 0 <= view_range <= bl.MAX_MAP or not 0 <= lookahead <= side:
        raise ValueError(f"gridobs: n_agents must be 1..{_lib.MAX_AGENTS}, side 1..{bl.MAX_MAP}, view_range 0..{bl.MAX_MAP} and lookahead 0..side")
    if not torch.is_tensor(state) or state.dim() != 2 or state.dtype != torch.float32 or state.shape[0] < 1 or state.shape[1] < 4 * n:
        raise ValueError(f"gridobs: state must be float32 [B, S] with B >= 1 and S >= 4 n_agents = {4 * n}")
    if not torch.is_tensor(grid) or grid.dtype != torch.int32 or tuple(grid.shape) != (state.shape[0], side * side) or grid.device != state.device:
        raise ValueError(f"gridobs: grid must be int32 [{state.shape[0]}, {side * side}] on the state's device")


# ---- one decision ----------------------------------------------------------------------------------------------------------------

def grid_features_torch(state, grid, n_agents, side, view_range, lookahead=None, return_sums=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grid int32 [B, side * side] (the grid a CoverageAgents or a
    BeliefAgents left after its call on the same state; neither tensor is written) -> features float32 [B, n, 16]; with
    return_sums also the sums, int64 [B, n, 16].  Stock EAGER torch ops on the tensors' device (baseline.coverage_actions_torch
    says why eager)."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check(state, grid, n, side, view_range, lookahead)
    i64, dev = torch.int64, state.device
    B, cells, R2 = int(state.shape[0]), side * side, (16 * view_range) ** 2
    X, Y, h = bl.quantise(state, n, side)
    D = grid.to(i64).clamp(0, be.CAP).view(B, 1, cells)
    ct, st = bl.trig_tables()
    centre = (16 * torch.arange(side, dtype=i64, device=dev) + 8).view(1, 1, side)
    zero = torch.zeros(1, 1, 1, dtype=i64, device=dev)
    sums = torch.empty(B, n, PROBES, dtype=i64, device=dev)
    for ring, dist in enumerate(DIST):
        d16 = dist * 16 * lookahead
        offx = torch.tensor([(d16 * v) >> 14 for v in ct], dtype=i64, device=dev)   # (Python's >> floors)
        offy = torch.tensor([(d16 * v) >> 14 for v in st], dtype=i64, device=dev)
        for b, rel in enumerate(REL):
            hp = (h + rel) % bl.HEADINGS
            px = torch.clamp(X + offx[hp], 0, 16 * side)
            py = torch.clamp(Y + offy[hp], 0, 16 * side)
            dx, dy = centre - px.view(B, n, 1), centre - py.view(B, n, 1)
            foot = ((dx * dx).view(B, n, side, 1) + (dy * dy).view(B, n, 1, side) <= R2).view(B, n, cells)
            sums[:, :, 8 * ring + b] = torch.where(foot, D, zero).sum(2)
    feat = (sums >> 8).to(torch.float32) * SCALE
    return (feat, sums) if return_sums else feat


def grid_features_hip(state, grid, n_agents, side, view_range, lookahead=None, out=None):
    """grid_features_torch on the kernel (csrc/gridobs.h): ONE launch on the current stream, no synchronisation.  out: a float32
    [B, n, 16] destination (default: a new tensor)."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check(state, grid, n, side, view_range, lookahead)
    if out is None:
        out = torch.empty(int(state.shape[0]), n, PROBES, dtype=torch.float32, device=state.device)
    _lib.torch_ops_for(NEEDS).grid_features(state, grid, out, n, side, view_range, lookahead)
    return out


def grid_features(state, grid, n_agents, side, view_range, lookahead=None, impl="auto"):
    """The sixteen features of every agent: float32 [B, n, 16].  impl "auto": the kernel when `state` is on a GPU, else the
    definition; "hip": the kernel or an error; "torch": the definition, on the tensors' device."""
    if impl not in ("auto", "hip", "torch"):
        raise ValueError("impl must be 'auto', 'hip' (one cs_grid_features launch) or 'torch' (the definition)")
    if impl == "hip" and not (torch.is_tensor(state) and state.is_cuda):
        raise ValueError("grid_features(impl='hip') needs tensors on a GPU: there is no CPU fallback (impl='torch' runs the definition anywhere)")
    if impl == "torch" or not (torch.is_tensor(state) and state.is_cuda):
        return grid_features_torch(state, grid, n_agents, side, view_range, lookahead)
    return grid_features_hip(state, grid, n_agents, side, view_range, lookahead)


# ---- a recorded batch ------------------------------------------------------------------------------------------------------------

def feature_episodes_torch(s, lens, expert_params):
    """The definition of cs_feature_episodes: imitate.label_episodes_torch's loop, with grid_features_torch applied to the grid as
    the step definition left it on row t.  s float32 [E, T, S >= 4n], lens int32 [E] with 0 <= lens[e] <= T, expert_params an
    `imitate.ExpertParams` (the FILTER's) -> (feat float32 [E, T, n, 16], labels int64 [E, T, n], grid_out int32 [E, side^2],
    prev_out int32 [E, 8, 2] or None for the coverage filter).  The rows t >= lens[e] get feature 0 and label 0 whatever they
    hold (NaN included: they are not read).  s and lens are not written."""
    p = expert_params
    if not isinstance(p, im.ExpertParams):
        raise TypeError("gridobs: expert_params must be an imitate.ExpertParams")
    im._check_episodes(s, lens, p.n_agents)
    E, T = int(s.shape[0]), int(s.shape[1])
    if bool(((lens < 0) | (lens > T)).any()):
        raise ValueError(f"gridobs: lens must lie in 0..T = {T}")
    dev = s.device
    grid = torch.full((E, p.side * p.side), bl.FRESH, dtype=torch.int32, device=dev)
    prev = torch.zeros(E, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=dev)
    labels = torch.zeros(E, T, p.n_agents, dtype=torch.int64, device=dev)
    feat = torch.zeros(E, T, p.n_agents, PROBES, dtype=torch.float32, device=dev)
    for t in range(T):
        live = lens > t
        rows = torch.where(live.view(E, 1), s[:, t], torch.zeros_like(s[:, t]))   # a row past the end is never read
        g, pv = grid.clone(), prev.clone()
        if p.expert == im.COVERAGE:
            a = bl.coverage_actions_torch(rows, g, p.n_agents, p.side, p.view_range, p.keep, p.regrow, p.lookahead)
        else:
            a = be.belief_actions_torch(rows, g, pv, p.n_agents, p.side, p.view_range, p.keep, p.model, p.moved(t), p.lookahead)
        f = grid_features_torch(rows, g, p.n_agents, p.side, p.view_range, p.lookahead)
        grid = torch.where(live.view(E, 1), g, grid)
        prev = torch.where(live.view(E, 1, 1), pv, prev)
        labels[:, t] = torch.where(live.view(E, 1), a, torch.zeros_like(a))
        feat[:, t] = torch.where(live.view(E, 1, 1), f, torch.zeros_like(f))
    return feat, labels, grid, (prev if p.expert == im.BELIEF else None)


def feature_episodes_hip(s, lens, expert_params, labels=True, grid_out=True, prev_out=True):
    """feature_episodes_torch on the kernel (csrc/gridobs.h): ONE launch on the current stream, no synchronisation.  labels /
    grid_out / prev_out False: that output is not written (None in its place); without labels the kernel skips the choose step.
    lens is read clamped to 0..T."""
    p = expert_params
    if not isinstance(p, im.ExpertParams):
        raise TypeError("gridobs: expert_params must be an imitate.ExpertParams")
    im._check_episodes(s, lens, p.n_agents)
    E, T, dev = int(s.shape[0]), int(s.shape[1]), s.device
    feat = torch.empty(E, T, p.n_agents, PROBES, dtype=torch.float32, device=dev)
    lab = torch.empty(E, T, p.n_agents, dtype=torch.int64, device=dev) if labels else None
    grid = torch.empty(E, p.side * p.side, dtype=torch.int32, device=dev) if grid_out else None
    prev = torch.empty(E, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=dev) if (prev_out and p.expert == im.BELIEF) else None
    ops = _lib.torch_ops_for(NEEDS)
    ops.feature_episodes(s, lens, feat, lab, grid, prev, p.expert, p.n_agents, p.side, p.view_range, p.keep, p.regrow, p.lookahead,
                         p.model.mode, p.model.sense16, p.every, p.moving, list(p.model.dx), list(p.model.dy))
    return feat, lab, grid, prev


def feature_episodes(filter, batch, labels=False, impl="auto"):
    """The features of every step of an episode dict, as `filter` (a CoverageAgents or a BeliefAgents, exactly those classes)
    would have produced them flying along: float32 [E, T, n, 16], 0 on the rows behind an episode's end; with labels=True
    (features, labels int64 [E, T, n]): what the filter would have done, from the same launch.  impl "auto": one
    cs_feature_episodes launch when batch["s"] is on a GPU, else the definition; "hip": that launch or an error; "torch": the
    definition.  The filter's own grid is neither read nor written."""
    if impl not in ("auto", "hip", "torch"):
        raise ValueError("impl must be 'auto', 'hip' (one cs_feature_episodes launch) or 'torch' (the definition)")
    p = im.expert_params(filter)
    s = batch["s"]
    if not torch.is_tensor(s) or s.dim() != 3:
        raise ValueError("gridobs: batch['s'] must be a [E, T, S] tensor")
    s = s.to(torch.float32).contiguous()
    lens = im.episode_lens(batch)
    if impl == "hip" and not s.is_cuda:
        raise ValueError("feature_episodes(impl='hip') needs an episode dict on a GPU: there is no CPU fallback (impl='torch' runs the "
                         "definition anywhere)")
    if impl != "torch" and s.is_cuda:
        feat, lab, _, _ = feature_episodes_hip(s, lens, p, labels=labels, grid_out=False, prev_out=False)
    else:
        feat, lab, _, _ = feature_episodes_torch(s, lens, p)
    return (feat, lab) if labels else feat


# ---- acting ------------------------------------------------------------------------------------------------------------------------

class GridAgents(FusedAgents):
    """FusedAgents that observe a filter's grid.  env_or_args: a BatchedFlightEnv / MovingTargetEnv or an args namespace after
    apply_env_info (flight_easy only: with a conv front end the 16 conv features and the 16 grid features together exceed the 32
    input columns of cs_policy_forward); filter: the `CoverageAgents` or `BeliefAgents` whose grid is read -- `choose_action`
    advances it; batch defaults to the filter's; net defaults to AgentRNN(rnn_input_shape(args) + 16, args).  The network's input
    row is the kernel's: [16 features | obs(4) | one-hot(last action) | one-hot(agent id)].

    One decision is three launches on the current stream, no synchronisation: filter.choose_action (its action is discarded),
    cs_grid_features, cs_policy_forward with the features in front of the obs columns.  load_weights, sync_weights, init_hidden,
    the selection rule and state_dict are FusedAgents'."""

    def __init__(self, env_or_args, filter, batch=None, net=None, seed=0, env_offset=0):
        args = getattr(env_or_args, "args", env_or_args)
        if getattr(args, "conv", False):
            raise ValueError("GridAgents serves flight_easy only: a conv front end's 16 features and the 16 grid features exceed the 32 "
                             "input columns of cs_policy_forward")
        if type(filter) not in (bl.CoverageAgents, be.BeliefAgents):
            raise TypeError("GridAgents: filter must be a CoverageAgents or a BeliefAgents")
        batch = filter.batch if batch is None else int(batch)
        if batch != filter.batch or int(args.n_agents) != filter.n_agents:
            raise ValueError(f"GridAgents: the filter serves {filter.batch} envs of {filter.n_agents} agents, not {batch} of {args.n_agents}")
        if net is None:
            net = AgentRNN(rnn_input_shape(args) + PROBES, args)
        if net.fc1.in_features != rnn_input_shape(args) + PROBES:
            raise ValueError(f"GridAgents: net.fc1 must take {rnn_input_shape(args) + PROBES} inputs (16 features in front of the plain row)")
        self.filter = filter
        super().__init__(args, batch, device=filter.device, net=net, seed=seed, env_offset=env_offset)
        self.features = torch.zeros(self.batch, self.n_agents, PROBES, device=self.device)

    def observe(self, state, moved=False):
        """Advance the filter on `state` (float32 [B, S]) and read its grid: -> self.features, float32 [B, n, 16] (overwritten by
        the next call).  moved: did the targets move in the step that led here?  (A CoverageAgents ignores it.)"""
        f = self.filter
        if not state.is_contiguous():
            state = state.contiguous()
        if type(f) is be.BeliefAgents:
            f.choose_action(state, moved)
        else:
            f.choose_action(state)
        if f.impl == "torch":
            self.features.copy_(grid_features_torch(state, f.grid, f.n_agents, f.side, f.view_range, f.lookahead))
        else:
            grid_features_hip(state, f.grid, f.n_agents, f.side, f.view_range, f.lookahead, out=self.features)
        return self.features

    def choose_action(self, obs, state, moved=False, epsilon=0.0, evaluate=False, want_q=False, last=None, out=None, eps_env=None):
        """obs float32 [B, n, 4] and state float32 [B, S] of the same step -> the int64 [B, n] action buffer; the other arguments
        are FusedAgents.choose_action's."""
        if obs.dtype != torch.float32 or obs.shape[-1] != 4 or obs.numel() != self.rows * 4:
            raise ValueError("obs must be float32 [B, n, 4]")
        if not obs.is_contiguous():
            obs = obs.contiguous()
        last = self.actions if last is None else last
        out = self.actions if out is None else out
        for t in (last, out):
            if t.dtype != torch.int64 or t.numel() != self.rows or not t.is_contiguous():
                raise ValueError("last / out must be contiguous int64 [B, n]")
        eps, sel = self.selection(epsilon, evaluate)
        if evaluate and not self.softmax:
            eps_env = None
        if eps_env is not None and (eps_env.dtype != torch.float64 or eps_env.numel() != self.batch or not eps_env.is_contiguous()):
            raise ValueError("eps_env must be a contiguous float64 [B] tensor")
        self.observe(state, moved)
        self._ops.policy_forward(self.packed, obs, 4, 0, last, self.features, 1, self.hidden, self.q if want_q else None, out,
                                 self.rows, self.n_agents, self.n_actions, eps, eps_env, self.seed, self.calls, self.row0, sel)
        self.calls += 1
        return out

    def forward_raw(self, x, want_q=True):
        raise NotImplementedError("GridAgents has no raw rows: its features come from the filter (choose_action)")

    def policy(self, epsilon=0.0, evaluate=True, trace=None):
        """A `policy(obs, state, last, t)` callable for EpisodeCollector.generate_episodes(policy=...) and collector.evaluate.  It
        resets the filter and the hidden state at t == 0 and tells the filter whether the targets moved, by BeliefAgents.policy's
        rule.  trace: a float32 [T, B, n, 16] tensor that receives the features of every step."""
        motion = getattr(self.filter, "motion", None)
        speed, every = (motion.speed, motion.every) if motion is not None else (0.0, 1)

        def fn(obs, state, last_onehot, t):
            if t == 0:
                self.filter.reset()
                self.init_hidden()
            out = self.choose_action(obs, state, t > 0 and speed > 0 and (t - 1) % every == 0, epsilon, evaluate)
            if trace is not None:
                trace[t].copy_(self.features)
            return out
        return fn


# ---- learning ----------------------------------------------------------------------------------------------------------------------

class GridImitationLearner(im.ImitationLearner):
    """ImitationLearner whose actor reads 16 grid features in front of the plain input row: AgentRNN(rnn_input_shape(args) + 16,
    args), what GridAgents flies.  `learn` needs one more key, batch["f"] (float [E, T, n, 16]: `feature_episodes`).  flight_easy
    only.  The checkpoint directory is named "bc_grid"; Runner(load_model=True) cannot load its files: the first layer is 16
    columns wider than the actor Runner builds."""

    def __init__(self, args, device="cuda", unroll="fused", conv_impl="torch"):
        if getattr(args, "conv", False):
            raise ValueError("GridImitationLearner serves flight_easy only (GridAgents says why)")
        super().__init__(args, device, unroll, conv_impl)
        torch.manual_seed(args.seed)   # the parent built the plain actor; the wider one replaces it, again a function of the seed alone
        self.eval_rnn = AgentRNN(rnn_input_shape(args) + PROBES, args).to(self.device)
        self.eval_rnn.conv_impl = self.conv_impl
        self.model_dir = self._dir("bc_grid")
        self.rnn_parameters = list(self.eval_rnn.parameters())
        self.rnn_optimizer = ln._make_optimizer(args, self.rnn_parameters, args.lr_actor)

    def learn(self, batch, max_episode_len=None, train_step=0, epsilon=0.0):
        """ImitationLearner.learn on rows [f | obs | last | id]: actor_inputs' X with batch["f"] in front, through unroll_q (fused
        or torch).  Returns the loss as a device tensor (no host synchronisation)."""
        for key in ("u_expert", "f"):
            if key not in batch:
                raise KeyError(f"GridImitationLearner.learn: the batch carries no '{key}' "
                               + ("(feature_episodes)" if key == "f" else "(label_episodes, or the actions an expert flew)"))
        labels = torch.as_tensor(batch["u_expert"], device=self.device)
        rest = {k: v for k, v in batch.items() if k != "u_expert"}
        rest, T, u, mask1 = ln._prepare(rest, self.device, max_episode_len, self.n_agents, self.n_actions, self.eval_rnn.fc1.weight.dtype)
        E, n = int(u.shape[0]), self.n_agents
        labels = labels.reshape(labels.shape[0], labels.shape[1], n)[:, :T].long().contiguous()
        f = rest["f"].reshape(E, -1, n, PROBES)[:, :T]
        X = ln.actor_inputs(self.args, n, rest, T)[0]
        X = torch.cat([f.transpose(0, 1).reshape(T, E * n, PROBES), X], 2)
        logits = ln.unroll_q(self.eval_rnn, X, None, self.unroll).view(T, E, n, -1).transpose(0, 1)
        mask = mask1.reshape(E, T)
        if self.unroll == "fused":
            loss, stats = im.BCLoss.apply(logits, rest["avail_u"], labels, mask, 1 / (n * mask.sum()))
        else:
            loss, stats = im.bc_loss_torch(logits, rest["avail_u"], labels, mask)
        self.rnn_optimizer.zero_grad()
        loss.backward()
        self.rnn_optimizer.step()
        self.last_stats = stats
        return loss.detach()

    def save_model(self, num, alg="bc_grid"):
        """<model_dir(args, alg)>/<num>_rnn_net_params.pkl; returns the path.  (Not an actor Runner can load: see the class.)"""
        return super().save_model(num, alg)


class FeatureRing(im.LabelledRing):
    """LabelledRing with one more key, "f" [size, T, n, 16]: the grid features of every stored step."""
    keys = im.LabelledRing.keys + ("f",)

    def __init__(self, args, buffer_size, device="cuda", dtype=torch.float32):
        super().__init__(args, buffer_size, device, dtype)
        self.buffers["f"] = torch.empty(self.size, self.episode_limit, self.n_agents, PROBES, dtype=dtype, device=self.device)


def distil_grid(env, expert, filter, learner, agents, ring, iterations, updates, sample, generator=None, impl="auto"):
    """imitate.distil for a student that reads the grid.  expert: whose actions are cloned; filter: the CoverageAgents or
    BeliefAgents whose grid the student observes (`agents.filter`, usually; it may be the expert itself); learner a
    GridImitationLearner, agents a GridAgents, ring a FeatureRing.  Iteration 0 is flown by expert.policy(), iterations >= 1 by
    agents.policy() greedily (three launches and an env step per step: the one-launch closed loop has no filter).  Every recorded
    batch gets its "f" from ONE feature_episodes launch; its labels come from the same launch when the expert is of the filter's
    own class (with the filter's parameters: the same decisions), from the actions flown in iteration 0 otherwise, and from
    label_episodes(expert, episode, impl) after that.  Then distil's steps: ring.store_episode, `updates` learn calls on
    ring.sample(sample, generator), the student's weights to `agents`.  Returns distil's history."""
    if iterations < 1 or updates < 0 or sample < 1:
        raise ValueError("distil_grid: iterations >= 1, updates >= 0 and sample >= 1")
    collector = EpisodeCollector(env)
    own = type(expert) is type(filter) and im.expert_params(expert) == im.expert_params(filter)
    feature_impl = "hip" if impl == "hip" else "auto"   # (impl is label_episodes': "rows" concerns the labels alone)
    history = []
    for it in range(int(iterations)):
        flown = expert.policy() if it == 0 else agents.policy()
        episode, _, _, found = collector.generate_episodes(policy=flown, init=False)
        if own:
            episode["f"], labels = feature_episodes(filter, episode, labels=True, impl=feature_impl)
        else:
            episode["f"] = feature_episodes(filter, episode, impl=feature_impl)
            labels = None if it == 0 else im.label_episodes(expert, episode, impl)
        episode["u_expert"] = episode["u"].clone() if labels is None else labels.unsqueeze(3).to(episode["u"].dtype)
        ring.store_episode(episode)
        loss = None
        for _ in range(int(updates)):
            loss = learner.learn(ring.sample(int(sample), generator))
        if agents.net is not learner.eval_rnn:
            agents.net.load_state_dict(learner.eval_rnn.state_dict())
        agents.sync_weights()
        stats = learner.last_stats if loss is not None else None
        history.append({"iteration": it, "flown_by": "expert" if it == 0 else "student",
                        "loss": None if stats is None else float(stats[0]), "agreement": None if stats is None else float(stats[1]),
                        "targets_find": float(found.to(torch.float64).mean())})
    return history
