"""Imitation learning: distil the training-free search policies into the agent network (include/coopsearch.h:
cs_label_episodes, cs_bc_loss).

`CoverageAgents`, `BeliefAgents`, `PlanAgents` and `ForecastAgents` search best in every regime of DESIGN.md sections 17 to 22,
but each decision is one to three launches and none of them runs inside the one-launch closed loop.  The agent network does.
This module teaches the network to fly like one of those policies -- the EXPERT -- by behaviour cloning followed by DAgger:
the student flies, the expert says what it would have done in every state the student reached, the student learns from
those labels.  The checkpoint is the actor file `ReinforceLearner` and `PPOLearner` load.

The student's fast path is one launch per episode batch, so there is no per-step hook for an expert to shadow: the expert
labels the recorded batch afterwards.  Every expert here decides from (state row, t) and its own grid alone -- their
`policy()` callables ignore `obs` and `last` -- so relabelling the recorded s[E, T, S] row by row gives exactly what
shadowing would have given.

  label_episodes_torch   the DEFINITION of the one-launch labeller: a loop over baseline.coverage_actions_torch or
                         belief.belief_actions_torch, which it does not restate.
  label_episodes         the labels of any expert for an episode dict: one cs_label_episodes launch for a CoverageAgents or a
                         BeliefAgents on a GPU (the expert's grid stays in LDS for the whole episode), T policy() calls otherwise.
  bc_loss_torch          the DEFINITION of cs_bc_loss: the masked cross-entropy over learner.action_prob, with its statistics.
  BCLoss                 the same on the kernel: loss, statistics and dloss/dlogits in one pass.
  ImitationLearner       ReinforceLearner's actor trained on batch["u_expert"].
  LabelledRing           DAgger's aggregate: an episode ring over replay.KEYS + ("u_expert",).
  distil                 the loop: iteration 0 clones the expert's own flights, iterations >= 1 relabel the student's.
"""
import dataclasses
import os

import torch

from . import _lib
from . import baseline as bl
from . import belief as be
from . import learner as ln
from . import replay as rp
from .agents import AgentRNN, rnn_input_shape
from .collector import EpisodeCollector

COVERAGE, BELIEF = 0, 1   # cs_label_params.expert


NEEDS = "the imitation kernels need"   # _lib.torch_ops_for's words


# ---- the labeller --------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class ExpertParams:
    """cs_label_params as host integers.  expert: COVERAGE (baseline.coverage_actions_torch per row) or BELIEF
    (belief.belief_actions_torch per row, with `model`, and moved = moving and t > 0 and (t - 1) % every == 0); the other fields
    are those of the two definitions.  regrow is the coverage expert's (checked, then unused, for belief); model, every and
    moving are the belief expert's."""
    expert: int
    n_agents: int
    side: int
    view_range: int
    keep: int
    regrow: int = 8
    lookahead: int = None
    model: be.BeliefModel = be.BeliefModel()
    every: int = 1
    moving: int = 0

    def __post_init__(self):
        if self.lookahead is None:
            object.__setattr__(self, "lookahead", min(int(self.view_range), int(self.side)))
        for k in ("expert", "n_agents", "side", "view_range", "keep", "regrow", "lookahead", "every", "moving"):
            object.__setattr__(self, k, int(getattr(self, k)))
        if self.expert not in (COVERAGE, BELIEF):
            raise ValueError("imitate: expert must be 0 (coverage) or 1 (belief)")
        if not isinstance(self.model, be.BeliefModel):
            raise TypeError("imitate: model must be a BeliefModel")
        bl._check_params(self.n_agents, self.side, self.view_range, self.keep, self.regrow, self.lookahead)
        if self.every < 1 or self.moving not in (0, 1):
            raise ValueError("imitate: every must be >= 1 and moving 0 or 1")

    def moved(self, t):
        """Did the targets move in the step that led to row t?  The rule BeliefAgents.policy encodes."""
        return 1 if (self.expert == BELIEF and self.moving and t > 0 and (t - 1) % self.every == 0) else 0


def expert_params(expert):
    """The `ExpertParams` of a CoverageAgents or a BeliefAgents (exactly those classes: a subclass may decide differently)."""
    if type(expert) is bl.CoverageAgents:
        return ExpertParams(COVERAGE, expert.n_agents, expert.side, expert.view_range, expert.keep, expert.regrow, expert.lookahead)
    if type(expert) is be.BeliefAgents:
        return ExpertParams(BELIEF, expert.n_agents, expert.side, expert.view_range, expert.keep, 8, expert.lookahead, expert.model,
                            expert.motion.every, 1 if expert.motion.speed > 0 else 0)
    raise TypeError(f"imitate: {type(expert).__name__} has no one-launch labeller (CoverageAgents and BeliefAgents have)")


def _check_episodes(s, lens, n):
    if not torch.is_tensor(s) or s.dim() != 3 or s.dtype != torch.float32 or s.shape[0] < 1 or s.shape[1] < 1 or s.shape[2] < 4 * n:
        raise ValueError(f"imitate: s must be float32 [E, T, S] with E >= 1, T >= 1 and S >= 4 n_agents = {4 * n}")
    if not torch.is_tensor(lens) or lens.dtype != torch.int32 or tuple(lens.shape) != (s.shape[0],) or lens.device != s.device:
        raise ValueError(f"imitate: lens must be int32 [{s.shape[0]}] on s's device")


def label_episodes_torch(s, lens, expert_params):
    """The definition of cs_label_episodes.  s float32 [E, T, S >= 4n] (the `s` of an episode dict), lens int32 [E] with 0 <=
    lens[e] <= T (the live rows, `episode_lens`), expert_params an `ExpertParams` -> (labels int64 [E, T, n], grid_out int32
    [E, side^2], prev_out int32 [E, 8, 2] or None for the coverage expert).  From a fresh grid (FRESH everywhere, prev zero),
    for t = 0..T-1, the expert's step definition is applied to row t of every episode; an episode with t >= lens[e] keeps
    its grid and prev as they were and its label is 0, whatever its row holds (NaN included: it is not read).  s and lens
    are not written.  Stock eager torch ops on s's device."""
    p = expert_params
    if not isinstance(p, ExpertParams):
        raise TypeError("imitate: expert_params must be an ExpertParams")
    _check_episodes(s, lens, p.n_agents)
    E, T = int(s.shape[0]), int(s.shape[1])
    if bool(((lens < 0) | (lens > T)).any()):
        raise ValueError(f"imitate: lens must lie in 0..T = {T}")
    dev = s.device
    grid = torch.full((E, p.side * p.side), bl.FRESH, dtype=torch.int32, device=dev)
    prev = torch.zeros(E, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=dev)
    labels = torch.zeros(E, T, p.n_agents, dtype=torch.int64, device=dev)
    for t in range(T):
        live = lens > t
        rows = torch.where(live.view(E, 1), s[:, t], torch.zeros_like(s[:, t]))   # a row past the end is never read
        g, pv = grid.clone(), prev.clone()
        if p.expert == COVERAGE:
            a = bl.coverage_actions_torch(rows, g, p.n_agents, p.side, p.view_range, p.keep, p.regrow, p.lookahead)
        else:
            a = be.belief_actions_torch(rows, g, pv, p.n_agents, p.side, p.view_range, p.keep, p.model, p.moved(t), p.lookahead)
        grid = torch.where(live.view(E, 1), g, grid)
        prev = torch.where(live.view(E, 1, 1), pv, prev)
        labels[:, t] = torch.where(live.view(E, 1), a, torch.zeros_like(a))
    return labels, grid, (prev if p.expert == BELIEF else None)


def label_episodes_hip(s, lens, expert_params, grid_out=True, prev_out=True):
    """label_episodes_torch on the kernel (csrc/label.h): ONE launch on the current stream, no synchronisation.  grid_out /
    prev_out False: that output is not written (None is returned in its place).  lens is read clamped to 0..T."""
    p = expert_params
    if not isinstance(p, ExpertParams):
        raise TypeError("imitate: expert_params must be an ExpertParams")
    _check_episodes(s, lens, p.n_agents)
    E, T = int(s.shape[0]), int(s.shape[1])
    labels = torch.empty(E, T, p.n_agents, dtype=torch.int64, device=s.device)
    grid = torch.empty(E, p.side * p.side, dtype=torch.int32, device=s.device) if grid_out else None
    prev = torch.empty(E, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=s.device) if (prev_out and p.expert == BELIEF) else None
    ops = _lib.torch_ops_for(NEEDS)
    ops.label_episodes(s, lens, labels, grid, prev, p.expert, p.n_agents, p.side, p.view_range, p.keep, p.regrow, p.lookahead,
                       p.model.mode, p.model.sense16, p.every, p.moving, list(p.model.dx), list(p.model.dy))
    return labels, grid, prev


def episode_lens(batch):
    """int32 [E]: the live rows of every episode of an episode dict, (1 - padded).sum(1)."""
    padded = batch["padded"]
    return (1 - padded.reshape(padded.shape[0], -1)).sum(1).to(torch.int32)


def _label_rows(expert, s, lens, return_state):
    """The generic path: the expert's own policy() on row t of every episode, t = 0..T-1."""
    E, T = int(s.shape[0]), int(s.shape[1])
    policy = expert.policy()
    holder = getattr(expert, "base", expert)   # a planner flies on its base policy's grid
    state = [x for x in (getattr(holder, "grid", None), getattr(holder, "prev", None)) if torch.is_tensor(x) and x.shape[0] == E]
    full = not state or bool((lens >= T).all())   # (one host synchronisation per call, none per row)
    labels = torch.zeros(E, T, int(expert.n_agents), dtype=torch.int64, device=s.device)
    for t in range(T):
        live = lens > t
        before = None if full else [x.clone() for x in state]
        a = torch.as_tensor(policy(None, s[:, t].contiguous(), None, t), device=s.device).to(torch.int64)
        labels[:, t] = torch.where(live.view(E, 1), a, torch.zeros_like(a))
        if before is not None:   # an episode that has ended keeps its grid and its positions
            for x, old in zip(state, before):
                x.copy_(torch.where(live.view(E, *([1] * (x.dim() - 1))), x, old))
    out = (labels, *(x.clone() for x in state)) if return_state else labels
    if hasattr(expert, "reset"):
        expert.reset()
    return out


def label_episodes(expert, batch, impl="auto", return_state=False):
    """What `expert` would have done in every state of an episode dict: labels int64 [E, T, n], 0 on the rows behind an
    episode's end.  impl "auto": one cs_label_episodes launch for a CoverageAgents or a BeliefAgents when batch["s"] is on a
    GPU, else the generic path; "hip": that launch or an error; "rows": the generic path, T calls of expert.policy()(None,
    s[:, t], None, t) -- it serves any object with policy() and n_agents (PlanAgents, ForecastAgents) whose batch is E.
    return_state: also the expert's grid (and stored positions, where it keeps any) after each episode's last live row.

    The expert's own state: the one-launch path neither reads nor writes it (the kernel starts from a fresh grid of its own);
    the generic path flies on it and ends with expert.reset(), so either way the expert is left as a fresh episode would
    find it -- and its policy() resets at t == 0 regardless."""
    if impl not in ("auto", "hip", "rows"):
        raise ValueError("impl must be 'auto', 'hip' (one cs_label_episodes launch) or 'rows' (T policy() calls)")
    s = batch["s"]
    if not torch.is_tensor(s) or s.dim() != 3:
        raise ValueError("imitate: batch['s'] must be a [E, T, S] tensor")
    s = s.to(torch.float32).contiguous()
    lens = episode_lens(batch)
    fusable = type(expert) in (bl.CoverageAgents, be.BeliefAgents)
    if impl == "hip" and not (fusable and s.is_cuda):
        raise ValueError("label_episodes(impl='hip') needs a CoverageAgents or a BeliefAgents and an episode dict on a GPU: there is no "
                         "CPU fallback (impl='rows' runs any expert anywhere)")
    if impl != "rows" and fusable and s.is_cuda:
        labels, grid, prev = label_episodes_hip(s, lens, expert_params(expert), grid_out=return_state, prev_out=return_state)
        return (labels, *(x for x in (grid, prev) if x is not None)) if return_state else labels
    if not hasattr(expert, "policy") or not hasattr(expert, "n_agents"):
        raise TypeError("imitate: an expert needs policy() and n_agents")
    return _label_rows(expert, s, lens, return_state)


# ---- the loss ------------------------------------------------------------------------------------------------------------------

def _check_loss_inputs(logits, avail_u, labels, mask):
    if logits.dim() != 4 or not 2 <= logits.shape[3] <= 8:
        raise ValueError("imitate: logits must be [E, T, n, A] with 2 to 8 actions")
    E, T, n, A = logits.shape
    if tuple(avail_u.shape) != (E, T, n, A):
        raise ValueError(f"imitate: avail_u must be [{E}, {T}, {n}, {A}]")
    if labels.dtype != torch.int64 or labels.numel() != E * T * n:
        raise ValueError(f"imitate: labels must be int64 [{E}, {T}, {n}]")
    if mask.numel() != E * T:
        raise ValueError(f"imitate: mask must be [{E}, {T}]")


def bc_loss_torch(logits, avail_u, labels, mask):
    """The definition of cs_bc_loss, in plain autograd over learner.action_prob: logits, avail_u [E, T, n, A], labels int64 [E,
    T, n] (or [E, T, n, 1]), mask [E, T] (or [E, T, 1]) -> (loss, stats [3]).  p = action_prob(logits, avail_u, 0.0); loss =
    -sum(mask log p[label]) / (n sum(mask)); stats = (the loss, the agreement = mean [argmax_a p_a == label] with the lowest
    index on ties, the mean entropy), means over the n sum(mask) live rows, detached.  A live row whose label is unavailable
    (or outside 0..A-1) adds no loss and no gradient and counts as a miss; a row with mask == 0 adds nothing."""
    _check_loss_inputs(logits, avail_u, labels, mask)
    E, T, n, A = logits.shape
    m = (mask.reshape(E, T, 1) != 0).expand(E, T, n)
    u = labels.reshape(E, T, n)
    inside = (u >= 0) & (u < A)
    idx = u.clamp(0, A - 1).unsqueeze(3)
    prob = ln.action_prob(logits, avail_u, 0.0)
    ok = m & inside & (torch.gather(avail_u, 3, idx).squeeze(3) != 0)
    pu = torch.gather(prob, 3, idx).squeeze(3)
    w = mask.reshape(E, T, 1).expand(E, T, n).to(logits.dtype)
    inv_count = 1 / (n * mask.sum())
    loss = -(torch.log(pu.masked_fill(~ok, 1.0)) * w).sum() * inv_count
    live = prob.masked_fill(~m.unsqueeze(3), 0.0)   # (a padded row has no available action: its probabilities are NaN)
    entropy = -(live * torch.log(live.masked_fill(live <= 0, 1.0))).sum(-1)
    hit = (ok & (live.argmax(-1) == u)).to(logits.dtype)   # torch's argmax takes the first of equal values
    stats = torch.stack([loss, (hit * w).sum() * inv_count, (entropy * w).sum() * inv_count])
    return loss, stats.detach()


BC_BLOCK = 256   # CS_PPO_BLOCK of include/coopsearch.h: rows per partial of cs_bc_loss's scratch buffer


class BCLoss(torch.autograd.Function):
    """bc_loss_torch on cs_bc_loss (csrc/bc_loss.h): (logits, avail_u, labels, mask, inv_count) -> (loss, stats [3]); inv_count:
    the device scalar 1 / (n * sum(mask)).  One pass over the rows computes the loss's sums and dloss/dlogits; backward is
    grad_out * dlogits.  stats carry no gradient."""

    @staticmethod
    def forward(ctx, logits, avail_u, labels, mask, inv_count):
        _check_loss_inputs(logits, avail_u, labels, mask)
        E, T, n, A = (int(x) for x in logits.shape)
        rows = E * T * n
        f32 = lambda x, *shape: x.detach().float().reshape(*shape).contiguous()
        z = f32(logits, rows, A)
        dlogits, stats = torch.empty_like(z), z.new_empty(3)
        scratch = z.new_empty(3 * ((rows + BC_BLOCK - 1) // BC_BLOCK))
        ops = _lib.torch_ops_for(NEEDS)
        ops.bc_loss(z, f32(avail_u, rows, A), labels.detach().reshape(rows).contiguous(), f32(mask, E * T), rows, n, A,
                    f32(inv_count, 1), dlogits, stats, scratch)
        ctx.save_for_backward(dlogits.view(logits.shape))
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        (dlogits,) = ctx.saved_tensors
        return (grad_loss * dlogits,) + (None,) * 4


# ---- the learner ---------------------------------------------------------------------------------------------------------------

def get_bc_args(args, seed=None):
    """The learner fields of ImitationLearner on an argparse-style namespace, shaped like get_reinforce_args (the same actor);
    seed as get_dop_args.  Supervised: no exploration, a larger step than the policy-gradient learners take."""
    args.off_policy = False
    args.rnn_hidden_dim, args.critic_dim = 64, 128
    args.lr_actor, args.lr_critic = 1e-3, 1e-3
    args.gamma, args.optimizer = getattr(args, "gamma", 0.99), getattr(args, "optimizer", "Adam")
    args.epsilon, args.anneal_epsilon, args.min_epsilon, args.epsilon_anneal_scale = 0.0, 0.0, 0.0, "epoch"
    args.batch_size, args.buffer_size = 32, 1000
    args.n_epoch, args.n_episodes, args.evaluate_cycle, args.save_cycle = 100000, 1, 200, 500
    args.grad_norm_clip = 10
    if seed is not None:
        args.seed = seed
    return args


class ImitationLearner:
    """Behaviour cloning of an expert's labels into ReinforceLearner's actor: the same network, the same initial parameters
    for the same seed, the same checkpoint file.  args: a namespace after get_bc_args (seed, lr_actor, optimizer,
    rnn_hidden_dim) and the env fields.  `learn` takes an episode dict with one more key, "u_expert" (int [E, T, n] or [E, T,
    n, 1]: `label_episodes`, or the actions an expert flew).  unroll: "fused" (GRUSequence and BCLoss, on a GPU) or "torch"
    (the reference's step loop and bc_loss_torch, on any device).  conv_impl: as QMixLearner's."""

    def __init__(self, args, device="cuda", unroll="fused", conv_impl="torch"):
        if unroll not in ("fused", "torch"):
            raise ValueError("unroll must be 'fused' or 'torch'")
        self.conv_impl = ln.check_conv_impl(args, device, unroll, conv_impl)
        self.args, self.device, self.unroll = args, torch.device(device), unroll
        if unroll == "fused" and self.device.type != "cuda":
            raise ValueError(f"ImitationLearner(unroll='fused') runs HIP kernels and {self.device} is not a GPU: there is no CPU "
                             "fallback (unroll='torch' runs anywhere)")
        self.n_actions, self.n_agents = args.n_actions, args.n_agents
        self.state_shape, self.obs_shape = args.state_shape, args.obs_shape
        torch.manual_seed(args.seed)   # as ReinforceLearner: the same seed gives the same actor
        self.eval_rnn = AgentRNN(rnn_input_shape(args), args).to(self.device)
        self.eval_rnn.conv_impl = self.conv_impl   # read by map_features / unroll_q
        self.model_dir = self._dir("bc")
        self.rnn_parameters = list(self.eval_rnn.parameters())
        self.rnn_optimizer = ln._make_optimizer(args, self.rnn_parameters, args.lr_actor)
        self.last_stats = None   # device tensor [3] of the last learn call: loss, agreement, mean entropy

    def _dir(self, alg):
        """learner.model_dir named after `alg` whatever args.alg says (args.alg selects the acting rule of FusedAgents; the
        checkpoint directory of a distilled actor is named after what it is for)."""
        args = self.args
        if getattr(args, "alg", alg) != alg:
            args = type("Args", (), {**vars(args), "alg": alg})()
        return ln.model_dir(args, alg)

    def learn(self, batch, max_episode_len=None, train_step=0, epsilon=0.0):
        """One supervised update on a dense or a map-once episode dict that carries "u_expert": loss = -sum(m log pi(u_expert)) /
        (n sum(m)) (bc_loss_torch), Adam or RMSprop.  epsilon is accepted for the learners' common signature and unused: the
        cloned policy is the network's own softmax.  Returns the loss as a device tensor (no host synchronisation)."""
        if "u_expert" not in batch:
            raise KeyError("ImitationLearner.learn: the batch carries no 'u_expert' (label_episodes, or the actions an expert flew)")
        labels = torch.as_tensor(batch["u_expert"], device=self.device)
        rest = {k: v for k, v in batch.items() if k != "u_expert"}
        rest, T, u, mask1 = ln._prepare(rest, self.device, max_episode_len, self.n_agents, self.n_actions, self.eval_rnn.fc1.weight.dtype)
        E, n = int(u.shape[0]), self.n_agents
        labels = labels.reshape(labels.shape[0], labels.shape[1], n)[:, :T].long().contiguous()
        logits = ln._policy_logits(self.eval_rnn, self.args, n, rest, T, self.unroll)
        mask = mask1.reshape(E, T)
        if self.unroll == "fused":
            loss, stats = BCLoss.apply(logits, rest["avail_u"], labels, mask, 1 / (n * mask.sum()))
        else:
            loss, stats = bc_loss_torch(logits, rest["avail_u"], labels, mask)
        self.rnn_optimizer.zero_grad()
        loss.backward()
        self.rnn_optimizer.step()
        self.last_stats = stats
        return loss.detach()

    def save_model(self, num, alg="bc"):
        """<model_dir(args, alg)>/<num>_rnn_net_params.pkl, ReinforceLearner's file.  alg="reinforce" (with args.alg unset or
        "reinforce") writes where Runner(..., load_model=True) looks for a REINFORCE actor; PPOLearner.eval_rnn.load_state_dict
        takes the same file.  Returns the path."""
        root = self._dir(alg)
        os.makedirs(root, exist_ok=True)
        path = os.path.join(root, str(num) + "_rnn_net_params.pkl")
        torch.save(self.eval_rnn.state_dict(), path)
        return path

    def load_model(self, rnn_root):
        self.eval_rnn.load_state_dict(torch.load(rnn_root, map_location=self.device))


# ---- DAgger's aggregate ----------------------------------------------------------------------------------------------------------

class LabelledRing(rp._EpisodeRing):
    """DeviceReplayBuffer with one more key, "u_expert" [size, T, n, 1]: the ring DAgger aggregates its labelled episodes in.
    Slots, cursor, sampling and generator use are DeviceReplayBuffer's (the same index sequences for the same calls)."""
    keys = rp.KEYS + ("u_expert",)

    def __init__(self, args, buffer_size, device="cuda", dtype=torch.float32):
        dense = rp.DeviceReplayBuffer(args, buffer_size, device, dtype)
        self.args = args
        self.n_actions, self.n_agents = dense.n_actions, dense.n_agents
        self.state_shape, self.obs_shape = dense.state_shape, dense.obs_shape
        self.size, self.episode_limit = dense.size, dense.episode_limit
        self.current_idx = 0
        self.current_size = 0
        self.device = dense.device
        self.buffers = dense.buffers
        self.buffers["u_expert"] = torch.empty(self.size, self.episode_limit, self.n_agents, 1, dtype=dtype, device=self.device)


# ---- the loop --------------------------------------------------------------------------------------------------------------------

def distil(env, expert, learner, agents, ring, iterations, updates, sample, generator=None, impl="auto"):
    """Behaviour cloning, then DAgger.  Iteration 0: one batch of episodes flown by expert.policy() (EpisodeCollector.
    generate_episodes(policy=...)); its labels are the actions flown.  Iterations >= 1: one batch flown greedily by the
    student, generate_episodes(agents=agents, evaluate=True) -- the one-launch closed loop where the env allows -- and
    relabelled by label_episodes(expert, episode, impl).  After each: ring.store_episode, `updates` learn calls on
    ring.sample(sample, generator), then the student's weights go to `agents` (agents.net takes learner.eval_rnn's parameters
    unless it IS that module, then agents.sync_weights()).  Works on BatchedFlightEnv and MovingTargetEnv, flight_easy and
    flight.  Returns the history: one dict per iteration with "iteration", "flown_by" ("expert" / "student"), "loss" and
    "agreement" (of the last update; None with updates == 0) and "targets_find" (the mean over the batch just flown) --
    floats, read once per iteration."""
    if iterations < 1 or updates < 0 or sample < 1:
        raise ValueError("distil: iterations >= 1, updates >= 0 and sample >= 1")
    collector = EpisodeCollector(env)
    history = []
    for it in range(int(iterations)):
        if it == 0:
            episode, _, _, found = collector.generate_episodes(policy=expert.policy(), init=False)
            episode["u_expert"] = episode["u"].clone()
        else:
            episode, _, _, found = collector.generate_episodes(agents=agents, evaluate=True)
            labels = label_episodes(expert, episode, impl)
            episode["u_expert"] = labels.unsqueeze(3).to(episode["u"].dtype)
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
