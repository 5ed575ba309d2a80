"""Private-grid observations: sixteen floats per agent that summarise ITS OWN grid under a communication range, and a student that
reads them (include/coopsearch.h: cs_local_grid_features, cs_local_feature_episodes).

gridobs.py lets the agent network read a summary of a centralised filter's one grid per env: a grid no single agent could own.
`LocalCoverageAgents` and `LocalBeliefAgents` keep one grid per AGENT and talk only inside a communication range.  Here agent i of
the student sees its own pose, its own last action, its id and sixteen probes of its own private grid: a learner that can be trained
centrally and then flown under the range (the setting of QMIX and DOP: centralised training, decentralised execution).

`local_grid_features_torch` is the DEFINITION, in stock eager torch ops on any device; the kernels (csrc/localobs.h) reproduce it bit
for bit.  Everything is gridobs.py's, local.py's and local_belief.py's, imported and not restated: row i of the features is row i of
`gridobs.grid_features_torch(state, grids[:, i], ...)` -- probe points from agent i's pose, sums of clamp(cell, 0, CAP) over agent
i's grid, float32(sum >> 8) * 2^-15 -- and a recorded batch is walked by `local_coverage_actions_torch` or
`local_belief_actions_torch`.

  local_grid_features_torch / local_grid_features        the definition / the kernel path of one decision.
  LocalExpertParams, local_expert_params                 imitate.ExpertParams plus comm_range; of a LocalCoverageAgents / LocalBeliefAgents.
  local_feature_episodes_torch / local_feature_episodes  the same for a recorded batch: gridobs.feature_episodes_torch's loop over the
                                                         local step definitions; one cs_local_feature_episodes launch, labels optional.
  local_label_episodes                                   the labels of that launch (the features are discarded), or imitate's rows path.
  LocalGridAgents                                        FusedAgents whose input rows are [16 features of MY grid | obs | last | id].
  distil_local_grid                                      gridobs.distil_grid with one local_feature_episodes launch per recorded batch.
"""
import dataclasses

import torch

from . import _lib
from . import baseline as bl
from . import gridobs as go
from . import imitate as im
from .agents import AgentRNN, FusedAgents, rnn_input_shape
from .baseline import FRESH, cell_centres, disc_mask, greedy_choose, quantise  # noqa: F401 -- the pieces the step definitions are made of
from .belief import CAP, targets_moved  # noqa: F401
from .collector import EpisodeCollector
from .gridobs import DIST, PROBES, REL, SCALE, grid_features_torch  # noqa: F401
from .imitate import BELIEF, COVERAGE
from .local import LocalCoverageAgents, _check_comm, links, local_coverage_actions_torch  # noqa: F401
from .local_belief import LocalBeliefAgents, local_belief_actions_torch

NEEDS = "the private-grid observation kernels need"   # _lib.torch_ops_for's words


def _check(state, grids, n, side, view_range, lookahead):
    if not 1 <= n <= _lib.MAX_AGENTS or not 1 <= side <= bl.MAX_MAP or not 0 <= view_range <= bl.MAX_MAP or not 0 <= lookahead <= side:
        raise ValueError(f"localobs: n_agents must be 1..{_lib.MAX_AGENTS}, side 1..{bl.MAX_MAP}, view_range 0..{bl.MAX_MAP} and lookahead 0..side")
    if not torch.is_tensor(state) or not torch.is_tensor(grids):
        raise ValueError("localobs: state and grids must be tensors")
    bl._check_state_grid("localobs", state, grids, n, (n, side * side), name="grids")


# ---- one decision ----------------------------------------------------------------------------------------------------------------

def local_grid_features_torch(state, grids, n_agents, side, view_range, lookahead=None, return_sums=False):
    """The definition (module docstring): state float32 [B, S >= 4n], grids int32 [B, n, side * side] (the grids a
    LocalCoverageAgents or a LocalBeliefAgents left after its call on the same state; neither tensor is written) -> features
    float32 [B, n, 16]: row i is row i of gridobs.grid_features_torch(state, grids[:, i], ...); with return_sums also the sums,
    int64 [B, n, 16].  Written as ONE grid_features_torch call on B n teams of one agent -- agent i's four floats and grids[:, i] --
    which is the same thing: a probe depends on its own agent's pose and on the grid it reads alone (tests/test_localobs_cpu.py
    holds the two forms together).  Stock EAGER torch ops on the tensors' device (baseline.coverage_actions_torch says why eager)."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check(state, grids, n, side, view_range, lookahead)
    B = int(state.shape[0])
    feat, sums = grid_features_torch(state[:, :4 * n].reshape(B * n, 4), grids.reshape(B * n, side * side), 1, side, view_range, lookahead,
                                     return_sums=True)
    feat, sums = feat.view(B, n, PROBES), sums.view(B, n, PROBES)
    return (feat, sums) if return_sums else feat


def local_grid_features_hip(state, grids, n_agents, side, view_range, lookahead=None, out=None):
    """local_grid_features_torch on the kernel (csrc/localobs.h): ONE launch on the current stream, no synchronisation.  out: a
    float32 [B, n, 16] destination (default: a new tensor)."""
    n, side, view_range = int(n_agents), int(side), int(view_range)
    lookahead = min(view_range, side) if lookahead is None else int(lookahead)
    _check(state, grids, n, side, view_range, lookahead)
    if out is None:
        out = torch.empty(int(state.shape[0]), n, PROBES, dtype=torch.float32, device=state.device)
    _lib.torch_ops_for(NEEDS).local_grid_features(state, grids, out, n, side, view_range, lookahead)
    return out


def local_grid_features(state, grids, n_agents, side, view_range, lookahead=None, impl="auto"):
    """The sixteen features of every agent's own grid: float32 [B, n, 16].  impl "auto": the kernel when `state` is on a GPU, else
    the definition; "hip": the kernel or an error; "torch": the definition, on the tensors' device."""
    if impl not in ("auto", "hip", "torch"):
        raise ValueError("impl must be 'auto', 'hip' (one cs_local_grid_features launch) or 'torch' (the definition)")
    if impl == "hip" and not (torch.is_tensor(state) and state.is_cuda):
        raise ValueError("local_grid_features(impl='hip') needs tensors on a GPU: there is no CPU fallback (impl='torch' runs the "
                         "definition anywhere)")
    if impl == "torch" or not (torch.is_tensor(state) and state.is_cuda):
        return local_grid_features_torch(state, grids, n_agents, side, view_range, lookahead)
    return local_grid_features_hip(state, grids, n_agents, side, view_range, lookahead)


# ---- a recorded batch ------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class LocalExpertParams(im.ExpertParams):
    """cs_local_label_params as host integers: imitate.ExpertParams' fields (expert COVERAGE: local.local_coverage_actions_torch per
    row; BELIEF: local_belief.local_belief_actions_torch per row, with `model` and ExpertParams' moved(t)) plus comm_range, -1
    (unlimited) or 0..128 cells.  Never equal to an ExpertParams: the centralised walk is another policy."""
    comm_range: int = -1

    def __post_init__(self):
        super().__post_init__()
        object.__setattr__(self, "comm_range", int(self.comm_range))
        _check_comm(self.comm_range)


def local_expert_params(expert):
    """The `LocalExpertParams` of a LocalCoverageAgents or a LocalBeliefAgents (exactly those classes: a subclass may decide
    differently)."""
    if type(expert) is LocalCoverageAgents:
        return LocalExpertParams(COVERAGE, expert.n_agents, expert.side, expert.view_range, expert.keep, expert.regrow, expert.lookahead,
                                 comm_range=expert.comm_range)
    if type(expert) is LocalBeliefAgents:
        return LocalExpertParams(BELIEF, expert.n_agents, expert.side, expert.view_range, expert.keep, 8, expert.lookahead, expert.model,
                                 expert.motion.every, 1 if expert.motion.speed > 0 else 0, comm_range=expert.comm_range)
    raise TypeError(f"localobs: {type(expert).__name__} keeps no private grids (LocalCoverageAgents and LocalBeliefAgents do)")


def _params(params):
    if type(params) is not LocalExpertParams:
        raise TypeError("localobs: params must be a LocalExpertParams")
    return params


def local_feature_episodes_torch(s, lens, params):
    """The definition of cs_local_feature_episodes: gridobs.feature_episodes_torch's loop with the local step definitions.  s float32
    [E, T, S >= 4n], lens int32 [E] with 0 <= lens[e] <= T, params a `LocalExpertParams` (the FILTER's) -> (feat float32 [E, T, n,
    16], labels int64 [E, T, n], grids_out int32 [E, n, side^2], prev_out int32 [E, 8, 2] and heard_out int32 [E, 8], both None
    for the coverage filter).  From n fresh grids (FRESH everywhere), prev and heard zero, for t = 0..T-1 the filter's step
    definition is applied to row t of every episode and local_grid_features_torch to the grids as it left them; an episode with t >=
    lens[e] keeps its grids, prev and heard, its features are +0.0 and its labels 0 whatever its row holds (NaN included: it is
    not read).  s and lens are not written."""
    p = _params(params)
    im._check_episodes(s, lens, p.n_agents)
    E, T = int(s.shape[0]), int(s.shape[1])
    if bool(((lens < 0) | (lens > T)).any()):
        raise ValueError(f"localobs: lens must lie in 0..T = {T}")
    dev, n = s.device, p.n_agents
    grids = torch.full((E, n, p.side * p.side), FRESH, dtype=torch.int32, device=dev)
    prev = torch.zeros(E, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=dev)
    heard = torch.zeros(E, _lib.MAX_AGENTS, dtype=torch.int32, device=dev)
    labels = torch.zeros(E, T, n, dtype=torch.int64, device=dev)
    feat = torch.zeros(E, T, n, PROBES, dtype=torch.float32, device=dev)
    for t in range(T):
        live = lens > t
        rows = torch.where(live.view(E, 1), s[:, t], torch.zeros_like(s[:, t]))   # a row past the end is never read
        g, pv, hd = grids.clone(), prev.clone(), heard.clone()
        if p.expert == COVERAGE:
            a = local_coverage_actions_torch(rows, g, n, p.side, p.view_range, p.keep, p.comm_range, p.regrow, p.lookahead)
        else:
            a = local_belief_actions_torch(rows, g, pv, hd, n, p.side, p.view_range, p.keep, p.model, p.moved(t), p.comm_range, p.lookahead)
        f = local_grid_features_torch(rows, g, n, p.side, p.view_range, p.lookahead)
        grids = torch.where(live.view(E, 1, 1), g, grids)
        prev = torch.where(live.view(E, 1, 1), pv, prev)
        heard = torch.where(live.view(E, 1), hd, heard)
        labels[:, t] = torch.where(live.view(E, 1), a, torch.zeros_like(a))
        feat[:, t] = torch.where(live.view(E, 1, 1), f, torch.zeros_like(f))
    belief = p.expert == BELIEF
    return feat, labels, grids, (prev if belief else None), (heard if belief else None)


def local_feature_episodes_hip(s, lens, params, labels=True, prev_out=True, heard_out=True):
    """local_feature_episodes_torch on the kernel (csrc/localobs.h): ONE launch on the current stream, no synchronisation.  labels /
    prev_out / heard_out False: that output is not written (None in its place); without labels the kernel skips the choose step.
    The grids are always returned: they are the kernel's workspace.  lens is read clamped to 0..T."""
    p = _params(params)
    im._check_episodes(s, lens, p.n_agents)
    E, T, dev, belief = int(s.shape[0]), int(s.shape[1]), s.device, p.expert == BELIEF
    feat = torch.empty(E, T, p.n_agents, PROBES, dtype=torch.float32, device=dev)
    lab = torch.empty(E, T, p.n_agents, dtype=torch.int64, device=dev) if labels else None
    grids = torch.empty(E, p.n_agents, p.side * p.side, dtype=torch.int32, device=dev)
    prev = torch.empty(E, _lib.MAX_AGENTS, 2, dtype=torch.int32, device=dev) if (prev_out and belief) else None
    heard = torch.empty(E, _lib.MAX_AGENTS, dtype=torch.int32, device=dev) if (heard_out and belief) else None
    ops = _lib.torch_ops_for(NEEDS)
    ops.local_feature_episodes(s, lens, feat, lab, grids, prev, heard, p.expert, p.n_agents, p.side, p.view_range, p.keep, p.regrow,
                               p.lookahead, p.model.mode, p.model.sense16, p.every, p.moving, list(p.model.dx), list(p.model.dy), p.comm_range)
    return feat, lab, grids, prev, heard


def _walk(what, filter, batch, labels, impl, torch_name):
    """(feat, labels or None) of an episode dict by one launch or by the definition: the shared body of local_feature_episodes and
    local_label_episodes."""
    p = local_expert_params(filter)
    s = batch["s"]
    if not torch.is_tensor(s) or s.dim() != 3:
        raise ValueError("localobs: batch['s'] must be a [E, T, S] tensor")
    s = s.to(torch.float32).contiguous()
    lens = im.episode_lens(batch)
    if impl == "hip" and not s.is_cuda:
        raise ValueError(f"{what}(impl='hip') needs an episode dict on a GPU: there is no CPU fallback (impl='{torch_name}' runs anywhere)")
    if impl != "torch" and s.is_cuda:
        feat, lab, _, _, _ = local_feature_episodes_hip(s, lens, p, labels=labels, prev_out=False, heard_out=False)
    else:
        feat, lab, _, _, _ = local_feature_episodes_torch(s, lens, p)
    return feat, lab


def local_feature_episodes(filter, batch, labels=False, impl="auto"):
    """The features of every step of an episode dict, as `filter` (a LocalCoverageAgents or a LocalBeliefAgents, exactly those
    classes) would have produced them flying along: float32 [E, T, n, 16], row i from agent i's own grid, 0 on the rows behind an
    episode's end; with labels=True (features, labels int64 [E, T, n]): what the filter would have done, from the same launch.
    impl "auto": one cs_local_feature_episodes launch when batch["s"] is on a GPU, else the definition; "hip": that launch or an
    error; "torch": the definition.  The filter's own grids are neither read nor written."""
    if impl not in ("auto", "hip", "torch"):
        raise ValueError("impl must be 'auto', 'hip' (one cs_local_feature_episodes launch) or 'torch' (the definition)")
    feat, lab = _walk("local_feature_episodes", filter, batch, labels, impl, "torch")
    return (feat, lab) if labels else feat


def local_label_episodes(expert, batch, impl="auto"):
    """What a LocalCoverageAgents or a LocalBeliefAgents would have done in every state of an episode dict: labels int64 [E, T, n], 0
    on the rows behind an episode's end.  impl "auto": one cs_local_feature_episodes launch when batch["s"] is on a GPU (the labels
    come from it; the features are discarded), else the rows path; "hip": that launch or an error; "rows":
    imitate.label_episodes(expert, batch, impl="rows"), T policy() calls.  The one-launch path neither reads nor writes the
    expert's own state."""
    if impl not in ("auto", "hip", "rows"):
        raise ValueError("impl must be 'auto', 'hip' (one cs_local_feature_episodes launch) or 'rows' (T policy() calls)")
    local_expert_params(expert)   # (the refusal comes first, whatever the path)
    s = batch["s"]
    if impl == "rows" or (impl == "auto" and not (torch.is_tensor(s) and s.is_cuda)):
        return im.label_episodes(expert, batch, impl="rows")
    return _walk("local_label_episodes", expert, batch, True, "hip", "rows")[1]


# ---- acting ------------------------------------------------------------------------------------------------------------------------

class LocalGridAgents(go.GridAgents):
    """FusedAgents whose agent i observes ITS OWN private grid.  env_or_args, batch, net, seed, env_offset: gridobs.GridAgents'
    (flight_easy only, for its reason); filter: the `LocalCoverageAgents` or `LocalBeliefAgents` whose grids are read (exactly those
    classes) -- `choose_action` advances it.  The network's input row is [16 features of MY grid | obs(4) | one-hot(last action) |
    one-hot(agent id)]: nothing in it needs more than the agent's own pose and what its filter heard inside the range.

    One decision is three launches on the current stream, no synchronisation: filter.choose_action (its action is discarded),
    cs_local_grid_features, cs_policy_forward with the features in front of the obs columns.  choose_action, forward_raw, the
    selection rule, load_weights, sync_weights, init_hidden and state_dict are gridobs.GridAgents' and FusedAgents'."""

    def __init__(self, env_or_args, filter, batch=None, net=None, seed=0, env_offset=0):
        args = getattr(env_or_args, "args", env_or_args)
        if getattr(args, "conv", False):
            raise ValueError("LocalGridAgents serves flight_easy only: a conv front end's 16 features and the 16 grid features exceed the "
                             "32 input columns of cs_policy_forward")
        if type(filter) not in (LocalCoverageAgents, LocalBeliefAgents):
            raise TypeError("LocalGridAgents: filter must be a LocalCoverageAgents or a LocalBeliefAgents")
        batch = filter.batch if batch is None else int(batch)
        if batch != filter.batch or int(args.n_agents) != filter.n_agents:
            raise ValueError(f"LocalGridAgents: the filter serves {filter.batch} envs of {filter.n_agents} agents, not {batch} of {args.n_agents}")
        if net is None:
            net = AgentRNN(rnn_input_shape(args) + PROBES, args)
        if net.fc1.in_features != rnn_input_shape(args) + PROBES:
            raise ValueError(f"LocalGridAgents: net.fc1 must take {rnn_input_shape(args) + PROBES} inputs (16 features in front of the plain row)")
        self.filter = filter
        FusedAgents.__init__(self, args, batch, device=filter.device, net=net, seed=seed, env_offset=env_offset)
        self.features = torch.zeros(self.batch, self.n_agents, PROBES, device=self.device)

    def observe(self, state, moved=False):
        """Advance the filter on `state` (float32 [B, S]) and read every agent's own grid: -> self.features, float32 [B, n, 16]
        (overwritten by the next call).  moved: did the targets move in the step that led here?  (A LocalCoverageAgents ignores it.)"""
        f = self.filter
        if not state.is_contiguous():
            state = state.contiguous()
        if type(f) is LocalBeliefAgents:
            f.choose_action(state, moved)
        else:
            f.choose_action(state)
        if f.impl == "torch":
            self.features.copy_(local_grid_features_torch(state, f.grids, f.n_agents, f.side, f.view_range, f.lookahead))
        else:
            local_grid_features_hip(state, f.grids, f.n_agents, f.side, f.view_range, f.lookahead, out=self.features)
        return self.features

    def policy(self, epsilon=0.0, evaluate=True, trace=None):
        """gridobs.GridAgents.policy: it resets the filter and the hidden state at t == 0 and tells the filter whether the targets
        moved, `belief.targets_moved(filter.motion, t)` (never, for a LocalCoverageAgents).  trace: a float32 [T, B, n, 16] tensor
        that receives the features of every step."""
        motion = getattr(self.filter, "motion", None)

        def fn(obs, state, last_onehot, t):
            if t == 0:
                self.filter.reset()
                self.init_hidden()
            out = self.choose_action(obs, state, motion is not None and targets_moved(motion, t), epsilon, evaluate)
            if trace is not None:
                trace[t].copy_(self.features)
            return out
        return fn


# ---- learning ----------------------------------------------------------------------------------------------------------------------

def distil_local_grid(env, expert, filter, learner, agents, ring, iterations, updates, sample, generator=None, impl="auto"):
    """gridobs.distil_grid for a student that reads private grids.  expert: whose actions are cloned; filter: the
    LocalCoverageAgents or LocalBeliefAgents whose grids the student observes (`agents.filter`, usually; it may be the expert
    itself); learner a gridobs.GridImitationLearner, agents a LocalGridAgents, ring a gridobs.FeatureRing (batch["f"] has the shape
    it has there).  Iteration 0 is flown by expert.policy(), iterations >= 1 by agents.policy() greedily.  Every recorded batch gets
    its "f" from ONE local_feature_episodes launch; its labels come from the same launch when the expert is of the filter's own
    class with equal `LocalExpertParams` (the same decisions), from the actions flown in iteration 0 otherwise, and from
    imitate.label_episodes(expert, episode, impl) after that.  Then distil's steps.  Returns distil's history."""
    if iterations < 1 or updates < 0 or sample < 1:
        raise ValueError("distil_local_grid: iterations >= 1, updates >= 0 and sample >= 1")
    collector = EpisodeCollector(env)
    p = local_expert_params(filter)
    own = type(expert) is type(filter) and local_expert_params(expert) == p
    feature_impl = "hip" if impl == "hip" else "auto"   # (impl is label_episodes': "rows" concerns the labels alone)
    history = []
    for it in range(int(iterations)):
        flown = expert.policy() if it == 0 else agents.policy()
        episode, _, _, found = collector.generate_episodes(policy=flown, init=False)
        if own:
            episode["f"], labels = local_feature_episodes(filter, episode, labels=True, impl=feature_impl)
        else:
            episode["f"] = local_feature_episodes(filter, episode, impl=feature_impl)
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
