"""QMIX, DOP, REINFORCE and PPO learners on the device: the consumers of DeviceReplayBuffer.sample() (policy/qmix.py,
policy/dop.py, policy/reinforce.py of the reference; PPO has no counterpart there).

The reference's `learn` (policy/qmix.py:85-130) unrolls the agent network one transition at a time (`get_q_values`,
:160-182): fc1 -> ReLU -> GRUCell -> fc2 for the eval and the target network on E*n rows per step, T = 200 steps, and autograd
walks the same graph back -- thousands of tiny launches per learn step.  Only the recurrence h_t = GRUCell(x_t, h_{t-1}) is
sequential.  Here everything else runs ONCE over all T*E*n rows as ordinary torch ops (the conv front end, fc1, the input
projection W_ih x + b_ih, fc2, the mixer, the masked TD loss, dW_hh / db_hh), and the recurrence is one HIP launch forward and
one backward (`GRUSequence`: cs_gru_seq_forward / cs_gru_seq_backward, csrc/gru_seq.h).  The number of launches of a learn step
does not depend on T, and `learn` never synchronises with the host.

`QMixLearner(..., unroll="torch")` keeps the reference's per-step loop over the same modules as the yardstick (it also runs on
the CPU).  Parameter names, initialisation order and saved file names are the reference's, so its checkpoints load and this
learner's checkpoints load into the reference.

`DOPLearner` and `ReinforceLearner` run their actor through the same unroll.  Their one other sequential part, the backward
recursion over t of the returns (DOP's TD(lambda) critic target, REINFORCE's discounted return), is one HIP launch
(`episode_returns`: cs_episode_returns, csrc/returns.h); DOP's critic, the mixers and the action-probability head run once
over all rows in torch.

Every `learn` also takes a batch in the map-once format of the flight variant (replay.COMPACT_KEYS) as
it is.  QMIX and REINFORCE never build `o` / `o_next` from it: the conv front end runs once per (episode, step) on the map
(`map_features`), its 16 features are broadcast over the agents, and the rest of the unroll is the one above.

`PPOLearner` is the on-policy learner shaped like the batched env: a clipped-surrogate actor-critic
with a central value function that reuses every collected episode for several epochs.  Its actor goes through the same
unroll; its two other loops are HIP kernels of the returns' family (csrc/ppo.h): `gae` (cs_gae: advantages and value targets,
one launch) and `PPOPolicyLoss` (cs_ppo_loss: the clipped surrogate, its entropy bonus, their statistics and the gradient
with respect to the logits in one pass over the rows).

`conv_impl="hip"` (opt-in on every learner) takes that conv front end from `ConvFeatures` instead of the
torch modules: the acting kernel (k_conv_features) forward, k_conv_features_bwd (csrc/conv_bwd.h) backward, so that a flight
learn step makes no MIOpen call.  The default, "torch", is the modules.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .agents import AgentRNN, FusedAgents, rnn_input_shape
from .replay import expand_compact

HIDDEN = 64   # rnn_hidden_dim: the recurrence kernels are built for it (get_mixer_args, common/arguments.py:58)


def get_mixer_args(args, seed=None):
    """The learner fields of the reference's get_mixer_args (common/arguments.py:57-110) on an argparse-style namespace;
    seed: args.seed (the reference draws one when training; here the caller chooses)."""
    args.off_policy = True
    args.rnn_hidden_dim, args.qmix_hidden_dim, args.two_hyper_layers, args.hyper_hidden_dim = 64, 32, False, 64
    args.lr, args.tau, args.gamma, args.grad_norm_clip = 0.0005, 0.05, getattr(args, "gamma", 0.99), 10
    args.optimizer = getattr(args, "optimizer", "Adam")
    args.batch_size, args.buffer_size = 32, 3000
    args.epsilon, args.min_epsilon, args.epsilon_anneal_scale = 1, 0.05, "step"
    args.anneal_epsilon = (args.epsilon - args.min_epsilon) / 10000
    if seed is not None:
        args.seed = seed
    return args


def _gru_forward(gi, w_hh, b_hh, h0, save):
    """cs_gru_seq_forward on torch tensors -> (H [T, R, 64], saved [T, R, 4, 64] or None)."""
    T, R = int(gi.shape[0]), int(gi.shape[1])
    if gi.shape[2] != 3 * HIDDEN or tuple(w_hh.shape) != (3 * HIDDEN, HIDDEN):
        raise ValueError(f"GRUSequence: gi must be [T, R, {3 * HIDDEN}] and w_hh [{3 * HIDDEN}, {HIDDEN}]")
    gi, w_hh, b_hh = gi.detach().contiguous(), w_hh.detach().contiguous(), b_hh.detach().contiguous()
    h0 = None if h0 is None else h0.detach().contiguous()
    H = gi.new_empty(T, R, HIDDEN)
    saved = gi.new_empty(T, R, 4, HIDDEN) if save else None
    _lib.torch_ops().gru_seq_forward(w_hh, b_hh, gi, h0, T, R, H, saved)
    return H, saved


class GRUSequence(torch.autograd.Function):
    """(gi [T, R, 192], w_hh [192, 64], b_hh [192], h0 [R, 64] or None) -> H [T, R, 64] = h_1 .. h_T of torch.nn.GRUCell with
    gi = W_ih x + b_ih given for all t.  Backward: (dgi, dW_hh, db_hh, dh0); the recurrence itself in one launch each way,
    dW_hh = sum_t dgh_t^T h_{t-1} and db_hh = sum_t dgh_t as one matrix product / sum over the T*R rows."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, h0):
        grad = any(ctx.needs_input_grad)
        H, saved = _gru_forward(gi, w_hh, b_hh, h0, grad)
        if grad:
            ctx.save_for_backward(w_hh.detach().contiguous(), H, None if h0 is None else h0.detach().contiguous(), saved)
        return H

    @staticmethod
    def backward(ctx, dH):
        w_hh, H, h0, saved = ctx.saved_tensors
        T, R = int(H.shape[0]), int(H.shape[1])
        need_gi, need_w, need_b, need_h0 = ctx.needs_input_grad
        dgi = H.new_empty(T, R, 3 * HIDDEN)
        dgh = H.new_empty(T, R, 3 * HIDDEN)
        dh0 = H.new_empty(R, HIDDEN) if need_h0 else None
        _lib.torch_ops().gru_seq_backward(w_hh, dH.contiguous(), H, h0, saved, T, R, dgi, dgh, dh0)
        dgh2 = dgh.view(T * R, 3 * HIDDEN)
        dw = db = None
        if need_w:
            first = h0.unsqueeze(0) if h0 is not None else H.new_zeros(1, R, HIDDEN)
            h_prev = torch.cat([first, H[:-1]], 0).view(T * R, HIDDEN)
            dw = dgh2.t() @ h_prev
        if need_b:
            db = dgh2.sum(0)
        return (dgi if need_gi else None), dw, db, dh0


CONV_IMPLS = ("torch", "hip")
CONV_FRONT_END = FusedAgents.CONV_HYPER   # what the conv kernels are built for: the reference's flight hyper-parameters
CONV_CELLS, CONV_FEATURES = 2500, 16


def check_conv_impl(args, device, unroll, conv_impl):
    """The learners' `conv_impl` argument: "torch" (the default: net.conv / net.linear, i.e. MIOpen) or "hip" (ConvFeatures: the
    acting kernel forward, k_conv_features_bwd backward).  "hip" needs what the kernels need; every refusal names its reason."""
    if conv_impl not in CONV_IMPLS:
        raise ValueError(f"conv_impl must be 'torch' or 'hip', not {conv_impl!r}")
    if conv_impl == "torch":
        return conv_impl
    if unroll != "fused":
        raise ValueError("conv_impl='hip' needs unroll='fused': the reference's step loop (unroll='torch') runs the torch modules")
    if torch.device(device).type != "cuda":
        raise ValueError(f"conv_impl='hip' needs a GPU device: the conv kernels do not run on {torch.device(device).type!r}")
    if not getattr(args, "conv", False):
        raise ValueError("conv_impl='hip' needs the conv front end (args.conv): this variant's network has none")
    other = {k: getattr(args, k, None) for k, v in CONV_FRONT_END.items() if getattr(args, k, None) != v}
    if other:
        raise ValueError(f"conv_impl='hip' is built for the reference's front-end hyper-parameters {CONV_FRONT_END}; "
                         f"these differ: {other}")
    return conv_impl


def _conv_weights(net):
    return (net.conv[0].weight, net.conv[0].bias, net.conv[2].weight, net.conv[2].bias, net.linear.weight, net.linear.bias)


def _conv_forward(weights, maps, map_stride, n_maps):
    """policy_conv_features on torch tensors -> feat [n_maps, 16] (no graph)."""
    feat = maps.new_empty(n_maps, CONV_FEATURES)
    _lib.torch_ops().policy_conv_features(*weights, maps, int(map_stride), int(n_maps), feat)
    return feat


_CONV_SCRATCH = {}   # (device, stream) -> the backward's partial-sum buffer, kept between calls (its contents mean nothing afterwards)


def _conv_scratch(like, floats):
    key = (like.device, torch.cuda.current_stream(like.device).cuda_stream)   # calls on one stream are ordered: one buffer serves them
    buf = _CONV_SCRATCH.get(key)
    if buf is None or buf.numel() < floats:
        buf = _CONV_SCRATCH[key] = like.new_empty(floats)
    return buf


class ConvFeatures(torch.autograd.Function):
    """(maps, map_stride, n_maps, conv1.weight, conv1.bias, conv2.weight, conv2.bias, linear.weight, linear.bias) -> feat
    [n_maps, 16]: the conv front end of AgentRNN.forward.  maps: a contiguous float32 tensor, map m = 2500 floats at element
    m * map_stride (a [n_maps, 2500] table, or rows that carry the map in front: map_stride = row width).  Forward is
    policy_conv_features as it is, so learning sees the acting kernel's features bit for bit; backward is
    policy_conv_features_backward (the six weight gradients; both activation planes recomputed from the maps, nothing but
    the maps kept).  The maps are data: one that requires grad is refused."""

    @staticmethod
    def forward(ctx, maps, map_stride, n_maps, *weights):
        if ctx.needs_input_grad[0]:
            raise ValueError("ConvFeatures: no gradient with respect to the maps (they are data); detach them")
        weights = tuple(w.detach().contiguous() for w in weights)
        maps = maps.detach()
        feat = _conv_forward(weights, maps, map_stride, n_maps)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(maps, *weights)
            ctx.geometry = (int(map_stride), int(n_maps))
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        maps, *weights = ctx.saved_tensors
        map_stride, n_maps = ctx.geometry
        ops = _lib.torch_ops()
        grads = [torch.empty_like(w) for w in weights]
        scratch = _conv_scratch(maps, int(ops.policy_conv_features_backward_scratch(n_maps)))
        ops.policy_conv_features_backward(*weights, maps, map_stride, n_maps, dfeat.contiguous(), *grads, scratch)
        return (None, None, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])])


def _conv_features(net, maps, map_stride, n_maps):
    """net's front end on the conv kernels: with a graph (ConvFeatures) when gradients are on, else the forward op alone."""
    weights = _conv_weights(net)
    if torch.is_grad_enabled():
        return ConvFeatures.apply(maps, int(map_stride), int(n_maps), *weights)
    return _conv_forward(tuple(w.detach().contiguous() for w in weights), maps, map_stride, n_maps)


def map_features(net, maps):
    """The conv front end of AgentRNN.forward on maps [..., cells] -> [..., conv_out_dim]: the same modules, one row per map
    (net.conv_impl == "hip", set by the learners: the conv kernels on the same weights)."""
    a = net.args
    if getattr(net, "conv_impl", "torch") == "hip":
        flat = maps.detach().reshape(-1, CONV_CELLS).contiguous()
        return _conv_features(net, flat, CONV_CELLS, flat.shape[0]).view(*maps.shape[:-1], -1)
    prob = maps.reshape(-1, 1, a.map_size, a.map_size)
    feat = net.linear(net.conv(prob).reshape(-1, a.dim_2 * net.conv_size ** 2))
    return feat.view(*maps.shape[:-1], -1)


def unroll_q(net, X, h0=None, impl="fused", featured=False):
    """Q-values of all T steps: X [T, R, in] (rows of get_inputs, policy/qmix.py:132-158), h0 [R, 64] or None (zeros) ->
    q [T, R, n_actions].  impl "fused": the conv front end (flight), fc1 and the input projection over all T*R rows at once,
    GRUSequence, then fc2 over all rows; "torch": the reference's loop of net(x_t, h) over t (get_q_values).
    featured: the rows of X already carry the conv features in place of the map (compact_actor_inputs): the front end is
    skipped, the rest is the same."""
    T, R = int(X.shape[0]), int(X.shape[1])
    if impl == "torch":
        h = h0 if h0 is not None else X.new_zeros(R, net.args.rnn_hidden_dim)
        qs = []
        for t in range(T):
            if featured:   # AgentRNN.forward behind its front end
                h = net.rnn(F.relu(net.fc1(X[t])), h)
                q = net.fc2(h)
            else:
                q, h = net(X[t], h)
            qs.append(q)
        return torch.stack(qs, 0)
    if impl != "fused":
        raise ValueError("impl must be 'fused' or 'torch'")
    if net.args.rnn_hidden_dim != HIDDEN:
        raise ValueError(f"the fused unroll is built for rnn_hidden_dim = {HIDDEN}")
    x = X.reshape(T * R, -1)
    if net.args.conv and not featured:   # the same modules on the same maps as AgentRNN.forward, all T*R maps in one call
        cells = net.args.map_size ** 2
        if getattr(net, "conv_impl", "torch") == "hip":   # the maps where they lie, in front of every row: no copy
            x = x.contiguous()
            feat = _conv_features(net, x.detach(), x.shape[1], T * R)
        else:
            prob = x[:, :cells].reshape(-1, 1, net.args.map_size, net.args.map_size)
            feat = net.linear(net.conv(prob).reshape(-1, net.args.dim_2 * net.conv_size ** 2))
        x = torch.cat([feat, x[:, cells:]], 1)
    x = F.relu(net.fc1(x))
    gi = F.linear(x, net.rnn.weight_ih, net.rnn.bias_ih).view(T, R, 3 * HIDDEN)
    if torch.is_grad_enabled():
        H = GRUSequence.apply(gi, net.rnn.weight_hh, net.rnn.bias_hh, h0)
    else:   # the target network: no graph, so nothing is saved for a backward
        H = _gru_forward(gi, net.rnn.weight_hh, net.rnn.bias_hh, h0, False)[0]
    return net.fc2(H.view(T * R, HIDDEN)).view(T, R, -1)


class MixerNet(nn.Module):
    """network/mixer_net.py with its parameter names, so the shipped *_qmix_net_params.pkl load by name.  Its quirks are kept:
    q_tot = q . k with k = |W1 s| |W2 s| normalised over the agents; V, hyper_b1 and hyper_b2 exist (and are saved) but take
    no part in the output, so they never receive a gradient and never change."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        S, n, Q = args.state_shape, args.n_agents, args.qmix_hidden_dim
        if args.two_hyper_layers:
            self.hyper_w1 = nn.Sequential(nn.Linear(S, args.hyper_hidden_dim), nn.ReLU(), nn.Linear(args.hyper_hidden_dim, n * Q))
            self.hyper_w2 = nn.Sequential(nn.Linear(S, args.hyper_hidden_dim), nn.ReLU(), nn.Linear(args.hyper_hidden_dim, Q))
        else:
            self.hyper_w1 = nn.Linear(S, n * Q)
            self.hyper_w2 = nn.Linear(S, Q)
        self.hyper_b1 = nn.Linear(S, Q)
        self.hyper_b2 = nn.Sequential(nn.Linear(S, Q), nn.ReLU(), nn.Linear(Q, 1))
        self.V = nn.Sequential(nn.Linear(S, Q), nn.ReLU(), nn.Linear(Q, 1))

    def forward(self, q_values, states):
        """q_values [E, T, n], states [E, T, state_shape] -> q_total [E, T, 1] (mixer_net.py:52-80)."""
        episode_num = q_values.size(0)
        n, Q = self.args.n_agents, self.args.qmix_hidden_dim
        q_values = q_values.view(-1, 1, n)
        states = states.reshape(-1, self.args.state_shape)
        w1 = torch.abs(self.hyper_w1(states)).view(-1, n, Q)
        w2 = torch.abs(self.hyper_w2(states)).view(-1, Q, 1)
        k = torch.bmm(w1, w2)
        k = k / torch.sum(k, dim=1, keepdim=True)
        return torch.bmm(q_values, k).view(episode_num, -1, 1)


# ---- shared by the learners ---------------------------------------------------------------------------------------------------

def model_dir(args, alg):
    """<model_dir><env>_Seed<seed>_<alg>_<n>a<targets>t(AM<agent_mode>TM<target_mode>): the reference's checkpoint directory
    (qmix.py / dop.py / reinforce.py __init__); alg: args.alg, or this default."""
    return (getattr(args, "model_dir", "./model/") + args.env + "_Seed" + str(args.seed) + "_" + getattr(args, "alg", alg) +
            "_{}a{}t(AM{}TM{})".format(args.n_agents, getattr(args, "target_num", 15), getattr(args, "agent_mode", 0),
                                      getattr(args, "target_mode", 0)))


def soft_update(pairs, tau):
    """target <- tau * eval + (1 - tau) * target for each (eval, target) module pair, in a few multi-tensor launches."""
    with torch.no_grad():
        for ev, tg in pairs:
            e, t = list(ev.parameters()), list(tg.parameters())
            new = torch._foreach_mul(e, tau)
            torch._foreach_add_(new, torch._foreach_mul(t, 1 - tau))
            torch._foreach_copy_(t, new)


def device_batch(batch, device, max_episode_len=None):
    """A sampled (or freshly collected) batch dict on `device`, every key cut to max_episode_len steps (what agent.py:112-122
    does before calling learn; None = the full T)."""
    if max_episode_len is not None:   # (a compact batch keeps one more row of map / s_full: the step after the last)
        batch = {k: v[:, :max_episode_len + (1 if k in ("map", "s_full") else 0)] for k, v in batch.items()}
    return {k: torch.as_tensor(v, device=device) for k, v in batch.items()}


def actor_inputs(args, n_agents, batch, T):
    """_get_inputs (qmix.py:132-158; _get_actor_inputs of dop.py / reinforce.py) for all T steps at once: X, X_next
    [T, E*n, in], row e*n + agent.  inputs = obs ++ previous one-hot action (zeros at t = 0) ++ agent id; inputs_next =
    obs_next ++ this step's one-hot ++ id."""
    o, o_next, u_onehot = batch["o"], batch["o_next"], batch["u_onehot"]
    E, n = int(o.shape[0]), n_agents
    parts, parts_next = [o], [o_next]
    if getattr(args, "last_action", True):
        parts.append(torch.cat([torch.zeros_like(u_onehot[:, :1]), u_onehot[:, :-1]], 1))
        parts_next.append(u_onehot)
    if getattr(args, "reuse_network", True):
        ids = torch.eye(n, device=o.device, dtype=o.dtype).expand(E, T, n, n)
        parts.append(ids)
        parts_next.append(ids)
    X = torch.cat(parts, 3).transpose(0, 1).reshape(T, E * n, -1)
    X_next = torch.cat(parts_next, 3).transpose(0, 1).reshape(T, E * n, -1)
    return X, X_next


def compact_actor_inputs(args, n_agents, batch, net, net_next=None):
    """actor_inputs for a map-once batch that has been through `with_narrow_keys`, without `o` / `o_next`: rows are
    conv features ++ own 4 floats ++ one-hot ++ agent id, [T, E*n, 16 + 4 + A + n] -- what AgentRNN.forward makes of
    actor_inputs' rows behind its conv front end.  The front end runs once per (episode, step): `net`'s on map[:, :T] * real
    (with a graph when gradients are on), `net_next`'s (the target network; None: no X_next) on map[:, 1:] * real, both
    broadcast over the agents."""
    if not (getattr(args, "last_action", True) and getattr(args, "reuse_network", True)):
        raise ValueError("a map-once batch needs last_action and reuse_network (the reference's defaults)")
    m, sf, u_onehot = batch["map"], batch["s_full"], batch["u_onehot"]
    E, T, n = int(u_onehot.shape[0]), int(u_onehot.shape[1]), n_agents
    real = 1 - batch["padded"]                                       # [E, T, 1]
    real4 = real.unsqueeze(-1)
    own = sf[..., :4 * n].reshape(E, T + 1, n, 4)                    # emit<N>: state[4i..4i+3] is agent i's observation tail
    ids = torch.eye(n, device=m.device, dtype=m.dtype).expand(E, T, n, n)

    def rows(front, lo, last):
        feat = map_features(front, m[:, lo:lo + T] * real).unsqueeze(2).expand(E, T, n, -1)
        return torch.cat([feat, own[:, lo:lo + T] * real4, last, ids], 3).transpose(0, 1).reshape(T, E * n, -1)
    X = rows(net, 0, torch.cat([torch.zeros_like(u_onehot[:, :1]), u_onehot[:, :-1]], 1))
    if net_next is None:
        return X, None
    with torch.no_grad():
        return X, rows(net_next, 1, u_onehot)


def with_narrow_keys(batch, n_agents, n_actions):
    """A map-once batch plus the dense keys that do not repeat the map (s, s_next, avail_u, avail_u_next, u_onehot: by
    expand_compact's definition); a dense batch as it is."""
    if "map" not in batch:
        return batch
    return {**batch, **expand_compact(batch, n_agents, n_actions, wide=False)}


class QMixLearner:
    """policy/qmix.py:QMIX on the device.  args: the reference's namespace after get_mixer_args (seed, lr, optimizer, gamma,
    tau, grad_norm_clip, qmix_hidden_dim, two_hyper_layers, hyper_hidden_dim, rnn_hidden_dim) and the env fields
    (apply_env_info).  unroll: "fused" (GRUSequence, needs the HIP library and a GPU) or "torch" (the reference's loop).
    conv_impl (flight's conv front end in `learn`): "torch" (the modules) or "hip" (ConvFeatures; check_conv_impl)."""

    def __init__(self, args, device="cuda", unroll="fused", conv_impl="torch"):
        if unroll not in ("fused", "torch"):
            raise ValueError("unroll must be 'fused' or 'torch'")
        self.conv_impl = check_conv_impl(args, device, unroll, conv_impl)
        self.args, self.device, self.unroll = args, torch.device(device), unroll
        self.n_actions, self.n_agents = args.n_actions, args.n_agents
        self.state_shape, self.obs_shape = args.state_shape, args.obs_shape
        self.tau = args.tau
        input_shape = rnn_input_shape(args)
        # the reference's order (qmix.py:28-38): seed, then eval / target RNN, eval / target mixer, initialised on the CPU
        torch.manual_seed(args.seed)
        self.eval_rnn = AgentRNN(input_shape, args)
        self.target_rnn = AgentRNN(input_shape, args)
        self.eval_qmix_net = MixerNet(args)
        self.target_qmix_net = MixerNet(args)
        for net in (self.eval_rnn, self.target_rnn, self.eval_qmix_net, self.target_qmix_net):
            net.to(self.device)
        self.eval_rnn.conv_impl = self.target_rnn.conv_impl = self.conv_impl   # read by map_features / unroll_q
        self.model_dir = model_dir(args, "qmix")
        self.target_rnn.load_state_dict(self.eval_rnn.state_dict())
        self.target_qmix_net.load_state_dict(self.eval_qmix_net.state_dict())
        self.eval_parameters = list(self.eval_qmix_net.parameters()) + list(self.eval_rnn.parameters())
        opt = getattr(args, "optimizer", "Adam")
        if opt == "RMS":
            self.optimizer = torch.optim.RMSprop(self.eval_parameters, lr=args.lr)
        elif opt == "Adam":
            self.optimizer = torch.optim.Adam(self.eval_parameters, lr=args.lr)
        else:
            raise ValueError("No such optimizer")
        self.eval_hidden = None
        self.target_hidden = None

    def init_hidden(self, episode_num):
        self.eval_hidden = torch.zeros(episode_num, self.n_agents, self.args.rnn_hidden_dim, device=self.device)
        self.target_hidden = torch.zeros(episode_num, self.n_agents, self.args.rnn_hidden_dim, device=self.device)

    def soft_update(self):
        """target <- tau * eval + (1 - tau) * target (qmix.py:78-83), the same arithmetic in a few multi-tensor launches."""
        soft_update(((self.eval_rnn, self.target_rnn), (self.eval_qmix_net, self.target_qmix_net)), self.tau)

    def get_inputs(self, batch, T):
        """_get_inputs (qmix.py:132-158) for all T steps at once: X, X_next [T, E*n, in], row e*n + agent (actor_inputs)."""
        return actor_inputs(self.args, self.n_agents, batch, T)

    def get_q_values(self, batch, T):
        """(q_evals, q_targets) [E, T, n, n_actions] (qmix.py:160-182); the target network runs without a graph."""
        E, n = int(batch["u"].shape[0]), self.n_agents
        featured = "map" in batch   # map-once: the front end once per (episode, step), eval on row t, target on row t + 1
        if featured:
            X, X_next = compact_actor_inputs(self.args, n, batch, self.eval_rnn, self.target_rnn)
        else:
            X, X_next = self.get_inputs(batch, T)
        self.init_hidden(E)
        q_eval = unroll_q(self.eval_rnn, X, None, self.unroll, featured)
        with torch.no_grad():
            q_target = unroll_q(self.target_rnn, X_next, None, self.unroll, featured)
        shape = (T, E, n, self.n_actions)
        return q_eval.view(shape).transpose(0, 1), q_target.view(shape).transpose(0, 1)

    def learn(self, batch, max_episode_len=None, train_step=0, epsilon=None):
        """One QMIX update (qmix.py:85-130) on a DeviceReplayBuffer.sample() dict as it is ([E, T, ...] float32; `u` is cast to
        long), or on a CompactReplayBuffer.sample() dict (the map-once keys; `o` / `o_next` are never built).  max_episode_len: cut every key to that many steps (what agent.py:112-122 does before calling learn); None = the
        full T, which is what the reference's _get_max_episode_len amounts to (it never shortens T).  Returns the loss (a device
        tensor: no host synchronisation)."""
        batch = with_narrow_keys(device_batch(batch, self.device, max_episode_len), self.n_agents, self.n_actions)
        T = int(batch["u"].shape[1])
        u = batch["u"].long()
        dt = self.eval_rnn.fc1.weight.dtype   # float32, unless the caller converted the networks
        s, s_next, r = batch["s"].to(dt), batch["s_next"].to(dt), batch["r"].to(dt)
        avail_u_next, terminated = batch["avail_u_next"], batch["terminated"].to(dt)
        batch = {k: (v.to(dt) if k in ("o", "o_next", "u_onehot", "map", "s_full", "padded") else v) for k, v in batch.items()}
        mask = 1 - batch["padded"]

        q_evals, q_targets = self.get_q_values(batch, T)
        q_evals = torch.gather(q_evals, dim=3, index=u).squeeze(3)
        q_targets = q_targets.masked_fill(avail_u_next == 0, -9999999)   # boolean-index assignment would synchronise
        q_targets = q_targets.max(dim=3)[0]
        q_total_eval = self.eval_qmix_net(q_evals, s)
        with torch.no_grad():
            q_total_target = self.target_qmix_net(q_targets, s_next)
        targets = r + self.args.gamma * q_total_target * (1 - terminated)
        td_error = q_total_eval - targets.detach()
        masked_td_error = mask * td_error
        loss = (masked_td_error ** 2).sum() / mask.sum()
        self.optimizer.zero_grad()
        loss.backward()
        self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self.eval_parameters, self.args.grad_norm_clip)
        self.optimizer.step()
        self.soft_update()
        return loss.detach()

    def save_model(self, num):
        """qmix.py:189-196: <model_dir>/<num>_qmix_net_params.pkl and <num>_rnn_net_params.pkl (state_dicts)."""
        os.makedirs(self.model_dir, exist_ok=True)
        idx = str(num)
        torch.save(self.eval_qmix_net.state_dict(), os.path.join(self.model_dir, idx + "_qmix_net_params.pkl"))
        torch.save(self.eval_rnn.state_dict(), os.path.join(self.model_dir, idx + "_rnn_net_params.pkl"))

    def load_model(self, rnn_root, qmix_root):
        """qmix.py:211-215: eval networks from the two files, targets copied from them."""
        self.eval_rnn.load_state_dict(torch.load(rnn_root, map_location=self.device))
        self.eval_qmix_net.load_state_dict(torch.load(qmix_root, map_location=self.device))
        self.target_rnn.load_state_dict(self.eval_rnn.state_dict())
        self.target_qmix_net.load_state_dict(self.eval_qmix_net.state_dict())


# ---- DOP and REINFORCE (policy/dop.py, policy/reinforce.py) -------------------------------------------------------------------

def get_dop_args(args, seed=None):
    """The learner fields of the reference's get_dop_args (common/arguments.py:112-169) on an argparse-style namespace; seed:
    args.seed (the reference draws one when training; here the caller chooses)."""
    args.off_policy = True
    args.rnn_hidden_dim, args.offpg_hidden_dim, args.qmix_hidden_dim = 64, 128, 32
    args.two_hyper_layers, args.hyper_hidden_dim = False, 64
    args.lr, args.critic_lr, args.td_lambda, args.tau = 5e-4, 1e-4, 0.8, 0.05
    args.gamma, args.optimizer = getattr(args, "gamma", 0.99), getattr(args, "optimizer", "Adam")
    args.epsilon, args.min_epsilon, args.epsilon_anneal_scale = 1, 0.05, "step"
    args.anneal_epsilon = (args.epsilon - args.min_epsilon) / 10000
    args.n_epoch, args.n_episodes, args.train_steps, args.evaluate_cycle = 500000, 1, 1, 200
    args.batch_size, args.buffer_size, args.onbuffer_size = 32, 3000, 32
    args.save_cycle, args.target_update_cycle, args.grad_norm_clip = 500, 200, 10
    if seed is not None:
        args.seed = seed
    return args


def get_reinforce_args(args, seed=None):
    """The learner fields of the reference's get_reinforce_args (common/arguments.py:172-216); seed as get_dop_args."""
    args.off_policy = False
    args.rnn_hidden_dim, args.critic_dim = 64, 128
    args.tau, args.lr_actor, args.lr_critic = 0.05, 1e-4, 1e-3
    args.gamma, args.optimizer = getattr(args, "gamma", 0.99), getattr(args, "optimizer", "Adam")
    args.epsilon, args.anneal_epsilon, args.min_epsilon, args.epsilon_anneal_scale = 0.5, 0.00064, 0.02, "epoch"
    args.batch_size, args.buffer_size = 32, 1000
    args.n_epoch, args.n_episodes, args.evaluate_cycle, args.save_cycle = 100000, 1, 200, 500
    args.grad_norm_clip = 10
    if seed is not None:
        args.seed = seed
    return args


class OffPGCritic(nn.Module):
    """network/offpg_net.py with its parameter names: relu(fc1) -> relu(fc2) -> q = fc3(x) + fc_v(x), one q per action."""

    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.input_shape = input_shape
        self.fc1 = nn.Linear(input_shape, args.offpg_hidden_dim)
        self.fc2 = nn.Linear(args.offpg_hidden_dim, args.offpg_hidden_dim)
        self.fc_v = nn.Linear(args.offpg_hidden_dim, 1)
        self.fc3 = nn.Linear(args.offpg_hidden_dim, args.n_actions)

    def forward(self, inputs):
        x = F.relu(self.fc2(F.relu(self.fc1(inputs))))
        return self.fc3(x) + self.fc_v(x)


def _make_optimizer(args, params, lr):
    opt = getattr(args, "optimizer", "Adam")
    if opt == "RMS":
        return torch.optim.RMSprop(params, lr=lr)
    if opt == "Adam":
        return torch.optim.Adam(params, lr=lr)
    raise ValueError("No such optimizer")


def action_prob(logits, avail_u, epsilon):
    """The action probabilities of the policy-gradient actors (_get_actor_output, dop.py:238-267 = _get_action_prob,
    reinforce.py:131-156): softmax over the actions, the epsilon mix over the available ones, unavailable actions zeroed,
    renormalised and zeroed again.  logits, avail_u [E, T, n, A]; epsilon: a float or a 0-dim device tensor.
    A padded step has no available action: its row is inf / 0 = NaN after the mix and the renormalisation, as in the
    reference, and ends as zeros.  The zeroing is masked_fill (boolean-index assignment would synchronise), whose backward
    also zeroes the NaN that the 0 / 0 of those rows sends back, so every gradient stays finite."""
    prob = F.softmax(logits, dim=-1)
    unavail = avail_u == 0
    action_num = avail_u.sum(dim=-1, keepdim=True).float()   # broadcast over the actions (the reference's repeat)
    p = (1 - epsilon) * prob + torch.ones_like(prob) * epsilon / action_num
    p = p.masked_fill(unavail, 0.0)
    p = p / p.sum(dim=-1, keepdim=True)
    return p.masked_fill(unavail, 0.0)


def log_pi_taken(prob, u, mask):
    """log pi(u) [E, T, n]; padded steps (mask == 0) read 1, so their log is 0 (dop.py:120-123, reinforce.py:82-84)."""
    pi = torch.gather(prob, dim=3, index=u).squeeze(3)
    return torch.log(pi.masked_fill(mask == 0, 1.0))


def episode_returns(r, terminated, padded, q=None, gamma=0.99, td_lambda=0.8):
    """cs_episode_returns (csrc/returns.h) on device tensors: r, terminated, padded (and q) [E, T] or [E, T, 1] float32 ->
    [E, T].  q None: REINFORCE's discounted return (reinforce.py:101-110); q = q_total_target: DOP's TD(lambda) target
    (dop.py:192-232).  One launch, whatever E and T."""
    E, T = int(r.shape[0]), int(r.shape[1])
    flat = lambda x: x.detach().float().reshape(E, T).contiguous()
    out = torch.empty(E, T, dtype=torch.float32, device=r.device)
    _lib.torch_ops().episode_returns(flat(r), flat(terminated), flat(padded), None if q is None else flat(q), E, T, float(gamma),
                           float(td_lambda), out)
    return out


def returns_torch(r, terminated, padded, gamma):
    """REINFORCE's _get_returns (reinforce.py:101-110) as the reference computes it: one step at a time, t = T-1 .. 0 ->
    [E, T]."""
    r, m, c = r.reshape(r.shape[0], -1), (1 - padded).reshape(r.shape[0], -1), (1 - terminated).reshape(r.shape[0], -1)
    R = torch.zeros_like(r)
    R[:, -1] = r[:, -1] * m[:, -1]
    for t in range(r.shape[1] - 2, -1, -1):
        R[:, t] = (r[:, t] + gamma * R[:, t + 1] * c[:, t]) * m[:, t]
    return R


def td_lambda_torch(r, terminated, padded, q, gamma, td_lambda):
    """DOP's _td_lambda_target (dop.py:192-232) as the reference computes it, on the CPU: the [E, T, T] table of n-step
    returns (entry [:, t, k] = the (k+1)-step return of step t) filled step by step, then the lambda-weighted sum of each row
    in a second loop -- ~T^2 small tensor ops -> [E, T] on q's device.  (The reference repeats every row over the agents
    first; the n columns are identical, so one is computed.)"""
    dev = q.device
    E, T = int(r.shape[0]), int(r.shape[1])
    r, m, c, q = (x.detach().float().reshape(E, T).cpu() for x in (r, 1 - padded, 1 - terminated, q))
    nstep = torch.zeros(E, T, T)
    for t in range(T - 1, -1, -1):
        nstep[:, t, 0] = (r[:, t] + gamma * q[:, t] * c[:, t]) * m[:, t]
        for k in range(1, T - t):
            nstep[:, t, k] = (r[:, t] + gamma * nstep[:, t + 1, k - 1]) * m[:, t]
    out = torch.zeros(E, T)
    for t in range(T):
        acc = torch.zeros(E)
        for k in range(1, T - t):
            acc += pow(td_lambda, k - 1) * nstep[:, t, k - 1]
        out[:, t] = (1 - td_lambda) * acc + pow(td_lambda, T - t - 1) * nstep[:, t, T - t - 1]
    return out.to(dev)


def _policy_logits(net, args, n_agents, batch, T, impl):
    """The actor's outputs [E, T, n, A] over all T steps: actor_inputs' X through unroll_q (the fused recurrence, or the
    reference's step loop)."""
    E = int(batch["u"].shape[0])
    featured = "map" in batch   # map-once: the front end once per (episode, step)
    X = compact_actor_inputs(args, n_agents, batch, net)[0] if featured else actor_inputs(args, n_agents, batch, T)[0]
    return unroll_q(net, X, None, impl, featured).view(T, E, n_agents, -1).transpose(0, 1)


def _prepare(batch, device, max_episode_len, n_agents, n_actions, dtype=torch.float32):
    """device_batch, then the reference's conversion (u -> long, everything else float32: `dtype`, the networks') ->
    (batch, T, u, mask [E, T, 1]).  A map-once batch gains the narrow dense keys (with_narrow_keys), never o / o_next."""
    batch = device_batch(batch, device, max_episode_len)
    batch = {k: (v.long() if k == "u" else v.to(dtype)) for k, v in batch.items()}
    batch = with_narrow_keys(batch, n_agents, n_actions)
    return batch, int(batch["u"].shape[1]), batch["u"], 1 - batch["padded"]


class DOPLearner:
    """policy/dop.py:DOP on the device.  args: the reference's namespace after get_dop_args (seed, lr, critic_lr, td_lambda,
    optimizer, gamma, tau, grad_norm_clip, offpg_hidden_dim, qmix_hidden_dim, two_hyper_layers, hyper_hidden_dim,
    rnn_hidden_dim) and the env fields (apply_env_info).  unroll: "fused" (the critic over all T*E*n rows at once, the actor
    through GRUSequence, the TD(lambda) target from cs_episode_returns; needs the HIP library and a GPU) or "torch" (the
    reference's per-transition loops and its O(T^2) lambda-return, over the same modules; also runs on the CPU).
    conv_impl: the ACTOR's conv front end, as QMixLearner's (the critic reads the raw map through its own linear layer)."""

    def __init__(self, args, device="cuda", unroll="fused", conv_impl="torch"):
        if unroll not in ("fused", "torch"):
            raise ValueError("unroll must be 'fused' or 'torch'")
        self.conv_impl = check_conv_impl(args, device, unroll, conv_impl)
        self.args, self.device, self.unroll = args, torch.device(device), unroll
        self.n_actions, self.n_agents = args.n_actions, args.n_agents
        self.state_shape, self.obs_shape = args.state_shape, args.obs_shape
        self.tau = args.tau
        # s ++ o ++ agent id (dop.py:25).  flight's o also carries the probability map (conv): the critic reads it as it is
        # (the reference counts obs_shape only, so its critic cannot take flight's observations)
        obs_width = self.obs_shape + (args.map_size ** 2 if getattr(args, "conv", False) else 0)
        critic_input_shape = self.state_shape + obs_width + self.n_agents
        # the reference's order (dop.py:30-47): seed, then actor, eval / target critic, eval / target mixer, on the CPU
        torch.manual_seed(args.seed)
        self.actor = AgentRNN(rnn_input_shape(args), args)
        self.eval_critic = OffPGCritic(critic_input_shape, args)
        self.target_critic = OffPGCritic(critic_input_shape, args)
        self.eval_mixer_net = MixerNet(args)
        self.target_mixer_net = MixerNet(args)
        for net in (self.actor, self.eval_critic, self.target_critic, self.eval_mixer_net, self.target_mixer_net):
            net.to(self.device)
        self.actor.conv_impl = self.conv_impl   # read by map_features / unroll_q
        self.model_dir = model_dir(args, "dop")
        self.target_critic.load_state_dict(self.eval_critic.state_dict())
        self.target_mixer_net.load_state_dict(self.eval_mixer_net.state_dict())
        self.actor_params = list(self.actor.parameters())
        self.critic_params = list(self.eval_critic.parameters())
        self.mixer_params = list(self.eval_mixer_net.parameters())
        self.c_params = self.critic_params + self.mixer_params
        self.agent_optimizer = _make_optimizer(args, self.actor_params, args.lr)
        self.critic_optimizer = _make_optimizer(args, self.critic_params, args.critic_lr)
        self.mixer_optimizer = _make_optimizer(args, self.mixer_params, args.critic_lr)
        self.last_critic_grad_norm = self.last_actor_grad_norm = None

    def soft_update(self):
        """dop.py:132-136: critic and mixer only (the actor has no target)."""
        soft_update(((self.eval_critic, self.target_critic), (self.eval_mixer_net, self.target_mixer_net)), self.tau)

    def critic_inputs(self, batch):
        """_get_critic_inputs (dop.py:269-310) for all steps: s ++ o ++ agent id and s_next ++ o_next ++ id, [E, T, n, in].
        The critic reads the raw map as inputs, so a map-once batch is expanded here (expand_compact), for the critic only:
        the actor goes through compact_actor_inputs."""
        if "map" in batch:
            batch = {**batch, **expand_compact(batch, self.n_agents, self.n_actions)}
        o = batch["o"]
        E, T, n = int(o.shape[0]), int(o.shape[1]), self.n_agents
        ids = torch.eye(n, device=o.device, dtype=o.dtype).expand(E, T, n, n)
        s, s_next = (batch[k].unsqueeze(2).expand(E, T, n, self.state_shape) for k in ("s", "s_next"))
        return torch.cat([s, o, ids], 3), torch.cat([s_next, batch["o_next"], ids], 3)

    def critic_q(self, batch):
        """(q_evals, q_targets) [E, T, n, A] (_get_q_values, dop.py:312-335); the target critic runs without a graph."""
        X, X_next = self.critic_inputs(batch)
        if self.unroll == "fused":
            q_eval = self.eval_critic(X)
            with torch.no_grad():
                q_target = self.target_critic(X_next)
            return q_eval, q_target
        E, T, n = X.shape[:3]
        q_eval = torch.stack([self.eval_critic(X[:, t].reshape(E * n, -1)).view(E, n, -1) for t in range(T)], 1)
        with torch.no_grad():
            q_target = torch.stack([self.target_critic(X_next[:, t].reshape(E * n, -1)).view(E, n, -1) for t in range(T)], 1)
        return q_eval, q_target

    def td_lambda_target(self, batch, q_total_target):
        """[E, T] TD(lambda) target of the critic (dop.py:192-232)."""
        a = self.args
        if self.unroll == "fused":
            return episode_returns(batch["r"], batch["terminated"], batch["padded"], q_total_target, a.gamma, a.td_lambda)
        return td_lambda_torch(batch["r"], batch["terminated"], batch["padded"], q_total_target, a.gamma, a.td_lambda)

    def learn(self, batch, max_episode_len=None, train_step=0, epsilon=0.0):
        """One DOP update (dop.py:89-130) on a DeviceReplayBuffer.sample() dict (or a CompactReplayBuffer's) as it is: the critic and mixer step (its TD(lambda)
        loss, one clip over both, soft update), then the actor step with the advantage of the critic's q-values from BEFORE its
        step (dop.py:161).  max_episode_len: as QMixLearner.learn; epsilon: a float or a 0-dim device tensor.  Returns
        (critic_loss, actor_loss) as device tensors (no host synchronisation); the pre-clip norms are last_critic_grad_norm and
        last_actor_grad_norm."""
        batch, T, u, mask1 = _prepare(batch, self.device, max_episode_len, self.n_agents, self.n_actions, self.actor.fc1.weight.dtype)
        E, n = int(u.shape[0]), self.n_agents
        mask = mask1.expand(E, T, n)
        s, s_next = batch["s"], batch["s_next"]

        # critic (_train_critic, dop.py:138-190)
        u_next = torch.cat([u[:, 1:], torch.zeros_like(u[:, :1])], 1)   # zero action after the last step (dop.py:146-148)
        q_evals, q_targets = self.critic_q(batch)
        q_values = q_evals.detach()
        q_total_eval = self.eval_mixer_net(torch.gather(q_evals, dim=3, index=u).squeeze(3), s)
        with torch.no_grad():
            q_total_target = self.target_mixer_net(torch.gather(q_targets, dim=3, index=u_next).squeeze(3), s_next)
        targets = self.td_lambda_target(batch, q_total_target).unsqueeze(2).expand(E, T, n)   # the reference's repeat
        td_error = targets - q_total_eval
        critic_loss = ((mask * td_error) ** 2).sum() / mask.sum()
        self.critic_optimizer.zero_grad()
        self.mixer_optimizer.zero_grad()
        critic_loss.backward()
        self.last_critic_grad_norm = torch.nn.utils.clip_grad_norm_(self.c_params, self.args.grad_norm_clip)
        self.critic_optimizer.step()
        self.mixer_optimizer.step()
        self.soft_update()

        # actor (dop.py:107-130)
        prob = action_prob(_policy_logits(self.actor, self.args, n, batch, T, self.unroll), batch["avail_u"], epsilon)
        q_taken = torch.gather(q_values, dim=3, index=u).squeeze(3)
        baseline = (q_values * prob).sum(dim=3, keepdim=True).squeeze(3).detach()
        advantage = (q_taken - baseline).detach()
        actor_loss = -((advantage * log_pi_taken(prob, u, mask)) * mask).sum() / mask.sum()
        self.agent_optimizer.zero_grad()
        actor_loss.backward()
        self.last_actor_grad_norm = torch.nn.utils.clip_grad_norm_(self.actor_params, self.args.grad_norm_clip)
        self.agent_optimizer.step()
        return critic_loss.detach(), actor_loss.detach()

    def save_model(self, num):
        """dop.py:341-350: <model_dir>/<num>_actor_net_params.pkl, <num>_mixer_net_params.pkl, <num>_critic_net_params.pkl."""
        os.makedirs(self.model_dir, exist_ok=True)
        idx = str(num)
        torch.save(self.actor.state_dict(), os.path.join(self.model_dir, idx + "_actor_net_params.pkl"))
        torch.save(self.eval_mixer_net.state_dict(), os.path.join(self.model_dir, idx + "_mixer_net_params.pkl"))
        torch.save(self.eval_critic.state_dict(), os.path.join(self.model_dir, idx + "_critic_net_params.pkl"))

    def load_model(self, actor_root, critic_root, mixer_root):
        """dop.py:352-357: actor, eval critic and eval mixer from the three files, targets copied from them."""
        self.actor.load_state_dict(torch.load(actor_root, map_location=self.device))
        self.eval_critic.load_state_dict(torch.load(critic_root, map_location=self.device))
        self.eval_mixer_net.load_state_dict(torch.load(mixer_root, map_location=self.device))
        self.target_critic.load_state_dict(self.eval_critic.state_dict())
        self.target_mixer_net.load_state_dict(self.eval_mixer_net.state_dict())


class ReinforceLearner:
    """policy/reinforce.py:Reinforce on the device.  args: the reference's namespace after get_reinforce_args (seed, lr_actor,
    optimizer, gamma, rnn_hidden_dim) and the env fields.  On-policy: `learn` takes the episode dict that
    EpisodeCollector.generate_episodes returns (or a sampled batch).  unroll: "fused" (GRUSequence and cs_episode_returns) or
    "torch" (the reference's step loops).  conv_impl: as QMixLearner's."""

    def __init__(self, args, device="cuda", unroll="fused", conv_impl="torch"):
        if unroll not in ("fused", "torch"):
            raise ValueError("unroll must be 'fused' or 'torch'")
        self.conv_impl = check_conv_impl(args, device, unroll, conv_impl)
        self.args, self.device, self.unroll = args, torch.device(device), unroll
        self.n_actions, self.n_agents = args.n_actions, args.n_agents
        self.state_shape, self.obs_shape = args.state_shape, args.obs_shape
        torch.manual_seed(args.seed)   # reinforce.py:22-31
        self.eval_rnn = AgentRNN(rnn_input_shape(args), args).to(self.device)
        self.eval_rnn.conv_impl = self.conv_impl   # read by map_features / unroll_q
        self.model_dir = model_dir(args, "reinforce")
        self.rnn_parameters = list(self.eval_rnn.parameters())
        self.rnn_optimizer = _make_optimizer(args, self.rnn_parameters, args.lr_actor)

    def get_returns(self, batch):
        """[E, T] discounted return of every step (_get_returns, reinforce.py:101-110)."""
        if self.unroll == "fused":
            return episode_returns(batch["r"], batch["terminated"], batch["padded"], None, self.args.gamma)
        return returns_torch(batch["r"], batch["terminated"], batch["padded"], self.args.gamma)

    def learn(self, batch, max_episode_len=None, train_step=0, epsilon=0.0):
        """One REINFORCE update (reinforce.py:63-99) on a dense or a map-once episode dict: loss = -sum(R log pi(u) m) / sum(m), Adam or RMSprop, no gradient clipping
        (reinforce.py:97 has it commented out).  Returns the loss as a device tensor (no host synchronisation)."""
        batch, T, u, mask1 = _prepare(batch, self.device, max_episode_len, self.n_agents, self.n_actions, self.eval_rnn.fc1.weight.dtype)
        E, n = int(u.shape[0]), self.n_agents
        mask = mask1.expand(E, T, n)
        n_return = self.get_returns(batch).unsqueeze(2).expand(E, T, n)
        prob = action_prob(_policy_logits(self.eval_rnn, self.args, n, batch, T, self.unroll), batch["avail_u"], epsilon)
        loss = -((n_return * log_pi_taken(prob, u, mask)) * mask).sum() / mask.sum()
        self.rnn_optimizer.zero_grad()
        loss.backward()
        self.rnn_optimizer.step()
        return loss.detach()

    def save_model(self, num):
        """<model_dir>/<num>_rnn_net_params.pkl, the reference's file (reinforce.py:158-164 numbers it itself)."""
        os.makedirs(self.model_dir, exist_ok=True)
        torch.save(self.eval_rnn.state_dict(), os.path.join(self.model_dir, str(num) + "_rnn_net_params.pkl"))

    def load_model(self, rnn_root):
        self.eval_rnn.load_state_dict(torch.load(rnn_root, map_location=self.device))


# ---- PPO with a central value function (MAPPO): no counterpart in the reference ----------------------------------------------

def get_ppo_args(args, seed=None):
    """The learner fields of PPOLearner on an argparse-style namespace, shaped like get_reinforce_args (on-policy, the same
    actor); seed as get_dop_args.  Exploration comes from the sampled softmax policy itself: epsilon stays 0."""
    args.off_policy = False
    args.rnn_hidden_dim, args.critic_dim = 64, 128
    args.lr_actor, args.lr_critic, args.gae_lambda = 5e-4, 1e-3, 0.95
    args.ppo_clip, args.ppo_epochs, args.ppo_minibatches, args.ppo_entropy, args.ppo_norm_adv = 0.2, 4, 1, 0.01, True
    args.gamma, args.optimizer = getattr(args, "gamma", 0.99), getattr(args, "optimizer", "Adam")
    args.epsilon, args.anneal_epsilon, args.min_epsilon, args.epsilon_anneal_scale = 0, 0, 0, "epoch"
    args.grad_norm_clip, args.n_episodes, args.evaluate_cycle, args.save_cycle = 10, 1, 200, 500
    if seed is not None:
        args.seed = seed
    return args


class ValueCritic(nn.Module):
    """The central value function: state -> relu(fc1) -> relu(fc2) -> fc3 = V(s), one value per (episode, step)."""

    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.fc1 = nn.Linear(input_shape, args.critic_dim)
        self.fc2 = nn.Linear(args.critic_dim, args.critic_dim)
        self.fc3 = nn.Linear(args.critic_dim, 1)

    def forward(self, state):
        return self.fc3(F.relu(self.fc2(F.relu(self.fc1(state)))))


def gae(r, terminated, padded, v, v_next, gamma=0.99, gae_lambda=0.95):
    """cs_gae (csrc/ppo.h) on device tensors: r, terminated, padded, v = V(s), v_next = V(s_next) [E, T] or [E, T, 1] float32
    -> (adv, ret) [E, T]: generalised advantage estimates and the value targets adv + v, zero on padded steps.  One launch."""
    E, T = int(r.shape[0]), int(r.shape[1])
    flat = lambda x: x.detach().float().reshape(E, T).contiguous()
    adv = torch.empty(E, T, dtype=torch.float32, device=r.device)
    ret = torch.empty_like(adv)
    _lib.torch_ops().gae(flat(r), flat(terminated), flat(padded), flat(v), flat(v_next), E, T, float(gamma), float(gae_lambda), adv, ret)
    return adv, ret


def gae_torch(r, terminated, padded, v, v_next, gamma, gae_lambda):
    """cs_gae's recursion one step at a time, t = T-1 .. 0, in its evaluation order (csrc/ppo.h) -> (adv, ret) [E, T]."""
    E = r.shape[0]
    r, v, v_next = r.reshape(E, -1), v.reshape(E, -1), v_next.reshape(E, -1)
    m, c = (1 - padded).reshape(E, -1), (1 - terminated).reshape(E, -1)
    gl = torch.tensor(gamma, dtype=r.dtype) * torch.tensor(gae_lambda, dtype=r.dtype)   # rounded once, in r's precision
    gl = gl.to(r.device)
    delta = (r + (gamma * v_next) * c) - v
    adv = torch.zeros_like(r)
    adv[:, -1] = delta[:, -1] * m[:, -1]
    for t in range(r.shape[1] - 2, -1, -1):
        adv[:, t] = (delta[:, t] + (gl * adv[:, t + 1]) * c[:, t]) * m[:, t]
    return adv, (adv + v) * m


def ppo_policy_loss_torch(logits, avail_u, u, old_logp, adv, mask, clip, ent_coef, epsilon):
    """PPO's actor loss in plain autograd, over action_prob / log_pi_taken: logits, avail_u [E, T, n, A], u [E, T, n, 1]
    long, old_logp [E, T, n], adv, mask [E, T] (or [E, T, 1]) -> (loss, stats [4]).  loss = policy loss - ent_coef * mean
    entropy; stats = (policy loss = -mean min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv), mean entropy, fraction of
    rows whose ratio lies outside the clip range, mean(old_logp - logp)), means over the n * sum(mask) live rows; detached."""
    E, T, n = logits.shape[:3]
    m = mask.reshape(E, T, 1).expand(E, T, n)
    a = adv.reshape(E, T, 1)
    prob = action_prob(logits, avail_u, epsilon)
    logp = log_pi_taken(prob, u, m)
    ratio = torch.exp(logp - old_logp)
    surr = torch.minimum(ratio * a, torch.clamp(ratio, 1 - clip, 1 + clip) * a)
    entropy = -(prob * torch.log(prob.masked_fill(prob <= 0, 1.0))).sum(dim=-1)   # 0 log 0 = 0
    inv_count = 1 / (n * mask.sum())
    policy_loss = -(surr * m).sum() * inv_count
    mean_entropy = (entropy * m).sum() * inv_count
    outside = ((ratio < 1 - clip) | (ratio > 1 + clip)).to(logits.dtype)
    stats = torch.stack([policy_loss, mean_entropy, (outside * m).sum() * inv_count, ((old_logp - logp) * m).sum() * inv_count])
    return policy_loss - ent_coef * mean_entropy, stats.detach()


def _ppo_rows(logits, avail_u, u, mask, epsilon):
    """cs_ppo_loss's view of the tensors above: (logits, avail [R, A], u [R], mask [E*T], rows, n, A, epsilon, epsilon_t)."""
    E, T, n, A = (int(x) for x in logits.shape)
    f32 = lambda x, *shape: x.detach().float().reshape(*shape).contiguous()
    eps_t = f32(epsilon, -1)[:1] if torch.is_tensor(epsilon) else None   # a device scalar stays on the device
    return (f32(logits, E * T * n, A), f32(avail_u, E * T * n, A), u.detach().reshape(E * T * n).contiguous(), f32(mask, E * T),
            E * T * n, n, A, 0.0 if eps_t is not None else float(epsilon), eps_t)


def ppo_logp(logits, avail_u, u, mask, epsilon):
    """log pi(u) [E, T, n] of the action probabilities (action_prob / log_pi_taken; 0 on padded steps) from cs_ppo_loss's
    no-grad mode: the instructions that compute logp inside PPOPolicyLoss, so an unchanged policy has ratio exactly 1."""
    z, av, uu, m, rows, n, A, eps, eps_t = _ppo_rows(logits, avail_u, u, mask, epsilon)
    out = z.new_empty(rows)
    _lib.torch_ops().ppo_loss(z, av, uu, None, None, m, rows, n, A, 0.0, 0.0, eps, eps_t, None, None, out, None, None)
    return out.view(logits.shape[:3])


PPO_BLOCK = 256   # CS_PPO_BLOCK of include/coopsearch.h: rows per partial of cs_ppo_loss's scratch buffer


class PPOPolicyLoss(torch.autograd.Function):
    """ppo_policy_loss_torch on cs_ppo_loss (csrc/ppo.h): (logits, avail_u, u, old_logp, adv, mask, clip, ent_coef, epsilon,
    inv_count) -> (loss, stats [4]); inv_count: the device scalar 1 / (n * sum(mask)).  One pass over the rows computes the
    loss's sums and dloss/dlogits; backward is grad_out * dlogits.  stats carry no gradient."""

    @staticmethod
    def forward(ctx, logits, avail_u, u, old_logp, adv, mask, clip, ent_coef, epsilon, inv_count):
        z, av, uu, m, rows, n, A, eps, eps_t = _ppo_rows(logits, avail_u, u, mask, epsilon)
        f32 = lambda x, k: x.detach().float().reshape(k).contiguous()
        dlogits, stats = torch.empty_like(z), z.new_empty(4)
        scratch = z.new_empty(4 * ((rows + PPO_BLOCK - 1) // PPO_BLOCK))
        _lib.torch_ops().ppo_loss(z, av, uu, f32(old_logp, rows), f32(adv, rows // n), m, rows, n, A, float(clip), float(ent_coef), eps, eps_t,
                        f32(inv_count, 1), dlogits, None, stats, scratch)
        ctx.save_for_backward(dlogits.view(logits.shape))
        ctx.mark_non_differentiable(stats)
        return stats[0] - float(ent_coef) * stats[1], stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        (dlogits,) = ctx.saved_tensors
        return (grad_loss * dlogits,) + (None,) * 9


class PPOLearner:
    """A clipped-surrogate actor-critic with a central value function (PPO; MAPPO for the team) on the device.  args: the
    namespace after get_ppo_args (seed, lr_actor, lr_critic, gamma, gae_lambda, ppo_clip, ppo_epochs, ppo_minibatches,
    ppo_entropy, ppo_norm_adv, grad_norm_clip, critic_dim, rnn_hidden_dim, optimizer) and the env fields.  On-policy: `learn`
    takes the episode dict that EpisodeCollector.generate_episodes returns and reuses it for ppo_epochs epochs.  The actor is
    REINFORCE's (the same initial parameters for the same seed, the same checkpoint file).  unroll: "fused" (GRUSequence,
    cs_gae, cs_ppo_loss; needs the HIP library and a GPU) or "torch" (the reference-style step loops and plain autograd over
    the same modules; also runs on the CPU).  conv_impl: as QMixLearner's."""

    def __init__(self, args, device="cuda", unroll="fused", conv_impl="torch"):
        if unroll not in ("fused", "torch"):
            raise ValueError("unroll must be 'fused' or 'torch'")
        self.conv_impl = check_conv_impl(args, device, unroll, conv_impl)
        self.args, self.device, self.unroll = args, torch.device(device), unroll
        self.n_actions, self.n_agents = args.n_actions, args.n_agents
        self.state_shape, self.obs_shape = args.state_shape, args.obs_shape
        torch.manual_seed(args.seed)   # the actor first: ReinforceLearner's initial parameters
        self.eval_rnn = AgentRNN(rnn_input_shape(args), args).to(self.device)
        self.critic = ValueCritic(self.state_shape, args).to(self.device)
        self.eval_rnn.conv_impl = self.conv_impl   # read by map_features / unroll_q
        self.model_dir = model_dir(args, "ppo")
        self.rnn_parameters = list(self.eval_rnn.parameters())
        self.critic_parameters = list(self.critic.parameters())
        self.rnn_optimizer = _make_optimizer(args, self.rnn_parameters, args.lr_actor)
        self.critic_optimizer = _make_optimizer(args, self.critic_parameters, args.lr_critic)
        self.last_actor_grad_norm = self.last_critic_grad_norm = None

    def advantages(self, batch, v, v_next):
        """(adv, ret) [E, T] from the batch's rewards and the critic's values (no graph)."""
        a = self.args
        fn = gae if self.unroll == "fused" else gae_torch
        return fn(batch["r"], batch["terminated"], batch["padded"], v, v_next, a.gamma, a.gae_lambda)

    def policy_loss(self, logits, avail_u, u, old_logp, adv, mask, epsilon):
        """(loss, stats [4]) of one group of episodes: PPOPolicyLoss, or its plain-autograd twin."""
        a = self.args
        if self.unroll == "fused":
            inv_count = 1 / (self.n_agents * mask.sum())
            return PPOPolicyLoss.apply(logits, avail_u, u, old_logp, adv, mask, a.ppo_clip, a.ppo_entropy, epsilon, inv_count)
        return ppo_policy_loss_torch(logits, avail_u, u, old_logp, adv, mask, a.ppo_clip, a.ppo_entropy, epsilon)

    def learn(self, batch, max_episode_len=None, train_step=0, epsilon=0.0):
        """ppo_epochs x ppo_minibatches updates of the actor and the critic on a dense or a map-once episode dict.  Once, without
        a graph: V(s), V(s_next), log pi_old(u), the advantages and value targets (GAE), the advantages standardised over the
        live steps when args.ppo_norm_adv.  Then every epoch splits the episodes into ppo_minibatches groups of whole episodes
        (torch.randperm on the device's global generator; no draw for one group) and steps both networks on each: the actor
        on the clipped surrogate minus ppo_entropy * entropy, the critic on 0.5 sum((V(s) - ret)^2 m) / sum(m), each clipped
        to grad_norm_clip.  epsilon: a float or a device scalar (action_prob's mix).  Returns a device tensor [ppo_epochs, 5]:
        policy loss, mean entropy, clip fraction, mean(log pi_old - log pi), value loss, averaged over the epoch's groups (no
        host synchronisation)."""
        a, n = self.args, self.n_agents
        batch, T, u, mask1 = _prepare(batch, self.device, max_episode_len, n, self.n_actions, self.eval_rnn.fc1.weight.dtype)
        E = int(u.shape[0])
        mask = mask1.reshape(E, T)
        fused = self.unroll == "fused"
        with torch.no_grad():
            v, v_next = self.critic(batch["s"]).reshape(E, T), self.critic(batch["s_next"]).reshape(E, T)
            logits = _policy_logits(self.eval_rnn, a, n, batch, T, self.unroll)
            if fused:
                old_logp = ppo_logp(logits, batch["avail_u"], u, mask, epsilon)
            else:
                old_logp = log_pi_taken(action_prob(logits, batch["avail_u"], epsilon), u, mask1.expand(E, T, n))
            adv, ret = self.advantages(batch, v, v_next)
            if a.ppo_norm_adv:
                count = mask.sum()
                mean = (adv * mask).sum() / count
                std = ((((adv - mean) * mask) ** 2).sum() / count).sqrt()
                adv = (adv - mean) / (std + 1e-8) * mask
        groups = int(a.ppo_minibatches)
        out = []
        for _ in range(int(a.ppo_epochs)):
            parts = [None] if groups == 1 else torch.randperm(E, device=self.device).chunk(groups)
            rows = []
            for idx in parts:
                take = (lambda x: x) if idx is None else (lambda x: x.index_select(0, idx))
                b = batch if idx is None else {k: take(x) for k, x in batch.items()}
                m = take(mask)
                logits = _policy_logits(self.eval_rnn, a, n, b, T, self.unroll)
                loss, stats = self.policy_loss(logits, b["avail_u"], b["u"], take(old_logp), take(adv), m, epsilon)
                self.rnn_optimizer.zero_grad()
                loss.backward()
                self.last_actor_grad_norm = torch.nn.utils.clip_grad_norm_(self.rnn_parameters, a.grad_norm_clip)
                self.rnn_optimizer.step()
                value = self.critic(b["s"]).reshape(m.shape)
                value_loss = 0.5 * (((value - take(ret)) * m) ** 2).sum() / m.sum()
                self.critic_optimizer.zero_grad()
                value_loss.backward()
                self.last_critic_grad_norm = torch.nn.utils.clip_grad_norm_(self.critic_parameters, a.grad_norm_clip)
                self.critic_optimizer.step()
                rows.append(torch.cat([stats, value_loss.detach().reshape(1)]))
            out.append(rows[0] if len(rows) == 1 else torch.stack(rows).mean(0))
        return torch.stack(out)

    def save_model(self, num):
        """<model_dir>/<num>_rnn_net_params.pkl (the reference's actor file: its loader and Runner.replay read it) and
        <num>_critic_net_params.pkl."""
        os.makedirs(self.model_dir, exist_ok=True)
        torch.save(self.eval_rnn.state_dict(), os.path.join(self.model_dir, str(num) + "_rnn_net_params.pkl"))
        torch.save(self.critic.state_dict(), os.path.join(self.model_dir, str(num) + "_critic_net_params.pkl"))

    def load_model(self, rnn_root, critic_root):
        self.eval_rnn.load_state_dict(torch.load(rnn_root, map_location=self.device))
        self.critic.load_state_dict(torch.load(critic_root, map_location=self.device))
