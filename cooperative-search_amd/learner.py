"""QMIX learner on the device: the consumer of DeviceReplayBuffer.sample() (policy/qmix.py of the reference).

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
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .agents import AgentRNN, rnn_input_shape

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


def _ops():
    from . import _lib
    return _lib.torch_ops()


def _gru_forward(gi, w_hh, b_hh, h0, save):
    """cs_gru_seq_forward on torch tensors -> (H [T, R, 64], saved [T, R, 4, 64] or None)."""
    T, R = int(gi.shape[0]), int(gi.shape[1])
    if gi.shape[2] != 3 * HIDDEN or tuple(w_hh.shape) != (3 * HIDDEN, HIDDEN):
        raise ValueError(f"GRUSequence: gi must be [T, R, {3 * HIDDEN}] and w_hh [{3 * HIDDEN}, {HIDDEN}]")
    gi, w_hh, b_hh = gi.detach().contiguous(), w_hh.detach().contiguous(), b_hh.detach().contiguous()
    h0 = None if h0 is None else h0.detach().contiguous()
    H = gi.new_empty(T, R, HIDDEN)
    saved = gi.new_empty(T, R, 4, HIDDEN) if save else None
    _ops().gru_seq_forward(w_hh, b_hh, gi, h0, T, R, H, saved)
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
        _ops().gru_seq_backward(w_hh, dH.contiguous(), H, h0, saved, T, R, dgi, dgh, dh0)
        dgh2 = dgh.view(T * R, 3 * HIDDEN)
        dw = db = None
        if need_w:
            first = h0.unsqueeze(0) if h0 is not None else H.new_zeros(1, R, HIDDEN)
            h_prev = torch.cat([first, H[:-1]], 0).view(T * R, HIDDEN)
            dw = dgh2.t() @ h_prev
        if need_b:
            db = dgh2.sum(0)
        return (dgi if need_gi else None), dw, db, dh0


def unroll_q(net, X, h0=None, impl="fused"):
    """Q-values of all T steps: X [T, R, in] (rows of get_inputs, policy/qmix.py:132-158), h0 [R, 64] or None (zeros) ->
    q [T, R, n_actions].  impl "fused": the conv front end (flight), fc1 and the input projection over all T*R rows at once,
    GRUSequence, then fc2 over all rows; "torch": the reference's loop of net(x_t, h) over t (get_q_values)."""
    T, R = int(X.shape[0]), int(X.shape[1])
    if impl == "torch":
        h = h0 if h0 is not None else X.new_zeros(R, net.args.rnn_hidden_dim)
        qs = []
        for t in range(T):
            q, h = net(X[t], h)
            qs.append(q)
        return torch.stack(qs, 0)
    if impl != "fused":
        raise ValueError("impl must be 'fused' or 'torch'")
    if net.args.rnn_hidden_dim != HIDDEN:
        raise ValueError(f"the fused unroll is built for rnn_hidden_dim = {HIDDEN}")
    x = X.reshape(T * R, -1)
    if net.args.conv:   # the same modules on the same maps as AgentRNN.forward, all T*R maps in one call
        cells = net.args.map_size ** 2
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


class QMixLearner:
    """policy/qmix.py:QMIX on the device.  args: the reference's namespace after get_mixer_args (seed, lr, optimizer, gamma,
    tau, grad_norm_clip, qmix_hidden_dim, two_hyper_layers, hyper_hidden_dim, rnn_hidden_dim) and the env fields
    (apply_env_info).  unroll: "fused" (GRUSequence, needs the HIP library and a GPU) or "torch" (the reference's loop)."""

    def __init__(self, args, device="cuda", unroll="fused"):
        if unroll not in ("fused", "torch"):
            raise ValueError("unroll must be 'fused' or 'torch'")
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
        self.model_dir = (getattr(args, "model_dir", "./model/") + args.env + "_Seed" + str(args.seed) + "_" +
                          getattr(args, "alg", "qmix") + "_{}a{}t(AM{}TM{})".format(args.n_agents, getattr(args, "target_num", 15),
                                                                                   getattr(args, "agent_mode", 0),
                                                                                   getattr(args, "target_mode", 0)))
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
        with torch.no_grad():
            for ev, tg in ((self.eval_rnn, self.target_rnn), (self.eval_qmix_net, self.target_qmix_net)):
                e, t = list(ev.parameters()), list(tg.parameters())
                new = torch._foreach_mul(e, self.tau)
                torch._foreach_add_(new, torch._foreach_mul(t, 1 - self.tau))
                torch._foreach_copy_(t, new)

    def get_inputs(self, batch, T):
        """_get_inputs (qmix.py:132-158) for all T steps at once: X, X_next [T, E*n, in], row e*n + agent.
        inputs = obs ++ previous one-hot action (zeros at t = 0) ++ agent id; inputs_next = obs_next ++ this step's one-hot ++ id."""
        o, o_next, u_onehot = batch["o"], batch["o_next"], batch["u_onehot"]
        E, n = int(o.shape[0]), self.n_agents
        parts, parts_next = [o], [o_next]
        if getattr(self.args, "last_action", True):
            parts.append(torch.cat([torch.zeros_like(u_onehot[:, :1]), u_onehot[:, :-1]], 1))
            parts_next.append(u_onehot)
        if getattr(self.args, "reuse_network", True):
            ids = torch.eye(n, device=o.device, dtype=o.dtype).expand(E, T, n, n)
            parts.append(ids)
            parts_next.append(ids)
        X = torch.cat(parts, 3).transpose(0, 1).reshape(T, E * n, -1)
        X_next = torch.cat(parts_next, 3).transpose(0, 1).reshape(T, E * n, -1)
        return X, X_next

    def get_q_values(self, batch, T):
        """(q_evals, q_targets) [E, T, n, n_actions] (qmix.py:160-182); the target network runs without a graph."""
        E, n = int(batch["o"].shape[0]), self.n_agents
        X, X_next = self.get_inputs(batch, T)
        self.init_hidden(E)
        q_eval = unroll_q(self.eval_rnn, X, None, self.unroll)
        with torch.no_grad():
            q_target = unroll_q(self.target_rnn, X_next, None, self.unroll)
        shape = (T, E, n, self.n_actions)
        return q_eval.view(shape).transpose(0, 1), q_target.view(shape).transpose(0, 1)

    def learn(self, batch, max_episode_len=None, train_step=0, epsilon=None):
        """One QMIX update (qmix.py:85-130) on a DeviceReplayBuffer.sample() dict as it is ([E, T, ...] float32; `u` is cast to
        long).  max_episode_len: cut every key to that many steps (what agent.py:112-122 does before calling learn); None = the
        full T, which is what the reference's _get_max_episode_len amounts to (it never shortens T).  Returns the loss (a device
        tensor: no host synchronisation)."""
        if max_episode_len is not None:
            batch = {k: v[:, :max_episode_len] for k, v in batch.items()}
        batch = {k: torch.as_tensor(v, device=self.device) for k, v in batch.items()}
        T = int(batch["o"].shape[1])
        u = batch["u"].long()
        s, s_next, r = batch["s"].float(), batch["s_next"].float(), batch["r"].float()
        avail_u_next, terminated = batch["avail_u_next"], batch["terminated"].float()
        batch = {k: (v.float() if k in ("o", "o_next", "u_onehot") else v) for k, v in batch.items()}
        mask = 1 - batch["padded"].float()

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
