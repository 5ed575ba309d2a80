"""Fused policy kernel (csrc/policy.hip, row f3) against the torch fp32 module of the same network, and against the
reference's own forward through the committed rnn_forward fixture."""
import os

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd.agents import AgentRNN, BatchedAgents, FusedAgents, rnn_input_shape

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2e-5  # fp32, different summation order (MFMA k-blocking) and expf/tanhf implementations


def _args(n=3):
    a = cs.make_env_args("flight_easy", n_agents=n)
    a.n_actions, a.obs_shape, a.rnn_hidden_dim, a.conv, a.last_action, a.reuse_network = 3, 4, 64, False, True, True
    return a


@pytest.mark.parametrize("n,B", [(3, 1), (3, 37), (5, 1000), (1, 64), (8, 129)])
def test_fused_forward_matches_torch_module(n, B):
    torch.manual_seed(n * 100 + B)
    a = _args(n)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    for p in net.parameters():  # larger weights than the default init so that every gate is exercised
        p.data.mul_(3.0)
    fused = FusedAgents(a, B, net=net)
    ref = BatchedAgents(a, B, net=net)
    last = torch.zeros(B, n, a.n_actions, device="cuda")
    for t in range(6):
        obs = torch.rand(B, n, 4, device="cuda") * 2 - 0.5
        act = fused.choose_action(obs, want_q=True).clone()
        x = torch.cat([obs, last, ref.agent_ids], 2).reshape(B * n, -1)
        with torch.no_grad():
            q_ref, ref.hidden = net(x, ref.hidden)
        q_ref = q_ref.reshape(B, n, -1)
        assert torch.allclose(fused.q, q_ref, atol=TOL, rtol=TOL), (t, (fused.q - q_ref).abs().max().item())
        assert torch.allclose(fused.hidden, ref.hidden, atol=TOL, rtol=TOL)
        top2 = q_ref.topk(2, dim=2).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-3
        assert (act == q_ref.argmax(2))[clear].all()
        ref.hidden = fused.hidden.clone()  # keep the two recurrences on the same state
        last = torch.nn.functional.one_hot(act, a.n_actions).float()


def test_activations_beyond_the_fp16_range_saturate_instead_of_turning_into_nan():
    """split_f16 (csrc/policy_dev.h) carries a float as hi = fp16(v), lo = fp16((v - hi) * 2048); above 65504 hi was inf
    and lo NaN, and every q-value of the row NaN.  Activations now saturate at +-65504 (one v_med3_f32 per conversion): with an fc1
    unit driven to 1e5 the kernel's q-values and hidden state are finite and equal those of the torch fp32 module whose relu output
    is clamped at 65504 -- and differ from the unclamped module's, i.e. the saturating unit does matter in this network.
    Reference network: /root/reference/network/base_net.py:5-46 (fc1 -> relu -> GRUCell -> fc2)."""
    torch.manual_seed(11)
    a = _args(3)
    B = 64
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    with torch.no_grad():
        net.fc1.weight[0].zero_()
        net.fc1.bias[0] = 1.0e5                 # relu(fc1 x)[0] = 1e5 for every row: beyond fp16's 65504
        net.rnn.weight_ih[:, 0] = torch.randn(3 * a.rnn_hidden_dim, device="cuda") * 1.0e-5   # ... weighted so that it moves the gates by O(1)
    fused = FusedAgents(a, B, net=net)
    ref = BatchedAgents(a, B, net=net)
    last = torch.zeros(B, 3, a.n_actions, device="cuda")
    for t in range(4):
        obs = torch.rand(B, 3, 4, device="cuda") * 2 - 0.5
        act = fused.choose_action(obs, want_q=True).clone()
        assert torch.isfinite(fused.q).all() and torch.isfinite(fused.hidden).all(), t
        x = torch.cat([obs, last, ref.agent_ids], 2).reshape(B * 3, -1)
        with torch.no_grad():
            x1 = torch.relu(net.fc1(x))
            assert float(x1[:, 0].min()) > 7.0e4
            h_sat = net.rnn(x1.clamp(max=65504.0), ref.hidden.reshape(-1, a.rnn_hidden_dim))
            q_sat = net.fc2(h_sat).reshape(B, 3, -1)
            h_raw = net.rnn(x1, ref.hidden.reshape(-1, a.rnn_hidden_dim))
        assert torch.allclose(fused.q, q_sat, atol=5e-5, rtol=5e-5), (t, (fused.q - q_sat).abs().max().item())
        assert torch.allclose(fused.hidden.reshape(h_sat.shape), h_sat, atol=5e-5, rtol=5e-5)
        assert (h_raw - h_sat).abs().max().item() > 1e-2      # the clamp is not a no-op here
        ref.hidden = fused.hidden.clone()
        last = torch.nn.functional.one_hot(act, a.n_actions).float()


def test_fused_forward_matches_reference_fixture():
    """tests/golden/rnn_forward.npz holds the reference RNN's own (fp64) outputs for a seeded state_dict and random
    full-width input rows: the kernel's raw-input mode reproduces them to fp32 accuracy."""
    z = np.load(os.path.join(GOLD, "rnn_forward.npz"))
    a = _args(3)
    net = AgentRNN(10, a).cuda()
    net.load_state_dict({k[len("easy_w_"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("easy_w_")})
    x = torch.from_numpy(z["easy_x"]).float().cuda()
    rows = x.shape[0]
    fused = FusedAgents(a, rows // 3, net=net)
    fused.hidden.copy_(torch.from_numpy(z["easy_h"]).float().cuda())
    act = fused.forward_raw(x, want_q=True)
    assert np.allclose(fused.q.reshape(rows, -1).cpu().numpy(), z["easy_q"], atol=TOL, rtol=TOL)
    assert np.allclose(fused.hidden.cpu().numpy(), z["easy_h2"], atol=TOL, rtol=TOL)
    assert np.array_equal(act.reshape(-1).cpu().numpy(), z["easy_q"].argmax(1))


def test_epsilon_greedy_statistics_and_determinism():
    a = _args(3)
    B = 20000
    fused = FusedAgents(a, B, seed=7)
    obs = torch.rand(B, 3, 4, device="cuda")
    greedy = fused.choose_action(obs, evaluate=True).clone()
    fused.init_hidden()
    fused.calls = 0
    eps = fused.choose_action(obs, epsilon=0.3).clone()
    fused.init_hidden()
    fused.calls = 0
    again = fused.choose_action(obs, epsilon=0.3).clone()
    assert torch.equal(eps, again)
    # P(changed) = eps * (1 - 1/A) = 0.2
    changed = (eps != greedy).float().mean().item()
    assert abs(changed - 0.2) < 0.01
    fused.init_hidden()
    full = fused.choose_action(obs, epsilon=1.0)
    counts = torch.bincount(full.flatten(), minlength=3).float() / full.numel()
    assert (counts - 1 / 3).abs().max() < 0.01


def test_closed_loop_with_fused_agents_matches_batched_agents():
    a = _args(3)
    B = 512
    torch.manual_seed(0)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    for p in net.parameters():
        p.data.mul_(4.0)
    res = []
    for cls in (FusedAgents, BatchedAgents):
        env = cs.BatchedFlightEnv(a, batch=B, freeze_done=True)
        ag = cls(a, B, net=net)
        last = torch.zeros(B, 3, a.n_actions, device="cuda")
        total = torch.zeros(B, device="cuda")
        for t in range(60):
            obs = env.get_obs()
            act = ag.choose_action(obs) if cls is FusedAgents else ag.choose_action(obs, last, evaluate=True)
            last = torch.nn.functional.one_hot(act, a.n_actions).float()
            r, _, _ = env.step(act)
            total += r
        res.append((total.clone(), env.target_find.clone()))
    # near-ties in q may flip a handful of envs; the bulk must agree exactly
    same = (res[0][0] == res[1][0]) & (res[0][1] == res[1][1])
    assert same.float().mean().item() > 0.97


def test_collector_and_evaluate_accept_the_fused_policy():
    a = _args(3)
    B = 256
    env = cs.BatchedFlightEnv(a, batch=B, freeze_done=True)
    cs.apply_env_info(a, env)
    torch.manual_seed(1)
    fused = FusedAgents(a, B)
    col = cs.EpisodeCollector(env)
    ep, rew, win, found = col.generate_episodes(policy=fused.policy(0.0, True))
    # the zero-copy path (policy kernel and env step write straight into the episode tables) gives the same batch
    env.seed(np.arange(B))
    ep_a, rew_a, win_a, found_a = col.generate_episodes(policy=fused.policy(0.0, True), init=True)
    env.seed(np.arange(B))
    ep_b, rew_b, win_b, found_b = col.generate_episodes(agents=fused, init=True)                      # one launch
    env.seed(np.arange(B))
    ep_c, rew_c, win_c, found_c = col.generate_episodes(agents=fused, init=True, one_launch=False)   # two per step
    for k in ep_a:
        assert torch.equal(ep_a[k], ep_b[k]), k
        assert torch.equal(ep_a[k], ep_c[k]), k
    assert torch.equal(rew_a, rew_b) and torch.equal(win_a, win_b) and torch.equal(found_a, found_b)
    assert torch.equal(env.get_obs(), ep_b["o_next"][:, -1]) or bool((ep_b["padded"][:, -1] == 1).any())
    assert ep["u"].shape[:3] == (B, a.episode_limit, 3) and ep["u"].min() >= 0 and ep["u"].max() <= 2
    # the recorded actions are what the network picks for the recorded observations (replay through the torch module)
    ref = BatchedAgents(a, B, net=fused.net)
    last = torch.zeros(B, 3, 3, device="cuda")
    agree, total = 0, 0
    for t in range(20):
        act = ref.choose_action(ep["o"][:, t], last, evaluate=True)
        agree += (act == ep["u"][:, t, :, 0].long()).sum().item()
        total += act.numel()
        last = torch.nn.functional.one_hot(ep["u"][:, t, :, 0].long(), 3).float()
    assert agree / total > 0.99
    win_rate, episode_reward, targets_find = cs.evaluate(env, fused.policy(0.0, True))
    assert 0.0 <= win_rate <= 1.0 and 0.0 <= targets_find <= 15.0


# ---- flight: conv front end (k_conv_features) + 26-wide fc1 -----------------------------------------------------------

def _flight_args(n=3):
    a = cs.make_env_args("flight", n_agents=n)
    a.n_actions, a.obs_shape, a.rnn_hidden_dim, a.last_action, a.reuse_network = 3, 4, 64, True, True
    return a


def test_flight_fused_forward_matches_reference_fixture():
    """The reference's own conv RNN outputs (fp64) for seeded weights and random 2510-wide rows (one map per row)."""
    z = np.load(os.path.join(GOLD, "rnn_forward.npz"))
    a = _flight_args(3)
    net = AgentRNN(26, a).cuda()
    net.load_state_dict({k[len("flight_w_"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("flight_w_")})
    x = torch.from_numpy(z["flight_x"]).float().cuda()
    rows = x.shape[0]
    fused = FusedAgents(a, rows // 3, net=net)
    fused.hidden.copy_(torch.from_numpy(z["flight_h"]).float().cuda())
    act = fused.forward_raw(x, want_q=True)
    assert np.allclose(fused.q.reshape(rows, -1).cpu().numpy(), z["flight_q"], atol=TOL, rtol=TOL)
    assert np.allclose(fused.hidden.cpu().numpy(), z["flight_h2"], atol=TOL, rtol=TOL)
    assert np.array_equal(act.reshape(-1).cpu().numpy(), z["flight_q"].argmax(1))


@pytest.mark.parametrize("n,B", [(3, 1), (3, 50), (5, 33)])
def test_flight_fused_forward_matches_torch_module(n, B):
    torch.manual_seed(7 * n + B)
    a = _flight_args(n)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    for p in net.parameters():
        p.data.mul_(2.0)
    fused = FusedAgents(a, B, net=net)
    ref = BatchedAgents(a, B, net=net)
    last = torch.zeros(B, n, 3, device="cuda")
    for t in range(4):
        maps = torch.rand(B, 1, 2500, device="cuda").expand(B, n, 2500)       # one map per env, as get_obs gives
        obs = torch.cat([maps, torch.rand(B, n, 4, device="cuda")], 2).contiguous()
        act = fused.choose_action(obs, want_q=True).clone()
        x = torch.cat([obs, last, ref.agent_ids], 2).reshape(B * n, -1)
        with torch.no_grad():
            q_ref, ref.hidden = net(x, ref.hidden)
        q_ref = q_ref.reshape(B, n, -1)
        assert torch.allclose(fused.q, q_ref, atol=5 * TOL, rtol=5 * TOL), (t, (fused.q - q_ref).abs().max().item())
        assert torch.allclose(fused.hidden, ref.hidden, atol=5 * TOL, rtol=5 * TOL)
        # the conv features themselves
        with torch.no_grad():
            f_ref = net.linear(net.conv(obs[:, 0, :2500].reshape(B, 1, 50, 50)).reshape(B, -1))
        assert torch.allclose(fused.feat, f_ref, atol=5 * TOL, rtol=5 * TOL)
        clear = (q_ref.topk(2, dim=2).values.diff(dim=2).abs()[..., 0]) > 1e-3
        assert (act == q_ref.argmax(2))[clear].all()
        ref.hidden = fused.hidden.clone()
        last = torch.nn.functional.one_hot(act, 3).float()


# ---- the persistent grids beyond one trip (cs_policy_forward / cs_policy_conv_features: grid = min(work, resident blocks)) ----
# A CU holds at most 32 wavefronts = 8 blocks of 256 threads, whatever occupancy the runtime reports for a kernel: more than
# 8 * CU tiles (maps) cannot be resident at once, so some block takes a second trip through its loop -- the prefetch hand-over
# (hv = nhv), wavefront 0 still selecting while the others stage the next tile, the late store of a map's features.  At most
# 16 * CU rows (CU maps) fit one trip for certain: a launch of that size is the single-trip statement of the same arithmetic.

def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _several_trips_batch(n):
    """Envs of n agents whose rows fill more than 8 * CU tiles and leave a ragged last one."""
    B = 16 * 8 * _cu() // n + 1
    while (B * n) % 16 == 0:
        B += 1
    rows = B * n
    assert (rows + 15) // 16 > 8 * _cu() and rows > 16 * 8 * _cu() and rows % 16 != 0   # more than one trip, whatever the occupancy
    print(f"{_cu()} CUs: {B} envs x {n} agents = {rows} rows = {(rows + 15) // 16} tiles > {8 * _cu()}")
    return B


def _steps(agents, obs_steps, lo, hi, **kw):
    """choose_action on envs lo..hi of every step's observations -> [(q, hidden, actions, feat)] as they were after each step."""
    out = []
    for obs in obs_steps:
        act = agents.choose_action(obs[lo:hi], want_q=True, **{k: (v[lo:hi] if torch.is_tensor(v) else v) for k, v in kw.items()})
        out.append((agents.q.clone(), agents.hidden.clone(), act.clone(), agents.feat.clone() if agents.conv else None))
    return out


def _assert_equals_single_trip_shards(a, net, B, E, obs_steps, whole, seed, **kw):
    """The same envs through shards of E envs, each a single-trip launch keyed on its global rows: bit for bit what the one
    launch over all of them left, step by step."""
    n = a.n_agents
    for lo in range(0, B, E):
        hi = min(B, lo + E)
        part = _steps(FusedAgents(a, hi - lo, net=net, seed=seed, env_offset=lo), obs_steps, lo, hi, **kw)
        for t, ((q, h, act, feat), (wq, wh, wact, wfeat)) in enumerate(zip(part, whole)):
            assert torch.equal(q, wq[lo:hi]), (lo, t, "q")
            assert torch.equal(h, wh[lo * n:hi * n]), (lo, t, "hidden")
            assert torch.equal(act, wact[lo:hi]), (lo, t, "actions")
            if feat is not None:
                assert torch.equal(feat, wfeat[lo:hi]), (lo, t, "feat")


def test_fused_forward_over_several_trips_matches_torch_module():
    """k_policy_h with more tiles than the device can hold (tiles > 8 * CU) and a ragged last tile, two steps (the second from
    a non-zero hidden state): every row to the bars of test_fused_forward_matches_torch_module."""
    n = 3
    B = _several_trips_batch(n)
    torch.manual_seed(41)
    a = _args(n)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    for p in net.parameters():
        p.data.mul_(3.0)
    fused = FusedAgents(a, B, net=net)
    ref = BatchedAgents(a, B, net=net)
    last = torch.zeros(B, n, a.n_actions, device="cuda")
    for t in range(2):
        obs = torch.rand(B, n, 4, device="cuda") * 2 - 0.5
        act = fused.choose_action(obs, want_q=True).clone()
        x = torch.cat([obs, last, ref.agent_ids], 2).reshape(B * n, -1)
        with torch.no_grad():
            q_ref, ref.hidden = net(x, ref.hidden)
        q_ref = q_ref.reshape(B, n, -1)
        assert torch.allclose(fused.q, q_ref, atol=TOL, rtol=TOL), (t, (fused.q - q_ref).abs().max().item())
        assert torch.allclose(fused.hidden, ref.hidden, atol=TOL, rtol=TOL), (t, (fused.hidden - ref.hidden).abs().max().item())
        top2 = q_ref.topk(2, dim=2).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-3
        assert clear.float().mean().item() > 0.9 and (act == q_ref.argmax(2))[clear].all()
        ref.hidden = fused.hidden.clone()
        last = torch.nn.functional.one_hot(act, a.n_actions).float()
    assert fused.hidden.abs().max().item() > 0.1


@pytest.mark.parametrize("rule", ["greedy", "epsilon", "epsilon_per_env", "softmax"])
def test_one_launch_over_several_trips_equals_single_trip_launches(rule):
    """A row's arithmetic and its noise do not depend on the tile it lands in or on the trip that tile is computed in: q, hidden
    state and actions of ONE launch over tiles > 8 * CU equal, bit for bit, those of shards of at most 16 * CU rows (one trip
    each), under every selection rule; the exploring rules do move actions away from the greedy ones."""
    n = 3
    B, cu = _several_trips_batch(n), _cu()
    E = 16 * cu // n
    assert n * E <= 16 * cu   # a shard's tiles <= CU <= resident blocks: a single trip
    a = _args(n)
    if rule == "softmax":
        a.alg = "reinforce"
    torch.manual_seed(43)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    for p in net.parameters():
        p.data.mul_(3.0)
    obs_steps = [torch.rand(B, n, 4, device="cuda") * 2 - 0.5 for _ in range(2)]
    kw = {"greedy": dict(evaluate=True), "epsilon": dict(epsilon=0.3), "softmax": dict(epsilon=0.25),
          "epsilon_per_env": dict(epsilon=0.9, eps_env=torch.linspace(0.05, 0.95, B, dtype=torch.float64, device="cuda"))}[rule]
    whole = _steps(FusedAgents(a, B, net=net, seed=77), obs_steps, 0, B, **kw)
    _assert_equals_single_trip_shards(a, net, B, E, obs_steps, whole, 77, **kw)
    assert whole[1][1].abs().max().item() > 0.1   # the second step started from a non-zero hidden state
    if rule != "greedy":
        greedy = _steps(FusedAgents(a, B, net=net, seed=77), obs_steps[:1], 0, B, evaluate=True)
        assert torch.equal(greedy[0][0], whole[0][0])          # the same q ...
        changed = (greedy[0][2] != whole[0][2]).float().mean().item()
        assert changed > 0.02, changed                          # ... other actions
        if rule == "epsilon_per_env":   # every env explored with its own epsilon: the last tenth far more often than the first
            moved = (greedy[0][2] != whole[0][2]).float().mean(1)
            assert moved[-B // 10:].mean().item() > 3 * moved[:B // 10].mean().item() > 0


def test_flight_forward_over_several_trips():
    """flight with B = 8 * CU + 5 envs: one map per env takes k_conv_features through several trips (n_maps > 8 * CU: the register
    prefetch of the next map, the features stored one iteration late), and k_policy_h runs with `feat` over 3 B rows.  Features,
    q and hidden state against the torch module at test_flight_fused_forward_matches_torch_module's bars, and bit for bit
    against shards of CU envs (one trip of either kernel)."""
    n, cu = 3, _cu()
    B, E = 8 * cu + 5, cu
    assert B > 8 * cu and E <= cu and n * E <= 16 * cu
    print(f"{cu} CUs: {B} maps > {8 * cu}, {B * n} rows; shards of {E} envs")
    torch.manual_seed(47)
    a = _flight_args(n)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    for p in net.parameters():
        p.data.mul_(2.0)
    obs_steps = []
    for t in range(2):
        maps = torch.rand(B, 1, 2500, device="cuda").expand(B, n, 2500)       # one map per env, as get_obs gives
        obs_steps.append(torch.cat([maps, torch.rand(B, n, 4, device="cuda")], 2).contiguous())
    fused = FusedAgents(a, B, net=net, seed=5)
    ref = BatchedAgents(a, B, net=net)
    last = torch.zeros(B, n, 3, device="cuda")
    whole = []
    for t, obs in enumerate(obs_steps):
        fused.feat.fill_(float("nan"))   # every env's features are written by this launch, the last map of every block too
        act = fused.choose_action(obs, want_q=True).clone()
        whole.append((fused.q.clone(), fused.hidden.clone(), act, fused.feat.clone()))
        x = torch.cat([obs, last, ref.agent_ids], 2).reshape(B * n, -1)
        with torch.no_grad():
            q_ref, ref.hidden = net(x, ref.hidden)
            f_ref = net.linear(net.conv(obs[:, 0, :2500].reshape(B, 1, 50, 50)).reshape(B, -1))
        q_ref = q_ref.reshape(B, n, -1)
        assert torch.isfinite(fused.feat).all()
        assert torch.allclose(fused.feat, f_ref, atol=5 * TOL, rtol=5 * TOL), (t, (fused.feat - f_ref).abs().max().item())
        assert torch.allclose(fused.q, q_ref, atol=5 * TOL, rtol=5 * TOL), (t, (fused.q - q_ref).abs().max().item())
        assert torch.allclose(fused.hidden, ref.hidden, atol=5 * TOL, rtol=5 * TOL)
        clear = (q_ref.topk(2, dim=2).values.diff(dim=2).abs()[..., 0]) > 1e-3
        assert (act == q_ref.argmax(2))[clear].all()
        ref.hidden = fused.hidden.clone()
        last = torch.nn.functional.one_hot(act, 3).float()
    del ref, x, q_ref, f_ref
    _assert_equals_single_trip_shards(a, net, B, E, obs_steps, whole, 5)


def test_flight_closed_loop_and_collector_with_fused_agents():
    a = _flight_args(3)
    B = 64
    env = cs.BatchedFlightEnv(a, batch=B, freeze_done=True)
    cs.apply_env_info(a, env)
    torch.manual_seed(3)
    fused = FusedAgents(a, B)
    ref = BatchedAgents(a, B, net=fused.net)
    col = cs.EpisodeCollector(env)
    env.seed(np.arange(B))
    ep_f, rew_f, win_f, found_f = col.generate_episodes(agents=fused, init=True)
    env.seed(np.arange(B))
    ep_t, rew_t, win_t, found_t = col.generate_episodes(policy=ref.policy(0.0, True), init=True)
    same = (ep_f["u"] == ep_t["u"]).reshape(B, -1).all(1) & (found_f == found_t)
    assert same.float().mean().item() > 0.9   # a near-tie in q flips an env's whole trajectory; the bulk is identical
    assert torch.equal(ep_f["o"][same], ep_t["o"][same]) and torch.equal(ep_f["r"][same], ep_t["r"][same])


# ---- fused closed-loop rollout (k_rollout_policy): T x (network forward -> env.step) in one launch -----------------

@pytest.mark.parametrize("n,B,T,eps,auto_reset", [(3, 64, 60, 0.0, False), (3, 37, 45, 0.25, False), (5, 50, 40, 0.1, False),
                                                  (1, 16, 30, 0.0, False), (4, 21, 230, 0.05, True),
                                                  (3, 4096, 200, 0.05, False), (2, 1001, 120, 0.3, True)])
def test_fused_closed_loop_rollout_equals_stepwise(n, B, T, eps, auto_reset):
    a = _args(n)
    torch.manual_seed(11 * n + B)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    for p in net.parameters():
        p.data.mul_(3.0)
    outs = []
    for fused_loop in (False, True):
        env = cs.BatchedFlightEnv(a, batch=B, freeze_done=not auto_reset, auto_reset=auto_reset)
        env.seed(np.arange(B) + 5)
        env.reset(init=True)
        ag = FusedAgents(a, B, net=net, seed=99)
        if fused_loop:
            o = env.rollout_policy(ag, T, epsilon=eps, evaluate=False)
        else:
            o = dict(actions=[], reward=[], terminated=[], win=[], obs=[], state=[])
            for t in range(T):
                act = ag.choose_action(env.get_obs(), epsilon=eps)
                r, term, win = env.step(act)
                for k, v in (("actions", act), ("reward", r), ("terminated", term), ("win", win), ("obs", env.get_obs()),
                             ("state", env.get_state())):
                    o[k].append(v.clone())
            o = {k: torch.stack(v) for k, v in o.items()}
        outs.append((o, ag.hidden.clone(), ag.actions.clone(), ag.calls, env.raw()["hdr"].clone(), env.raw()["agent"].clone(),
                     env.get_obs().clone()))
    (oa, ha, la, ca, hdra, aga, obsa), (ob, hb, lb, cb, hdrb, agb, obsb) = outs
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(ha, hb) and torch.equal(la, lb) and ca == cb
    assert torch.equal(hdra, hdrb) and torch.equal(aga, agb) and torch.equal(obsa, obsb)
    if eps > 0:
        assert (oa["actions"] != oa["actions"][0:1]).any()


@pytest.mark.parametrize("n,B,T,eps,auto_reset,emit", [(3, 64, 30, 0.0, False, True), (3, 37, 25, 0.25, True, False),
                                                       (5, 50, 12, 0.1, True, True), (2, 300, 21, 0.3, True, False)])
def test_flight_closed_loop_call_equals_stepwise(n, B, T, eps, auto_reset, emit):
    """cs_rollout_policy_flight (conv on the map where it lives, no observation copies when emit=False) against T x
    (choose_action(get_obs) -> step): same actions, rewards, hidden state, env state and probability maps."""
    a = cs.make_env_args("flight", n_agents=n)
    a.time_limit = 9
    torch.manual_seed(7 * n + B)
    outs = []
    net = None
    for fused_loop in (False, True):
        env = cs.BatchedFlightEnv(a, batch=B, freeze_done=not auto_reset, auto_reset=auto_reset)
        cs.apply_env_info(a, env)
        if net is None:
            net = AgentRNN(rnn_input_shape(a), a).cuda()
            for p in net.parameters():
                p.data.mul_(2.0)
        env.seed(np.arange(B) + 5)
        env.reset(init=True)
        ag = FusedAgents(a, B, net=net, seed=99)
        if fused_loop:
            o = env.rollout_policy(ag, T, epsilon=eps, evaluate=False, emit=emit)
            o = {k: v for k, v in o.items() if v is not None}
        else:
            o = dict(actions=[], reward=[], terminated=[], win=[], obs=[], state=[])
            for t in range(T):
                act = ag.choose_action(env.get_obs(), epsilon=eps)
                r, term, win = env.step(act)
                for k, v in (("actions", act), ("reward", r), ("terminated", term), ("win", win), ("obs", env.get_obs()),
                             ("state", env.get_state())):
                    o[k].append(v.clone())
            o = {k: torch.stack(v) for k, v in o.items()}
        raw = env.raw()
        outs.append((o, ag.hidden.clone(), ag.actions.clone(), ag.calls, raw["hdr"].clone(), raw["agent"].clone(),
                     raw["prob"].clone(), env.get_obs().clone(), env.get_state().clone()))
    (oa, ha, la, ca, hdra, aga, pa, obsa, sta), (ob, hb, lb, cb, hdrb, agb, pb, obsb, stb) = outs
    assert ("obs" in ob) == emit
    for k in ob:
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(ha, hb) and torch.equal(la, lb) and ca == cb
    assert torch.equal(hdra, hdrb) and torch.equal(aga, agb) and torch.equal(pa, pb)
    assert torch.equal(obsa, obsb) and torch.equal(sta, stb)
    if eps > 0:
        assert (oa["actions"] != oa["actions"][0:1]).any()


def test_closed_loop_c_example_runs(tmp_path):
    """examples/closed_loop_demo.cpp: cs_policy_pack -> cs_rollout_policy -> cs_store_episodes from plain C++/HIP."""
    import re, subprocess
    from cooperative_search_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.dirname(_lib.library_path())
    exe = tmp_path / "closed_loop_demo"
    subprocess.check_call([build.hipcc_path(), "--offload-arch=gfx950", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "closed_loop_demo.cpp"), "-L", csrc, "-lcoopsearch_hip",
                           f"-Wl,-rpath,{csrc}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"episodes (\d+)\s+mean episode_reward (-?[\d.]+)\s+win rate ([\d.]+)\s+mean targets_find ([\d.]+)", out.stdout)
    assert m and int(m.group(1)) == 4096, out.stdout
    assert 0.0 <= float(m.group(4)) <= 15.0 and "yes" in out.stdout


def _row_uniform(seed, step, rows):
    """numpy restatement of csrc/policy_dev.h row_bits -> the 24-bit uniform a row's selection uses."""
    M = (1 << 64) - 1

    def mix64(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    return np.array([(mix64((mix64((mix64(seed & M) + (step & 0xFFFFFFFF)) & M) + int(r) * 0x9E3779B97F4A7C15) & M) >> 40) / 16777216.0
                     for r in rows], dtype=np.float64)


@pytest.mark.parametrize("eps", [0.0, 0.25])
def test_softmax_selection_matches_the_reference_statement(eps):
    """agent/agent.py:77-97 (_choose_action_from_softmax, alg == 'reinforce'): prob = (1 - eps) softmax(q) + eps / |A|,
    one Categorical draw -- restated with torch on the kernel's own q values and the row's uniform (inverse CDF);
    rows whose uniform falls within 1e-5 of a CDF step are not compared."""
    a = _args(3)
    a.alg = "reinforce"
    B, off = 3000, 5000
    torch.manual_seed(11)
    fused = FusedAgents(a, B, seed=1234, env_offset=off)
    for p in fused.net.parameters():
        p.data.mul_(4.0)   # spread the q values so that the distribution is far from uniform
    fused.load_weights()
    obs = torch.rand(B, 3, 4, device="cuda") * 2 - 1
    for call in range(3):
        act = fused.choose_action(obs, epsilon=eps, evaluate=False, want_q=True).clone()
        q = fused.q.reshape(B * 3, 3)
        prob = (1 - eps) * torch.softmax(q, dim=-1) + eps / 3
        cdf = (prob / prob.sum(-1, keepdim=True)).cumsum(-1).double().cpu().numpy()
        u = _row_uniform(1234, call, off * 3 + np.arange(B * 3))
        want = np.minimum((u[:, None] >= cdf).sum(1), 2)
        clear = np.abs(cdf - u[:, None]).min(1) > 1e-5
        got = act.reshape(-1).cpu().numpy()
        assert clear.mean() > 0.99 and np.array_equal(got[clear], want[clear])
        # and the empirical distribution follows prob
        assert abs((got == 0).mean() - prob[:, 0].mean().item()) < 0.02
    # epsilon == 0 and evaluate: argmax(prob) == argmax(q)
    act = fused.choose_action(obs, epsilon=0.0, evaluate=True, want_q=True).clone()
    top2 = fused.q.topk(2, dim=2).values
    clear = (top2[..., 0] - top2[..., 1]) > 1e-4
    assert (act == fused.q.argmax(2))[clear].all()


@pytest.mark.parametrize("softmax", [False, True])
def test_exploration_noise_does_not_depend_on_the_sharding(softmax):
    """the per-row generator is keyed on the GLOBAL (env, agent) row.  A batch split into two shards with
    env_offset picks, with epsilon > 0, exactly the actions of the whole batch -- through cs_policy_forward and through
    the fused closed-loop kernel."""
    n, B, T = 3, 512, 40
    a = _args(n)
    if softmax:
        a.alg = "reinforce"
    torch.manual_seed(5)
    net = AgentRNN(rnn_input_shape(a), a).cuda()
    args = cs.make_env_args("flight_easy", n_agents=n)
    whole_env = cs.BatchedFlightEnv(args, batch=B, freeze_done=True)
    whole = FusedAgents(a, B, net=net, seed=77)
    ow = whole_env.rollout_policy(whole, T, epsilon=0.3, evaluate=False)
    half = B // 2
    for k in range(2):
        env = cs.BatchedFlightEnv(args, batch=half, env_offset=k * half, freeze_done=True)
        ag = FusedAgents(a, half, net=net, seed=77, env_offset=k * half)
        op = env.rollout_policy(ag, T, epsilon=0.3, evaluate=False)
        for key in ("actions", "reward", "terminated", "obs"):
            assert torch.equal(op[key], ow[key][:, k * half:(k + 1) * half]), (k, key)
        # the two-kernel loop on the shard draws the same noise as well
        env2 = cs.BatchedFlightEnv(args, batch=half, env_offset=k * half, freeze_done=True)
        ag2 = FusedAgents(a, half, net=net, seed=77, env_offset=k * half)
        for t in range(5):
            act = ag2.choose_action(env2.get_obs(), epsilon=0.3, evaluate=False)
            assert torch.equal(act, ow["actions"][t, k * half:(k + 1) * half]), (k, t)
            env2.step(act)
    assert (ow["actions"] != ow["actions"][0:1]).any()


def _trained(tag):
    z = np.load(os.path.join(GOLD, f"trained_{tag}.npz"))
    n, am = int(z["n_agents"]), int(z["agent_mode"])
    env_name = "flight" if tag.startswith("flight") else "flight_easy"
    args = cs.make_env_args(env_name, n_agents=n, agent_mode=am)
    return z, args, n


IDX = [10, 20, 40, 60, 80, 100, 150, 199]   # the indices runner.py:168 prints


EASY_TAGS = ["easy3_qmix", "easy5_qmix", "easy3_reinforce", "easy3_dop", "easy5_dop", "easy3_qmix_am3", "easy3_qmix_am2"]
FLIGHT_TAGS = ["flight3_qmix", "flight1_qmix", "flight5_qmix", "flight3_reinforce"]


def _load_net(z, args):
    net = AgentRNN(rnn_input_shape(args), args)
    net.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w_")})
    return net


def _report_lockstep(tag, compared, total, episodes):
    """the walked fraction per checkpoint tag, printed (pytest -rP / -s shows it) and appended to
    gpurun_out/lockstep_fractions.txt, which the measurement script copies to profiles/."""
    line = f"{tag}: {compared} of {total} recorded steps walked in lockstep over {episodes} episodes ({compared / max(total, 1):.3f})"
    print(line)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "lockstep_fractions.txt"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("tag", EASY_TAGS + FLIGHT_TAGS)
def test_trained_checkpoint_exact_trajectories(tag):
    """next to the statistical curves, EXACT closed-loop trajectories.  gen_trained.py starts its first four
    replays of every shipped checkpoint from recorded np.random.seed values and records every action, reward and found
    count of the reference's own env + network; the HIP env seeded identically and driven by the HIP network kernels
    (k_rollout_policy / cs_rollout_policy_flight) must take the SAME actions and collect the SAME rewards, step for step,
    until the first step where they pick differently -- which must be a step where the reference network's top two outputs are
    within 1e-3 of each other (a near-tie that fp32 summation order may break differently).  Covers the DOP actors (agent.py:61-62), the softmax rule's argmax branch
    (agent.py:92-93) and the AM2 / AM3 start modes, whose resets draw (quirk Q3)."""
    z, args, n = _trained(tag)
    seeds = z["traj_seeds"].astype(np.uint32)
    K, T = len(seeds), 200
    env = cs.BatchedFlightEnv(args, batch=K, freeze_done=True, seeds=seeds)
    cs.apply_env_info(args, env)
    if "reinforce" in tag:
        args.alg = "reinforce"
    fused = FusedAgents(args, K, net=_load_net(z, args))
    env.seed(seeds)            # the ctor's own reset(init=True) consumed RNG, like the reference's ctor
    env.reset(init=True)
    fused.init_hidden()
    out = env.rollout_policy(fused, T, epsilon=0.0, evaluate=True, emit=not env.flight)
    acts = out["actions"].cpu().numpy()
    rew = out["reward"].cpu().numpy()
    compared = total = 0
    for k in range(K):
        L = int(z["traj_len"][k])
        steps = 0
        for st in range(L):   # in lockstep as long as the actions agree; the first disagreement must be a near-tie
            if not np.array_equal(acts[st, k], z["traj_actions"][k, st]):
                assert z["traj_qgap"][k, st] < 1e-3, \
                    f"{tag} episode {k}: actions differ at step {st} where the reference's top two outputs are {z['traj_qgap'][k, st]} apart"
                break
            assert rew[st, k] == np.float32(z["traj_rewards"][k, st]), f"{tag} episode {k}: reward at step {st}"
            steps += 1
        if steps == L:   # the whole episode walked in lockstep: it ends where the reference's ended
            assert bool(out["terminated"][L - 1, k]) and (L == 1 or not bool(out["terminated"][L - 2, k]))
            assert int(env.target_find[k]) == int(z["traj_found"][k, L - 1])
        compared += steps
        total += L
    _report_lockstep(tag, compared, total, K)
    assert compared >= 0.3 * total, f"{tag}: only {compared} of {total} steps walked in lockstep before a near-tie broke it"


@pytest.mark.parametrize("tag", EASY_TAGS)
def test_trained_checkpoint_closed_loop_flight_easy(tag):
    """Policy-in-the-loop parity with the reference's SHIPPED checkpoints: the checkpoint's weights
    (tests/golden/trained_*.npz, written by gen_trained.py from model/<run>/<N>_rnn_net_params.pkl) drive 4096 envs through
    the fused closed-loop kernel (k_rollout_policy: network forward + env step per step, 200 steps in one launch) under
    generate_replay's protocol (reset(init=True), greedy); the found-fraction curve must agree with the curve the
    reference's own env + RNN produce with the same weights (100 replays, s.e. <= 2 points) at the printed indices."""
    z, args, n = _trained(tag)
    B, T = 4096, 200
    env = cs.BatchedFlightEnv(args, batch=B, freeze_done=True)
    cs.apply_env_info(args, env)
    if "reinforce" in tag:
        args.alg = "reinforce"   # softmax rule; epsilon = 0 and evaluate -> argmax(prob), agent.py:92-93
    net = _load_net(z, args)
    fused = FusedAgents(args, B, net=net)
    env.reset(init=True)
    fused.init_hidden()
    out = env.rollout_policy(fused, T, epsilon=0.0, evaluate=True)
    found = out["state"][:, :, 4 * n + 2::3].sum(-1)                 # [T, B] targets found after each step
    curve = (found.double().mean(1) / 15 * 100).cpu().numpy()
    assert (np.diff(curve) >= -1e-9).all() and found.max().item() <= 15
    ref = z["ref_curve"]
    np.testing.assert_allclose(curve[IDX], ref[IDX], rtol=0, atol=4.0,
                               err_msg=f"{tag}: ours {np.round(curve[IDX], 2)} reference replay {np.round(ref[IDX], 2)} "
                                       f"shipped result (checkpoint {int(z['shipped_num'])}) {np.round(z['shipped_curve'][IDX], 2)}")
    # where every episode of the trained policy finds all 15 targets in the reference replay, so must (nearly) all of ours
    if float(z["ref_found"].mean()) == 15.0:
        assert curve[199] > 99.5
    # the shipped result file was made with the shipped weights (for the REINFORCE run the numbers agree too, but its shipped
    # curve -- 6.7 % flat -- is not what its shipped weights do -- 100 % found in the reference's own replay: not asserted)
    if int(z["checkpoint"]) == int(z["shipped_num"]) and "reinforce" not in tag:
        np.testing.assert_allclose(curve[IDX], z["shipped_curve"][IDX], rtol=0, atol=6.0,
                                   err_msg=f"{tag}: ours {np.round(curve[IDX], 2)} shipped {np.round(z['shipped_curve'][IDX], 2)}")
    # the two-kernel loop (cs_policy_forward + cs_step per step) walks the same trajectories
    seeds = np.arange(256, dtype=np.uint32) + 5
    env2 = cs.BatchedFlightEnv(args, batch=256, freeze_done=True, seeds=seeds)
    env3 = cs.BatchedFlightEnv(args, batch=256, freeze_done=True, seeds=seeds)
    f2, f3 = FusedAgents(args, 256, net=net), FusedAgents(args, 256, net=net)
    env2.reset(init=True)
    env3.reset(init=True)
    o3 = env3.rollout_policy(f3, 60, evaluate=True)
    for t in range(60):
        a = f2.choose_action(env2.get_obs(), evaluate=True)
        assert torch.equal(a, o3["actions"][t]), t
        env2.step(a)


@pytest.mark.parametrize("tag", FLIGHT_TAGS)
def test_trained_checkpoint_closed_loop_flight(tag):
    """flight (probability-map observation, conv front end): the shipped QMIX checkpoints of the 3-, 1- and 5-agent runs
    (each the one its shipped result file average_res_<N>.npy was made with) and the shipped REINFORCE run.  1024 envs
    through cs_policy_conv_features + cs_policy_forward + cs_step; compared with the reference replay of the same weights
    (20-30 episodes: s.e. up to 4 points) and, where one exists, with the shipped curve (100 episodes)."""
    z, args, n = _trained(tag)
    B = 1024
    env = cs.BatchedFlightEnv(args, batch=B, freeze_done=True)
    cs.apply_env_info(args, env)
    if "reinforce" in tag:
        args.alg = "reinforce"
    fused = FusedAgents(args, B, net=_load_net(z, args))
    curve = cs.collect_experiment_data(env, fused.policy(evaluate=True))
    msg = (f"{tag}: ours {np.round(curve[IDX], 2)} reference replay {np.round(z['ref_curve'][IDX], 2)} "
           f"shipped {np.round(z['shipped_curve'][IDX], 2)}")
    if int(z["shipped_num"]) >= 0:
        assert int(z["checkpoint"]) == int(z["shipped_num"])
        np.testing.assert_allclose(curve[IDX], z["shipped_curve"][IDX], rtol=0, atol=5.0 if tag == "flight3_qmix" else 7.0,
                                   err_msg=msg)
    np.testing.assert_allclose(curve[IDX], z["ref_curve"][IDX], rtol=0, atol=7.0 if tag == "flight3_qmix" else 9.0, err_msg=msg)


# ---------------------------------------------------------------------------------------------------------------------------
# Exploration schedule: the epsilon the reference's OWN RolloutWorker hands to Agents.choose_action at every step
# (tests/golden/epsilon_schedule.json, recorded by gen_epsilon.py with alg = 'qmix' and the shipped argument setters) against
# the epsilon the HIP closed loop uses, env by env, step by step, as exact doubles.
# ---------------------------------------------------------------------------------------------------------------------------
def _schedule_fixture(case):
    import json
    d = json.load(open(os.path.join(GOLD, "epsilon_schedule.json")))[case]
    d["used_f"] = np.array([float(x) for x in d["used"]], dtype=np.float64)
    return d


def _schedule_args(n, d, flight=False):
    a = _flight_args(n) if flight else _args(n)
    a.epsilon, a.anneal_epsilon, a.min_epsilon = d["epsilon0"], float(d["anneal_epsilon"]), float(d["min_epsilon"])
    a.epsilon_anneal_scale = d["scale"]
    return a


@pytest.mark.parametrize("case,one_launch,binding", [("default", True, None), ("default", False, None), ("fast", True, None),
                                                     ("fast", False, None), ("fast", True, "ctypes")])
def test_epsilon_step_schedule_equals_the_reference_worker(case, one_launch, binding):
    """epsilon_anneal_scale == 'step' (the QMIX / DOP default): after every EXECUTED env step epsilon = epsilon - anneal if
    epsilon > min_epsilon else epsilon (common/rollout.py:75-76), carried across episodes (:133-135).  The j-th step a worker
    executes uses the j-th iterate of that rule, whatever the episode lengths: every env of the batch is its own worker, so
    env b's step t of episode k must use used[steps b executed before + t] of the reference's recording -- bit for bit --
    in the fused launch (the anneal runs inside k_rollout_policy) and in the per-step loop (cs_epsilon_step)."""
    d = _schedule_fixture(case)
    n, B, T = 3, 96, 200
    a = _schedule_args(n, d)
    torch.manual_seed(7)
    env = cs.BatchedFlightEnv(a, batch=B, binding=binding)
    cs.apply_env_info(a, env)
    agents = FusedAgents(a, B, seed=5)
    sched = cs.EpsilonSchedule(a, B)
    col = cs.EpisodeCollector(env, schedule=sched)
    done_before = np.zeros(B, dtype=np.int64)
    used = d["used_f"]
    for k in range(3):
        trace = torch.full((T, B), -1.0, dtype=torch.float64, device="cuda")
        ep, _r, _w, _f = col.generate_episodes(agents=agents, evaluate=False, one_launch=one_launch, episode_num=k, eps_trace=trace)
        steps = (ep["padded"][:, :, 0] == 0).sum(1).cpu().numpy()   # executed steps of each env's episode
        tr = trace.cpu().numpy()
        for b in range(B):
            want = used[done_before[b]:done_before[b] + steps[b]]
            assert np.array_equal(tr[:steps[b], b], want), (case, k, b, steps[b])
        done_before += steps
        assert done_before.max() < len(used) - 1, "fixture too short for this run"
        assert np.array_equal(sched.values.cpu().numpy(), used[done_before]), f"{case}: carried epsilon after episode {k}"
    if case == "fast":   # the floor was crossed inside the run
        assert (sched.values.cpu().numpy() <= float(d["min_epsilon"])).all()


@pytest.mark.parametrize("case", ["episode", "epoch"])
def test_epsilon_episode_and_epoch_scales_equal_the_reference_worker(case):
    """'episode': one anneal before every episode (rollout.py:36-38); 'epoch': only before the episode with episode_num == 0
    (:39-41).  The value of every step of episode k is the reference's (including its stepping below min_epsilon: the rule
    tests `epsilon > min_epsilon` BEFORE subtracting)."""
    d = _schedule_fixture(case)
    n, B, T = 3, 16, 200
    a = _schedule_args(n, d)
    env = cs.BatchedFlightEnv(a, batch=B)
    cs.apply_env_info(a, env)
    agents = FusedAgents(a, B, seed=5)
    sched = cs.EpsilonSchedule(a, B)
    col = cs.EpisodeCollector(env, schedule=sched)
    starts = np.concatenate([[0], np.cumsum(d["steps"])])
    k = 0
    for _epoch in range(d["epochs"]):
        for num in range(d["episodes_per_epoch"]):
            trace = torch.full((T, B), -1.0, dtype=torch.float64, device="cuda")
            ep, *_ = col.generate_episodes(agents=agents, evaluate=False, episode_num=num, eps_trace=trace)
            steps = (ep["padded"][:, :, 0] == 0).sum(1).cpu().numpy()
            want = d["used_f"][starts[k]]   # constant over the reference's episode k
            tr = trace.cpu().numpy()
            for b in range(B):
                assert np.array_equal(tr[:steps[b], b], np.full(steps[b], want)), (case, k, b)
            assert np.array_equal(sched.values.cpu().numpy(), np.full(B, float(d["carried_after_episode"][k])))
            k += 1


def test_epsilon_schedule_in_the_flight_closed_loop():
    """cs_rollout_policy_flight with a schedule: per step cs_policy_forward(eps_env) -> k_eps_step -> k_step, enqueued by the one
    call; same iterates."""
    d = _schedule_fixture("fast")
    n, B, T = 3, 8, 200
    a = _schedule_args(n, d, flight=True)
    env = cs.BatchedFlightEnv(a, batch=B)
    cs.apply_env_info(a, env)
    agents = FusedAgents(a, B, seed=3)
    sched = cs.EpsilonSchedule(a, B)
    col = cs.EpisodeCollector(env, schedule=sched)
    trace = torch.full((T, B), -1.0, dtype=torch.float64, device="cuda")
    ep, *_ = col.generate_episodes(agents=agents, evaluate=False, eps_trace=trace, init=True)
    steps = (ep["padded"][:, :, 0] == 0).sum(1).cpu().numpy()
    tr = trace.cpu().numpy()
    for b in range(B):
        assert np.array_equal(tr[:steps[b], b], d["used_f"][:steps[b]]), b
    assert np.array_equal(sched.values.cpu().numpy(), d["used_f"][steps])


def test_evaluation_ignores_the_schedule():
    """epsilon = 0 if evaluate (rollout.py:35) and self.epsilon is left alone (:133-134)."""
    d = _schedule_fixture("default")
    a = _schedule_args(3, d)
    env = cs.BatchedFlightEnv(a, batch=32)
    cs.apply_env_info(a, env)
    agents = FusedAgents(a, 32, seed=5)
    sched = cs.EpsilonSchedule(a, 32)
    col = cs.EpisodeCollector(env, schedule=sched)
    ep1, *_ = col.generate_episodes(agents=agents, evaluate=True)
    assert (sched.values == 1.0).all()
    env2 = cs.BatchedFlightEnv(a, batch=32)
    ep2, *_ = cs.EpisodeCollector(env2).generate_episodes(agents=FusedAgents(a, 32, net=agents.net, seed=5), evaluate=True)
    assert torch.equal(ep1["u"], ep2["u"])
