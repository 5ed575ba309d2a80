"""GPU tests of the device pack kernel (cs_policy_pack_device, FusedAgents.sync_weights) and of the training driver
(cooperative-search_amd/runner.py): bit identity with the host packer, the all-or-nothing refusal, no host synchronisation in
the repack or in an epoch, and Runner.run == the hand-written loop of INTEGRATION.md with load_weights()."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import runner as rn

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORDER = ("fc1.weight", "fc1.bias", "rnn.weight_ih", "rnn.bias_ih", "rnn.weight_hh", "rnn.bias_hh", "fc2.0.weight", "fc2.0.bias",
         "fc2.2.weight", "fc2.2.bias")
WEIGHTS = (0, 2, 4, 6, 8)   # positions in ORDER of the five matrices, in cs_policy_pack's check order
NAN_FILL = (0x7FC00000, 0xFFC00001, 0x7F800001)   # quiet, negative quiet and signalling NaN patterns


def shapes(in_dim, A):
    return ((64, in_dim), (64,), (192, 64), (192,), (192, 64), (192,), (64, 64), (64,), (A, 64), (A,))


def host_pack(ws):
    """cs_policy_pack on numpy arrays -> (rc, blob as int32, message)."""
    L = _lib.load()
    ws = [np.ascontiguousarray(w, dtype=np.float32) for w in ws]
    out = np.zeros(L.cs_policy_packed_floats(), dtype=np.float32)
    rc = L.cs_policy_pack(*[C.c_void_p(w.ctypes.data) for w in ws], ws[0].shape[1], ws[8].shape[0], C.c_void_p(out.ctypes.data))
    return rc, out.view(np.int32), L.cs_policy_last_error().decode()


def device_pack(ws, fill):
    """policy_pack_device into a blob pre-filled with the int32 pattern `fill` -> (blob as int32, status)."""
    ops = _lib.torch_ops()
    n = _lib.load().cs_policy_packed_floats()
    packed = torch.tensor(np.full(n, fill, dtype=np.uint32).view(np.int32), device="cuda").view(torch.float32)
    status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    ops.policy_pack_device(*[torch.as_tensor(np.asarray(w, dtype=np.float32), device="cuda").contiguous() for w in ws], packed, status)
    return packed.view(torch.int32).cpu().numpy(), status.cpu().numpy()


def assert_pack_equal(ws):
    rc, want, msg = host_pack(ws)
    assert rc == 0, msg
    for fill in NAN_FILL:
        got, status = device_pack(ws, fill)
        assert status.tolist() == [0, -1, -1, 0]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} words differ, first at {bad[:8]}: {got[bad[:4]]} vs {want[bad[:4]]}"


def random_weights(rng, in_dim, A, scale):
    return [(rng.standard_normal(s) * scale).astype(np.float32) for s in shapes(in_dim, A)]


# ---- the pack kernel against the host packer --------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1e-7, 1e-5, 6e-5, 1e-3, 0.1, 1.0, 30.0, 1e3, 1e4])
def test_pack_is_bit_identical_across_scales(scale):
    rng = np.random.default_rng(int(scale * 1e7) % 9973)
    ws = random_weights(rng, 10, 3, scale)
    ws = [np.clip(w, -65504, 65504) for w in ws]
    assert_pack_equal(ws)


@pytest.mark.parametrize("in_dim, A", [(7, 3), (10, 3), (16, 16), (23, 3), (31, 16), (32, 3), (32, 16)])
def test_pack_is_bit_identical_for_every_width(in_dim, A):
    rng = np.random.default_rng(in_dim * 100 + A)
    assert_pack_equal(random_weights(rng, in_dim, A, 0.3))


def test_pack_is_bit_identical_on_subnormals_ties_and_the_range_limits():
    rng = np.random.default_rng(5)
    ws = random_weights(rng, 12, 3, 0.2)
    # fp16 subnormals (below 6.1e-5) and their low parts, fp32 subnormals, signed zeros
    sub = np.concatenate([rng.uniform(-6.1e-5, 6.1e-5, 400), rng.uniform(-1e-7, 1e-7, 100),
                          np.array([0.0, -0.0, 1e-40, -1e-40, 5.96e-8, 2.98e-8, 6.097e-5, 6.104e-5])]).astype(np.float32)
    # rounding ties of fp32 -> fp16: exactly halfway between two halves (odd and even lower neighbours), and of the low part
    halves = rng.integers(0x0400, 0x7BFF, 300).astype(np.uint16).view(np.float16).astype(np.float32)
    ulp = np.spacing(halves.astype(np.float16)).astype(np.float32)
    ties = np.concatenate([halves + ulp / 2, -(halves + ulp / 2), halves + ulp / 2 + ulp / 4096])
    w_hh = ws[4].reshape(-1)
    w_hh[:sub.size] = sub
    w_hh[sub.size:sub.size + ties.size] = ties
    ws[2].reshape(-1)[:4] = [65504.0, -65504.0, 65503.996, -65503.996]
    ws[0][0, :3] = [65504.0, -65504.0, 32768.5]
    ws[6].reshape(-1)[-2:] = [-65504.0, 65504.0]
    ws[8][0, 0] = 65504.0
    ws[1][:3] = [np.float32(np.nan), np.float32(np.inf), 1e30]   # biases are not range-checked: copied bit for bit
    assert_pack_equal(ws)


@pytest.mark.parametrize("name", ["trained_easy3_qmix", "trained_easy3_dop", "trained_easy3_qmix_am2", "trained_easy3_qmix_am3"])
def test_pack_is_bit_identical_on_the_shipped_checkpoints(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert_pack_equal([d["w_" + k] for k in ORDER])


# ---- the refusal ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [65505.0, float("inf"), float("-inf"), float("nan"), -1e9])
@pytest.mark.parametrize("t", range(5))
def test_out_of_range_weights_leave_the_blob_and_report_like_the_host(t, bad):
    rng = np.random.default_rng(11 + t)
    ws = random_weights(rng, 10, 3, 0.5)
    w = ws[WEIGHTS[t]].reshape(-1)
    first = int(rng.integers(0, w.size // 2))
    w[first] = bad
    w[first + 1 + int(rng.integers(0, w.size // 2 - 1))] = float("inf")   # a later offender: the first one is reported
    if t < 4:
        ws[WEIGHTS[t + 1]].reshape(-1)[0] = float("nan")                   # and one in a later tensor
    rc, _, msg = host_pack(ws)
    assert rc != 0
    fill = 0x7FC00000
    got, status = device_pack(ws, fill)
    assert (got.view(np.uint32) == fill).all(), "a refused network must leave the blob untouched"
    assert status[0] == 1 and status[1] == t and status[2] == first
    assert np.array([status[3]], dtype=np.int32).view(np.float32)[0].tobytes() == np.float32(bad).tobytes()
    # FusedAgents: the previous network keeps acting; check_weights() raises the host packer's message
    args = cs.make_env_args("flight_easy", n_agents=3)
    args.n_actions, args.obs_shape, args.state_shape = 3, 4, 57
    args.rnn_hidden_dim = 64
    ag = cs.FusedAgents(args, 4)
    before = ag.packed.clone()
    with torch.no_grad():
        for k, v in zip(ORDER, ws):
            ag.net.state_dict()[k].copy_(torch.from_numpy(v))
    ag.sync_weights()
    assert torch.equal(ag.packed.view(torch.int32), before.view(torch.int32))
    with pytest.raises(_lib.CoopSearchError) as e:
        ag.check_weights()
    assert str(e.value) == msg
    with pytest.raises(_lib.CoopSearchError) as e:   # and load_weights refuses it with the same text
        ag.load_weights()
    assert str(e.value) == msg


# ---- sync_weights: no host synchronisation, and the fused agents follow `net` -----------------------------------------------

def agent_args(env_name, n=3):
    args = cs.make_env_args(env_name, n_agents=n)
    env = cs.BatchedFlightEnv(args, batch=4)
    cs.apply_env_info(args, env)
    return args, env


@pytest.mark.parametrize("env_name", ["flight_easy", "flight"])
def test_sync_weights_never_synchronises_and_the_agents_follow_net(env_name):
    args, env = agent_args(env_name)
    B = 4
    ag = cs.FusedAgents(args, B, seed=3)
    torch.manual_seed(7)
    with torch.no_grad():
        for p in ag.net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ag.sync_weights()
        with pytest.raises(RuntimeError):
            ag.load_weights()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    ag.check_weights()
    # the fused forward on the new weights against the network in torch
    obs = env.get_obs().contiguous()
    ag.init_hidden()
    ag.choose_action(obs, 0.0, True, want_q=True)
    n, A = args.n_agents, args.n_actions
    last = torch.zeros(B, n, A, device="cuda")
    ids = torch.eye(n, device="cuda").expand(B, n, n)
    x = torch.cat([obs, last, ids], 2).reshape(B * n, -1)
    with torch.no_grad():
        q, _ = ag.net(x, torch.zeros(B * n, 64, device="cuda"))
    assert (ag.q.reshape(B * n, A) - q).abs().max().item() <= 1e-4


# ---- Runner ------------------------------------------------------------------------------------------------------------------

ARGS_FN = {"qmix": cs.get_mixer_args, "dop": cs.get_dop_args, "reinforce": cs.get_reinforce_args}


def run_args(alg, env_name, n, B, root, **over):
    args = cs.make_env_args(env_name, n_agents=n)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 101)
    cs.apply_env_info(args, env)
    args.alg = alg
    ARGS_FN[alg](args, seed=17)
    args.n_episodes, args.train_steps, args.batch_size, args.buffer_size = 1, 1, 32, 2 * B
    args.evaluate_cycle, args.save_cycle, args.evaluate_epoch = 3, 4, B
    args.model_dir, args.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
    for k, v in over.items():
        setattr(args, k, v)
    return args, env


@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_an_epoch_between_evaluation_and_save_points_never_synchronises(alg, tmp_path):
    args, env = run_args(alg, "flight_easy", 3, 64, str(tmp_path), evaluate_cycle=4, save_cycle=3)
    r = rn.Runner(env, args)
    modes, quiet = [], {"n": 0}

    def host_side(fn):   # evaluation and save points: the host waits there anyway
        def wrapped(*a, **k):
            prev = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode(0)
            quiet["n"] += 1
            try:
                return fn(*a, **k)
            finally:
                torch.cuda.set_sync_debug_mode(prev)
        return wrapped
    r.evaluate = host_side(r.evaluate)
    r.save_results = host_side(r.save_results)
    r.learner.save_model = host_side(r.learner.save_model)
    r.agents.check_weights = host_side(r.agents.check_weights)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r.run(0, n_epoch=8)
        modes.append(torch.cuda.get_sync_debug_mode())
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert modes == [2] and quiet["n"] > 0
    assert len(r.targets_find) == 2


def learner_state(lr):
    nets = {"qmix": ("eval_rnn", "target_rnn", "eval_qmix_net", "target_qmix_net"),
            "dop": ("actor", "eval_critic", "target_critic", "eval_mixer_net", "target_mixer_net"),
            "reinforce": ("eval_rnn",)}
    opts = {"qmix": ("optimizer",), "dop": ("agent_optimizer", "critic_optimizer", "mixer_optimizer"), "reinforce": ("rnn_optimizer",)}
    alg = "qmix" if hasattr(lr, "eval_qmix_net") else ("dop" if hasattr(lr, "actor") else "reinforce")
    out = {}
    for m in nets[alg]:
        for k, v in getattr(lr, m).state_dict().items():
            out[f"{m}.{k}"] = v
    for o in opts[alg]:
        for i, st in getattr(lr, o).state_dict()["state"].items():
            for k, v in st.items():
                out[f"{o}.{i}.{k}"] = v if torch.is_tensor(v) else torch.tensor(v)
    return out


def hand_loop(alg, env_name, n, B, root, n_epoch):
    """INTEGRATION.md section 3's loop, written out: the same calls as Runner.run, with load_weights() after every learn."""
    args, env = run_args(alg, env_name, n, B, root)
    rn.apply_run_defaults(args)
    learner = rn.LEARNERS[alg](args, "cuda")
    agents = cs.FusedAgents(args, B, "cuda", net=learner.actor if alg == "dop" else learner.eval_rnn, seed=args.seed)
    sched = cs.EpsilonSchedule(args, B, "cuda")
    col = cs.EpisodeCollector(env, sched)
    buf = cs.DeviceReplayBuffer(args, args.buffer_size, "cuda") if args.off_policy else None
    model_path = args.model_dir + rn.run_name(args)
    os.makedirs(model_path, exist_ok=True)
    evals, train_steps = [], 0
    for epoch in range(n_epoch):
        if epoch % args.evaluate_cycle == 0:
            evals.append(cs.evaluate(env, agents.policy(0.0, True), math.ceil(args.evaluate_epoch / B)))
        if buf is not None:
            col.generate_episodes(agents=agents, evaluate=False, episode_num=0, into=buf)
            batches = [buf.sample(min(buf.current_size, args.batch_size)) for _ in range(1)]
        else:
            batches = [col.generate_episodes(agents=agents, evaluate=False, episode_num=0)[0]]
        for batch in batches:
            if alg == "qmix":
                learner.learn(batch, None, train_steps)
            else:
                learner.learn(batch, None, train_steps, sched.values[0])
            agents.load_weights()
            if train_steps > 0 and train_steps % args.save_cycle == 0:
                learner.save_model(rn.get_model_idx(model_path))
            train_steps += 1
    return dict(learner=learner_state(learner), ring=None if buf is None else {k: v[:buf.current_size] for k, v in buf.buffers.items()},
                eps=sched.values.clone(), evals=evals, model_path=model_path, packed=agents.packed)


def checkpoints(path):
    return {f: torch.load(os.path.join(path, f), map_location="cuda") for f in sorted(os.listdir(path))}


def max_diff(a, b):
    return max(((x.double() - y.double()).abs().max().item() if x.numel() else 0.0) for x, y in zip(a, b)) if a else 0.0


@pytest.mark.parametrize("alg, env_name, B", [("qmix", "flight_easy", 16), ("dop", "flight_easy", 16),
                                               ("reinforce", "flight_easy", 16), ("qmix", "flight", 8)])
def test_runner_equals_the_hand_written_loop(alg, env_name, B, tmp_path):
    """Runner.run(0, n_epoch=6) against the explicit loop with load_weights(), from the same seeds.  The hand loop runs twice
    first: if two identical runs differ (an order-dependent reduction in some torch op), their spread is the tolerance --
    it is 0 (bitwise) when they agree, as they do on this stack."""
    n = 3
    h1 = hand_loop(alg, env_name, n, B, str(tmp_path / "h1"), 6)
    h2 = hand_loop(alg, env_name, n, B, str(tmp_path / "h2"), 6)
    keys = sorted(h1["learner"])
    spread = max_diff([h1["learner"][k] for k in keys], [h2["learner"][k] for k in keys])
    args, env = run_args(alg, env_name, n, B, str(tmp_path / "r"))
    r = rn.Runner(env, args)
    r.run(0, n_epoch=6)
    got = learner_state(r.learner)
    assert sorted(got) == keys
    d = max_diff([got[k] for k in keys], [h1["learner"][k] for k in keys])
    assert d <= spread, (d, spread)
    if spread == 0:
        assert torch.equal(r.agents.packed.view(torch.int32), h1["packed"].view(torch.int32))
        assert torch.equal(r.schedule.values, h1["eps"])
        if h1["ring"] is not None:
            for k, v in h1["ring"].items():
                assert torch.equal(r.buffer.buffers[k][:r.buffer.current_size], v), k
        assert [tuple(e) for e in h1["evals"]] == list(zip(r.win_rates, r.episode_rewards, r.targets_find))
    want, have = checkpoints(h1["model_path"]), checkpoints(r.model_path)
    assert sorted(have) == sorted(want) and have
    for f in want:
        assert sorted(have[f]) == sorted(want[f])
        assert max_diff([have[f][k] for k in sorted(want[f])], [want[f][k] for k in sorted(want[f])]) <= spread, f


@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_artefacts_checkpoints_and_resume(alg, tmp_path):
    args, env = run_args(alg, "flight_easy", 3, 16, str(tmp_path), save_cycle=2)
    r = rn.Runner(env, args)
    r.run(5, n_epoch=7)
    assert os.path.basename(r.result_path) == rn.run_name(args) == f"flight_easy_Seed17_{alg}_3a15t(AM0TM0)"
    rewards = np.load(os.path.join(r.result_path, "episode_rewards_5.npy"))
    found = np.load(os.path.join(r.result_path, "targets_find_5.npy"))
    assert rewards.shape == found.shape == (3,)   # evaluations at epochs 0, 3, 6
    assert np.allclose(found, r.targets_find) and np.allclose(rewards, r.episode_rewards)
    idx = sorted({int(f.split("_")[0]) for f in os.listdir(r.model_path)})
    assert idx == [1, 2, 3]   # train steps 2, 4, 6
    # the newest checkpoint loads back into a fresh learner and into FusedAgents.net, and resuming picks it
    acting = r.learner.actor if alg == "dop" else r.learner.eval_rnn
    r.agents.check_weights()
    want = {k: v.clone() for k, v in acting.state_dict().items()}
    args2, env2 = run_args(alg, "flight_easy", 3, 16, str(tmp_path), load_model=True)
    r2 = rn.Runner(env2, args2)
    acting2 = r2.learner.actor if alg == "dop" else r2.learner.eval_rnn
    for k, v in acting2.state_dict().items():
        assert torch.equal(v, want[k]), k
    assert r2.agents.net is acting2
    # the resumed agents act with the loaded network: their blob is the host packer's of it
    rc, blob, msg = host_pack([want[k].cpu().numpy() for k in ORDER])
    assert rc == 0, msg
    assert np.array_equal(r2.agents.packed.view(torch.int32).cpu().numpy(), blob)


def test_pack_after_learner_steps(tmp_path):
    args, env = run_args("qmix", "flight_easy", 3, 16, str(tmp_path))
    r = rn.Runner(env, args)
    r.run(0, n_epoch=4)
    ws = [r.agents.net.state_dict()[k].cpu().numpy() for k in ORDER]
    assert_pack_equal(ws)
    rc, blob, _ = host_pack(ws)
    assert np.array_equal(r.agents.packed.view(torch.int32).cpu().numpy(), blob)
