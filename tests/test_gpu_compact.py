"""GPU tests of the map-once episode storage on the flight variant: the fact the format rests on,
cs_collect_flight against cs_rollout_policy_flight, cs_store_episodes_compact against the torch definition, the compact
collector against the dense one, the memory the collection takes, the fused learners on compact samples, and the Runner."""
import contextlib
import os

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import runner as rn
from cooperative_search_amd.agents import AgentRNN, rnn_input_shape
from cooperative_search_amd.collector import assemble_episodes_compact, assemble_episodes_torch
from cooperative_search_amd.replay import COMPACT_KEYS, KEYS, compact_from_dense, expand_compact
from test_compact_cpu import ARGS_FN, compare_learn_on, tables
from test_gpu_runner import ORDER, host_pack

pytestmark = pytest.mark.gpu
CELLS = 2500
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def flight(n, B, time_limit=40, alg="qmix", seed0=11):
    """(args, env) of the flight variant with the learner fields of `alg`; equal arguments give equal envs."""
    args = cs.make_env_args("flight", n_agents=n)
    args.time_limit = time_limit
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + seed0)
    cs.apply_env_info(args, env)
    args.alg = alg
    ARGS_FN[alg](args, seed=5)
    return args, env


def fused_agents(args, B, trained=False):
    """Equal calls give equal networks: a fresh one, or the shipped QMIX checkpoint of this team size (its greedy actions vary)."""
    torch.manual_seed(21)
    net = None
    if trained:
        z = np.load(os.path.join(GOLDEN, f"trained_flight{args.n_agents}_qmix.npz"))
        net = AgentRNN(rnn_input_shape(args), args)
        net.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w_")})
    return cs.FusedAgents(args, B, net=net, seed=9)


# ---- the fact the format rests on --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 5])
def test_an_agents_own_floats_are_the_head_of_the_state(n):
    """emit<N> writes one float4 to an agent's observation tail and to state[4i..4i+3]; and every agent's map is the env's."""
    B = 64
    args, env = flight(n, B, time_limit=12)
    g = torch.Generator(device="cuda").manual_seed(n)

    def check():
        obs, state = env.get_obs(), env.get_state()
        assert torch.equal(obs[:, :, CELLS:], state[:, :4 * n].reshape(B, n, 4))
        assert torch.equal(obs[:, :, :CELLS], env.raw()["prob"].reshape(B, 1, CELLS).expand(B, n, CELLS))
    env.reset(init=True)
    check()
    for t in range(16):   # past the time limit: frozen envs too
        env.step(torch.randint(0, 3, (B, n), device="cuda", generator=g))
        check()
    env.reset(init=False)
    check()


# ---- the closed loop ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["greedy", "epsilon_schedule", "softmax"])
@pytest.mark.parametrize("n", [3, 5])
def test_collect_flight_equals_rollout_policy_flight(n, mode):
    B, limit = 48, 24
    T = limit + 4   # the last steps find every env finished and frozen: their snapshots are plain copies
    alg = "reinforce" if mode == "softmax" else "qmix"
    runs = []
    for compact in (False, True):
        args, env = flight(n, B, limit, alg)
        env.freeze_done, env.auto_reset = True, False
        agents = fused_agents(args, B, trained=mode == "greedy")
        agents.init_hidden()
        eps = torch.linspace(0.2, 0.9, B, dtype=torch.float64, device="cuda")
        trace = torch.zeros(T, B, dtype=torch.float64, device="cuda")
        kw = dict(epsilon=0.4, evaluate=mode == "greedy")
        if mode == "epsilon_schedule":
            kw.update(eps_env=eps, anneal=0.01, min_epsilon=0.3, per_step=True, eps_trace=trace)
        entry = (env.raw()["prob"].reshape(B, CELLS).clone(), env.get_state().clone())
        out = env.collect_flight(agents, T, **kw) if compact else env.rollout_policy(agents, T, **kw)
        runs.append((out, env._blob.clone(), agents.hidden.clone(), eps, trace, entry, agents.calls))
    (d, blob_d, hid_d, eps_d, tr_d, entry, calls_d), (c, blob_c, hid_c, eps_c, tr_c, _, calls_c) = runs
    for k in ("actions", "reward", "terminated", "win"):
        assert torch.equal(c[k], d[k]), k
    assert torch.equal(eps_c, eps_d) and torch.equal(tr_c, tr_d) and torch.equal(hid_c, hid_d) and calls_c == calls_d
    assert torch.equal(blob_c, blob_d)
    assert "obs" not in c and c["map"].shape == (T + 1, B, CELLS) and c["state"].shape == (T + 1, B, 4 * n + 45)
    assert torch.equal(c["map"][0], entry[0]) and torch.equal(c["state"][0], entry[1])
    assert torch.equal(c["state"][1:], d["state"])
    for a in range(n):
        assert torch.equal(c["map"][1:], d["obs"][:, :, a, :CELLS]), a
    assert d["terminated"][limit - 1].all() and d["actions"].unique().numel() > 1
    if mode == "epsilon_schedule":
        assert (eps_d < torch.linspace(0.2, 0.9, B, dtype=torch.float64, device="cuda"))[B // 2:].all()


# ---- the assembly ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,B,n", [(20, 7, 3), (9, 5, 5), (200, 24, 3), (3, 300, 5)])
def test_store_episodes_compact_equals_the_torch_definition(T, B, n):
    lengths = [1 + (7 * j + T) % (T + 3) for j in range(B)]   # 1 .. T + 2: early terminations and episodes that never end
    m, s, o, u, r, term = (t.cuda() for t in tables(lengths, T, n, seed=T + B))
    want = compact_from_dense(assemble_episodes_torch(o, s, u, r, term, 3))
    got = assemble_episodes_compact(m, s, u, r, term)
    assert tuple(got) == COMPACT_KEYS
    for k in COMPACT_KEYS:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    # ring slots that wrap, in a ring with room to spare
    size = B + 3
    ring = {k: torch.full((size,) + tuple(v.shape[1:]), -7.0, device="cuda") for k, v in want.items()}
    slots = (torch.arange(B, device="cuda") + size - 2) % size
    assemble_episodes_compact(m, s, u, r, term, out=ring, slots=slots)
    untouched = torch.ones(size, dtype=torch.bool, device="cuda")
    untouched[slots] = False
    for k in COMPACT_KEYS:
        assert torch.equal(ring[k][slots], want[k]), k
        assert (ring[k][untouched] == -7.0).all() and int(untouched.sum()) == 3


def tables_of(lengths, T, n, cells, seed):
    """test_compact_cpu.tables for any map width: (m, s, o, u, r, term) on the device."""
    g = torch.Generator().manual_seed(seed)
    B, S = len(lengths), 4 * n + 45
    m = torch.rand(T + 1, B, cells, generator=g)
    s = torch.rand(T + 1, B, S, generator=g) * 2 - 1
    o = torch.cat([m[:, :, None, :].expand(T + 1, B, n, cells), s[..., :4 * n].reshape(T + 1, B, n, 4)], 3).contiguous()
    u = torch.randint(0, 3, (T, B, n), generator=g)
    r = torch.randint(-3, 111, (T, B), generator=g).float()
    term = torch.arange(T)[:, None] >= (torch.as_tensor(lengths) - 1)[None, :]
    return tuple(t.cuda() for t in (m, s, o, u, r, term))


# (T, B, cells, what) -- each case takes a branch the host picks from a shape or a pointer (cs_store_episodes_compact):
#   vec4 = cells % 4 == 0 and map_tab, out->map on 16-byte boundaries, else k_compact_rows<1>; the T + 1 rows of an env are
#   split into chunks until B * chunks reaches 2048 blocks
COMPACT_BRANCH_CASES = [
    (9, 5, 2501, "width"),        # cells % 4 == 1: the first clause fails
    (9, 5, 2500, "map_tab"),      # the table 4 bytes off a 16-byte boundary: the second
    (9, 5, 2500, "map"),          # the destination: the third
    (3, 2053, 12, "unsplit"),     # B >= 2048: chunks == 1, one block per env walks all T + 1 rows (k_compact_rows<4>)
]


@pytest.mark.parametrize("T,B,cells,what", COMPACT_BRANCH_CASES, ids=[c[-1] for c in COMPACT_BRANCH_CASES])
def test_store_episodes_compact_scalar_copies_and_unsplit_grid(T, B, cells, what):
    """k_compact_rows<1> (every clause of the host's vec4 rule, one at a time) and the chunks == 1 grid against the torch
    definition, into ring slots that wrap in a ring with room to spare."""
    from test_gpu_collector import assert_all_kinds_of_episode, off_boundary, t_chunks
    n = 3
    lengths = [1, T + 2, T // 2 + 1] + [1 + (7 * j + T) % (T + 3) for j in range(3, B)]   # first step, never, middle; then 1 .. T + 2
    m, s, o, u, r, term = tables_of(lengths, T, n, cells, seed=T + B)
    assert_all_kinds_of_episode(term)
    if what == "map_tab":
        m = off_boundary(m.shape).copy_(m)
    want = compact_from_dense(assemble_episodes_torch(o, s, u, r, term, 3))
    size = B + 3
    ring = {k: torch.full((size,) + tuple(v.shape[1:]), -7.0, device="cuda") for k, v in want.items()}
    if what == "map":
        ring["map"] = off_boundary(ring["map"].shape).fill_(-7.0)
    # the branch, by the host's own rule
    aligned = [t.data_ptr() % 16 == 0 for t in (m, ring["map"])]
    if what == "width":
        assert cells % 4 != 0 and all(aligned)
    elif what == "unsplit":
        assert B >= 2048 and t_chunks(B, T + 1) == 1 and cells % 4 == 0 and all(aligned)
    else:
        assert cells % 4 == 0 and aligned == [what != "map_tab", what != "map"]
        assert (m if what == "map_tab" else ring["map"]).data_ptr() % 16 != 0
    if what != "unsplit":
        assert t_chunks(B, T + 1) > 1
    if what != "map":   # fresh destinations are torch allocations: aligned
        got = assemble_episodes_compact(m, s, u, r, term)
        for k in COMPACT_KEYS:
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    slots = (torch.arange(B, device="cuda") * 5 + size - 2) % size   # a permutation of B of the size slots (size % 5 != 0), wrapping
    assert slots.unique().numel() == B
    assemble_episodes_compact(m, s, u, r, term, out=ring, slots=slots)
    untouched = torch.ones(size, dtype=torch.bool, device="cuda")
    untouched[slots] = False
    for k in COMPACT_KEYS:
        assert torch.equal(ring[k][slots], want[k]), k
        assert (ring[k][untouched] == -7.0).all() and int(untouched.sum()) == 3


# ---- the collector -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 5])
def test_compact_collection_equals_the_dense_one(n):
    B, limit = 32, 40
    got = {}
    for compact in (False, True):
        args, env = flight(n, B, limit)
        agents = fused_agents(args, B)
        col = cs.EpisodeCollector(env, cs.EpsilonSchedule(args, B))
        ring = (cs.CompactReplayBuffer if compact else cs.DeviceReplayBuffer)(args, B + 5)
        ring._get_storage_idx(inc=B)   # the next store wraps
        kw = dict(compact=True) if compact else {}
        first = col.generate_episodes(agents=agents, evaluate=False, episode_num=0, **kw)
        env.seed(np.arange(B) + 500)
        agents.calls = 0
        eps = col.schedule.values.clone()
        second = col.generate_episodes(agents=agents, evaluate=False, episode_num=1, init=True, **kw)   # init: a fresh map
        env.seed(np.arange(B) + 500)
        agents.calls = 0
        col.schedule.values = eps.clone()
        into = col.generate_episodes(agents=agents, evaluate=False, episode_num=1, init=True, into=ring, **kw)
        assert into[0] is None and all(torch.equal(a, b) for a, b in zip(into[1:], second[1:]))
        slots = (torch.arange(B, device="cuda") + B) % (B + 5)
        for k, v in second[0].items():
            assert torch.equal(ring.buffers[k][slots], v), k
        got[compact] = (first, second, col.schedule.values)
    for (ep_d, *rest_d), (ep_c, *rest_c) in zip(got[False][:2], got[True][:2]):
        assert tuple(ep_c) == COMPACT_KEYS
        full = expand_compact(ep_c, n, 3)
        for k in KEYS:
            assert full[k].shape == ep_d[k].shape and torch.equal(full[k], ep_d[k]), k
        for a, b in zip(rest_c, rest_d):   # episode_reward, win_tag, targets_find
            assert torch.equal(a, b)
    assert torch.equal(got[False][2], got[True][2])


def test_compact_collection_is_refused_where_it_cannot_run():
    args, env = flight(3, 4, 8)
    col = cs.EpisodeCollector(env)
    with pytest.raises(ValueError, match="compact"):
        col.generate_episodes(policy=cs.random_policy(), compact=True)
    easy_args = cs.make_env_args("flight_easy", n_agents=3)
    easy = cs.BatchedFlightEnv(easy_args, batch=4)
    cs.apply_env_info(easy_args, easy)
    with pytest.raises(ValueError, match="compact"):
        cs.EpisodeCollector(easy).generate_episodes(agents=cs.FusedAgents(easy_args, 4), compact=True)
    with pytest.raises(ValueError, match="CompactReplayBuffer"):
        col.generate_episodes(agents=fused_agents(args, 4), compact=True, into=cs.DeviceReplayBuffer(args, 8))


def test_compact_collection_memory_does_not_grow_with_the_team():
    """Peak allocation growth over one compact collection into a ring, 5 agents minus 3 agents, is smaller than ONE map table
    ((T+1) * B * cells * 4 bytes): the map tables do not depend on n, and any hidden per-agent copy of the maps would add at
    least two of them."""
    B = 256
    growth = {}
    for n in (3, 5):
        args, env = flight(n, B, 200)
        agents = fused_agents(args, B)
        col = cs.EpisodeCollector(env, cs.EpsilonSchedule(args, B))
        ring = cs.CompactReplayBuffer(args, B)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        col.generate_episodes(agents=agents, evaluate=False, episode_num=0, into=ring, compact=True)
        torch.cuda.synchronize()
        growth[n] = torch.cuda.max_memory_allocated() - before
        del ring, col, agents, env
        torch.cuda.empty_cache()
    table = 201 * B * CELLS * 4
    print(f"peak growth: 3 agents {growth[3]} B, 5 agents {growth[5]} B, difference {growth[5] - growth[3]} B, one map table {table} B")
    assert growth[3] >= table          # the table itself is in the growth: the measurement sees the collection
    assert growth[5] - growth[3] < table


# ---- the learners ------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def no_sync():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("max_len", [None, 25])
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_fused_learn_on_a_compact_sample_equals_learn_on_its_expansion(alg, n, max_len):
    """1e-4 relative Frobenius, the project's pin for two unrolls of one learner in float32, per
    parameter; learn never synchronises with the host on either format."""
    B, limit = 16, 40
    args, env = flight(n, B, limit, alg)
    ring = cs.CompactReplayBuffer(args, B)
    cs.EpisodeCollector(env, cs.EpsilonSchedule(args, B)).generate_episodes(agents=fused_agents(args, B), evaluate=False,
                                                                            episode_num=0, into=ring, compact=True)
    c = ring.sample(8, generator=torch.Generator(device="cuda").manual_seed(n))
    d = expand_compact(c, n, 3)
    compare_learn_on(alg, n, limit, c, d, max_len, torch.float32, 1e-4, unroll="fused", device="cuda", guard=no_sync)


# ---- the Runner --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_runner_on_compact_episodes(alg, tmp_path):
    saved = {}
    for compact in (False, True):
        args, env = flight(3, 8, 30, alg)
        args.n_episodes, args.train_steps, args.batch_size, args.buffer_size = 1, 1, 6, 16
        args.evaluate_cycle, args.save_cycle, args.evaluate_epoch = 3, 2, 8
        root = str(tmp_path / str(compact))
        args.model_dir, args.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
        args.compact_episodes = compact
        r = rn.Runner(env, args)
        assert type(r.buffer) is (type(None) if alg == "reinforce" else cs.CompactReplayBuffer if compact else cs.DeviceReplayBuffer)
        r.run(0, n_epoch=7)
        r.agents.check_weights()
        acting = r.learner.actor if alg == "dop" else r.learner.eval_rnn
        assert r.agents.net is acting
        rc, blob, msg = host_pack([acting.state_dict()[k].cpu().numpy() for k in ORDER])   # the acting network follows the learner
        assert rc == 0, msg
        assert np.array_equal(r.agents.packed.view(torch.int32).cpu().numpy(), blob)
        for w, k in zip(r.agents.conv_w, cs.FusedAgents.CONV_KEYS):
            assert torch.equal(w, acting.state_dict()[k]), k
        assert all(torch.isfinite(p).all() for p in acting.parameters())
        saved[compact] = sorted(os.listdir(r.model_path))
        assert len(r.targets_find) == 3
        if r.buffer is not None:
            assert r.buffer.current_size == 16
    assert saved[True] == saved[False] and saved[True]   # checkpoints at the same train steps (2, 4, 6)
    assert sorted({int(f.split("_")[0]) for f in saved[True]}) == [1, 2, 3]
