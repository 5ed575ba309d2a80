"""GPU tests of the 'next' rows f1 / f4: the batched episode collector against episode dicts
captured from the reference's own RolloutWorker.generate_episode, and the evaluation harness against the
random-policy curves the reference ships."""
import json
import os

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu
KEYS = ["o", "s", "u", "r", "avail_u", "o_next", "s_next", "avail_u_next", "u_onehot", "padded", "terminated"]


@pytest.mark.parametrize("name", ["episode_easy_n3_am0_s0_a1", "episode_easy_n5_am0_s0_a1", "episode_flight_n3_am3_s3_a2"])
@pytest.mark.parametrize("closed_loop", [False, True])
def test_collector_matches_reference_episode_dict(name, closed_loop):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    args = cs.make_env_args(meta["env"], n_agents=meta["n_agents"], agent_mode=meta["agent_mode"])
    B = 3   # three copies of the same episode
    env = cs.BatchedFlightEnv(args, batch=B, seeds=[meta["seed"]] * B)
    env.seed([meta["seed"]] * B)   # generate_episode's own reset() is the first RNG consumer after the seed
    table = torch.from_numpy(z["actions_table"].astype(np.int64)).cuda()      # [T, n]
    acts = table[:, None, :].expand(-1, B, -1).contiguous()
    col = cs.EpisodeCollector(env)
    if closed_loop:
        ep, rew, win, found = col.generate_episodes(policy=lambda o, s, last, t: acts[t])
    else:
        ep, rew, win, found = col.generate_episodes(actions=acts)
    assert set(ep) == set(KEYS)
    for k in KEYS:
        want = z[k][0]
        for b in range(B):
            got = ep[k][b].cpu().numpy()
            assert got.shape == want.shape, (k, got.shape, want.shape)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-6, err_msg=f"{name} key {k}")
    assert rew.tolist() == [float(meta["episode_reward"])] * B
    assert win.tolist() == [meta["win_tag"]] * B and found.tolist() == [meta["targets_find"]] * B


def _random_curves():
    """tests/golden/random_curves.json: 1500 episodes of the IMPORTED reference env under iid uniform actions per
    configuration (gen_golden.py:capture_random_curves, regenerated bit-identically by its main()), next to the 100-episode
    curves the reference ships (result/flight_easy_Seed0_random_*a15t(AM*TM0)/average_res_529.npy)."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "random_curves.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("n,agent_mode", [(3, 0), (5, 0), (3, 3), (3, 2)])
def test_random_policy_curve_matches_reference_results(n, agent_mode):
    """4096 on-device episodes against (a) the 1500-episode curve of the imported reference (s.e. <= 0.9 points: +-2.0 at
    every printed index) and (b) the curve the reference ships (mean of 100 replays, s.e. 2-3 points: +-3.5; for AM2 the
    shipped sample is 2 sigma low at four indices -- its own 1500-episode rerun says so -- and gets +-5.5)."""
    rc = _random_curves()
    ent = [c for c in rc["curves"] if c["n_agents"] == n and c["agent_mode"] == agent_mode][0]
    idx = rc["index"]
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n, agent_mode=agent_mode), batch=4096)
    g = torch.Generator("cuda").manual_seed(123)
    curve = cs.collect_experiment_data(env, cs.random_policy(g))
    got = curve[idx]
    assert curve.shape == (200,) and (np.diff(curve) >= -1e-9).all()
    np.testing.assert_allclose(got, ent["at_index"], rtol=0, atol=2.0)
    np.testing.assert_allclose(curve, ent["curve"], rtol=0, atol=2.5)          # the whole curve, not only eight points
    np.testing.assert_allclose(got, ent["shipped_100_episodes_at_index"], rtol=0, atol=5.5 if agent_mode == 2 else 3.5)
    win_rate, reward, found = cs.evaluate(env, cs.random_policy(g))
    assert 0.0 <= win_rate <= 1.0 and abs(found / 15 * 100 - ent["at_index"][-1]) < 2.5 and reward < 0


@pytest.mark.parametrize("env_name", ["flight_easy", "flight"])
def test_closed_loop_collect_store_sample(env_name):
    """f1 + f2 + f3 together: a recurrent policy picks the actions of all (env, agent) pairs in one forward per step,
    the collector builds the episode batch, the HBM replay buffer stores and samples it."""
    B = 64 if env_name == "flight" else 256
    args = cs.make_env_args(env_name, n_agents=3)
    env = cs.BatchedFlightEnv(args, batch=B)
    cs.apply_env_info(args, env)
    torch.manual_seed(3)
    agents = cs.BatchedAgents(args, B)
    g = torch.Generator("cuda").manual_seed(5)
    ep, rew, win, found = cs.EpisodeCollector(env).generate_episodes(policy=agents.policy(0.3, False, g))
    T = args.episode_limit
    assert ep["o"].shape == (B, T, 3, 2504 if env_name == "flight" else 4) and ep["u_onehot"].shape == (B, T, 3, 3)
    real = ep["padded"][:, :, 0] == 0
    assert (ep["u_onehot"].sum(-1)[real] == 1).all() and (ep["u_onehot"][~real] == 0).all()
    assert torch.equal((ep["r"][:, :, 0] * real).sum(1), rew)
    assert (ep["terminated"][:, -1, 0] == 1).all()
    rb = cs.DeviceReplayBuffer(args, 2 * B + 10)
    rb.store_episode(ep)
    rb.store_episode(ep)
    rb.store_episode({k: v[:20] for k, v in ep.items()})     # wraps around
    assert rb.current_size == 2 * B + 10 and rb.current_idx == 10
    s = rb.sample(32, generator=g)
    assert s["o"].shape == (32, T, 3, ep["o"].shape[-1]) and s["s"].device.type == "cuda"
    assert torch.equal(rb.buffers["r"][:10], ep["r"][10:20])


@pytest.mark.parametrize("T,B,n,w,S", [(200, 64, 3, 4, 57), (50, 7, 5, 4, 65), (20, 5, 3, 2504, 57), (9, 3, 1, 4, 49)])
def test_episode_assembly_kernel_equals_torch_definition(T, B, n, w, S):
    """cs_store_episodes (csrc/episodes.hip) against the stock-torch statement of rollout.py:66-76,105-132."""
    from cooperative_search_amd.collector import assemble_episodes, assemble_episodes_torch
    g = torch.Generator(device="cuda").manual_seed(T * 1000 + B)
    o = torch.rand(T + 1, B, n, w, device="cuda", generator=g)
    s = torch.rand(T + 1, B, S, device="cuda", generator=g)
    u = torch.randint(0, 3, (T, B, n), device="cuda", generator=g)
    r = torch.randint(-3, 111, (T, B), device="cuda", generator=g).float()
    end = torch.randint(1, T + 5, (B,), device="cuda", generator=g)           # some episodes never terminate
    term = (torch.arange(T, device="cuda")[:, None] >= (end - 1)[None, :])   # monotone, like a frozen env
    a = assemble_episodes(o, s, u, r, term, 3)
    b = assemble_episodes_torch(o, s, u, r, term, 3)
    assert set(a) == set(b)
    for k in b:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    # scattered slots of a larger ring
    ring = {k: torch.full((B + 3,) + tuple(v.shape[1:]), -7.0, device="cuda") for k, v in b.items()}
    slots = torch.randperm(B + 3, device="cuda", generator=g)[:B]
    assemble_episodes(o, s, u, r, term, 3, out=ring, slots=slots)
    untouched = torch.ones(B + 3, dtype=torch.bool, device="cuda")
    untouched[slots] = False
    for k in b:
        assert torch.equal(ring[k][slots], b[k]), k
        assert (ring[k][untouched] == -7.0).all()


def off_boundary(shape, device="cuda"):
    """A contiguous float32 tensor of `shape` that starts one float into an allocation: 4 bytes past a 16-byte boundary."""
    numel = int(np.prod(shape))
    base = torch.zeros(numel + 4, device=device)
    view = base[1:1 + numel].view(shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def t_chunks(B, rows):
    """cs_store_episodes' own rule (csrc/episodes.hip): the time rows of an env are split until B * chunks reaches 2048 blocks."""
    chunks = 1
    while B * chunks < 2048 and chunks < rows:
        chunks *= 2
    return chunks


def assert_all_kinds_of_episode(term):
    """term [T, B]: some episode terminates at its first step, some in the middle, some never."""
    first = term.to(torch.int64).argmax(0)
    ended = term.any(0)
    T = term.shape[0]
    assert bool((ended & (first == 0)).any()) and bool((ended & (first > 0) & (first < T - 1)).any()) and bool((~ended).any())


# (T, B, n, w, S, what) -- each case takes a branch the host picks from a shape or a pointer (cs_store_episodes):
#   vec4 = n * w % 4 == 0 and o_tab, out->o, out->o_next on 16-byte boundaries, else k_episode_rows<1>; chunks as t_chunks
BRANCH_CASES = [
    (20, 7, 3, 5, 57, "width"),          # n * w = 15: the first clause fails
    (20, 7, 3, 4, 57, "o_tab"),          # n * w = 12, the table 4 bytes off: the second clause fails
    (20, 7, 3, 4, 57, "o"),              # ... the destination of o: the third
    (20, 7, 3, 4, 57, "o_next"),         # ... the destination of o_next: the fourth
    (3, 2053, 3, 4, 57, "unsplit"),      # B >= 2048: chunks == 1, one block per env walks all of T (k_episode_rows<4>)
]


@pytest.mark.parametrize("T,B,n,w,S,what", BRANCH_CASES, ids=[c[-1] for c in BRANCH_CASES])
def test_episode_assembly_scalar_copies_and_unsplit_grid(T, B, n, w, S, what):
    """k_episode_rows<1> (every clause of the host's vec4 rule, one at a time) and the chunks == 1 grid against the stock-torch
    statement, into scattered slots of a larger ring whose other slots keep their fill."""
    from cooperative_search_amd.collector import assemble_episodes, assemble_episodes_torch
    g = torch.Generator(device="cuda").manual_seed(T * 1000 + B)
    o = torch.rand(T + 1, B, n, w, device="cuda", generator=g)
    s = torch.rand(T + 1, B, S, device="cuda", generator=g)
    u = torch.randint(0, 3, (T, B, n), device="cuda", generator=g)
    r = torch.randint(-3, 111, (T, B), device="cuda", generator=g).float()
    end = torch.randint(1, T + 5, (B,), device="cuda", generator=g)           # some episodes never terminate
    end[:3] = torch.tensor([1, T + 2, T // 2 + 1], device="cuda")             # at the first step, never, in the middle
    term = (torch.arange(T, device="cuda")[:, None] >= (end - 1)[None, :])   # monotone, like a frozen env
    assert_all_kinds_of_episode(term)
    if what == "o_tab":
        o = off_boundary(o.shape).copy_(o)
    b = assemble_episodes_torch(o, s, u, r, term, 3)
    ring = {k: torch.full((B + 3,) + tuple(v.shape[1:]), -7.0, device="cuda") for k, v in b.items()}
    if what in ("o", "o_next"):
        ring[what] = off_boundary(ring[what].shape).fill_(-7.0)
    # the branch, by the host's own rule
    aligned = [t.data_ptr() % 16 == 0 for t in (o, ring["o"], ring["o_next"])]
    if what == "width":
        assert (n * w) % 4 != 0 and all(aligned)
    elif what == "unsplit":
        assert B >= 2048 and t_chunks(B, T) == 1 and (n * w) % 4 == 0 and all(aligned)
    else:
        assert (n * w) % 4 == 0 and aligned == [what != k for k in ("o_tab", "o", "o_next")]
        assert (o if what == "o_tab" else ring[what]).data_ptr() % 16 != 0
    if what != "unsplit":
        assert t_chunks(B, T) > 1
    if what in ("width", "o_tab", "unsplit"):   # fresh destinations are torch allocations: aligned
        a = assemble_episodes(o, s, u, r, term, 3)
        for k in b:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    slots = torch.randperm(B + 3, device="cuda", generator=g)[:B]
    assemble_episodes(o, s, u, r, term, 3, out=ring, slots=slots)
    untouched = torch.ones(B + 3, dtype=torch.bool, device="cuda")
    untouched[slots] = False
    for k in b:
        assert torch.equal(ring[k][slots], b[k]), k
        assert (ring[k][untouched] == -7.0).all() and int(untouched.sum()) == 3


def test_generate_episodes_straight_into_the_replay_ring():
    args = cs.make_env_args("flight_easy", n_agents=3)
    B = 48
    env = cs.BatchedFlightEnv(args, batch=B, freeze_done=True)
    cs.apply_env_info(args, env)
    col = cs.EpisodeCollector(env)
    rb_a, rb_b = cs.DeviceReplayBuffer(args, 100), cs.DeviceReplayBuffer(args, 100)
    for rnd in range(3):   # 144 episodes into 100 slots: the third batch wraps
        acts = torch.randint(0, 3, (args.episode_limit, B, 3), device="cuda",
                             generator=torch.Generator(device="cuda").manual_seed(rnd))
        env.seed(np.arange(B) + 100 * rnd)
        ep, rew, win, found = col.generate_episodes(actions=acts, init=True)
        rb_a.store_episode(ep)
        env.seed(np.arange(B) + 100 * rnd)
        ep2, rew2, win2, found2 = col.generate_episodes(actions=acts, init=True, into=rb_b)
        assert ep2 is None and torch.equal(rew, rew2) and torch.equal(found, found2)
        assert (rb_a.current_idx, rb_a.current_size) == (rb_b.current_idx, rb_b.current_size)
        filled = rb_a.current_size
        for k in rb_a.buffers:
            assert torch.equal(rb_a.buffers[k][:filled], rb_b.buffers[k][:filled]), (rnd, k)


def _tagged_batch(rb, first_seq, k):
    """k episodes whose every element of every key carries the episode's sequence number (+ a per-key offset)."""
    seq = torch.arange(first_seq, first_seq + k, dtype=torch.float32, device="cuda")
    d = {}
    for j, (key, buf) in enumerate(rb.buffers.items()):
        d[key] = (seq + 0.01 * j).reshape((k,) + (1,) * (buf.dim() - 1)).expand((k,) + tuple(buf.shape[1:])).contiguous()
    return d


@pytest.mark.parametrize("route", ["store_episode", "cs_store_episodes"])
def test_replay_ring_contents_match_reference_recordings(route):
    """Row f2 on the device (common/replay_buffer.py:63-101): every recorded store sequence of the REFERENCE ReplayBuffer
    (tests/golden/replay_indices.json, gen_golden.py:capture_replay_indices) is replayed on the HBM ring with episodes
    tagged by sequence number; after every store the ring's contents must sit in the slots the reference handed out, and
    current_idx / current_size / the latest-k slots (and what sample_latest returns) must be the recorded ones.
    route 'cs_store_episodes': the episodes are assembled by the HIP kernel straight into the ring slots
    (collector.assemble_episodes(out=rb.buffers, slots=...), what generate_episodes(into=rb) does)."""
    import types
    from cooperative_search_amd.collector import assemble_episodes
    cases = json.load(open(os.path.join(GOLDEN_DIR, "replay_indices.json")))
    args = types.SimpleNamespace(n_actions=3, n_agents=3, state_shape=57, obs_shape=4, episode_limit=4, conv=False, map_size=50)
    T, n, A = args.episode_limit, args.n_agents, args.n_actions
    for case in cases:
        size = case["size"]
        rb = cs.DeviceReplayBuffer(args, size, device="cuda")
        for buf in rb.buffers.values():
            buf.fill_(-1.0)
        want_tag = np.full(size, -1.0)          # sequence number the reference's slot holds
        seq = 0
        for st in case["steps"]:
            k = st["inc"]
            if route == "store_episode":
                rb.store_episode(_tagged_batch(rb, seq, k))
            else:
                # raw rollout tables [T(+1), k, ...] whose reward column carries the sequence number; never terminated, so
                # no step is padded and r[slot, t] = seq for every t
                o = torch.zeros(T + 1, k, n, 4, device="cuda")
                s = torch.zeros(T + 1, k, 57, device="cuda")
                tagv = torch.arange(seq, seq + k, dtype=torch.float32, device="cuda")
                o[:] = tagv[None, :, None, None]
                s[:] = tagv[None, :, None] + 0.5
                u = torch.zeros(T, k, n, dtype=torch.int64, device="cuda")
                r = tagv[None, :].expand(T, k).contiguous()
                term = torch.zeros(T, k, dtype=torch.bool, device="cuda")
                slots = torch.as_tensor(rb._get_storage_idx(inc=k), device="cuda")
                assemble_episodes(o, s, u, r, term, A, out=rb.buffers, slots=slots)
            want_tag[np.asarray(st["idx"])] = np.arange(seq, seq + k)
            seq += k
            assert (rb.current_idx, rb.current_size) == (st["current_idx"], st["current_size"])
            got_r = rb.buffers["r"][:, :, 0].cpu().numpy()
            if route == "store_episode":
                j_r = list(rb.buffers).index("r")
                np.testing.assert_allclose(got_r, np.where(want_tag >= 0, want_tag + 0.01 * j_r, -1.0)[:, None].repeat(T, 1), rtol=0, atol=1e-4)
                for j, (key, buf) in enumerate(rb.buffers.items()):     # every key of a slot belongs to the same episode
                    flat = buf.reshape(size, -1).cpu().numpy()
                    np.testing.assert_allclose(flat, np.where(want_tag >= 0, want_tag + 0.01 * j, -1.0)[:, None].repeat(flat.shape[1], 1),
                                               rtol=0, atol=1e-4, err_msg=key)
            else:
                np.testing.assert_array_equal(got_r, want_tag[:, None].repeat(T, 1))
                filled = want_tag >= 0
                np.testing.assert_array_equal(rb.buffers["o"][:, :, 0, 0].cpu().numpy()[filled], want_tag[filled, None].repeat(T, 1))
                np.testing.assert_array_equal(rb.buffers["s_next"][:, :, 0].cpu().numpy()[filled], want_tag[filled, None].repeat(T, 1) + 0.5)
                assert (rb.buffers["o"][:, :, 0, 0].cpu().numpy()[~filled] == -1.0).all()
            if st["latest3"] is not None:
                kk = min(3, rb.current_size)
                assert rb.latest_indices(kk) == st["latest3"]
                lat = rb.sample_latest(kk)["r"][:, 0, 0].cpu().numpy()
                off = 0.01 * list(rb.buffers).index("r") if route == "store_episode" else 0.0
                np.testing.assert_allclose(lat, want_tag[np.asarray(st["latest3"])] + off, rtol=0, atol=1e-4)
        # sample(): uniform over the filled part, with replacement (:63-68) -- every drawn row is a stored episode
        g = torch.Generator(device="cuda").manual_seed(size)
        smp = rb.sample(64, generator=g)["r"][:, 0, 0].cpu().numpy()
        off = 0.01 * list(rb.buffers).index("r") if route == "store_episode" else 0.0
        assert np.isin(np.round(smp - off).astype(int), want_tag[want_tag >= 0].astype(int)).all()


def test_generate_episodes_into_ring_follows_reference_slots():
    """The collector's `into=` route against the reference's recorded slot sequence (case size 16: stores of 1..7 episodes):
    an env of `inc` copies is run per store, the ring must hold the batch's rewards in the recorded slots."""
    cases = json.load(open(os.path.join(GOLDEN_DIR, "replay_indices.json")))
    case = [c for c in cases if c["size"] == 16][0]
    args = cs.make_env_args("flight_easy", n_agents=3)
    envs = {}
    rb = None
    want = {}
    for step_no, st in enumerate(case["steps"][:16]):
        k = st["inc"]
        if k not in envs:
            envs[k] = cs.BatchedFlightEnv(args, batch=k, freeze_done=True)
            cs.apply_env_info(args, envs[k])
        env = envs[k]
        if rb is None:
            rb = cs.DeviceReplayBuffer(args, case["size"])
        env.seed(np.arange(k) + 1000 * step_no)
        acts = torch.randint(0, 3, (args.episode_limit, k, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(step_no))
        col = cs.EpisodeCollector(env)
        ep, rew, win, found = col.generate_episodes(actions=acts, init=True)
        env.seed(np.arange(k) + 1000 * step_no)
        ep2, rew2, _, _ = col.generate_episodes(actions=acts, init=True, into=rb)
        assert ep2 is None and torch.equal(rew, rew2)
        assert (rb.current_idx, rb.current_size) == (st["current_idx"], st["current_size"])
        for j, slot in enumerate(st["idx"]):
            want[slot] = {key: ep[key][j].clone() for key in ep}
        for slot, epd in want.items():
            for key in epd:
                assert torch.equal(rb.buffers[key][slot], epd[key]), (step_no, slot, key)
