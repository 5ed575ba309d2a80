"""GPU parity tests: the HIP path, called through the C ABI, against (a) golden vectors captured from the
imported reference and (b) the C oracle on identical seeds and actions.

Bars (written here, per the numerics contract in DESIGN.md section 3):
  * every integer quantity (reward, terminated, win, found flags, target_find, out flags, number of MT words
    consumed per step) is EXACT against the reference goldens and against the oracle;
  * agent positions / yaw are BIT-IDENTICAL (atol = 0) to the oracle run in its HIP-equivalent arithmetic
    (correctly rounded trig, x*x), and within 1e-9 of the reference goldens (libm pow / sin / cos differ by
    1 ulp in ~0.1 % of evaluations);
  * target positions within 1e-12 (device log vs glibc log in the polar gaussian);
  * emitted fp32 obs / state within 1e-6 of the fp64 reference values (north-star tolerance: 1e-5).
"""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from golden_util import load_trace, trace_names
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

F32_TOL = 1e-6


def make_env(meta, batch=1, seeds=None, **kw):
    args = cs.make_env_args(meta["env"], n_agents=meta["n_agents"], agent_mode=meta["agent_mode"],
                            target_mode=meta["target_mode"])
    return cs.BatchedFlightEnv(args, batch=batch, seeds=seeds, **kw)


def hdr(env):
    return env.raw()["hdr"].cpu().numpy()


def raw_state(env):
    """tgt / agent / hdr views plus the MT19937 rows in canonical form (the lane kernel twists words ahead of the
    cursor, the group kernels on demand: same stream, different `ahead`; cs_mt_canonical removes that difference)."""
    r = env.raw()
    d = {k: r[k] for k in ("tgt", "agent", "hdr")}
    d["mt"] = env.mt_canonical()
    if "prob" in r:
        d["prob"] = r["prob"]
    return d


def words(h):
    return (h[:, _lib.H_WORDS_LO].astype(np.uint32).astype(np.uint64)
            | (h[:, _lib.H_WORDS_HI].astype(np.uint32).astype(np.uint64) << np.uint64(32)))



GOLDEN_CASES = [(n, k) for n in trace_names() for k in (("group", "lane") if n.startswith("easy") else ("group",))]


@pytest.mark.parametrize("name,kernel", GOLDEN_CASES)
def test_hip_replays_reference_golden_trace(name, kernel):
    meta, z = load_trace(name)
    n, m = meta["n_agents"], 15
    flight = meta["env"] == "flight"
    env = make_env(meta, batch=1, seeds=[meta["seed"]], freeze_done=False, kernel=kernel)
    env.seed([meta["seed"]])   # golden protocol: the ctor's reset ate RNG; np.random.seed(seed) comes after it
    for e, ep in enumerate(meta["episodes"]):
        p = f"e{e}_"
        env.reset(init=ep["init"])
        raw = env.raw()
        tgt = raw["tgt"][0, :m].cpu().numpy()
        np.testing.assert_allclose(tgt, z[p + "target_pos"], rtol=0, atol=1e-12, err_msg=name + " target_pos")
        h = hdr(env)[0]
        assert [(h[_lib.H_FOUND] >> j) & 1 for j in range(m)] == list(z[p + "reset_found"])
        assert h[_lib.H_TARGET_FIND] == int(z[p + "reset_target_find"])
        ag = raw["agent"][0, :n].cpu().numpy()
        np.testing.assert_array_equal(ag[:, :2], z[p + "reset_agent_pos"])
        np.testing.assert_array_equal(ag[:, 2], z[p + "reset_yaw"])
        np.testing.assert_allclose(env.get_obs()[0, :, -4:].cpu().numpy(), z[p + "reset_obs"], rtol=0, atol=F32_TOL)
        np.testing.assert_allclose(env.get_state()[0].cpu().numpy(), z[p + "reset_state"], rtol=0, atol=F32_TOL)
        if flight:
            np.testing.assert_allclose(raw["prob"][0].cpu().numpy(), z[p + "reset_prob_map"], rtol=0, atol=F32_TOL)
            np.testing.assert_allclose(env.get_obs()[0, :, :-4].cpu().numpy().reshape(n, 50, 50),
                                       np.broadcast_to(z[p + "reset_prob_map"], (n, 50, 50)), rtol=0, atol=F32_TOL)
        pokes = {}
        if p + "poke_steps" in z:
            pokes = {int(t): k for k, t in enumerate(z[p + "poke_steps"])}
        maps = {}
        if p + "prob_map_steps" in z:
            maps = {int(t): z[p + "prob_maps"][k] for k, t in enumerate(z[p + "prob_map_steps"])}
        acts = z[p + "actions"]
        w_prev = int(words(hdr(env))[0])
        for t in range(ep["steps"]):
            tag = f"{name} {p}step {t}"
            if t in pokes:
                k = pokes[t]
                a = env.raw()["agent"]
                a[0, :n, 0:2] = torch.from_numpy(z[p + "poke_agent_pos"][k]).to(a.device)
                a[0, :n, 2] = torch.from_numpy(z[p + "poke_yaw_idx"][k] * (np.pi / 18.0)).to(a.device)
            r, term, win = env.step(torch.from_numpy(acts[t:t + 1].astype(np.int32)))
            assert int(r.item()) == int(z[p + "reward"][t]), tag + " reward"
            assert int(term.item()) == int(z[p + "terminated"][t]), tag + " terminated"
            assert int(win.item()) == int(z[p + "win"][t]), tag + " win"
            h = hdr(env)[0]
            assert h[_lib.H_TARGET_FIND] == int(z[p + "target_find"][t]), tag
            assert h[_lib.H_TIME_STEP] == int(z[p + "time_step"][t]), tag
            assert [(h[_lib.H_FOUND] >> j) & 1 for j in range(m)] == list(z[p + "found"][t]), tag + " found"
            assert [(h[_lib.H_FLAGS] >> (8 + i)) & 1 for i in range(n)] == list(z[p + "out_flag"][t]), tag + " out"
            w_now = int(words(hdr(env))[0])
            assert w_now - w_prev == 2 * int(z[p + "n_draws"][t]), tag + " draws consumed"
            w_prev = w_now
            ag = env.raw()["agent"][0, :n].cpu().numpy()
            np.testing.assert_allclose(ag[:, :2], z[p + "agent_pos"][t], rtol=0, atol=1e-9, err_msg=tag + " pos")
            np.testing.assert_allclose(ag[:, 2], z[p + "yaw"][t], rtol=0, atol=0, err_msg=tag + " yaw")
            np.testing.assert_allclose(env.get_obs()[0, :, -4:].cpu().numpy(), z[p + "obs"][t], rtol=0, atol=F32_TOL,
                                       err_msg=tag + " obs")
            np.testing.assert_allclose(env.get_state()[0].cpu().numpy(), z[p + "state"][t], rtol=0, atol=F32_TOL,
                                       err_msg=tag + " state")
            if (t + 1) in maps:
                np.testing.assert_allclose(env.raw()["prob"][0].cpu().numpy(), maps[t + 1], rtol=0, atol=F32_TOL,
                                           err_msg=tag + " prob_map")
                np.testing.assert_array_equal(env.get_obs()[0, 0, :-4].cpu().numpy(),
                                              env.raw()["prob"][0].cpu().numpy().reshape(-1))


ROLLOUT_GOLDEN_CASES = [(n, k) for n in trace_names() if n.startswith("easy") for k in ("oct", "od", "ode", "lane", "lanev")]


@pytest.mark.parametrize("name,kernel", ROLLOUT_GOLDEN_CASES)
def test_rollout_kernels_replay_reference_golden_trace(name, kernel):
    """The T-step rollout kernels against the reference's own traces, directly (the octet kernels were only
    linked to the goldens through the oracle).  64 copies of the trace's env (one full wavefront of every layout: the VEC
    variants, and the emitting wavefront of "ode") run each episode as cs_rollout launches over the recorded action table --
    one launch per stretch between two hand-placed pokes -- and every step's reward / terminated / win / obs / state, the
    header after every stretch and the draws consumed are the golden's."""
    meta, z = load_trace(name)
    n, m, B = meta["n_agents"], 15, 64
    if kernel == "lanev" and n > 5:
        pytest.skip("k_rollout_lanev serves teams of up to 5")
    seeds = [meta["seed"]] * B
    env = make_env(meta, batch=B, seeds=seeds, freeze_done=False, kernel=kernel)
    env.seed(seeds)
    for e, ep in enumerate(meta["episodes"]):
        p = f"e{e}_"
        env.reset(init=ep["init"])
        acts = z[p + "actions"][:ep["steps"]].astype(np.int32)
        pokes = {}
        if p + "poke_steps" in z:
            pokes = {int(t): k for k, t in enumerate(z[p + "poke_steps"])}
        cuts = sorted({0, ep["steps"]} | {t for t in pokes if 0 < t < ep["steps"]})
        w_prev = int(words(hdr(env))[0])
        for t0, t1 in zip(cuts[:-1], cuts[1:]):
            tag = f"{name} {p}steps {t0}..{t1 - 1} ({kernel})"
            if t0 in pokes:
                k = pokes[t0]
                a = env.raw()["agent"]
                a[:, :n, 0:2] = torch.from_numpy(z[p + "poke_agent_pos"][k]).to(a.device)
                a[:, :n, 2] = torch.from_numpy(z[p + "poke_yaw_idx"][k] * (np.pi / 18.0)).to(a.device)
            table = torch.from_numpy(np.repeat(acts[t0:t1, None, :], B, axis=1).copy())
            out = env.rollout(table)
            for key, gold in (("reward", "reward"), ("terminated", "terminated"), ("win", "win")):
                got = out[key].cpu().numpy().astype(np.int64)
                want = np.asarray(z[p + gold][t0:t1]).astype(np.int64)
                assert np.array_equal(got, np.repeat(want[:, None], B, axis=1)), f"{tag} {key}"
            obs, st = out["obs"].cpu().numpy(), out["state"].cpu().numpy()
            for b in (0, 7, 8, B - 1):
                np.testing.assert_allclose(obs[:, b], z[p + "obs"][t0:t1], rtol=0, atol=F32_TOL, err_msg=f"{tag} obs env {b}")
                np.testing.assert_allclose(st[:, b], z[p + "state"][t0:t1], rtol=0, atol=F32_TOL, err_msg=f"{tag} state env {b}")
            assert np.array_equal(obs, np.repeat(obs[:, :1], B, axis=1)) and np.array_equal(st, np.repeat(st[:, :1], B, axis=1))
            h = hdr(env)
            t = t1 - 1
            for b in (0, B - 1):
                assert h[b, _lib.H_TARGET_FIND] == int(z[p + "target_find"][t]), tag
                assert h[b, _lib.H_TIME_STEP] == int(z[p + "time_step"][t]), tag
                assert [(h[b, _lib.H_FOUND] >> j) & 1 for j in range(m)] == list(z[p + "found"][t]), tag + " found"
                assert [(h[b, _lib.H_FLAGS] >> (8 + i)) & 1 for i in range(n)] == list(z[p + "out_flag"][t]), tag + " out"
            w_now = words(h)
            assert np.all(w_now == w_now[0])
            assert int(w_now[0]) - w_prev == 2 * int(np.sum(z[p + "n_draws"][t0:t1])), tag + " draws consumed"
            w_prev = int(w_now[0])
            ag = env.raw()["agent"][:, :n].cpu().numpy()
            np.testing.assert_allclose(ag[0, :, :2], z[p + "agent_pos"][t], rtol=0, atol=1e-9, err_msg=tag + " pos")
            np.testing.assert_allclose(ag[0, :, 2], z[p + "yaw"][t], rtol=0, atol=0, err_msg=tag + " yaw")
            assert np.array_equal(ag, np.repeat(ag[:1], B, axis=0))


def compare_with_oracle(env, ob, B, n, m, tag, check_pos=True):
    h = hdr(env)
    raw = env.raw()
    ag = raw["agent"][:, :n].cpu().numpy()
    tg = raw["tgt"][:, :m].cpu().numpy()
    for b in range(B):
        oe = ob.env(b)
        c = oe.counters()
        pos, yaw, out = oe.agents()
        tp, found = oe.targets()
        assert h[b, _lib.H_TARGET_FIND] == c["target_find"], f"{tag} env {b} target_find"
        assert h[b, _lib.H_TIME_STEP] == c["time_step"], f"{tag} env {b} time_step"
        assert h[b, _lib.H_TOTAL_REWARD] == c["total_reward"], f"{tag} env {b} total_reward"
        assert (h[b, _lib.H_FLAGS] & 1) == c["win"], f"{tag} env {b} win"
        assert [(h[b, _lib.H_FOUND] >> j) & 1 for j in range(m)] == list(found), f"{tag} env {b} found"
        assert [(h[b, _lib.H_FLAGS] >> (8 + i)) & 1 for i in range(n)] == list(out), f"{tag} env {b} out"
        assert int(words(h)[b]) == oe.words_consumed(), f"{tag} env {b} MT words consumed"
        if check_pos:
            np.testing.assert_array_equal(ag[b, :, :2], pos, err_msg=f"{tag} env {b} pos")
            np.testing.assert_array_equal(ag[b, :, 2], yaw, err_msg=f"{tag} env {b} yaw")
            np.testing.assert_allclose(tg[b], tp, rtol=0, atol=1e-12, err_msg=f"{tag} env {b} targets")


@pytest.mark.parametrize("kernel", ["group", "group-ondemand", "lane", "lanev"])
@pytest.mark.parametrize("variant,n,agent_mode,target_mode,B,T", [
    ("flight_easy", 3, 0, 0, 512, 200),
    ("flight_easy", 5, 0, 0, 256, 200),
    ("flight_easy", 3, 3, 0, 128, 120),
    ("flight_easy", 3, 2, 1, 128, 120),
    ("flight_easy", 1, 1, 0, 64, 200),
    ("flight_easy", 8, 0, 0, 64, 100),
    ("flight_easy", 2, 1, 0, 100, 100),
])
def test_batched_step_matches_oracle_bit_exact(variant, n, agent_mode, target_mode, B, T, kernel):
    """Frozen-when-done batch against B oracle envs, every step: outputs exact, raw state bit-identical.
    "group-ondemand": no periodic tape refresh, the step kernel twists every word it draws itself."""
    m = 15
    seeds = (777 + 13 * np.arange(B)).astype(np.uint32)
    args = cs.make_env_args(variant, n_agents=n, agent_mode=agent_mode, target_mode=target_mode)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=True, kernel=kernel.split("-")[0],
                              step_advance=not kernel.endswith("ondemand"))
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant=variant, n_agents=n, agent_mode=agent_mode, target_mode=target_mode)
    rng = np.random.RandomState(n * 100 + agent_mode)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        compare_with_oracle(env, ob, B, n, m, "reset")
        for t in range(T):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            r, term, win = env.step(torch.from_numpy(a))
            orr, ot, ow = ob.step(a, freeze_done=True, threads=8)
            np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"reward step {t}")
            np.testing.assert_array_equal(term.cpu().numpy().astype(np.uint8), ot, err_msg=f"terminated step {t}")
            np.testing.assert_array_equal(win.cpu().numpy().astype(np.uint8), ow, err_msg=f"win step {t}")
            np.testing.assert_allclose(env.get_obs().cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL)
            np.testing.assert_allclose(env.get_state().cpu().numpy(), ob.state, rtol=0, atol=F32_TOL)
            if t % 25 == 24 or t == T - 1:
                compare_with_oracle(env, ob, B, n, m, f"step {t}")


@pytest.mark.parametrize("kernel", ["group", "group-ondemand", "lane", "lanev"])
def test_auto_reset_and_unfrozen_modes_match_oracle(kernel):
    B, n, m, T = 128, 5, 15, 420   # > 2 episodes per env
    seeds = np.arange(B, dtype=np.uint32) + 5
    args = cs.make_env_args("flight_easy", n_agents=n)
    cfg = orc.make_config(n_agents=n)
    for mode in ("auto_reset", "unfrozen"):
        env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=(mode == "auto_reset"),
                                  kernel=kernel.split("-")[0], step_advance=not kernel.endswith("ondemand"))
        env.seed(seeds)
        env.reset(init=True)
        rng = np.random.RandomState(9)
        with orc.hip_equivalent_arithmetic():
            ob = orc.OracleBatch(cfg, B, seeds)
            ob.reset(init=True, threads=8)
            for t in range(T if mode == "auto_reset" else 230):
                a = rng.randint(0, 3, size=(B, n)).astype(np.int64)   # int64 actions path
                r, term, win = env.step(torch.from_numpy(a))
                orr, ot, ow = ob.step(a, auto_reset=(mode == "auto_reset"), freeze_done=False, threads=8)
                np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"{mode} reward step {t}")
                np.testing.assert_array_equal(term.cpu().numpy().astype(np.uint8), ot)
                np.testing.assert_array_equal(win.cpu().numpy().astype(np.uint8), ow)
            compare_with_oracle(env, ob, B, n, m, mode)
            if mode == "auto_reset":
                assert hdr(env)[:, _lib.H_EPISODES].min() >= 3


@pytest.mark.parametrize("n,agent_mode,B,T", [(3, 0, 48, 90), (5, 2, 16, 60), (3, 3, 16, 40)])
def test_flight_prob_map_matches_oracle(n, agent_mode, B, T):
    m = 15
    seeds = np.arange(B, dtype=np.uint32) + 31
    args = cs.make_env_args("flight", n_agents=n, agent_mode=agent_mode)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=True)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant="flight", n_agents=n, agent_mode=agent_mode)
    rng = np.random.RandomState(3)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        for t in range(T):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            r, term, win = env.step(torch.from_numpy(a))
            orr, ot, ow = ob.step(a, freeze_done=True, threads=8)
            np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"reward step {t}")
            np.testing.assert_array_equal(term.cpu().numpy().astype(np.uint8), ot)
            if t % 10 == 9 or t == T - 1:
                np.testing.assert_allclose(env.get_obs().cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL,
                                           err_msg=f"obs (map + feats) step {t}")
                np.testing.assert_allclose(env.get_state().cpu().numpy(), ob.state, rtol=0, atol=F32_TOL)
        compare_with_oracle(env, ob, B, n, m, "flight final")
        # second episode without init: the map persists (quirk Q9)
        env.reset(init=False)
        ob.reset(init=False, threads=8)
        for t in range(15):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            env.step(torch.from_numpy(a))
            ob.step(a, freeze_done=True, threads=8)
        np.testing.assert_allclose(env.get_obs().cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL)
        pm = env.raw()["prob"].cpu().numpy()
        assert (pm != 0.5).any()


@pytest.mark.parametrize("n,agent_mode", [(3, 0), (3, 3), (5, 1)])
def test_flight_fused_auto_reset_matches_oracle(n, agent_mode):
    """flight + CS_AUTO_RESET: the reset-time map update (start positions) and the step's update are applied in
    one k_map sweep; short episodes (time_limit 25) force several resets per env."""
    B, T, m = 24, 110, 15
    seeds = np.arange(B, dtype=np.uint32) + 77
    args = cs.make_env_args("flight", n_agents=n, agent_mode=agent_mode)
    args.time_limit = 25
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant="flight", n_agents=n, agent_mode=agent_mode, time_limit=25)
    rng = np.random.RandomState(17)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        for t in range(T):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            r, term, win = env.step(torch.from_numpy(a))
            orr, ot, ow = ob.step(a, auto_reset=True, freeze_done=False, threads=8)
            np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"reward step {t}")
            np.testing.assert_array_equal(term.cpu().numpy().astype(np.uint8), ot)
            if t % 7 == 6 or t == T - 1:
                np.testing.assert_allclose(env.get_obs().cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL,
                                           err_msg=f"obs (map + feats) step {t}")
        compare_with_oracle(env, ob, B, n, m, "flight auto-reset")
        assert hdr(env)[:, _lib.H_EPISODES].min() >= 4


@pytest.mark.parametrize("kernel", ["oct", "od", "ode"])
@pytest.mark.parametrize("variant,n,agent_mode,target_mode,B,T,kw", [
    ("flight_easy", 3, 0, 0, 509, 230, {}),                    # 509 = 63 full octet wavefronts' worth + a tail of 5 envs
    ("flight_easy", 5, 0, 0, 256, 230, {}),
    ("flight_easy", 3, 3, 0, 128, 120, {}),                    # AM3: every reset draws (quirk Q3)
    ("flight_easy", 3, 2, 1, 130, 120, {}),                    # AM2, uniform targets
    ("flight_easy", 1, 1, 0, 64, 220, {}),
    ("flight_easy", 8, 0, 0, 64, 100, {}),                     # 8 agents = every lane of the octet owns one
    ("flight_easy", 2, 1, 0, 100, 100, {}),
    ("flight_easy", 8, 0, 1, 72, 90, dict(target_num=16)),     # 8 x 16 pairs: the tape's worst case per step
    ("flight_easy", 7, 0, 1, 72, 90, dict(target_num=16, view_range=30)),   # nearly every pair in range
    ("flight_easy", 2, 0, 1, 40, 90, dict(target_num=1)),      # one target: lanes 1..7 own none
    ("flight_easy", 3, 0, 0, 96, 90, dict(detect_prob=1.0)),
    ("flight_easy", 4, 1, 0, 96, 90, dict(map_size=20, view_range=3)),      # agents crowd: the sequential loop every step
    ("flight_easy", 5, 2, 0, 96, 90, dict(agent_velocity=2, force_dist=6, safe_dist=2)),
    ("flight_easy", 3, 0, 0, 96, 90, dict(time_limit=7)),      # a reset every 7 steps
    ("flight_easy", 6, 3, 0, 48, 120, {}),
])
@pytest.mark.parametrize("mode", ["frozen", "auto_reset", "unfrozen"])
def test_octet_rollout_matches_oracle_bit_exact(variant, n, agent_mode, target_mode, B, T, kw, mode, kernel):
    """The 8-lanes-per-env rollout kernels (k_rollout_oct: lane t owns agent t and targets t, t + 8; k_rollout_od: the same
    layout with a kinematics wavefront running one step ahead of a detection wavefront) against the oracle:
    every reward / terminated / win of every step, observations and get_state rows at three steps, the raw fp64 state and
    the canonical MT19937 rows at the end -- in two rollout calls of uneven length, so the state also survives the
    kernel's epilogue / prologue (tape hand-over included)."""
    args = _custom_args(variant, n_agents=n, agent_mode=agent_mode, target_mode=target_mode, **kw)
    m = args.target_num
    seeds = (4242 + 17 * np.arange(B)).astype(np.uint32)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=(mode == "frozen"), auto_reset=(mode == "auto_reset"),
                              kernel=kernel)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant=variant, n_agents=n, n_targets=m, agent_mode=args.agent_mode, target_mode=args.target_mode,
                          map_size=args.map_size, view_range=args.view_range, time_limit=args.time_limit,
                          velocity=float(args.agent_velocity), safe_dist=float(args.safe_dist),
                          detect_prob=float(args.detect_prob), force_dist=float(args.force_dist))
    a = np.random.RandomState(n * 1000 + B).randint(0, 3, size=(T, B, n)).astype(np.int32)
    cut = 37
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        t0 = 0
        for part in (a[:cut], a[cut:]):
            out = env.rollout(torch.from_numpy(part))
            want = ob.rollout(part, auto_reset=(mode == "auto_reset"), freeze_done=(mode == "frozen"), threads=8)
            np.testing.assert_array_equal(out["reward"].cpu().numpy(), want["reward"], err_msg=f"reward from step {t0}")
            np.testing.assert_array_equal(out["terminated"].cpu().numpy().astype(np.uint8), want["terminated"])
            np.testing.assert_array_equal(out["win"].cpu().numpy().astype(np.uint8), want["win"])
            for t in (0, len(part) // 2, len(part) - 1):
                np.testing.assert_allclose(out["obs"][t].cpu().numpy(), want["obs"][t], rtol=0, atol=F32_TOL)
                np.testing.assert_allclose(out["state"][t].cpu().numpy(), want["state"][t], rtol=0, atol=F32_TOL)
            compare_with_oracle(env, ob, B, n, m, f"{mode} after step {t0 + len(part)}")
            t0 += len(part)
    if mode == "auto_reset" and args.time_limit <= 200 and T > args.time_limit:
        assert hdr(env)[:, _lib.H_EPISODES].min() >= 2


@pytest.mark.parametrize("kernel", ["group", "lane", "lanev", "oct", "od", "ode"])
def test_rollout_kernel_equals_stepwise(kernel):
    B, n, T = 1000, 3, 200   # not a multiple of 64: exercises the partial last wavefront
    args = cs.make_env_args("flight_easy", n_agents=n)
    seeds = np.arange(B, dtype=np.uint32) + 99
    acts = torch.randint(0, 3, (T, B, n), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    for kw in (dict(freeze_done=True), dict(freeze_done=False, auto_reset=True)):
        e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel="group", **kw)   # step-by-step, group kernel
        e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, **kw)    # fused rollout, either kernel
        out = e2.rollout(acts)
        for t in range(T):
            r, term, win = e1.step(acts[t])
            assert torch.equal(r, out["reward"][t]) and torch.equal(term, out["terminated"][t]) and torch.equal(win, out["win"][t])
            if t % 40 == 0 or t == T - 1:
                assert torch.equal(e1.get_obs(), out["obs"][t]) and torch.equal(e1.get_state(), out["state"][t])
        r1, r2 = raw_state(e1), raw_state(e2)
        for k in ("tgt", "agent", "hdr", "mt"):
            assert torch.equal(r1[k], r2[k]), k


@pytest.mark.parametrize("kernel", ["oct", "od", "ode"])
@pytest.mark.parametrize("n,time_limit", [(3, 200), (3, 1), (3, 2), (5, 3), (2, 5)])
def test_octet_kernels_short_launches_and_back_to_back_resets(kernel, n, time_limit):
    """Launch lengths around and below the pair kernels' ring depth (1, 2, 3, 4, 5, 9 steps: pipeline fill and drain with
    nothing in between), chained on one env so that every hand-over between launches is exercised, with episodes as short as
    ONE step (time_limit 1: every env resets at every step -- the emitting wavefront may still be writing a step's rows
    when the detection wavefront resets their targets).  Bit for bit against the 16-lane step kernel, step by step, in
    every output and in the raw state after each launch.  B = 77: nine full octet wavefronts' worth + a tail of 5 envs."""
    B = 77
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = time_limit
    seeds = np.arange(B, dtype=np.uint32) + 31 * n + time_limit
    g = torch.Generator("cuda").manual_seed(5 + n)
    for kw in (dict(freeze_done=False, auto_reset=True), dict(freeze_done=True), dict(freeze_done=False)):
        e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel="group", **kw)
        e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, **kw)
        t = 0
        for T in (1, 2, 3, 4, 5, 9, 1, 4, 2):
            acts = torch.randint(0, 3, (T, B, n), dtype=torch.int32, device="cuda", generator=g)
            out = e2.rollout(acts)
            for k in range(T):
                r, term, win = e1.step(acts[k])
                assert torch.equal(r, out["reward"][k]) and torch.equal(term, out["terminated"][k]) and torch.equal(win, out["win"][k]), (kw, t + k)
                assert torch.equal(e1.get_obs(), out["obs"][k]) and torch.equal(e1.get_state(), out["state"][k]), (kw, t + k)
            r1, r2 = raw_state(e1), raw_state(e2)
            for key in ("tgt", "agent", "hdr", "mt"):
                assert torch.equal(r1[key], r2[key]), (key, kw, t)
            t += T


@pytest.mark.parametrize("kernel", ["od", "ode"])
@pytest.mark.parametrize("kw", [
    dict(n_agents=3, target_num=1, target_mode=1, detect_prob=1.0, view_range=40),   # a win within a step or two of every reset
    dict(n_agents=2, target_num=2, target_mode=1, detect_prob=1.0, view_range=25),
    dict(n_agents=5, target_num=3, target_mode=0, detect_prob=0.9, view_range=30, agent_mode=3),
])
def test_pair_kernels_under_constant_mispredictions(kernel, kw):
    """The kinematics wavefront runs ahead on the assumption that only the step counter ends an episode; here nearly every
    episode ends with a WIN a step or two after its reset, so the detection wavefront's fix requests (restore from the
    ring, redo the speculative steps, acknowledge) and the resets behind them come every other step in every workgroup --
    also while the emitting wavefront is still writing the previous step out.  1000 envs x 300 steps in launches of uneven
    length, bit for bit against the 16-lane step kernel."""
    B, T = 1000, 300
    args = _custom_args("flight_easy", **dict(kw))
    n = args.n_agents
    seeds = np.arange(B, dtype=np.uint32) + 5150
    g = torch.Generator("cuda").manual_seed(17)
    for mode in (dict(freeze_done=False, auto_reset=True), dict(freeze_done=True)):
        e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel="group", **mode)
        e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, **mode)
        t, wins = 0, 0
        for L in (7, 64, 3, 100, 26, 100):
            acts = torch.randint(0, 3, (L, B, n), dtype=torch.int32, device="cuda", generator=g)
            out = e2.rollout(acts)
            for k in range(L):
                r, term, win = e1.step(acts[k])
                assert torch.equal(r, out["reward"][k]) and torch.equal(term, out["terminated"][k]) and torch.equal(win, out["win"][k]), (mode, t + k)
                if k % 9 == 0 or k == L - 1:
                    assert torch.equal(e1.get_obs(), out["obs"][k]) and torch.equal(e1.get_state(), out["state"][k]), (mode, t + k)
            wins += int(out["win"].sum().item())
            r1, r2 = raw_state(e1), raw_state(e2)
            for key in ("tgt", "agent", "hdr", "mt"):
                assert torch.equal(r1[key], r2[key]), (key, mode, t)
            t += L
        assert t == T
        if mode.get("auto_reset"):
            assert wins > B * 10, wins   # the scenario does what it says: tens of wins per env


@pytest.mark.parametrize("kernel", ["oct", "od", "ode"])
def test_octet_kernels_partial_outputs(kernel):
    """rollout(out=...) without obs / state buffers (the pair kernel then runs without its emitting wavefront): rewards,
    flags and the final state equal the full-output run's."""
    B, n, T = 264, 3, 60
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = 25
    seeds = np.arange(B, dtype=np.uint32) + 1234
    acts = torch.randint(0, 3, (T, B, n), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, freeze_done=False, auto_reset=True)
    e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, freeze_done=False, auto_reset=True)
    full = e1.rollout(acts)
    lean = e2.rollout(acts, emit=False)
    assert lean.get("obs") is None and lean.get("state") is None
    for key in ("reward", "terminated", "win"):
        assert torch.equal(full[key], lean[key]), key
    r1, r2 = raw_state(e1), raw_state(e2)
    for key in ("tgt", "agent", "hdr", "mt"):
        assert torch.equal(r1[key], r2[key]), key
    assert torch.equal(e1.get_obs(), e2.get_obs()) and torch.equal(e1.get_state(), e2.get_state())


@pytest.mark.parametrize("kernel", ["oct", "od", "lanev"])
def test_rollout_output_alignment_rules(kernel):
    """an (env, agent) observation is ONE 16-byte store in the octet and lane kernels, so cs_rollout refuses an obs table
    that is not 16-byte aligned (include/coopsearch.h) instead of issuing misaligned dwordx4 stores; the state table may sit anywhere
    -- off a 16-byte boundary it takes the scalar-store launch -- and must then hold exactly what the aligned run writes."""
    B, n, T = 264, 3, 30
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = 25
    seeds = np.arange(B, dtype=np.uint32) + 77
    acts = torch.randint(0, 3, (T, B, n), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, freeze_done=False, auto_reset=True)
    e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, freeze_done=False, auto_reset=True)
    e3 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, freeze_done=False, auto_reset=True)
    full = e1.rollout(acts)
    W = e1.state_shape

    def off_by_one_float(shape):
        flat = torch.zeros(int(np.prod(shape)) + 1, dtype=torch.float32, device="cuda")
        view = flat[1:].view(*shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    out = dict(reward=torch.empty_like(full["reward"]), terminated=torch.empty_like(full["terminated"]),
               win=torch.empty_like(full["win"]), obs=torch.empty_like(full["obs"]), state=off_by_one_float((T, B, W)))
    got = e2.rollout(acts, out=out)
    for key in ("reward", "terminated", "win", "obs", "state"):
        assert torch.equal(full[key], got[key]), key
    bad = dict(out, obs=off_by_one_float((T, B, n, 4)), state=torch.empty_like(full["state"]))
    with pytest.raises(Exception, match="obs_dev must be 16-byte aligned"):
        e3.rollout(acts, out=bad)


@pytest.mark.parametrize("n", [3, 5])
def test_group_and_lane_kernels_can_be_interleaved(n):
    """Both kernels share one state layout (incl. the mirrored head of the MT rows that only the lane kernel reads
    and every writer must maintain): alternating them step by step -- single steps and short rollouts, with
    auto-resets -- must reproduce a pure group-kernel run bit for bit."""
    B, T = 1000, 330
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.time_limit = 60   # frequent resets: the reset path writes MT words too
    seeds = np.arange(B, dtype=np.uint32) + 9000
    ref = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True, kernel="group")
    mix = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True, kernel="group")
    g = torch.Generator("cuda").manual_seed(77)
    t = 0
    k = 0
    while t < T:
        chunk = (1, 3, 1, 7)[k % 4]
        mix.kernel = ("lane", "group")[k % 2]
        a = torch.randint(0, 3, (chunk, B, n), dtype=torch.int32, device="cuda", generator=g)
        if chunk == 1:
            r1, t1, w1 = ref.step(a[0])
            r2, t2, w2 = mix.step(a[0])
            assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(w1, w2), f"step {t}"
        else:
            o1, o2 = ref.rollout(a), mix.rollout(a)
            for key in ("reward", "terminated", "win", "obs", "state"):
                assert torch.equal(o1[key], o2[key]), f"{key} at step {t}"
        t += chunk
        k += 1
    r1, r2 = raw_state(ref), raw_state(mix)
    for key in ("tgt", "agent", "hdr", "mt"):
        assert torch.equal(r1[key], r2[key]), key
    assert hdr(ref)[:, _lib.H_EPISODES].min() >= 5


@pytest.mark.parametrize("n,B,T", [(3, 4096, 260), (5, 16384, 230)])
def test_full_size_rollout_matches_oracle(n, B, T):
    """BASELINE configs 2 / 3 at full size through the kernels the bench runs (c2: the wavefront-pair kernel, c3: the
    octet kernel), auto-reset through at least one episode boundary per env: every reward, terminated and win
    flag of every step, the emitted observation / state of the last step, and the full raw state against the oracle."""
    m = 15
    seeds = np.arange(B, dtype=np.uint32) + 20240000          # env seeds base 20240000
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=seeds, freeze_done=False,
                              auto_reset=True)
    env.seed(seeds)
    env.reset(init=True)
    a = np.random.RandomState(1).randint(0, 3, size=(T, B, n)).astype(np.int32)
    out = env.rollout(torch.from_numpy(a))
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(orc.make_config(n_agents=n), B, seeds)
        ob.reset(init=True, threads=8)
        want = ob.rollout(a, auto_reset=True, freeze_done=False, threads=8)
        np.testing.assert_array_equal(out["reward"].cpu().numpy(), want["reward"])
        np.testing.assert_array_equal(out["terminated"].cpu().numpy().astype(np.uint8), want["terminated"])
        np.testing.assert_array_equal(out["win"].cpu().numpy().astype(np.uint8), want["win"])
        for t in (0, T // 2, T - 1):
            np.testing.assert_allclose(out["obs"][t].cpu().numpy(), want["obs"][t], rtol=0, atol=F32_TOL)
            np.testing.assert_allclose(out["state"][t].cpu().numpy(), want["state"][t], rtol=0, atol=F32_TOL)
        compare_with_oracle(env, ob, B, n, m, f"c{2 if n == 3 else 3} full size")
    assert hdr(env)[:, _lib.H_EPISODES].min() >= 2     # the constructor's reset + at least one auto-reset


@pytest.mark.parametrize("n,B", [(3, 4096), (5, 16384)])
def test_full_size_properties_and_shard_invariance(n, B):
    """BASELINE configs 2/3 at full size: domain invariants + bit-exact shard invariance (rank-local halves with
    env_offset reproduce the single-device batch)."""
    T = 200
    args = cs.make_env_args("flight_easy", n_agents=n)
    whole = cs.BatchedFlightEnv(args, batch=B)
    half = B // 2
    parts = [cs.BatchedFlightEnv(args, batch=half, env_offset=0), cs.BatchedFlightEnv(args, batch=half, env_offset=half)]
    g = torch.Generator("cuda").manual_seed(7)
    last_find = torch.zeros(B, dtype=torch.int32, device="cuda")
    tot = torch.zeros(B, dtype=torch.float64, device="cuda")
    for t in range(T):
        a = torch.randint(0, 3, (B, n), dtype=torch.int32, device="cuda", generator=g)
        r, term, win = whole.step(a)
        assert torch.equal(r, r.round()) and (r >= -1 - n).all() and (r <= -1 + 10 * 15 + 100).all()
        tf = whole.target_find
        assert (tf >= last_find).all() and (tf <= 15).all()
        last_find = tf.clone()
        tot += r.double()
        ag = whole.raw()["agent"][:, :n]
        assert (ag[:, :, :2] >= 0).all() and (ag[:, :, :2] <= 50).all()
        assert (ag[:, :, 2] >= 0).all() and (ag[:, :, 2] <= 2 * np.pi).all()
        assert torch.equal(term, (tf >= 15) | (whole.time_step >= 200))
        assert torch.equal(win, whole.win_flag) and (~win | (tf == 15)).all()
        for k, pe in enumerate(parts):
            rr, tt, ww = pe.step(a[k * half:(k + 1) * half])
            assert torch.equal(rr, r[k * half:(k + 1) * half]) and torch.equal(tt, term[k * half:(k + 1) * half])
    assert torch.equal(tot, whole.total_reward.double())
    rw = raw_state(whole)
    for k, pe in enumerate(parts):
        rp = raw_state(pe)
        for key in ("tgt", "agent", "hdr", "mt"):
            assert torch.equal(rp[key], rw[key][k * half:(k + 1) * half]), key
    assert whole.get_state().abs().max() <= 1.5
    mp = whole.metric_partials().cpu().numpy()
    h = hdr(whole)
    assert mp[3] == B and mp[0] == h[:, _lib.H_TOTAL_REWARD].sum() and mp[2] == h[:, _lib.H_TARGET_FIND].sum()
    assert mp[1] == (h[:, _lib.H_FLAGS] & 1).sum()
    # statistical pin shipped by the reference (result/flight_easy_Seed0_random_{3,5}a15t(AM0TM0)/average_res_529.npy,
    # BASELINE.md section 1): % of targets found after 200 random steps, 84.87 (3 agents) / 95.80 (5 agents)
    found_pct = 100.0 * whole.target_find.double().mean().item() / 15.0
    assert abs(found_pct - {3: 84.87, 5: 95.80}[n]) < 3.0, found_pct


def test_flight_full_size_smoke_properties():
    """BASELINE config 4 (flight, 3 agents, B = 8192): map values stay in [0, 1], untouched cells stay 0.5,
    the obs rows replicate the map, reward bounds hold."""
    B, n = 8192, 3
    env = cs.BatchedFlightEnv(cs.make_env_args("flight", n_agents=n), batch=B)
    g = torch.Generator("cuda").manual_seed(11)
    for t in range(30):
        a = torch.randint(0, 3, (B, n), dtype=torch.int32, device="cuda", generator=g)
        r, term, win = env.step(a)
    pm = env.raw()["prob"]
    assert (pm >= 0).all() and (pm <= 1).all()
    assert (pm[:, :, 45:] == 0.5).float().mean() > 0.5   # far corner strip is rarely visited in 30 steps from y = 0
    obs = env.get_obs()
    for i in range(n):
        assert torch.equal(obs[:, i, :2500], pm.reshape(B, 2500))
    assert torch.equal(obs[:, :, 2500:], env.get_state()[:, :4 * n].reshape(B, n, 4))


def _custom_args(variant, **kw):
    args = cs.make_env_args(variant, n_agents=kw.pop("n_agents", 3), agent_mode=kw.pop("agent_mode", 0),
                            target_mode=kw.pop("target_mode", 0))
    for k, v in kw.items():
        setattr(args, k, v)
    return args


@pytest.mark.parametrize("kernel", ["group", "lane", "lanev"])
@pytest.mark.parametrize("variant,kw", [
    ("flight_easy", dict(n_agents=8, target_num=16, target_mode=1)),             # maximum sizes: 8 x 16 pairs, 2-phase draws
    ("flight_easy", dict(n_agents=7, target_num=16, target_mode=1, view_range=30)),  # nearly every pair in range: > 7 draws/step
    ("flight_easy", dict(n_agents=2, target_num=1, target_mode=1)),              # a single target
    ("flight_easy", dict(n_agents=3, detect_prob=1.0)),                          # every in-range pair detects
    ("flight_easy", dict(n_agents=3, detect_prob=0.0)),                          # draws consumed, nothing found (U <= 0 never... only U == 0)
    ("flight_easy", dict(n_agents=4, map_size=20, view_range=3, agent_mode=1)),  # small map: agents crowd, force + walls every step
    ("flight_easy", dict(n_agents=5, agent_velocity=2, force_dist=6, safe_dist=2, agent_mode=2)),
    ("flight_easy", dict(n_agents=3, time_limit=7)),                             # many episode boundaries
])
def test_unusual_configurations_match_oracle(variant, kw, kernel):
    B, T, kw = 96, 90, dict(kw)
    args = _custom_args(variant, **kw)
    n, m = args.n_agents, args.target_num
    seeds = np.arange(B, dtype=np.uint32) * 3 + 11
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True, kernel=kernel)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant=variant, n_agents=n, n_targets=m, agent_mode=args.agent_mode, target_mode=args.target_mode,
                          map_size=args.map_size, view_range=args.view_range, time_limit=args.time_limit,
                          velocity=float(args.agent_velocity), safe_dist=float(args.safe_dist),
                          detect_prob=float(args.detect_prob), force_dist=float(args.force_dist))
    rng = np.random.RandomState(2)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        compare_with_oracle(env, ob, B, n, m, "reset")
        for t in range(T):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            r, term, win = env.step(torch.from_numpy(a))
            orr, ot, ow = ob.step(a, auto_reset=True, freeze_done=False, threads=8)
            np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"reward step {t}")
            np.testing.assert_array_equal(term.cpu().numpy().astype(np.uint8), ot, err_msg=f"terminated step {t}")
            np.testing.assert_array_equal(win.cpu().numpy().astype(np.uint8), ow, err_msg=f"win step {t}")
            np.testing.assert_allclose(env.get_state().cpu().numpy(), ob.state, rtol=0, atol=F32_TOL)
        compare_with_oracle(env, ob, B, n, m, "final")


@pytest.mark.parametrize("kw", [
    dict(n_agents=3, map_size=20, view_range=4, agent_mode=1),
    dict(n_agents=4, map_size=62, view_range=9, agent_mode=3),      # largest map the u64 lattice rows allow
    dict(n_agents=2, map_size=50, view_range=7, detect_prob=1.0, agent_mode=2),
    dict(n_agents=8, map_size=30, view_range=5, target_num=16, target_mode=1),
])
def test_flight_unusual_configurations_match_oracle(kw):
    B, T, kw = 12, 45, dict(kw)
    args = _custom_args("flight", **kw)
    n, m, L = args.n_agents, args.target_num, args.map_size
    seeds = np.arange(B, dtype=np.uint32) + 400
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant="flight", n_agents=n, n_targets=m, agent_mode=args.agent_mode, target_mode=args.target_mode,
                          map_size=L, view_range=args.view_range, detect_prob=float(args.detect_prob))
    rng = np.random.RandomState(4)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        for t in range(T):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            r, term, win = env.step(torch.from_numpy(a))
            orr, ot, ow = ob.step(a, auto_reset=True, freeze_done=False, threads=8)
            np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"reward step {t}")
            if t % 5 == 4 or t == T - 1:
                np.testing.assert_allclose(env.get_obs().cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL,
                                           err_msg=f"obs (map + feats) step {t}")
        compare_with_oracle(env, ob, B, n, m, "flight final")


@pytest.mark.parametrize("kw", [
    dict(n_agents=3, map_size=20, view_range=4, agent_mode=1),
    dict(n_agents=4, map_size=62, view_range=9, agent_mode=3),      # 961 chunks: two sweep workgroups per env in k_flight_pipe
    dict(n_agents=8, map_size=30, view_range=5, target_num=16, target_mode=1),
])
def test_flight_unusual_configurations_pipelined_rollout_equals_stepwise(kw):
    """The pipelined cs_rollout (k_flight_pipe) on map sizes / team sizes other than the shipped one, against cs_step."""
    B, T, kw = 21, 13, dict(kw)
    args = _custom_args("flight", **kw)
    args.time_limit = 6
    n = args.n_agents
    seeds = np.arange(B, dtype=np.uint32) + 77
    acts = torch.randint(0, 3, (T, B, n), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    out = e2.rollout(acts)
    for t in range(T):
        r, term, win = e1.step(acts[t])
        assert torch.equal(r, out["reward"][t]) and torch.equal(term, out["terminated"][t]) and torch.equal(win, out["win"][t])
        assert torch.equal(e1.get_obs(), out["obs"][t]) and torch.equal(e1.get_state(), out["state"][t])
    r1, r2 = raw_state(e1), raw_state(e2)
    for k in ("tgt", "agent", "hdr", "mt", "prob"):
        assert torch.equal(r1[k], r2[k]), k


def test_b1_adapter_runs_a_rollout_shaped_loop():
    """BASELINE config 1: the reference-typed B = 1 adapter driven like common/rollout.py:43-76."""
    meta, z = load_trace("easy_n3_am0_s0_a1")
    args = cs.make_env_args("flight_easy", n_agents=3)
    env = cs.FlightSearchEnvEasy(args, cs.load_targets(), seed=meta["seed"])
    info = env.get_env_info()
    assert info == {"n_actions": 3, "state_shape": 57, "obs_shape": 4, "episode_limit": 200}
    env.seed(meta["seed"])
    env.reset()
    terminated, step, episode_reward = False, 0, 0
    while not terminated and step < info["episode_limit"]:
        obs, state = env.get_obs(), env.get_state()
        assert obs.dtype == np.float64 and obs.shape == (3, 4) and state.shape == (57,)
        acts = []
        for agent_id in range(3):
            avail = env.get_avail_agent_actions(agent_id)
            assert avail.tolist() == [1.0, 1.0, 1.0]
            acts.append(torch.tensor(int(z["e0_actions"][step][agent_id])))   # 0-dim LongTensor like torch.argmax
        reward, terminated, info_win = env.step(acts)
        assert isinstance(reward, int) and isinstance(terminated, bool) and isinstance(info_win, bool)
        assert reward == int(z["e0_reward"][step])
        episode_reward += reward
        step += 1
    assert (step, episode_reward, env.target_find) == (200, -470, 8)
    with pytest.raises(Exception, match="Act num mismatch agent"):
        env.step([0, 1])
    with pytest.raises(Exception, match="Agent id out of range"):
        env.get_avail_agent_actions(3)


def test_b1_flight_adapter_matches_golden_trace():
    """FlightSearchEnv (probability-map variant) through the reference-typed B = 1 adapter."""
    meta, z = load_trace("flight_n3_am3_s3_a2")
    args = cs.make_env_args("flight", n_agents=3, agent_mode=3)
    env = cs.FlightSearchEnv(args, cs.load_targets(), seed=meta["seed"])
    assert env.get_env_info()["obs_shape"] == 4      # quirk Q8: reported as 4 although get_obs is 2504 wide
    env.seed(meta["seed"])
    env.reset(init=True)
    np.testing.assert_allclose(env.prob_map, z["e0_reset_prob_map"], atol=F32_TOL)
    for t in range(30):
        obs = env.get_obs()
        assert obs.shape == (3, 2504) and obs.dtype == np.float64
        r, term, win = env.step([int(a) for a in z["e0_actions"][t]])
        assert (r, int(term), int(win)) == (int(z["e0_reward"][t]), int(z["e0_terminated"][t]), int(z["e0_win"][t]))
        assert env.target_find == int(z["e0_target_find"][t]) and env.out_flag == list(z["e0_out_flag"][t])
        np.testing.assert_allclose(np.array(env.agent_pos), z["e0_agent_pos"][t], atol=1e-9)
    m15 = z["e0_prob_maps"][list(z["e0_prob_map_steps"]).index(30)]
    np.testing.assert_allclose(env.prob_map, m15, atol=F32_TOL)
    np.testing.assert_allclose(env.get_obs()[0, :2500], m15.reshape(-1), atol=F32_TOL)


def test_c_example_runs_and_reproduces_the_random_policy_statistics(tmp_path):
    """The plain C++/HIP consumer of the C ABI (no Python, no torch in that process)."""
    import os, re, subprocess
    from cooperative_search_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.dirname(_lib.library_path())
    exe = tmp_path / "c_api_demo"
    subprocess.check_call([build.hipcc_path(), "--offload-arch=gfx950", "-I", os.path.join(root, "include"),
                           os.path.join(root, "examples", "c_api_demo.cpp"), "-L", csrc, "-lcoopsearch_hip",
                           f"-Wl,-rpath,{csrc}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    m = re.search(r"episodes (\d+)\s+mean episode_reward (-?[\d.]+)\s+win rate ([\d.]+)\s+mean targets_find ([\d.]+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) == 4096
    assert abs(float(m.group(4)) / 15 * 100 - 84.87) < 3.0     # shipped random-policy figure for 3a15t AM0


@pytest.mark.parametrize("B,n,T", [(96, 3, 40), (37, 3, 1), (37, 5, 7), (300, 3, 2), (1, 3, 5), (530, 4, 33), (8192, 3, 6)])
def test_flight_rollout_call_equals_stepwise(B, n, T):
    """cs_rollout(flight) sweeps step t's map in the same launch that runs step t + 1 (k_flight_pipe, double-buffered
    map-update records): it must leave exactly what T cs_step calls leave, for odd and even T, ragged batches, resets
    inside the horizon, and whatever call (step / rollout / reset) comes next."""
    args = cs.make_env_args("flight", n_agents=n)
    args.time_limit = 17
    seeds = np.arange(B, dtype=np.uint32) + 321
    acts = torch.randint(0, 3, (2 * T + 1, B, n), dtype=torch.int64, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    out = e2.rollout(acts[:T])
    assert out["obs"].shape == (T, B, n, 2504)
    for t in range(T):
        r, term, win = e1.step(acts[t])
        assert torch.equal(r, out["reward"][t]) and torch.equal(term, out["terminated"][t]) and torch.equal(win, out["win"][t])
        assert torch.equal(e1.get_obs(), out["obs"][t]) and torch.equal(e1.get_state(), out["state"][t])
    r1, r2 = raw_state(e1), raw_state(e2)
    for k in ("tgt", "agent", "hdr", "mt", "prob"):
        assert torch.equal(r1[k], r2[k]), k
    # a single step after the rollout (the step's record parity differs from the rollout's last one when T is even) ...
    ra, rb = e1.step(acts[T]), e2.step(acts[T])
    assert all(torch.equal(x, y) for x, y in zip(ra, rb)) and torch.equal(e1.get_obs(), e2.get_obs())
    # ... then a rollout without observation buffers (the sweeps still have to update the map), then a masked reset
    e2.rollout(acts[T + 1:], emit=False)
    for t in range(T + 1, 2 * T + 1):
        e1.step(acts[t])
    mask = torch.arange(B, device="cuda") % 3 == 0
    e1.reset(mask=mask)
    e2.reset(mask=mask)
    assert torch.equal(e1.get_obs(), e2.get_obs()) and torch.equal(e1.get_state(), e2.get_state())
    r1, r2 = raw_state(e1), raw_state(e2)
    for k in ("tgt", "agent", "hdr", "mt", "prob"):
        assert torch.equal(r1[k], r2[k]), k


@pytest.mark.parametrize("kernel", ["group", "lane", "lanev", "oct", "od", "ode"])
def test_long_horizon_matches_oracle(kernel):
    """20 000 steps per env with auto-reset: ~100+ episodes, the circular MT19937 state wraps ~70 times (cursor,
    mirrored head, reset-time batches landing anywhere in the ring).  Rewards are compared every step (in rollout
    chunks), the full raw state at the end."""
    B, n, m, chunk, chunks = 64, 3, 15, 250, 80
    seeds = np.arange(B, dtype=np.uint32) * 7 + 5
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=n), batch=B, seeds=seeds, freeze_done=False,
                              auto_reset=True, kernel=kernel)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(n_agents=n)
    rng = np.random.RandomState(99)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        for c in range(chunks):
            a = rng.randint(0, 3, size=(chunk, B, n)).astype(np.int32)
            out = env.rollout(torch.from_numpy(a), emit=False, update_views=False)
            want = np.empty((chunk, B), dtype=np.float32)
            for t in range(chunk):
                r, _, _ = ob.step(a[t], auto_reset=True, freeze_done=False, threads=8, emit=False)
                want[t] = r
            np.testing.assert_array_equal(out["reward"].cpu().numpy(), want, err_msg=f"chunk {c}")
        compare_with_oracle(env, ob, B, n, m, "after 20000 steps")
    h = hdr(env)
    assert h[:, _lib.H_EPISODES].min() >= 100 and int(words(h).min()) > 40 * 624


def test_flight_long_horizon_matches_oracle():
    """flight, default time limit, 1000 steps with auto-reset (5 episodes per env): the probability map persists
    across episodes and decays towards 0 where the agents keep looking; rewards / flags exact throughout."""
    B, T, n, m = 8, 1000, 3, 15
    seeds = np.arange(B, dtype=np.uint32) + 901
    args = cs.make_env_args("flight", n_agents=n, agent_mode=0)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant="flight", n_agents=n, agent_mode=0)
    rng = np.random.RandomState(23)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        for t in range(T):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            r, term, win = env.step(torch.from_numpy(a))
            orr, ot, ow = ob.step(a, auto_reset=True, freeze_done=False, threads=8)
            np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"reward step {t}")
            np.testing.assert_array_equal(term.cpu().numpy().astype(np.uint8), ot)
            if t % 100 == 99:
                np.testing.assert_allclose(env.get_obs().cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL,
                                           err_msg=f"obs (map + feats) step {t}")
        compare_with_oracle(env, ob, B, n, m, "flight long horizon")
        assert hdr(env)[:, _lib.H_EPISODES].min() >= 5


def test_flight_full_size_pipelined_rollout_matches_oracle():
    """BASELINE config 4 at full size (8192 envs) through cs_rollout's pipelined launches (k_flight_pipe: the map sweep
    of step t beside step t + 1), 48 steps with a time limit of 20 so that every env resets twice inside the call:
    rewards and flags of every step, the 2504-wide observation (map first) at three steps, the raw state at the end."""
    B, n, m, T = 8192, 3, 15, 48
    seeds = np.arange(B, dtype=np.uint32) + 20240000
    args = cs.make_env_args("flight", n_agents=n)
    args.time_limit = 20
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    env.seed(seeds)
    env.reset(init=True)
    a = np.random.RandomState(5).randint(0, 3, size=(T, B, n)).astype(np.int32)
    out = env.rollout(torch.from_numpy(a))
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(orc.make_config(variant="flight", n_agents=n, time_limit=20), B, seeds)
        ob.reset(init=True, threads=8)
        for t in range(T):
            emit = t in (0, 21, T - 1)
            orr, ot, ow = ob.step(a[t], auto_reset=True, freeze_done=False, threads=8, emit=emit)
            np.testing.assert_array_equal(out["reward"][t].cpu().numpy(), orr, err_msg=f"reward step {t}")
            np.testing.assert_array_equal(out["terminated"][t].cpu().numpy().astype(np.uint8), ot)
            np.testing.assert_array_equal(out["win"][t].cpu().numpy().astype(np.uint8), ow)
            if emit:
                np.testing.assert_allclose(out["obs"][t].cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL,
                                           err_msg=f"obs (map + feats) step {t}")
                np.testing.assert_allclose(out["state"][t].cpu().numpy(), ob.state, rtol=0, atol=F32_TOL)
        compare_with_oracle(env, ob, B, n, m, "c4 full size, pipelined")
    assert hdr(env)[:, _lib.H_EPISODES].min() >= 3


def test_mt_advance_changes_when_not_what():
    """cs_mt_advance (the lane kernel's pre-pass) twists rows ahead of their cursors: canonical rows, cursors and every
    later draw are unchanged; only `ahead` moves."""
    B, n = 300, 3
    args = cs.make_env_args("flight_easy", n_agents=n)
    seeds = np.arange(B, dtype=np.uint32) + 4242
    e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True, kernel="group", step_advance=False)
    e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True, kernel="group", step_advance=False)
    g = torch.Generator("cuda").manual_seed(3)
    for t in range(260):
        a = torch.randint(0, 3, (B, n), dtype=torch.int32, device="cuda", generator=g)
        if t % 37 == 5:
            before = e2.mt_canonical()
            e2.mt_advance(10 ** 6 if t % 2 else 300)
            assert torch.equal(before, e2.mt_canonical())
            assert int(e2.raw()["ahead"].max().item()) == 624
        r1, t1, w1 = e1.step(a)
        r2, t2, w2 = e2.step(a)
        assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(w1, w2), f"step {t}"
    assert int(e1.raw()["ahead"].max().item()) == 0     # without the periodic refresh the step kernel never twists ahead
    r1, r2 = raw_state(e1), raw_state(e2)
    for k in ("tgt", "agent", "hdr", "mt"):
        assert torch.equal(r1[k], r2[k]), k


def test_flight_c4_scale_auto_reset_matches_oracle():
    """BASELINE config 4's variant at B = 1024 (the oracle's flight step costs ~20 us per env and thread): 200 steps with
    auto-reset through the default episode length, every integer compared every step, the 2504-wide observation
    (map first) every 25 steps, the full raw state at the end."""
    B, n, T, m = 1024, 3, 200, 15
    seeds = np.arange(B, dtype=np.uint32) + 4040
    args = cs.make_env_args("flight", n_agents=n)
    args.time_limit = 60   # three full episodes per env: resets (map kept, quirk Q9) inside the horizon
    env = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, freeze_done=False, auto_reset=True)
    env.seed(seeds)
    env.reset(init=True)
    cfg = orc.make_config(variant="flight", n_agents=n, time_limit=60)
    rng = np.random.RandomState(44)
    with orc.hip_equivalent_arithmetic():
        ob = orc.OracleBatch(cfg, B, seeds)
        ob.reset(init=True, threads=8)
        for t in range(T):
            a = rng.randint(0, 3, size=(B, n)).astype(np.int32)
            r, term, win = env.step(torch.from_numpy(a))
            emit = t % 25 == 24 or t == T - 1
            orr, ot, ow = ob.step(a, auto_reset=True, freeze_done=False, threads=8, emit=emit)
            np.testing.assert_array_equal(r.cpu().numpy(), orr, err_msg=f"reward step {t}")
            np.testing.assert_array_equal(term.cpu().numpy().astype(np.uint8), ot)
            np.testing.assert_array_equal(win.cpu().numpy().astype(np.uint8), ow)
            if emit:
                np.testing.assert_allclose(env.get_obs().cpu().numpy(), ob.obs, rtol=0, atol=F32_TOL,
                                           err_msg=f"obs (map + feats) step {t}")
                np.testing.assert_allclose(env.get_state().cpu().numpy(), ob.state, rtol=0, atol=F32_TOL)
        compare_with_oracle(env, ob, B, n, m, "flight B=1024 auto-reset")
        assert hdr(env)[:, _lib.H_EPISODES].min() >= 3


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("call", ["step", "rollout"])
@pytest.mark.parametrize("variant", ["flight_easy", "flight"])
def test_check_actions_refuses_out_of_range_values_like_the_reference(binding, call, variant):
    """CS_CHECK_ACTIONS (include/coopsearch.h): the reference raises IndexError at dyaw[act] for an action >= 3
    (flight_env_easy.py:259-262); the batched kernels have no bounds check in their loops (any value other than 1 / 2 acts
    as 0), so the check runs on the device before the call steps anything: IndexError with the reference's wording, the
    env state untouched.  On by default for batches of up to 64 envs; a 3 and a -1 (Python's negative index is the B = 1
    adapter's business, not the batched path's) are both refused."""
    B, n, T = 8, 3, 5
    env = cs.BatchedFlightEnv(cs.make_env_args(variant, n_agents=n), batch=B, binding=binding)
    assert env.check_actions          # B <= 64
    before = {k: v.clone() for k, v in raw_state(env).items()}
    good = torch.randint(0, 3, (T, B, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    for bad_value, where in ((3, (2, 5, 1)), (-1, (0, 0, 0)), (7, (4, 7, 2))):
        acts = good.clone()
        acts[where] = bad_value
        with pytest.raises(IndexError, match="list index out of range") as ei:
            if call == "rollout":
                env.rollout(acts)
            else:
                env.step(acts[where[0]])
        msg = str(ei.value)
        assert f"action {bad_value} " in msg and f"env {where[1]}, agent {where[2]}" in msg
        if call == "rollout":
            assert f"step {where[0]}," in msg
        after = raw_state(env)
        for k in before:
            assert torch.equal(before[k], after[k]), (k, "a refused call must not step anything")
    # int32 tables too; and the call goes through once the table is clean
    with pytest.raises(IndexError):
        bad32 = good.to(torch.int32)
        bad32[1, 1, 1] = 3
        env.rollout(bad32) if call == "rollout" else env.step(bad32[1])
    if call == "rollout":
        env.rollout(good)
    else:
        env.step(good[0])
    assert not torch.equal(before["agent"], raw_state(env)["agent"])
    # large batches: unchecked by default (no synchronisation in the production loop), checked on request
    big = cs.BatchedFlightEnv(cs.make_env_args(variant, n_agents=n), batch=256, binding=binding)
    assert not big.check_actions
    a = torch.full((256, n), 3, dtype=torch.int64, device="cuda")
    big.step(a)                                           # acts as action 0, like every value other than 1 / 2
    chk = cs.BatchedFlightEnv(cs.make_env_args(variant, n_agents=n), batch=256, binding=binding, check_actions=True)
    with pytest.raises(IndexError, match="list index out of range"):
        chk.step(a)
    #  several offenders: the one with the LOWEST flat index (step, env, agent) is reported -- the one the reference's
    # sequential loops would raise on -- whatever order the device's threads found them in; 40 000 offenders, 20 repetitions
    many = torch.randint(0, 3, (40, 256, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    many[3:] = torch.where(torch.rand(37, 256, n, device="cuda") < 0.5, torch.full_like(many[3:], 5), many[3:])
    many[2, 200, 1] = 4
    for _ in range(20):
        with pytest.raises(IndexError, match=r"action 4 of step 2, env 200, agent 1 ") as ei:
            chk.rollout(many)
    #  check_actions=False is honoured for a small batch too, on both bindings (the op layer applies its default only
    # when the caller has not decided)
    off = cs.BatchedFlightEnv(cs.make_env_args(variant, n_agents=n), batch=8, binding=binding, check_actions=False)
    off.step(torch.full((8, n), 3, dtype=torch.int64, device="cuda"))   # no IndexError: acts as action 0


@pytest.mark.parametrize("flag", ["KERNEL_SOLO", "KERNEL_DUO"])
def test_removed_rollout_kernels_are_refused_not_rerouted(flag):
    """CS_KERNEL_SOLO / CS_KERNEL_DUO named the 16-lane rollout kernels of rounds 1-2, removed in round 6: cs_rollout answers them
    with CS_E_CONFIG at every batch size (a forced kernel must never silently become another one -- at 65536 envs the
    request used to fall into the lane kernel's branch), the env untouched; cs_has_legacy_kernels() says 0."""
    assert not _lib.has_legacy_kernels()
    for B in (64, 65536):
        env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=3), batch=B, binding="ctypes", kernel="group")
        plain = env._flags
        env._flags = lambda a: plain(a) | getattr(_lib, flag)
        before = env.raw()["agent"].clone()
        acts = torch.zeros(4, B, 3, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.CoopSearchError, match="removed in round 6"):
            env.rollout(acts)
        assert torch.equal(env.raw()["agent"], before)
        env._flags = plain
        env.rollout(acts)   # "group" itself: T launches of the step kernel
        assert not torch.equal(env.raw()["agent"], before)


def test_render_of_one_env_of_the_batch(tmp_path):
    """Row a13: BatchedFlightEnv.render(env, path) draws that env's targets (found ones orange), agents and found count from the
    device state -- the picture of flight_env_easy.py:324-343 -- and leaves the state untouched."""
    pytest.importorskip("matplotlib")
    env = cs.BatchedFlightEnv(cs.make_env_args("flight_easy", n_agents=3), batch=64, seeds=np.arange(64, dtype=np.uint32) + 3)
    acts = torch.randint(0, 3, (120, 64, 3), dtype=torch.int32, device="cuda")
    env.rollout(acts)
    before = {k: v.clone() for k, v in env.raw().items()}
    b = int(env.target_find.argmax().item())
    ax = env.render(b, path=str(tmp_path / "e.png"))
    assert ax is not None and (tmp_path / "e.png").exists()
    k = int(env.target_find[b].item())
    assert ax.get_title() == f"target_find:{k}/15" and len(ax.collections) == 15 + 3
    import matplotlib.colors as mc
    orange = sum(tuple(np.round(c.get_facecolor()[0][:3], 3)) == tuple(np.round(mc.to_rgb("orange"), 3)) for c in ax.collections[:15])
    assert orange == k and k > 0
    pos = env.raw()["agent"][b, :3, :2].cpu().numpy()
    assert np.allclose([c.get_offsets()[0] for c in ax.collections[15:]], pos)
    for key, v in env.raw().items():
        assert torch.equal(v, before[key]), key
    with pytest.raises(IndexError):
        env.render(64, path=str(tmp_path / "x.png"))


def test_b1_adapter_action_indices_follow_python_list_indexing():
    """dyaw[act] (flight_env_easy.py:259-262): 3 raises IndexError, -1 is dyaw[-1] = -pi/18 (action 2)."""
    args = cs.make_env_args("flight_easy", n_agents=3)
    a, b = cs.FlightSearchEnvEasy(args, cs.load_targets(), seed=3), cs.FlightSearchEnvEasy(args, cs.load_targets(), seed=3)
    for e in (a, b):
        e.seed(3)
        e.reset()
    with pytest.raises(IndexError, match="list index out of range"):
        a.step([0, 3, 1])
    ra, rb = a.step([-1, -2, -3]), b.step([2, 1, 0])
    assert ra == rb and np.array_equal(a.get_state(), b.get_state())


@pytest.mark.parametrize("n,B", [(3, 524288 + 37), (2, 524288), (1, 524288 + 64)])
def test_three_wavefront_lane_kernel_at_its_batch_equals_the_octet_kernel(n, B):
    """From CS_LV_W_FROM = 524288 envs teams of up to 3 run k_rollout_lanev compiled for three wavefronts per SIMD (168 VGPRs, a few
    spilled registers: another binary of the same source).  No small-batch test reaches it, so: the default dispatch at that batch
    (the full wavefronts through the three-wavefront build, a ragged tail through the plain one) against the one-wavefront octet
    kernel on the same seeds and actions -- every reward / flag / observation / state row of every step, the raw state and the
    canonical MT rows, bit for bit; two launches back to back, auto-reset."""
    T = 24
    args = cs.make_env_args("flight_easy", n_agents=n)
    seeds = (np.arange(B, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    g = torch.Generator("cuda").manual_seed(n)
    e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel="oct", freeze_done=False, auto_reset=True)
    e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel="auto", freeze_done=False, auto_reset=True)
    for launch in range(2):
        acts = torch.randint(0, 3, (T, B, n), dtype=torch.int32, device="cuda", generator=g)
        o1, o2 = e1.rollout(acts), e2.rollout(acts)
        for k in ("reward", "terminated", "win", "obs", "state"):
            assert torch.equal(o1[k], o2[k]), (launch, k)
        del o1, o2
    r1, r2 = raw_state(e1), raw_state(e2)
    for k in ("tgt", "agent", "hdr", "mt"):
        assert torch.equal(r1[k], r2[k]), k


@pytest.mark.parametrize("kernel", ["oct", "od", "ode", "lanev", "lane"])
@pytest.mark.parametrize("n", [5, 8])
def test_every_target_in_view_of_every_agent_draws_past_slot_63(kernel, n):
    """view_range = 70 on the 50 x 50 map: all 15 targets are within every agent's sensor range in every step, so a step makes
    15 n draws -- 75 at 5 agents, 120 at 8: past the first 64-bit window of the hit tape, the side path the octet kernels'
    detection pass takes when an env has more than 64 pairs in range (round 5) -- and a row of 624 stream words lasts four
    steps (two at 8 agents): the row refresh machinery of every kernel runs flat out.  detect_prob 0.3 keeps episodes long.
    Against the 16-lane step kernel, step by step: rewards, flags, obs / state rows, raw state, canonical MT rows."""
    if kernel == "lanev" and n > 5:
        pytest.skip("k_rollout_lanev serves teams of up to 5")
    B, T = 200, 48
    args = cs.make_env_args("flight_easy", n_agents=n)
    args.view_range, args.detect_prob = 70, 0.3
    seeds = np.arange(B, dtype=np.uint32) + 4242
    acts = torch.randint(0, 3, (T, B, n), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
    e1 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel="group", freeze_done=False, auto_reset=True)
    e2 = cs.BatchedFlightEnv(args, batch=B, seeds=seeds, kernel=kernel, freeze_done=False, auto_reset=True)
    out = e2.rollout(acts)
    drew = 0
    for t in range(T):
        w0 = words(hdr(e1))
        r, term, win = e1.step(acts[t])
        drew = max(drew, int((words(hdr(e1)) - w0).max()))
        assert torch.equal(r, out["reward"][t]) and torch.equal(term, out["terminated"][t]) and torch.equal(win, out["win"][t]), t
        if t % 6 == 0 or t == T - 1:
            assert torch.equal(e1.get_obs(), out["obs"][t]) and torch.equal(e1.get_state(), out["state"][t]), t
    assert drew >= 2 * 15 * n          # every (agent, target) pair drew in some step: 150 / 240 stream words in one step
    r1, r2 = raw_state(e1), raw_state(e2)
    for k in ("tgt", "agent", "hdr", "mt"):
        assert torch.equal(r1[k], r2[k]), k
