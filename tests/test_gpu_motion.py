"""GPU tests of moving targets (cs_move_targets, csrc/motion.h; motion.MovingTargetEnv): the kernel equals the definition
(motion.move_targets_torch) bit for bit on the cases of tests/motion_cases.py, and the env -- step, rollout, rollout_policy,
collect_flight, shards, resume, the static path -- equals a plain BatchedFlightEnv whose targets the definition moves by hand.
Everything is torch.equal: no tolerance."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import motion as mo
from cooperative_search_amd import runner as rn
from cooperative_search_amd.learner import get_ppo_args
import motion_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(t):
    return t.contiguous().view(torch.int64)


def make_args(env_name="flight_easy", n=3, m=15, time_limit=None, **motion):
    args = cs.make_env_args(env_name, n_agents=n, target_num=m, target_mode=0 if m <= 15 else 1)
    if time_limit is not None:
        args.time_limit = time_limit
    for k, v in motion.items():
        setattr(args, k, v)
    return args


def records(env):
    return env.snapshot().records


# ---- 1. the kernel equals the definition --------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,n,m", mc.SHAPES)
def test_kernel_equals_the_definition(B, n, m):
    """The generator's cases (what each holds: test_motion_cpu.py) in a real env's raw() views; 257 envs make a ragged last
    block, the second offset exercises the high key word."""
    env = cs.BatchedFlightEnv(make_args(n=n, m=m), batch=B)
    assert env.time_limit == mc.LIMIT and env.map_size == mc.MAP
    raw = env.raw()
    for mode in ("walk", "evade"):
        for speed in (0.5, 30.0):
            case = mc.make_case(B, n, m, mode, speed)
            for persist in (1, 4):
                for off in (0, (1 << 32) + 7):
                    motion = mo.TargetMotion(mode=mode, speed=speed, persist=persist, sense=mc.SENSE, seed=0xC0FFEE)
                    for k in ("tgt", "agent", "hdr"):
                        raw[k].copy_(case[k])
                    mo.move_targets(env, motion, env_offset=off)
                    want = mo.move_targets_torch(case["tgt"], case["agent"], case["hdr"], motion, env, off)
                    assert torch.equal(bits(raw["tgt"].cpu()), bits(want)), (mode, speed, persist, off)
                    assert torch.equal(bits(raw["agent"].cpu()), bits(case["agent"])) and torch.equal(raw["hdr"].cpu(), case["hdr"])
                    assert not torch.equal(bits(want), bits(case["tgt"]))
                    on_dev = mo.move_targets_torch(*(case[k].to(DEV) for k in ("tgt", "agent", "hdr")), motion, env, off)
                    assert torch.equal(bits(on_dev.cpu()), bits(want))   # the definition is the same on either device


# ---- 2. MovingTargetEnv equals the plain env driven by hand -------------------------------------------------------------------

def drive_by_hand(plain, motion, actions, phase=0):
    """The plain env stepped through `actions` [T, B, n], its targets moved by the DEFINITION on the CPU before every due step.
    -> per-step (reward, terminated, win, obs, state) clones."""
    rows = []
    for t in range(actions.shape[0]):
        if (phase + t) % motion.every == 0:
            raw = plain.raw()
            moved = mo.move_targets_torch(raw["tgt"].cpu(), raw["agent"].cpu(), raw["hdr"].cpu(), motion, plain, plain.env_offset)
            raw["tgt"].copy_(moved)
        r, term, win = plain.step(actions[t])
        rows.append(tuple(x.clone() for x in (r, term, win, plain.get_obs(), plain.get_state())))
    return rows


@pytest.mark.parametrize("env_name,B,T,every,mode", [("flight_easy", 33, 24, 1, "walk"), ("flight_easy", 33, 24, 3, "evade"),
                                                     ("flight", 5, 8, 1, "evade")])
def test_moving_env_equals_the_plain_env_moved_by_the_definition(env_name, B, T, every, mode):
    """time_limit 16 on flight_easy: every env runs out of time inside the 24 steps, so finished envs are met too."""
    limit = 16 if env_name == "flight_easy" else None
    motion = mo.TargetMotion(mode=mode, speed=0.75, every=every, persist=2, sense=12.0, seed=5)
    moving = mo.MovingTargetEnv(make_args(env_name, time_limit=limit), batch=B, target_motion=motion, env_offset=3)
    plain = cs.BatchedFlightEnv(make_args(env_name, time_limit=limit), batch=B, env_offset=3)
    assert torch.equal(records(moving), records(plain)) and moving.motion_phase == 0
    g = torch.Generator().manual_seed(B + T)
    actions = torch.randint(0, 3, (T, B, 3), generator=g).to(DEV)
    start = plain.raw()["tgt"].clone()
    want = drive_by_hand(plain, motion, actions)
    for t in range(T):
        r, term, win = moving.step(actions[t])
        got = (r, term, win, moving.get_obs(), moving.get_state())
        for name, a, b in zip(("reward", "terminated", "win", "obs", "state"), got, want[t]):
            assert torch.equal(a, b), (t, name)
    assert moving.motion_phase == T
    assert torch.equal(records(moving), records(plain))
    assert not torch.equal(moving.raw()["tgt"], start)


# ---- 2b. ... through every rollout layout, team and reset mode -----------------------------------------------------------------

SWEEP_B, SWEEP_CALLS, SWEEP_LIMIT = 77, (1, 2, 5, 9, 7), 7   # nine full octet wavefronts' worth + a tail of 5; every env ends
SWEEP_KERNELS = ("group", "oct", "od", "ode", "lane", "lanev")
SWEEP_TEAMS = [(1, 1, 1), (3, 15, 0), (5, 16, 1), (8, 16, 1)]   # (n_agents, n_targets, target_mode)
SWEEP_MODES = dict(frozen=dict(freeze_done=True), auto_reset=dict(freeze_done=False, auto_reset=True), unfrozen=dict(freeze_done=False))
SWEEP_CASES = [(k, n, m, tm, mode, "evade") for k in SWEEP_KERNELS for (n, m, tm) in SWEEP_TEAMS for mode in SWEEP_MODES
               if not (k == "lanev" and n > 5)]                  # k_rollout_lanev serves teams of up to 5
SWEEP_CASES += [(k, 5, 16, 1, "auto_reset", "walk") for k in SWEEP_KERNELS]


def sweep_args(n, m, tmode):
    # agent_mode 1, the start line across the middle of the map: within the 7 steps of an episode every team comes within range of
    # targets (from y = 0 the three agents of the circle layout reach none), so targets are found and evade at the sensing radius
    args = cs.make_env_args("flight_easy", n_agents=n, agent_mode=1, target_num=m, target_mode=tmode)
    args.time_limit = SWEEP_LIMIT
    return args


def sweep_motion(args, how):
    if how == "walk":    # a move before every step: every launch is one step
        return mo.TargetMotion(mode="walk", speed=0.75, every=1, persist=2, seed=6)
    return mo.TargetMotion(mode="evade", speed=0.75, every=3, persist=2, sense=float(args.view_range), seed=6)   # hovering at the sensing radius


_by_hand = {}


def sweep_by_hand(n, m, tmode, mode, how):
    """The yardstick, once per (team, mode, motion) for the six kernels' cases: a plain kernel="group" env stepped one step at a
    time, its targets moved by the DEFINITION on the CPU.  -> per call (actions, rows, records after it)."""
    key = (n, m, tmode, mode, how)
    if key not in _by_hand:
        args = sweep_args(n, m, tmode)
        motion = sweep_motion(args, how)
        plain = cs.BatchedFlightEnv(args, batch=SWEEP_B, kernel="group", **SWEEP_MODES[mode])
        g = torch.Generator().manual_seed(100 * n + m)
        start, calls, phase = plain.raw()["tgt"].clone(), [], 0
        for T in SWEEP_CALLS:
            actions = torch.randint(0, 3, (T, SWEEP_B, n), generator=g).to(DEV)
            rows = drive_by_hand(plain, motion, actions, phase)
            phase += T
            calls.append((actions, rows, records(plain).clone()))
        # reach: some target moved, some target was found, and under auto_reset every env has started a second episode
        hdr = plain.raw()["hdr"].cpu()
        assert not torch.equal(plain.raw()["tgt"][:, :m], start[:, :m])
        assert sum(float((r[0] > 0).sum()) for _a, rows, _r in calls for r in rows) > 0    # a step's reward is positive only by a find
        if mode == "auto_reset":
            assert int(hdr[:, _lib.H_EPISODES].min()) >= 2
        _by_hand[key] = calls
    return _by_hand[key]


@pytest.mark.parametrize("kernel,n,m,tmode,mode,how", SWEEP_CASES,
                         ids=[f"{k}-n{n}-m{m}-{mode}-{how}" for (k, n, m, _t, mode, how) in SWEEP_CASES])
def test_moving_env_on_every_rollout_kernel_equals_the_group_env_moved_by_the_definition(kernel, n, m, tmode, mode, how):
    """Every rollout kernel reloads tgt at launch entry (k_rollout_lanev and k_rollout_od keep the normalised floats in registers
    from there on), and until now only the pair kernel that "auto" picks had met a target that moved between launches.
    time_limit 7: every env ends -- and under auto_reset restarts, on the reset's targets -- several times in the 24 steps."""
    args = sweep_args(n, m, tmode)
    moving = mo.MovingTargetEnv(args, batch=SWEEP_B, target_motion=sweep_motion(args, how), kernel=kernel, **SWEEP_MODES[mode])
    phase = 0
    for actions, rows, recs in sweep_by_hand(n, m, tmode, mode, how):
        out = moving.rollout(actions)
        for t, row in enumerate(rows):
            for name, b in zip(TABLES, row):
                assert torch.equal(out[name][t], b), (phase + t, name)
        phase += actions.shape[0]
        assert moving.motion_phase == phase
        assert torch.equal(records(moving), recs), phase


# ---- 3. one call equals many --------------------------------------------------------------------------------------------------

MOTION3 = mo.TargetMotion(mode="evade", speed=0.5, every=3, persist=2, sense=10.0, seed=11)
TABLES = ("reward", "terminated", "win", "obs", "state")


def test_one_rollout_equals_two_and_equals_single_steps():
    B, T = 33, 20
    envs = [mo.MovingTargetEnv(make_args(time_limit=14), batch=B, target_motion=MOTION3) for _ in range(3)]
    actions = torch.randint(0, 3, (T, B, 3), generator=torch.Generator().manual_seed(1)).to(DEV)
    one = envs[0].rollout(actions)
    a, b = envs[1].rollout(actions[:7]), envs[1].rollout(actions[7:])
    assert envs[1].motion_phase == envs[0].motion_phase == T
    for k in TABLES:
        assert torch.equal(one[k], torch.cat((a[k], b[k]))), k
    for t in range(T):
        r, term, win = envs[2].step(actions[t])
        for k, v in zip(TABLES, (r, term, win, envs[2].get_obs(), envs[2].get_state())):
            assert torch.equal(one[k][t], v), (t, k)
    assert torch.equal(envs[0].get_state(), envs[2].get_state()) and torch.equal(envs[0].get_obs(), envs[2].get_obs())
    assert torch.equal(records(envs[0]), records(envs[1])) and torch.equal(records(envs[0]), records(envs[2]))
    # caller buffers, no emission
    env = mo.MovingTargetEnv(make_args(time_limit=14), batch=B, target_motion=MOTION3)
    out = dict(reward=torch.empty(T, B, device=DEV), terminated=torch.empty(T, B, dtype=torch.bool, device=DEV),
               win=torch.empty(T, B, dtype=torch.uint8, device=DEV))
    res = env.rollout(actions, out=out)
    assert res["reward"].data_ptr() == out["reward"].data_ptr() and res.get("obs") is None
    assert all(torch.equal(res[k], one[k]) for k in TABLES[:3]) and torch.equal(env.get_state(), envs[0].get_state())


def fused(args, B, seed=3):
    torch.manual_seed(7)   # the same fresh network every time
    return cs.FusedAgents(args, B, seed=seed)


@pytest.mark.parametrize("softmax", [False, True])
def test_one_rollout_policy_equals_two_and_equals_the_choose_action_step_loop(softmax):
    B, T, n = 64, 20, 3
    args = make_args(time_limit=14)
    envs = [mo.MovingTargetEnv(args, batch=B, target_motion=MOTION3) for _ in range(3)]
    cs.apply_env_info(args, envs[0])
    if softmax:
        args.alg = "reinforce"
    agents = [fused(args, B) for _ in range(3)]
    assert agents[0].softmax == softmax
    kw = [dict(epsilon=0.0, evaluate=True) for _ in range(3)]
    eps = trace = None
    if softmax:   # sampling, with a carried per-env epsilon that anneals per executed step
        eps = [torch.linspace(0.2, 0.9, B, dtype=torch.float64, device=DEV) for _ in range(3)]
        trace = [torch.zeros(T, B, dtype=torch.float64, device=DEV) for _ in range(3)]
        kw = [dict(epsilon=0.5, evaluate=False, eps_env=eps[i], anneal=0.01, min_epsilon=0.3, per_step=True) for i in range(3)]
    one = envs[0].rollout_policy(agents[0], T, eps_trace=None if trace is None else trace[0], **kw[0])
    a = envs[1].rollout_policy(agents[1], 7, eps_trace=None if trace is None else trace[1][:7], **kw[1])
    b = envs[1].rollout_policy(agents[1], 13, eps_trace=None if trace is None else trace[1][7:], **kw[1])
    for k in TABLES + ("actions",):
        assert torch.equal(one[k], torch.cat((a[k], b[k]))), k
    env, ag = envs[2], agents[2]
    for t in range(T):
        u = ag.choose_action(env.get_obs(), kw[2]["epsilon"], kw[2]["evaluate"], eps_env=None if eps is None else eps[2])
        if softmax:
            env.epsilon_step(eps[2], 0.01, 0.3, trace[2][t])
        r, term, win = env.step(u)
        for k, v in zip(TABLES + ("actions",), (r, term, win, env.get_obs(), env.get_state(), u)):
            assert torch.equal(one[k][t], v), (t, k)
    for i in (1, 2):
        assert torch.equal(records(envs[0]), records(envs[i])), i
        assert torch.equal(agents[0].hidden, agents[i].hidden) and torch.equal(agents[0].actions, agents[i].actions)
        assert agents[0].calls == agents[i].calls == T and envs[i].motion_phase == T
        if softmax:
            assert torch.equal(eps[0], eps[i]) and torch.equal(trace[0], trace[i])
    if softmax:
        assert len(torch.unique(one["actions"])) == 3 and not torch.equal(trace[0][0], trace[0][-1])


def test_collect_flight_equals_rollout_policy():
    B, T, n = 4, 20, 3
    args = make_args("flight", time_limit=14)
    envs = [mo.MovingTargetEnv(args, batch=B, target_motion=MOTION3) for _ in range(2)]
    cs.apply_env_info(args, envs[0])
    agents = [fused(args, B) for _ in range(2)]
    entry = envs[0].get_state().clone()
    got = envs[0].collect_flight(agents[0], T)
    want = envs[1].rollout_policy(agents[1], T)
    for k in ("actions", "reward", "terminated", "win"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["state"][0], entry)              # the state the call found, before the first move
    assert torch.equal(got["state"][1:], want["state"])      # row t + 1: after step t, before the next move
    assert torch.equal(got["map"][1:], want["obs"][:, :, 0, :envs[0].cells])
    assert torch.equal(records(envs[0]), records(envs[1])) and torch.equal(agents[0].hidden, agents[1].hidden)
    assert torch.equal(envs[0].get_state(), envs[1].get_state())
    moved = got["state"][1:, :, 4 * n:] != got["state"][:-1, :, 4 * n:]
    assert bool(moved.any())


# ---- 4. the static path -------------------------------------------------------------------------------------------------------

def test_speed_zero_never_launches_and_equals_the_plain_env(monkeypatch):
    calls = []
    real = mo._ops()

    class Counting:
        def __getattr__(self, name):
            if name == "move_targets":
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(mo, "_ops", lambda: Counting())
    B, T = 33, 20
    args = make_args(time_limit=14, target_speed=0.0, target_motion="evade", target_sense=10.0)
    plain = mo.make_env(args, batch=B)
    assert type(plain) is cs.BatchedFlightEnv
    static = mo.MovingTargetEnv(args, batch=B)
    assert not static.moving
    actions = torch.randint(0, 3, (T, B, 3), generator=torch.Generator().manual_seed(2)).to(DEV)
    for env in (plain, static):
        env.rollout(actions[:8])
        for t in range(8, T):
            env.step(actions[t])
    static.move_targets()
    assert calls == [] and torch.equal(records(static), records(plain))
    args.target_speed = 0.5
    moving = mo.make_env(args, batch=B)
    assert type(moving) is mo.MovingTargetEnv and moving.motion == mo.TargetMotion("evade", 0.5, 1, 1, 10.0, 0)
    moving.step(actions[0])
    assert calls == ["move_targets"]


# ---- 5. shards ----------------------------------------------------------------------------------------------------------------

def test_two_shards_equal_one_batch():
    T = 12
    motion = mo.TargetMotion(mode="walk", speed=1.0, every=2, persist=3, seed=9)
    whole = mo.MovingTargetEnv(make_args(), batch=32, target_motion=motion)
    shards = [mo.MovingTargetEnv(make_args(), batch=16, target_motion=motion, env_offset=off) for off in (0, 16)]
    actions = torch.randint(0, 3, (T, 32, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    out = whole.rollout(actions)
    parts = [s.rollout(actions[:, 16 * i:16 * i + 16].contiguous()) for i, s in enumerate(shards)]
    for k in TABLES:
        assert torch.equal(out[k], torch.cat([p[k] for p in parts], 1)), k
    assert torch.equal(records(whole), torch.cat([records(s) for s in shards]))
    assert not torch.equal(records(shards[0])[:, 128:384], records(shards[1])[:, 128:384])


# ---- 6. resume ----------------------------------------------------------------------------------------------------------------

def test_a_restored_env_goes_on_as_the_original_and_a_forked_record_diffuses_on_its_own():
    B, T = 16, 20
    motion = mo.TargetMotion(mode="walk", speed=0.5, every=3, persist=2, seed=4)
    first = mo.MovingTargetEnv(make_args(), batch=B, target_motion=motion)
    second = mo.MovingTargetEnv(make_args(), batch=B, target_motion=motion, seeds=np.arange(B) + 999)
    actions = torch.randint(0, 3, (T, B, 3), generator=torch.Generator().manual_seed(4)).to(DEV)
    first.rollout(actions[:7])
    snap = first.snapshot()
    second.restore(snap)
    second.motion_phase = 7
    a, b = first.rollout(actions[7:]), second.rollout(actions[7:])
    for k in TABLES:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(records(first), records(second)) and first.motion_phase == second.motion_phase == T
    # one record forked into env 0 and env 5: the same stream and agents, another walk
    third = mo.MovingTargetEnv(make_args(), batch=B, target_motion=mo.TargetMotion(mode="walk", speed=0.5, seed=4))
    third.restore(snap, src=[0, 0], dst=[0, 5])
    act = actions[7].clone()
    act[5] = act[0]
    third.step(act)
    raw = third.raw()
    assert torch.equal(raw["agent"][0], raw["agent"][5]) and not torch.equal(raw["tgt"][0], raw["tgt"][5])


# ---- 7. a bad action ----------------------------------------------------------------------------------------------------------

def test_a_bad_action_in_a_later_run_leaves_the_envs_untouched():
    B, T = 8, 9
    env = mo.MovingTargetEnv(make_args(), batch=B, target_motion=MOTION3, check_actions=True)
    actions = torch.randint(0, 3, (T, B, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    actions[7, 2, 1] = 3     # the third run: steps 6..8
    assert mo.split_runs(0, T, 3)[2] == (6, 9, True)
    before, tgt = records(env).clone(), env.raw()["tgt"].clone()
    with pytest.raises(IndexError, match=r"list index out of range: action 3 of step 7, env 2, agent 1 is not in 0\.\.2"):
        env.rollout(actions)
    assert torch.equal(records(env), before) and torch.equal(env.raw()["tgt"], tgt) and env.motion_phase == 0 and env.check_actions
    with pytest.raises(IndexError, match="list index out of range: action 3 of step 0, env 2, agent 1"):
        env.step(actions[7])
    assert torch.equal(records(env), before) and env.motion_phase == 0
    plain = cs.BatchedFlightEnv(make_args(), batch=B, check_actions=True)
    with pytest.raises(IndexError) as parent:    # the parent's wording, word for word
        plain.rollout(actions)
    with pytest.raises(IndexError) as mine:
        env.rollout(actions)
    assert str(mine.value).splitlines()[0] == str(parent.value).splitlines()[0]
    actions[7, 2, 1] = 0
    env.rollout(actions)
    assert env.motion_phase == T and not torch.equal(records(env), before)


# ---- 8. consumers take the object unchanged -----------------------------------------------------------------------------------

def check_recorded_targets(s, s_next, padded, n, m):
    """Episode state rows [E, T, S], target j = (xn, yn, found) at 4n + 3j: between a real step's s and s_next some unfound
    target has moved, and no target that was found in both rows has."""
    real = padded.reshape(padded.shape[0], -1)[:, :, None] == 0
    t0, t1 = s[:, :, 4 * n:].reshape(*s.shape[:2], m, 3), s_next[:, :, 4 * n:].reshape(*s.shape[:2], m, 3)
    differs = (t0[..., :2] != t1[..., :2]).any(-1)
    found_both = (t0[..., 2] != 0) & (t1[..., 2] != 0)
    assert bool((real & found_both).any()) and bool((real & (t0[..., 2] == 0)).any())
    assert not bool((differs & found_both & real).any())
    assert bool((differs & (t0[..., 2] == 0) & real).any())


def test_collector_buffer_and_runner_take_the_moving_env(tmp_path):
    B, n, m = 64, 3, 15
    args = make_args(time_limit=60, target_speed=0.5, target_motion="evade", target_sense=8.0, target_move_every=2)
    env = mo.make_env(args, batch=B)
    assert isinstance(env, mo.MovingTargetEnv) and env.motion.every == 2
    cs.apply_env_info(args, env)
    col = cs.EpisodeCollector(env)
    episode, _r, _w, found = col.generate_episodes(policy=cs.CoverageAgents(env).policy())
    assert episode["s"].shape == (B, 60, 4 * n + 3 * m) and int(found.sum()) > 0 and env.motion_phase == 60
    check_recorded_targets(episode["s"], episode["s_next"], episode["padded"], n, m)
    sw = cs.sweep_batch(episode, env)
    assert int(sw.new_cells.sum()) > 0
    # a FusedAgents straight into a ring
    get_ppo_args(args, seed=3)
    args.alg = "ppo"
    ring = cs.DeviceReplayBuffer(args, B)
    col.generate_episodes(agents=fused(args, B), epsilon=0.2, evaluate=False, into=ring)
    batch = ring.sample(B)
    check_recorded_targets(batch["s"], batch["s_next"], batch["padded"], n, m)
    # one Runner epoch
    args.evaluate_cycle, args.evaluate_epoch, args.save_cycle = 1, B, 1000
    args.model_dir, args.result_dir = str(tmp_path / "model") + "/", str(tmp_path / "result") + "/"
    runner = rn.Runner(env, args)
    seen = []
    train = runner.train
    runner.train = lambda b, step: (seen.append(b), train(b, step))[1]
    runner.run(0, n_epoch=1)
    assert len(seen) == 1 and runner.epoch == 1
    check_recorded_targets(seen[0]["s"], seen[0]["s_next"], seen[0]["padded"], n, m)
