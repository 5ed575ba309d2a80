"""GPU tests of env snapshot / restore (cs_snapshot, cs_restore; cooperative-search_amd/snapshot.py): a restored env continues
bit for bit, whichever kernel runs it; records are canonical; a stale hit tape cannot survive a restore; forks, subsets,
re-batching, refusals, flight's map, and no host synchronisation.

Shapes are the smallest at which the kernels take their different paths: B = 24 for flight_easy (more than an octet and a
16-env workgroup, a multiple of neither 16 nor 64), B = 8 for flight, teams of 3 and 5, 6 for the first lane kernel, T = 40.
time_limit is 25 so that episodes end -- and auto-reset, drawing from the env's stream -- inside every window."""
import functools

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd.snapshot import EnvSnapshot

pytestmark = pytest.mark.gpu
B_EASY, B_FLIGHT, T = 24, 8, 40
WARM = 7   # steps before the snapshot: mid-episode


def make_env(variant="flight_easy", n=3, B=None, kernel="auto", seed0=500, time_limit=25, **kw):
    B = B or (B_FLIGHT if variant == "flight" else B_EASY)
    args = cs.make_env_args(variant, n_agents=n)
    args.time_limit = time_limit
    kw.setdefault("freeze_done", False)
    kw.setdefault("auto_reset", True)
    return cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + seed0, kernel=kernel, **kw)


@functools.lru_cache(maxsize=None)
def actions(B, n, steps=T, seed=3):
    """int32 [steps, B, n] on the device; computed once per shape and never written."""
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 3, size=(steps, B, n)).astype(np.int32)).cuda()


def run_steps(env, acts):
    keep = []
    for a in acts:
        r, t, w = env.step(a)
        keep.append([x.clone() for x in (r, t, w, env.get_obs(), env.get_state())])
    return [torch.stack(c) for c in zip(*keep)]


def run_rollout(env, acts):
    out = env.rollout(acts)
    return [out[k] for k in ("reward", "terminated", "win", "obs", "state")]


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same(a, b, what=""):
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(bits(x), bits(y)), (what, k)


def tape_of(env):
    lay = env.layout
    return env._view(lay.tape_off, env.batch * 16, torch.int32, (env.batch, 16))


def words_of(env):
    h = env.raw()["hdr"].to(torch.int64)
    return (h[:, _lib.H_WORDS_LO] & 0xFFFFFFFF) | ((h[:, _lib.H_WORDS_HI] & 0xFFFFFFFF) << 32)


# ---- 1. round trip ----------------------------------------------------------------------------------------------------------

CASES = [("flight_easy", n, k) for n in (3, 5) for k in ("group", "oct", "od", "ode", "lanev")] + \
        [("flight_easy", 6, "lane"), ("flight", 3, "auto"), ("flight", 5, "auto")]


@pytest.mark.parametrize("mode", ["step", "rollout"])
@pytest.mark.parametrize("variant, n, kernel", CASES)
def test_a_restored_env_repeats_itself_bit_for_bit(variant, n, kernel, mode):
    env = make_env(variant, n, kernel=kernel)
    run = run_steps if mode == "step" else run_rollout
    run_steps(env, actions(env.batch, n, WARM, seed=1))
    snap = env.snapshot()
    assert snap.records.shape == (env.batch, 3136 + (10000 if variant == "flight" else 0)) and snap.records.dtype == torch.uint8
    first = run(env, actions(env.batch, n))
    end1 = env.snapshot()
    assert not torch.equal(end1.records, snap.records)
    env.restore(snap)
    assert torch.equal(env.snapshot().records, snap.records)
    second = run(env, actions(env.batch, n))
    assert_same(first, second, (variant, n, kernel, mode))
    assert torch.equal(env.snapshot().records, end1.records)


# ---- 2. canonical form ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def reference_records(n):
    """The records after WARM single steps and a T-step rollout on the 16-lane kernels."""
    env = make_env("flight_easy", n, kernel="group")
    run_steps(env, actions(B_EASY, n, WARM, seed=1))
    env.rollout(actions(B_EASY, n))
    return env.snapshot().records


@pytest.mark.parametrize("n, kernel", [(3, "oct"), (3, "od"), (3, "ode"), (3, "lanev"), (5, "ode"), (5, "lanev"), (6, "lane"), (6, "oct")])
def test_records_do_not_depend_on_the_kernel(n, kernel):
    env = make_env("flight_easy", n, kernel=kernel)
    run_steps(env, actions(B_EASY, n, WARM, seed=1))
    env.rollout(actions(B_EASY, n))
    got, want = env.snapshot().records, reference_records(n)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} bytes differ, first (env, byte) {bad[:6].tolist()}"


def test_a_record_is_the_same_before_and_after_mt_advance():
    env = make_env("flight_easy", 3, step_advance=False)
    run_steps(env, actions(B_EASY, 3, 20, seed=1))
    before = env.snapshot().records
    assert int((env.raw()["ahead"] < 624).sum()) > 0   # rows in the plain circular form: the two states differ in the blob
    env.mt_advance(625)
    assert int((env.raw()["ahead"] < 624).sum()) == 0
    assert torch.equal(env.snapshot().records, before)


# ---- 3. the stale tape ------------------------------------------------------------------------------------------------------

def test_a_tape_of_another_stream_does_not_survive_a_restore():
    """Y's stored tapes carry the restoring config's threshold and a base at or below X's consumed-word count.  tape_finish
    also wants `used + ahead <= 624`, which after a restore (ahead = 624) holds only for base == X's word count exactly: that
    accepting case is built by the next test; here a stale tape must simply not matter, whatever restore does with it."""
    n = 3
    x = make_env("flight_easy", n, seed0=500)
    y = make_env("flight_easy", n, seed0=90000)
    run_steps(x, actions(B_EASY, n, 60, seed=11))
    snap = x.snapshot()
    run_steps(y, actions(B_EASY, n, 33, seed=12))   # step() refreshed the tapes before steps 0 and 32
    tape = tape_of(y).to(torch.int64) & 0xFFFFFFFF
    base, K = tape[:, 10] | (tape[:, 11] << 32), tape[:, 12] | (tape[:, 13] << 32)
    want_K = int(np.floor(float(y.detect_prob) * 2.0 ** 53))
    hazard = (K == want_K) & (base <= words_of(x))
    assert int(hazard.sum()) >= 1, "precondition: no env of Y holds a tape that X's word count would accept"
    assert not torch.equal(y.snapshot().records, snap.records)
    y.restore(snap)
    acts = actions(B_EASY, n, 40, seed=13)
    for t, a in enumerate(acts):
        rx, ry = x.step(a), y.step(a)
        assert_same(rx, ry, ("step", t))
        hx, hy = x.raw()["hdr"], y.raw()["hdr"]
        assert torch.equal(hx[:, _lib.H_FOUND], hy[:, _lib.H_FOUND]), t
        assert torch.equal(words_of(x), words_of(y)), t
        assert_same([x.get_obs(), x.get_state()], [y.get_obs(), y.get_state()], ("views", t))
    assert torch.equal(x.snapshot().records, y.snapshot().records)


def test_a_tape_that_tape_finish_would_accept_is_replaced_by_restore():
    """The case in which a foreign tape passes ALL of tape_finish's checks: same threshold, base == the restored word count
    (used = 0, so used + ahead = 624).  X and Y are fresh after their first reset, from different seeds; with uniform targets
    (target_mode 1) a reset draws 4 words per target plus two per in-range pair, so several env pairs sit at the same word
    count.  Y's tapes are written there by mt_advance.  If restore left them, Y's hazard envs would answer X's detections with
    their own stream's hit bits (a draw hits with probability 0.9: two streams disagree on 18 % of the draws)."""
    n = 3

    def fresh(seed0):
        args = cs.make_env_args("flight_easy", n_agents=n, target_mode=1)
        return cs.BatchedFlightEnv(args, batch=B_EASY, seeds=np.arange(B_EASY, dtype=np.uint32) + seed0, freeze_done=False,
                                   auto_reset=True)
    x, y = fresh(500), fresh(90000)
    y.mt_advance(625)   # every row twisted fully ahead, every tape written at Y's current word count
    snap = x.snapshot()
    old = tape_of(y).clone()
    tape = old.to(torch.int64) & 0xFFFFFFFF
    base, K = tape[:, 10] | (tape[:, 11] << 32), tape[:, 12] | (tape[:, 13] << 32)
    want_K = int(np.floor(float(y.detect_prob) * 2.0 ** 53))
    hazard = (K == want_K) & (base == words_of(x)) & (y.raw()["ahead"] == 624)
    print("envs whose stored tape tape_finish would accept after a raw copy:", int(hazard.sum()), "of", B_EASY)
    assert int(hazard.sum()) >= 1, "precondition: no env of Y holds a tape that passes tape_finish for X's record"
    y.restore(snap)
    new = tape_of(y)
    assert bool((new[hazard][:, :10] != old[hazard][:, :10]).any(dim=1).all())   # other hit bits: the tape was rebuilt from X's row
    assert torch.equal(new[hazard][:, 10:14], old[hazard][:, 10:14])             # ... under the very base and threshold that matched
    for t, a in enumerate(actions(B_EASY, n, 40, seed=13)):
        assert_same(x.step(a), y.step(a), ("step", t))
        assert torch.equal(x.raw()["hdr"][:, _lib.H_FOUND], y.raw()["hdr"][:, _lib.H_FOUND]), t
        assert torch.equal(words_of(x), words_of(y)), t
        assert_same([x.get_obs(), x.get_state()], [y.get_obs(), y.get_state()], ("views", t))
    assert torch.equal(x.snapshot().records, y.snapshot().records)


# ---- 4. fork ----------------------------------------------------------------------------------------------------------------

def test_one_record_forked_into_a_whole_batch():
    n = 3
    env = make_env("flight_easy", n)
    run_steps(env, actions(B_EASY, n, WARM, seed=1))
    snap = env.snapshot()
    env.restore(snap, src=torch.zeros(B_EASY, dtype=torch.int64, device="cuda"))
    recs = env.snapshot().records
    assert torch.equal(recs, snap.records[:1].expand_as(recs))
    same = actions(1, n).expand(T, B_EASY, n).contiguous()
    out = run_rollout(env, same)
    for k, v in enumerate(out):
        assert torch.equal(bits(v), bits(v[:, :1].expand_as(v))), k


# ---- 5. subset --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["flight_easy", "flight"])
def test_envs_not_named_are_untouched(variant):
    n = 3
    a, b = make_env(variant, n, seed0=500), make_env(variant, n, seed0=7000)
    B = a.batch
    run_steps(a, actions(B, n, WARM, seed=1))
    run_steps(b, actions(B, n, 12, seed=2))
    snap = a.snapshot()
    src, dst = [0, 0, 5], [1, B - 2, 4]
    before = b.snapshot().records.clone()
    blob = b._blob.clone()
    raw_before = {k: v.clone() for k, v in b.raw().items()}
    tape_before = tape_of(b).clone()
    b.restore(snap, src=src, dst=dst)
    after = b.snapshot().records
    others = [i for i in range(B) if i not in dst]
    assert torch.equal(after[others], before[others])
    assert torch.equal(after[dst], snap.records[src])
    for k, v in b.raw().items():
        assert torch.equal(v[others], raw_before[k][others]), k
    assert torch.equal(tape_of(b)[others], tape_before[others])
    assert not torch.equal(b._blob, blob)
    assert torch.equal(b.get_state()[dst], a.get_state()[src]) and torch.equal(b.get_obs()[dst], a.get_obs()[src])


# ---- 6. re-batching ---------------------------------------------------------------------------------------------------------

def test_records_of_one_batch_continue_in_three_smaller_ones():
    n = 3
    big = make_env("flight_easy", n)
    run_steps(big, actions(B_EASY, n, WARM, seed=1))
    snap = big.snapshot()
    acts = actions(B_EASY, n)
    want = run_rollout(big, acts)
    end = big.snapshot().records
    for part in range(3):
        lo = 8 * part
        small = make_env("flight_easy", n, B=8, seed0=31337 + part)
        small.restore(snap, src=torch.arange(lo, lo + 8, device="cuda"))
        got = run_rollout(small, acts[:, lo:lo + 8].contiguous())
        assert_same(got, [w[:, lo:lo + 8] for w in want], part)
        assert torch.equal(small.snapshot().records, end[lo:lo + 8])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

def test_a_snapshot_of_another_team_size_is_refused_on_the_host():
    three, five = make_env("flight_easy", 3), make_env("flight_easy", 5)
    before = five.snapshot().records.clone()
    blob = five._blob.clone()
    with pytest.raises(ValueError, match="n_agents"):
        five.restore(three.snapshot())
    assert torch.equal(five._blob, blob) and torch.equal(five.snapshot().records, before)


@pytest.mark.parametrize("what", ["header", "cursor", "unused", "dst", "src"])
def test_the_op_names_the_first_refused_entry_and_leaves_its_env(what):
    ops = _lib.torch_ops()
    n = 3
    a, b = make_env("flight_easy", n, seed0=500), make_env("flight_easy", n, seed0=7000)
    recs = a.snapshot().records.clone()
    src = torch.arange(4, dtype=torch.int64, device="cuda")
    dst = torch.tensor([3, 10, 17, 20], dtype=torch.int64, device="cuda")
    if what == "header":
        recs.view(torch.int32)[2, 3] = 5          # record 2 claims n_agents = 5
        want, untouched = [1, 3, 2, 3], 17
    elif what == "cursor":
        recs.view(torch.int32)[1, 16 + _lib.H_MT_POS] = 625
        want, untouched = [1, 3, 1, 16 + _lib.H_MT_POS], 10
    elif what == "unused":
        recs.view(torch.int32)[3, 16 + 13] = 1    # header words 12..15 of a record are zero
        want, untouched = [1, 3, 3, 16 + 13], 20
    elif what == "dst":
        dst[1], dst[3] = B_EASY, -1               # two offenders: the first is named
        want, untouched = [1, 2, 1, B_EASY], None
    else:
        src[2] = B_EASY
        want, untouched = [1, 1, 2, B_EASY], 17
    before = b.snapshot().records.clone()
    status = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    ops.env_restore(b._cfg_t, b._blob, recs, src, dst, status, None, None)
    assert status.tolist() == want
    after = b.snapshot().records
    applied = [int(d) for i, d in enumerate(dst.tolist()) if 0 <= d < B_EASY and i != want[2]]
    others = [i for i in range(B_EASY) if i not in applied]
    assert torch.equal(after[others], before[others])
    if untouched is not None:
        assert untouched in others
    assert torch.equal(after[applied], recs[src[[i for i, d in enumerate(dst.tolist()) if int(d) in applied]]])
    # and a clean call says so
    ops.env_restore(b._cfg_t, b._blob, a.snapshot().records, None, None, status, None, None)
    assert status.tolist() == [0, -1, -1, 0]


# ---- 8. flight's map --------------------------------------------------------------------------------------------------------

def test_the_probability_map_travels_and_survives_a_reset():
    n = 3
    a, b = make_env("flight", n, seed0=500), make_env("flight", n, seed0=7000)
    run_steps(a, actions(B_FLIGHT, n, 20, seed=1))
    cells = a.cells
    amap = a.get_obs()[:, :, :cells].clone()
    assert float((amap != 0.5).float().mean()) > 0.01   # the sweeps have written into it
    b.restore(a.snapshot())
    assert torch.equal(bits(b.get_obs()), bits(a.get_obs())) and torch.equal(bits(b.get_state()), bits(a.get_state()))
    assert torch.equal(bits(b.raw()["prob"]), bits(a.raw()["prob"]))
    a.reset()
    b.reset()   # init=False: the map persists across episodes (flight_env.py:84-86)
    assert torch.equal(bits(b.get_obs()), bits(a.get_obs()))
    assert float((b.get_obs()[:, 0, :cells] != 0.5).float().mean()) > 0.01   # not cleared: init=True alone sets 0.5 everywhere
    assert torch.equal(b.snapshot().records, a.snapshot().records)


# ---- 9. no synchronisation --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["flight_easy", "flight"])
def test_snapshot_and_restore_never_synchronise(variant):
    env = make_env(variant, 3)
    idx = torch.tensor([2, 0, 5], dtype=torch.int64, device="cuda")
    dst = torch.tensor([1, 7, 3], dtype=torch.int64, device="cuda")
    src = torch.tensor([0, 0, 2], dtype=torch.int64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        whole = env.snapshot()
        part = env.snapshot(idx)
        env.restore(part, src=src, dst=dst, status=status)
        env.restore(whole)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert isinstance(part, EnvSnapshot) and len(part) == 3 and len(whole) == env.batch
    assert status.tolist() == [0, -1, -1, 0]
    assert torch.equal(env.snapshot().records, whole.records)


# ---- 10. the B = 1 adapters and the ctypes binding ----------------------------------------------------------------------------

@pytest.mark.parametrize("variant, cls", [("flight_easy", cs.FlightSearchEnvEasy), ("flight", cs.FlightSearchEnv)])
def test_one_env_of_a_batch_continues_in_the_b1_adapter(variant, cls):
    n, pick = 3, 5
    env = make_env(variant, n, auto_reset=False, time_limit=200)   # the adapters: no terminal guard, no auto-reset
    run_steps(env, actions(env.batch, n, WARM, seed=1))
    args = cs.make_env_args(variant, n_agents=n)
    one = cls(args, cs.default_circle_dict(), seed=1)
    one.restore(env.snapshot(), src=pick)
    assert torch.equal(one.snapshot().records, env.snapshot([pick]).records)
    assert one.target_find == int(env.target_find[pick]) and one.time_step == WARM
    assert np.array_equal(np.asarray(one.agent_pos), env.raw()["agent"][pick, :n, :2].cpu().numpy())
    for t, a in enumerate(actions(env.batch, n, 10, seed=2)):
        r, term, win = env.step(a)
        r1, t1, w1 = one.step(a[pick].tolist())
        assert (r1, t1, w1) == (int(r[pick]), bool(term[pick]), bool(win[pick])), t
        assert np.array_equal(one.get_obs(), env.get_obs()[pick].double().cpu().numpy()), t
        assert np.array_equal(one.get_state(), env.get_state()[pick].double().cpu().numpy()), t
    assert torch.equal(one.snapshot().records, env.snapshot([pick]).records)
    with pytest.raises(ValueError, match="n_agents"):
        one.restore(make_env(variant, 5).snapshot())


@pytest.mark.parametrize("variant", ["flight_easy", "flight"])
def test_a_ctypes_bound_env_snapshots_through_the_torch_ops(variant):
    n = 3
    a, b = make_env(variant, n, binding="ctypes"), make_env(variant, n, binding="torch")
    assert a.binding == "ctypes" and b.binding == "torch"
    for env in (a, b):
        run_steps(env, actions(env.batch, n, WARM, seed=1))
    snap = a.snapshot()
    assert torch.equal(snap.records, b.snapshot().records)
    first = run_rollout(a, actions(a.batch, n))
    a.restore(snap)
    assert torch.equal(a.snapshot().records, snap.records)
    assert_same(first, run_rollout(a, actions(a.batch, n)), variant)
    assert_same(first, run_rollout(b, actions(b.batch, n)), variant)
