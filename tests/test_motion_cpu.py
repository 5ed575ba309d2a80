"""CPU tests of moving targets (motion.py, include/coopsearch.h: cs_move_targets): the boundary declares, exports and registers
the call; the kernel header holds the definition's heading tables; the definition (motion.move_targets_torch) has the properties
DESIGN.md section 19 states; the shared case generator plants what the GPU test relies on; the run-splitting rule of
MovingTargetEnv; and the refusals of TargetMotion, the entry point and the op.  Everything is bit equality: no tolerance."""
import ctypes as C
import math
import os
import re
import types

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import motion as mo
import motion_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEEDS, MODES = (0.5, 30.0), ("walk", "evade")
CASES = [(B, n, m, mode, speed) for (B, n, m) in mc.SHAPES for mode in MODES for speed in SPEEDS]


def bits(t):
    return t.contiguous().view(torch.int64)


def spec(mode="walk", speed=0.5, **kw):
    return mo.TargetMotion(mode=mode, speed=speed, sense=kw.pop("sense", mc.SENSE if mode == "evade" else 0.0), **kw)


def move(case, motion, n, m, env_offset=0):
    return mo.move_targets_torch(case["tgt"], case["agent"], case["hdr"], motion, mc.Team(n, m), env_offset)


# ---- 1. the boundary ----------------------------------------------------------------------------------------------------------

def test_header_library_binding_and_op_layer_agree():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+cs_move_targets\s*\(\s*const\s+cs_config\s*\*\w*\s*,\s*void\s*\*\w*\s*,\s*const\s+cs_motion_params\s*\*", header)
    assert re.search(r"#define\s+CS_ABI_VERSION\s+7\b", header)
    assert "cs_move_targets" in _lib.EXPORTS
    L = _lib.load()
    assert hasattr(L, "cs_move_targets") and L.cs_move_targets.argtypes is not None
    fields = re.search(r"typedef struct cs_motion_params \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"\b(?:u?int32_t|int64_t|double)\s+(\w+);", fields) == [k for k, _ in _lib.CsMotionParams._fields_]
    assert C.sizeof(_lib.CsMotionParams) == 40
    schema = str(_lib.torch_ops().move_targets.default._schema)
    assert schema == ("coopsearch::move_targets(Tensor cfg, Tensor(a!) blob, int mode, int persist, int seed, float speed, "
                      "float sense, int env_offset) -> ()")
    from cooperative_search_amd import build
    assert "motion.h" in build.SOURCES
    assert not hasattr(_lib.CtypesOps, "move_targets")
    for name in ("TargetMotion", "MovingTargetEnv", "move_targets_torch", "make_env"):
        assert getattr(cs, name) is getattr(mo, name)
    assert issubclass(mo.MovingTargetEnv, cs.BatchedFlightEnv)


def test_the_kernel_header_holds_the_definitions_heading_tables():
    src = open(os.path.join(ROOT, "cooperative-search_amd", "csrc", "motion.h")).read()
    for name, want in (("MOT_CX", mo.CX), ("MOT_CY", mo.CY)):
        body = re.search(name + r"\[MOT_HEADINGS\]\s*=\s*\{(.*?)\}", src, flags=re.S).group(1)
        got = [float.fromhex(v.strip()) for v in body.split(",")]
        assert [v.hex() for v in got] == [v.hex() for v in want], name
    assert list(mo.CX) == [math.cos(2 * math.pi * k / 16) for k in range(16)]
    assert list(mo.CY) == [math.sin(2 * math.pi * k / 16) for k in range(16)]
    assert int(re.search(r"MOT_HEADINGS\s*=\s*(\d+)", src).group(1)) == mo.HEADINGS == 16


# ---- 2. the definition --------------------------------------------------------------------------------------------------------

def test_the_walk_key_restated_in_plain_python_integers():
    """walk_headings against the issue's pseudo-code on Python ints, high key word included."""
    def fmix(x):
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)

    case = mc.make_case(5, 3, 15, "walk", 0.5)
    for off, persist, seed in ((0, 1, 0), ((1 << 32) + 7, 4, 0xDEADBEEF)):
        got = mo.walk_headings(case["hdr"], spec(persist=persist, seed=seed), off)
        for b in range(5):
            for j in range(16):
                h, g = seed, off + b
                for w in (g & 0xFFFFFFFF, g >> 32, int(case["hdr"][b, _lib.H_EPISODES]), int(case["hdr"][b, _lib.H_TIME_STEP]) // persist, j):
                    h = (fmix(h ^ w) + 0x9E3779B9) & 0xFFFFFFFF
                assert int(got[b, j]) == h >> 28, (off, b, j)


def test_all_headings_occur_and_evenly():
    hdr = torch.zeros(257, 16, dtype=torch.int32)
    k = mo.walk_headings(hdr, spec())[:, :15]
    counts = torch.bincount(k.reshape(-1), minlength=16)
    assert int(counts.sum()) == 3855 and int(counts.min()) >= 180 and int(counts.max()) <= 300, counts.tolist()


@pytest.mark.parametrize("B,n,m,mode,speed", CASES)
def test_what_does_not_move_keeps_its_bits_and_what_moves_stays_on_the_map(B, n, m, mode, speed):
    case = mc.make_case(B, n, m, mode, speed)
    before = {k: v.clone() for k, v in case.items()}
    out = move(case, spec(mode, speed), n, m)
    assert all(torch.equal(bits(case[k]) if k != "hdr" else case[k], bits(before[k]) if k != "hdr" else before[k]) for k in case)
    assert torch.equal(bits(out), bits(move(case, spec(mode, speed), n, m)))                     # two calls are equal
    hdr = case["hdr"].to(torch.int64)
    j = torch.arange(16).view(1, 16)
    found = ((hdr[:, _lib.H_FOUND].view(B, 1) >> j) & 1) == 1
    won, late = (hdr[:, _lib.H_FLAGS] & 1) == 1, hdr[:, _lib.H_TIME_STEP] >= mc.LIMIT
    still = found | (j >= m) | won.view(B, 1) | late.view(B, 1)
    same = (bits(out) == bits(case["tgt"])).all(2)
    assert bool(same[still].all())
    assert bool((won & ~late).any()) == bool((late & ~won).any()) == (B >= 5)                     # each kind alone
    moved = out[~still]
    assert moved.numel() and bool(((moved >= 0.0) & (moved <= mc.MAP)).all())
    assert not bool(same[~still].all())


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_split_in_two_equals_the_whole(mode):
    B, n, m = 64, 8, 15
    case = mc.make_case(B, n, m, mode, 0.5)
    motion = spec(mode, 0.5, persist=4, seed=77)
    for off in (0, (1 << 32) - 20):     # the second: the low key word wraps inside the batch
        whole = move(case, motion, n, m, off)
        lo, hi = ({k: v[:23] for k, v in case.items()}, {k: v[23:] for k, v in case.items()})
        parts = torch.cat((move(lo, motion, n, m, off), move(hi, motion, n, m, off + 23)))
        assert torch.equal(bits(whole), bits(parts))
        assert not torch.equal(bits(whole[23:]), bits(move(hi, motion, n, m, off)))


def test_persist_holds_a_heading_over_its_time_steps():
    hdr = torch.zeros(64, 16, dtype=torch.int32)
    heads = {}
    for persist in (1, 4):
        rows = []
        for ts in range(16):
            hdr[:, _lib.H_TIME_STEP] = ts
            rows.append(mo.walk_headings(hdr, spec(persist=persist, seed=5), 9))
        heads[persist] = torch.stack(rows)                    # [16 time steps, 64, 16]
    four = heads[4].view(4, 4, 64, 16)
    assert bool((four == four[:, :1]).all())                  # 4q .. 4q + 3 share a heading
    assert not torch.equal(four[0, 0], four[1, 0]) and not torch.equal(four[1, 0], four[2, 0])
    one = heads[1].view(4, 4, 64, 16)
    assert not bool((one == one[:, :1]).all())
    assert torch.equal(heads[1][0], heads[4][0])              # time step 0 gives word 0 either way


def test_evade_without_a_radius_is_the_walk():
    B, n, m = 64, 8, 15
    case = mc.make_case(B, n, m, "walk", 0.5)
    case["tgt"][0, 1, 0] += 0.25                    # the planted target under agent 0 steps aside: d2 = 0 <= 0 would evade
    d2 = ((case["tgt"][:, :, None, :] - case["agent"][:, None, :, :2]) ** 2).sum(3)
    assert float(d2.min()) > 0.0
    assert torch.equal(bits(move(case, spec("evade", 0.5, sense=0.0), n, m)), bits(move(case, spec("walk", 0.5), n, m)))
    assert not torch.equal(bits(move(case, spec("evade", 0.5, sense=10.0), n, m)), bits(move(case, spec("walk", 0.5), n, m)))


@pytest.mark.parametrize("B,n,m", mc.SHAPES)
def test_a_target_that_sees_every_agent_does_not_come_nearer_to_the_nearest(B, n, m):
    """sense beyond the map: with (dx, dy) to the nearest agent and the best of 16 headings, dx CX + dy CY >= |d| cos(pi / 16) > 0,
    so the squared distance to THAT agent grows by at least speed^2 > 0 -- far above rounding at these magnitudes -- unless a
    clamp bound the move (an output coordinate on a wall) or the target stands under the agent (heading 0: it grows too)."""
    case = mc.make_case(B, n, m, "evade", 0.5)
    out = move(case, spec("evade", 0.5, sense=2.0 * mc.MAP), n, m)
    ag = case["agent"][:, None, :n, :2]
    d_before = ((case["tgt"][:, :, None, :] - ag) ** 2).sum(3)
    near = d_before.argmin(2, keepdim=True)
    d_after = ((out[:, :, None, :] - ag) ** 2).sum(3)
    moved = ~(bits(out) == bits(case["tgt"])).all(2)
    clamped = ((out == 0.0) | (out == mc.MAP)).any(2)
    free = moved & ~clamped
    assert bool(free.any()) or B < 5      # (the single target of the smallest shape stands at a wall)
    assert bool((d_after.gather(2, near)[free] >= d_before.gather(2, near)[free]).all())


@pytest.mark.parametrize("mode", MODES)
def test_speed_zero_returns_the_input(mode):
    case = mc.make_case(64, 8, 15, mode, 0.5)
    case["tgt"][0, 1, 0] = -0.0                     # x + 0 would lose the sign: nothing is added at speed 0
    out = move(case, spec(mode, 0.0), 8, 15)
    assert torch.equal(bits(out), bits(case["tgt"])) and out.data_ptr() != case["tgt"].data_ptr()


# ---- 3. the case generator ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,n,m,mode,speed", CASES)
def test_every_case_holds_what_the_gpu_test_relies_on(B, n, m, mode, speed):
    """The one-env, one-agent, one-target shape cannot hold a found target, a finished env or two agents: it holds one live,
    unfound target that a wall clamps or an agent drives (what a shape of that size can go wrong on).  Every other shape holds
    everything."""
    case = mc.make_case(B, n, m, mode, speed)
    got = mc.holds(case, move(case, spec(mode, speed), n, m), n, m, mode)
    if B >= 5:
        assert got >= (mc.WANTED_EVADE if mode == "evade" else mc.WANTED), (mc.WANTED_EVADE - got)
    else:
        hdr = case["hdr"]
        assert int(hdr[0, _lib.H_FOUND]) == 0 and not int(hdr[0, _lib.H_FLAGS]) & 1 and int(hdr[0, _lib.H_TIME_STEP]) < mc.LIMIT
        assert float(case["tgt"][0, 0, 0]) <= 0.2 * speed


# ---- 4. the run-splitting rule ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("phase,T,every,want", [
    (0, 1, 3, [(0, 1, True)]), (1, 1, 3, [(0, 1, False)]),                                  # T = 1
    (0, 2, 5, [(0, 2, True)]), (1, 2, 5, [(0, 2, False)]), (4, 2, 5, [(0, 1, False), (1, 2, True)]),   # T < every
    (0, 6, 3, [(0, 3, True), (3, 6, True)]), (0, 3, 3, [(0, 3, True)]),                     # T a multiple of every
    (7, 13, 3, [(0, 2, False), (2, 5, True), (5, 8, True), (8, 11, True), (11, 13, True)]),   # a phase in the middle of a period
    (5, 3, 1, [(0, 1, True), (1, 2, True), (2, 3, True)]),                                  # every = 1
    (0, 20, 3, [(0, 3, True), (3, 6, True), (6, 9, True), (9, 12, True), (12, 15, True), (15, 18, True), (18, 20, True)]),
    (3, 0, 2, [])])
def test_split_runs(phase, T, every, want):
    assert mo.split_runs(phase, T, every) == want


def test_split_runs_cover_every_step_once_and_move_exactly_where_due():
    for every in range(1, 8):
        for phase in range(0, 15):
            for T in range(0, 24):
                runs = mo.split_runs(phase, T, every)
                assert [t for a, b, _ in runs for t in range(a, b)] == list(range(T))
                assert all(b > a for a, b, _ in runs)
                for a, b, move_first in runs:
                    assert move_first == ((phase + a) % every == 0)
                    assert all((phase + t) % every != 0 for t in range(a + 1, b))      # no move inside a run
    with pytest.raises(ValueError):
        mo.split_runs(0, 4, 0)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(mode="drift"), dict(speed=-0.5), dict(speed=math.inf), dict(speed=math.nan), dict(every=0),
                                dict(every=1.5), dict(persist=0), dict(persist=65537), dict(sense=-1.0), dict(sense=math.nan),
                                dict(seed=-1), dict(seed=1 << 32)])
def test_target_motion_refuses_out_of_range_fields(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        mo.TargetMotion(**kw)


def test_target_motion_bounds_that_depend_on_the_map_and_from_args():
    ok = mo.TargetMotion(mode="evade", speed=50, every=2, persist=65536, sense=100, seed=(1 << 32) - 1)
    assert ok.check(50) is ok and isinstance(ok.speed, float)
    with pytest.raises(ValueError, match="speed"):
        mo.TargetMotion(speed=50.5).check(50)
    with pytest.raises(ValueError, match="sense"):
        mo.TargetMotion(sense=100.5).check(50)
    with pytest.raises(ValueError, match="speed"):
        mo.move_targets_torch(*mc.make_case(5, 3, 15, "walk", 0.5).values(), mo.TargetMotion(speed=51.0), mc.Team(3, 15))
    with pytest.raises(ValueError, match="env_offset"):
        mo.move_targets_torch(*mc.make_case(5, 3, 15, "walk", 0.5).values(), spec(), mc.Team(3, 15), -1)
    assert mo.TargetMotion.from_args(types.SimpleNamespace()) == mo.TargetMotion()
    args = types.SimpleNamespace(target_speed=0.25, target_motion="evade", target_move_every=5, target_persist=3, target_sense=9,
                                 target_motion_seed=12)
    assert mo.TargetMotion.from_args(args) == mo.TargetMotion("evade", 0.25, 5, 3, 9.0, 12)


def _cfg(**kw):
    from cooperative_search_amd.env import _cfg_from_args
    return _cfg_from_args(cs.make_env_args("flight_easy", n_agents=3), cs.default_circle_dict(), kw.get("batch", 64), 0)


@pytest.mark.parametrize("field, value, msg", [("mode", 2, "mode"), ("mode", -1, "mode"), ("persist", 0, "persist"),
                                               ("persist", 65537, "persist"), ("reserved", 1, "reserved"), ("speed", -0.25, "speed"),
                                               ("speed", 50.5, "speed"), ("speed", math.nan, "speed"), ("sense", -1.0, "sense"),
                                               ("sense", 100.5, "sense"), ("sense", math.inf, "sense"), ("env_offset", -1, "env_offset"),
                                               ("state", None, "NULL"), ("params", None, "NULL"), ("cfg", None, "n_agents"),
                                               ("align", None, "aligned")])
def test_entry_point_refuses_bad_arguments_before_any_launch(field, value, msg):
    """No device here: a call that got as far as a launch would fail another way.  The pointers are never dereferenced."""
    L = _lib.load()
    cfg = _cfg()
    p = _lib.CsMotionParams(0, 1, 7, 0, 0.5, 10.0, 0)
    state, pp = C.c_void_p(4096), C.byref(p)
    if field == "state":
        state = None
    elif field == "params":
        pp = None
    elif field == "cfg":
        cfg.n_agents = 9
    elif field == "align":
        state = C.c_void_p(4104)
    else:
        setattr(p, field, value)
    assert L.cs_move_targets(C.byref(cfg), state, pp, None) == -1   # CS_E_CONFIG
    assert msg in L.cs_episodes_last_error().decode() and "cs_move_targets" in L.cs_episodes_last_error().decode()
    assert msg in L.cs_last_error().decode()


def test_speed_zero_is_accepted_without_a_launch():
    L = _lib.load()
    cfg = _cfg()
    p = _lib.CsMotionParams(1, 4, 7, 0, 0.0, 10.0, 1 << 40)
    assert L.cs_move_targets(C.byref(cfg), C.c_void_p(4096), C.byref(p), None) == 0   # (a launch would fail without a device)


def test_op_refuses_bad_fields_and_a_cpu_blob():
    ops = _lib.torch_ops()
    cfg = _cfg()
    t = torch.frombuffer(bytearray(bytes(cfg)), dtype=torch.uint8)
    blob = torch.zeros(int(ops.state_bytes(t)), dtype=torch.uint8)
    for args, msg in (((2, 1, 0, 0.5, 0.0, 0), "mode"), ((0, 0, 0, 0.5, 0.0, 0), "persist"), ((0, 1, -1, 0.5, 0.0, 0), "seed"),
                      ((0, 1, 1 << 32, 0.5, 0.0, 0), "seed"), ((0, 1, 0, 51.0, 0.0, 0), "speed"), ((0, 1, 0, math.nan, 0.0, 0), "speed"),
                      ((0, 1, 0, 0.5, 101.0, 0), "sense"), ((0, 1, 0, 0.5, 0.0, -1), "env_offset"),
                      ((0, 1, 0, 0.5, 0.0, 0), "GPU")):   # a CPU tensor must be refused, not dereferenced
        with pytest.raises(RuntimeError, match=msg):
            ops.move_targets(t, blob, *args)


def test_make_env_and_the_env_class_without_a_device():
    """No GPU here: construction raises the parent's error -- after the spec has been checked."""
    args = cs.make_env_args("flight_easy")
    args.target_speed = 60.0
    with pytest.raises(ValueError, match="speed"):
        mo.make_env(args, batch=4)
    with pytest.raises(TypeError, match="TargetMotion"):
        mo.MovingTargetEnv(args, batch=4, target_motion=dict(speed=1))
    if not torch.cuda.is_available():
        args.target_speed = 0.5
        with pytest.raises(RuntimeError, match="GPU"):
            mo.make_env(args, batch=4)
    for name in ("step", "rollout", "rollout_policy", "collect_flight", "reset"):
        assert name in vars(mo.MovingTargetEnv)
    src = open(os.path.join(ROOT, "cooperative-search_amd", "motion.py")).read()
    assert "_lib.torch_ops()" in src and "data_ptr()" not in src
