"""CPU tests of the frame definition (cooperative-search_amd/render.py), of cs_render_episodes' boundary and of
Runner.replay / Runner.collect_experiment_data's host logic.  Everything here is exact: the definition is integer arithmetic
after one quantisation, so no test carries a tolerance."""
import ctypes as C
import dataclasses
import json
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import render as rd
from cooperative_search_amd import runner as rn
from cooperative_search_amd.replay import KEYS, compact_from_dense
import render_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "runner_schedule.json")))
T = FIXTURE["episode_limit"]
SAVE_FILES = {"qmix": ("qmix", "rnn"), "dop": ("actor", "mixer", "critic"), "reinforce": ("rnn",)}


def quantised(states, n, W):
    """The definition's quantisation, restated in numpy float32: (ax, ay, tx, ty) int64 [K, n] / [K, m]."""
    s = states.numpy()
    U = 16 * W

    def q(v):
        return np.rint((v + np.float32(1)) * np.float32(8 * W)).astype(np.int64)
    return q(s[:, 0:4 * n:4]), U - q(s[:, 1:4 * n:4]), q(s[:, 4 * n::3]), U - q(s[:, 4 * n + 1::3])


# ---- 1. pins of the definition on the reference's recorded traces ----------------------------------------------------------

@pytest.mark.parametrize("name, n", [("easy_n3_am0_s0_a1", 3), ("flight_n3_am0_s0_a1", 3), ("easy_n5_am3_s9_a5", 5)])
def test_recorded_agents_targets_and_bar_are_where_the_frames_show_them(name, n):
    """Measured when the definition was written: 5 of 765, 6 of 765 and 7 of 255 (frame, target) pairs left out, no agent
    or target pin missed."""
    W, m = 128, 15
    U = 16 * W
    st = rc.golden_states(name)
    found, target_find = rc.golden_found(name)
    K = len(st)
    spec = rd.RenderSpec(size=W, n_agents=n)
    L = spec.radii()[3]
    fr = rd.render_episodes_torch(st[None], None, torch.tensor([K]), spec)[0].numpy()
    ax, ay, tx, ty = quantised(st, n, W)
    pinned = 0
    for t in range(K):
        for i in range(n):
            c, r = ax[t, i] // 16, ay[t, i] // 16
            if 0 <= c < W and 4 <= r < W:
                pinned += 1
                assert tuple(fr[t, r, c]) == spec.palette[i], (t, i)
    assert pinned >= K   # (many recorded agents are outside the map: SURVEY section 6.2)
    left_out = 0
    for t in range(K):
        for j in range(m):
            c, r = tx[t, j] // 16, ty[t, j] // 16
            near = ((ax[t] - tx[t, j]) ** 2 + (ay[t] - ty[t, j]) ** 2 <= (L + 32) ** 2).any()
            if not (0 <= c < W and 4 <= r < W) or near:
                left_out += 1
                continue
            assert tuple(fr[t, r, c]) == (spec.target_found if found[t, j] else spec.target), (t, j)
    print(f"{name}: {left_out} of {K * m} (frame, target) pairs left out, {pinned} agent pins")
    assert left_out <= 0.10 * K * m
    for t in range(K):
        green = math.ceil(int(target_find[t]) * W / m)
        for r in range(4):
            assert (fr[t, r, :green] == np.array(spec.bar_on, dtype=np.uint8)).all(), t
            assert (fr[t, r, green:] == np.array(spec.bar_off, dtype=np.uint8)).all(), t


# ---- 2. frames at or after `counts` repeat the last real one ----------------------------------------------------------------

def test_frames_past_the_count_repeat_and_counts_clamp():
    R, W = 8, 32
    g = rc.golden_states("easy_n3_am0_s0_a1")[:R]
    counts = torch.tensor([5, 0, 100, R, 1])
    states = g[None].repeat(len(counts), 1, 1).contiguous()
    spec = rd.RenderSpec(size=W, n_agents=3)
    fr = rd.render_episodes_torch(states, None, counts, spec)
    for e, c in enumerate([5, 1, R, R, 1]):   # 0 clamps to 1, 100 to R
        for t in range(c, R):
            assert torch.equal(fr[e, t], fr[e, c - 1]), (e, t)
        assert torch.equal(fr[e, :c], fr[3, :c])   # the real frames are those of the whole episode
    assert not torch.equal(fr[3, R - 1], fr[3, 0])
    # rows past the count are never read: NaN there changes nothing
    poisoned = states.clone()
    for e, c in enumerate([5, 1, R, R, 1]):
        poisoned[e, c:] = float("nan")
    assert torch.equal(rd.render_episodes_torch(poisoned, None, counts.to(torch.int32), spec), fr)
    assert rd.frame_rows(counts, R).tolist()[0] == [0, 1, 2, 3, 4, 4, 4, 4]


# ---- 3. the heat layer alone -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [100, 36])
def test_heat_layer_alone_is_the_lookup_of_the_recorded_maps(W):
    side, U = rc.SIDE, 16 * W
    maps = rc.golden_maps()
    R = len(maps)
    states = rc.golden_states("flight_n3_am0_s0_a1")[:R]
    spec = rd.RenderSpec(size=W, n_agents=3, sensor=False, trail=False, targets=False, agents=False, bar=False)
    fr = rd.render_episodes_torch(states[None], maps[None], torch.tensor([R]), spec)[0].numpy()
    lut = np.frombuffer(spec.lut, dtype=np.uint8).reshape(256, 3)
    P = 16 * np.arange(W) + 8
    ix = np.clip((P * side) // U, 0, side - 1)            # by column
    iy = np.clip(((U - P) * side) // U, 0, side - 1)      # by row
    p = maps.numpy().reshape(R, side, side)[:, ix[None, :], iy[:, None]]   # [R, row, column] = map[ix(column), iy(row)]
    want = lut[np.rint(np.clip(p, 0, 1) * np.float32(255)).astype(np.int64)]
    assert np.array_equal(fr, want)
    assert len(np.unique(fr.reshape(-1, 3), axis=0)) > 3   # the recorded maps are not flat
    # without maps, or with the layer off, the background is the spec's
    off = rd.render_episodes_torch(states[None], maps[None], torch.tensor([R]), dataclasses.replace(spec, heat=False))
    assert torch.equal(off, rd.render_episodes_torch(states[None], None, torch.tensor([R]), spec))
    assert (off.numpy() == 255).all()


def test_special_map_values_follow_the_rounding_rule():
    sv = rc.special_map_values()
    lut = np.frombuffer(rd.DEFAULT_LUT, dtype=np.uint8).reshape(256, 3)
    side, W = 8, 32   # 4 x 4 pixels per cell
    sv = sv[np.arange(side * side) % len(sv)]
    cells = torch.from_numpy(sv.copy()).reshape(1, 1, side * side)
    spec = rd.RenderSpec(size=W, n_agents=1, sensor=False, trail=False, targets=False, agents=False, bar=False)
    fr = rd.render_episodes_torch(torch.zeros(1, 1, 7), cells, torch.tensor([1]), spec)[0, 0].numpy()
    for k, p in enumerate(sv):
        i, j = divmod(k, side)
        pc = np.float32(0) if not p > 0 else min(p, np.float32(1))
        want = lut[int(np.rint(pc * np.float32(255)))]
        block = fr[W - 4 * (j + 1):W - 4 * j, 4 * i:4 * (i + 1)]   # cell (ix = i, iy = j): columns 4i.., rows from the bottom
        assert (block == want).all(), (k, p)


# ---- 4. episode_tables ------------------------------------------------------------------------------------------------------

def test_episode_tables_agree_for_dense_and_compact_batches():
    z = np.load(os.path.join(HERE, "golden", "episode_flight_n3_am3_s3_a2.npz"))
    dense = {k: torch.from_numpy(z[k].astype(np.float32)) for k in KEYS}
    args = cs.make_env_args("flight", n_agents=3)
    s1, m1, c1 = rd.episode_tables(dense, args)
    s2, m2, c2 = rd.episode_tables(compact_from_dense(dense), args)
    assert torch.equal(s1, s2) and torch.equal(m1, m2) and torch.equal(c1, c2)
    steps = int(json.loads(str(z["meta"]))["steps"])
    assert s1.shape == (1, 201, 57) and m1.shape == (1, 201, 2500) and c1.dtype == torch.int32 and c1.tolist() == [steps + 1]
    assert torch.equal(s1[0, 0], dense["s"][0, 0]) and torch.equal(s1[0, 1:], dense["s_next"][0])
    assert torch.equal(m1[0, 0], dense["o"][0, 0, 0, :2500]) and torch.equal(m1[0, 5], dense["o_next"][0, 4, 1, :2500])
    # a flight_easy batch has no map; padded steps shorten the count
    easy = {k: v.clone() for k, v in dense.items()}
    easy["o"], easy["o_next"] = dense["o"][..., 2500:], dense["o_next"][..., 2500:]
    easy["padded"][0, 150:] = 1.0
    s3, m3, c3 = rd.episode_tables(easy, cs.make_env_args("flight_easy", n_agents=3))
    assert m3 is None and c3.tolist() == [151] and torch.equal(s3, s1)
    fr = rd.render_episodes(s3[:, ::25].contiguous(), None, torch.tensor([7]), rd.RenderSpec(size=16, n_agents=3))
    assert fr.shape == (1, 9, 16, 16, 3) and fr.dtype == torch.uint8 and torch.equal(fr[0, 8], fr[0, 6])


# ---- 5. the op, the C ABI's refusals, write_frames --------------------------------------------------------------------------

def test_render_is_declared_exported_and_registered():
    L = _lib.load()
    assert "cs_render_episodes" in _lib.EXPORTS and hasattr(L, "cs_render_episodes")
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "coopsearch.h")).read()
    assert "int cs_render_episodes(" in hdr and "typedef struct cs_render_params" in hdr
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    assert hasattr(_lib.torch_ops(), "render_episodes")
    for name, bit in (("HEAT", 1), ("SENSOR", 2), ("TRAIL", 4), ("TARGETS", 8), ("AGENTS", 16), ("BAR", 32)):
        assert f"CS_RENDER_{name} = {bit}" in hdr and getattr(rd, name) == bit
    from cooperative_search_amd import build
    assert "render.h" in build.SOURCES


def op_args(n=3, m=15, W=32, E=2, R=3, side=None, **over):
    spec = rd.RenderSpec(size=32, n_agents=3)
    a = dict(states=torch.zeros(E, R, 4 * n + 3 * m), maps=None if side is None else torch.zeros(E, R, side * side),
             counts=torch.ones(E, dtype=torch.int32), n=n, m=m, side=side or 0, W=W, radii=list(spec.radii()), layers=spec.layers(),
             colours=spec.colours(), palette=torch.zeros(8, 3, dtype=torch.uint8), lut=torch.zeros(256, 3, dtype=torch.uint8),
             frames=torch.zeros(E, R, W, W, 3, dtype=torch.uint8))
    a.update(over)
    return a


def call_op(a):
    _lib.torch_ops().render_episodes(a["states"], a["maps"], a["counts"], a["n"], a["m"], a["side"], a["W"], a["radii"], a["layers"],
                                     a["colours"], a["palette"], a["lut"], a["frames"])


def test_the_op_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU"):
        call_op(op_args())
    with pytest.raises(RuntimeError, match="GPU"):
        call_op(op_args(side=50))


@pytest.mark.parametrize("over, message", [
    (dict(n=0), "n_agents"), (dict(n=9), "n_agents"), (dict(m=0), "n_targets"), (dict(m=17), "n_targets"),
    (dict(W=18), "size"), (dict(W=12), "size"), (dict(W=1028), "size"), (dict(R=0), "R must"),
    (dict(side=50, maps=torch.zeros(2, 3, 2499)), "maps"), (dict(side=65), "maps"), (dict(states=torch.zeros(2, 3, 56)), "states"),
    (dict(radii=[40000, 16, 8, 15]), "radii"), (dict(colours=[0] * 20), "colours")])
def test_the_op_refuses_what_the_host_can_check_before_any_tensor_is_looked_at(over, message):
    with pytest.raises(RuntimeError, match=message):
        call_op(op_args(**over))


def abi_call(E=2, R=3, null=None, aligned=True, with_maps=False, **fields):
    """cs_render_episodes with pointers that must never be dereferenced (there is no device here)."""
    L = _lib.load()
    spec = rd.RenderSpec(size=32, n_agents=3)
    p = _lib.CsRenderParams()
    p.n_agents, p.n_targets, p.state_width, p.size, p.side, p.map_width = 3, 15, 57, 32, 50, 2500
    p.rv, p.rt, p.rtr, p.tri_len = spec.radii()
    p.layers = spec.layers()
    p.palette_dev, p.lut_dev = 4096 * 5, 4096 * 6
    for k, v in fields.items():
        setattr(p, k, v)
    ptrs = {"states": 4096, "maps": 8192 if with_maps else None, "counts": 12288, "frames": 16384 if aligned else 16386}
    if null in ptrs:
        ptrs[null] = None
    pp = None if null == "params" else C.byref(p)
    rc_ = L.cs_render_episodes(pp, ptrs["states"], ptrs["maps"], ptrs["counts"], E, R, ptrs["frames"], None)
    return rc_, L.cs_episodes_last_error().decode()


@pytest.mark.parametrize("kw", [
    dict(n_agents=0), dict(n_agents=9), dict(n_targets=0), dict(n_targets=17), dict(state_width=56), dict(size=18), dict(size=12),
    dict(size=1028), dict(R=0), dict(E=0), dict(null="params"), dict(null="states"), dict(null="counts"), dict(null="frames"),
    dict(palette_dev=None), dict(lut_dev=None), dict(with_maps=True, map_width=2499), dict(with_maps=True, side=0, map_width=0),
    dict(with_maps=True, side=65, map_width=65 * 65), dict(rv=32768), dict(rt=-1), dict(rtr=40000), dict(tri_len=16384),
    dict(aligned=False)])
def test_the_abi_refuses_with_config_errors_before_any_launch(kw):
    code, msg = abi_call(**kw)
    assert code == -1 and msg.startswith("cs_render_episodes: ")   # CS_E_CONFIG


def test_render_episodes_refuses_tables_that_do_not_fit_the_spec():
    spec = rd.RenderSpec(size=16, n_agents=3)
    with pytest.raises(ValueError, match="state row"):
        rd.render_episodes(torch.zeros(1, 1, 56), None, torch.ones(1, dtype=torch.int32), spec)
    with pytest.raises(ValueError, match="maps"):
        rd.render_episodes(torch.zeros(1, 1, 57), torch.zeros(1, 1, 2499), torch.ones(1, dtype=torch.int32), spec)
    with pytest.raises(ValueError, match="counts"):
        rd.render_episodes(torch.zeros(1, 1, 57), None, torch.ones(2, dtype=torch.int32), spec)
    for bad in (18, 12, 1028):
        with pytest.raises(ValueError, match="size"):
            rd.RenderSpec(size=bad)
    assert rd.RenderSpec(size=128).radii() == (287, 25, 12, 61)   # round(7 / 50 * 2048), max(16, round(24.576)), ...


def test_write_frames_with_and_without_pil(tmp_path, monkeypatch):
    st = rc.golden_states("easy_n3_am0_s0_a1")[:6]
    fr = rd.render_episodes_torch(st[None].repeat(2, 1, 1), None, torch.tensor([6, 3]), rd.RenderSpec(size=16, n_agents=3))
    from PIL import Image
    gif = rd.write_frames(fr, str(tmp_path / "a.gif"))
    assert gif == str(tmp_path / "a.gif") and os.path.getsize(gif) > 0
    with Image.open(gif) as im:
        assert im.n_frames == 6 and im.size == (32, 16)   # two episodes side by side
    png = rd.write_frames(fr[0], str(tmp_path / "sheet"))
    assert png == str(tmp_path / "sheet.png")
    with Image.open(png) as im:
        assert im.size == (48, 32)                        # 6 pictures on a 3 x 2 sheet
        assert np.array_equal(np.asarray(im.convert("RGB"))[:16, 16:32], fr[0, 1].numpy())
    monkeypatch.setitem(sys.modules, "PIL", None)   # `from PIL import Image` now raises ImportError
    npy = rd.write_frames(fr, str(tmp_path / "b.gif"))
    assert npy == str(tmp_path / "b.gif") + ".npy" and not os.path.exists(str(tmp_path / "b.gif"))
    assert np.array_equal(np.load(npy), fr.numpy())


# ---- 6. Runner.replay / Runner.collect_experiment_data on the CPU -----------------------------------------------------------
# (the stand-ins of tests/test_runner_cpu.py, with a collector that also answers the greedy calls)

class Recorder:
    def __init__(self, args, batch=2):
        self.trace, self.args, self.batch = [], args, batch
        self.env = types.SimpleNamespace(batch=batch, device=torch.device("cpu"))
        self.loaded = []
        rec = self
        rows = rc.golden_states("easy_n3_am0_s0_a1", stride=1)[:T + 1]

        class Buffer:
            current_size = 0

        class Collector:
            def generate_episodes(self, agents=None, evaluate=True, episode_num=None, into=None, init=False, **kw):
                assert agents is rec.agents and evaluate and init and into is None
                rec.trace.append(["generate_episode", "greedy"])
                ep = rec.episode(rec.batch)
                ep["s"], ep["s_next"] = rows[None, :T].repeat(rec.batch, 1, 1), rows[None, 1:].repeat(rec.batch, 1, 1)
                ep["o"] = ep["o_next"] = torch.zeros(rec.batch, T, 3, 4)
                ep["padded"][1, T - 1] = 1.0   # the second episode ended a step early
                return ep, torch.tensor([-7, -9][:rec.batch]), torch.zeros(rec.batch, dtype=torch.bool), torch.tensor([2, 1][:rec.batch])

            def collect_experiment_data(self, policy, batches=1, num=None, result_path=None, return_stats=False):
                rec.trace.append(["collect", int(batches)])
                res = np.linspace(0.0, 50.0, T)
                np.save(os.path.join(result_path, "average_res_{}".format(num)), res)
                return res, {"targets_find": 2.0, "episode_reward": -7.0, "steps": float(T), "episodes": batches * rec.batch}

        class Learner:
            def load_model(self, *files):
                rec.loaded.append([os.path.basename(f) for f in files])

        class Agents:
            syncs = 0

            def sync_weights(self):
                self.syncs += 1

            def check_weights(self):
                pass

            def policy(self, epsilon=0.0, evaluate=True):
                assert epsilon == 0.0 and evaluate
                return None

        self.buffer, self.collector, self.learner, self.agents = Buffer(), Collector(), Learner(), Agents()
        self.model_dir = args.model_dir + rn.run_name(args)
        self.schedule = types.SimpleNamespace(values=torch.full((batch,), 0.5, dtype=torch.float64))

    def episode(self, k):
        return {key: torch.zeros(k, T, 1) for key in KEYS}

    def runner(self):
        return rn.Runner(self.env, self.args, learner=self.learner, agents=self.agents, schedule=self.schedule,
                         collector=self.collector, buffer=self.buffer)

    def checkpoint(self, num):
        for part in SAVE_FILES[self.args.alg]:
            open(os.path.join(self.model_dir, f"{num}_{part}_net_params.pkl"), "w").close()


def make_args(cfg, root, **over):
    a = cs.make_env_args("flight_easy", n_agents=3)
    a.n_actions, a.state_shape, a.obs_shape, a.episode_limit = 3, 57, 4, T
    a.alg, a.seed = cfg["alg"], 1234
    {"qmix": cs.get_mixer_args, "dop": cs.get_dop_args, "reinforce": cs.get_reinforce_args}[cfg["alg"]](a)
    for k, v in cfg["fields"].items():
        setattr(a, k, v)
    a.model_dir, a.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("cfg", FIXTURE["configs"], ids=[c["name"] for c in FIXTURE["configs"]])
def test_replay_and_collect_raise_the_reference_error_for_a_missing_checkpoint(cfg, tmp_path):
    rec = Recorder(make_args(cfg, str(tmp_path)))
    r = rec.runner()
    with pytest.raises(FileNotFoundError, match="3_"):   # torch.load's, runner.py:121-131
        r.replay(3)
    with pytest.raises(FileNotFoundError, match="3_"):
        r.collect_experiment_data(3, 10)
    assert rec.trace == [] and rec.loaded == [] and rec.agents.syncs == 0 and os.listdir(r.result_path) == []


@pytest.mark.parametrize("cfg", FIXTURE["configs"], ids=[c["name"] for c in FIXTURE["configs"]])
def test_replay_and_collect_load_the_checkpoint_and_write_their_files(cfg, tmp_path, capsys):
    rec = Recorder(make_args(cfg, str(tmp_path)))
    r = rec.runner()
    rec.checkpoint(3)
    frames, targets_find, episode_reward, steps = r.replay(3, size=32)
    want = [[f"3_{part}_net_params.pkl" for part in rn._RESUME[cfg["alg"]]]]
    assert rec.loaded == want and rec.agents.syncs == 1 and rec.trace == [["generate_episode", "greedy"]]
    assert frames.shape == (2, T + 1, 32, 32, 3) and frames.dtype == torch.uint8
    assert targets_find.tolist() == [2, 1] and episode_reward.tolist() == [-7, -9] and steps.tolist() == [T, T - 1]
    assert torch.equal(frames[1, T], frames[1, T - 1]) and torch.equal(frames[0, :T], frames[1, :T])
    assert os.path.getsize(os.path.join(r.result_path, "replay_3.gif")) > 0
    assert "targets_find:  2  reward:  -7" in capsys.readouterr().out   # runner.py:137
    one, *_ = r.replay(3, episodes=1, size=16, path=str(tmp_path / "one.gif"))
    assert one.shape == (1, T + 1, 16, 16, 3) and os.path.exists(str(tmp_path / "one.gif"))
    res, stats = r.collect_experiment_data(3, 5)
    assert rec.trace[-1] == ["collect", 3] and rec.loaded == want * 3   # ceil(5 / 2) batches
    assert np.array_equal(np.load(os.path.join(r.result_path, "average_res_3.npy")), res) and stats["episodes"] == 6
