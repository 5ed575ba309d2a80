"""GPU tests of the frame kernel (cs_render_episodes, csrc/render.h): it equals the definition (render.render_episodes_torch)
byte for byte, and env.render_frames / Runner.replay sit on it.  Everything is torch.equal on uint8: no tolerance."""
import math
import os

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import render as rd
from cooperative_search_amd import runner as rn
import render_cases as rc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(t):
    return None if t is None else t.cuda().contiguous()


def kernel_frames(states, maps, counts, spec):
    """The kernel's frames into a buffer pre-filled with 0xAB: every byte must be written."""
    E, R = states.shape[:2]
    out = torch.full((E, R, spec.size, spec.size, 3), 0xAB, dtype=torch.uint8, device="cuda")
    got = rd.render_episodes(dev(states), dev(maps), dev(counts), spec, out=out)
    assert got is out
    return out.cpu()


# ---- 1. the kernel equals the definition ------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 7])
@pytest.mark.parametrize("W", [16, 36, 64])
@pytest.mark.parametrize("n, m", [(1, 1), (3, 15), (5, 15), (8, 16)])
def test_kernel_equals_the_definition_on_small_shapes(n, m, W, R):
    """E = 3 with counts (1, 4, R), with and without maps, all layers and every layer switched off in turn; recorded rows and
    rows on the definition's edges (render_cases.case_tables).  W = 16 leaves three quarters of a workgroup idle, W = 36 ends
    inside the second workgroup, W = 64 fills four."""
    for with_maps in (False, True):
        states, maps, counts = rc.case_tables(n, m, R, with_maps)
        for name, spec in rc.layer_specs(rd.RenderSpec(size=W, n_agents=n)):
            want = rd.render_episodes_torch(states, maps, counts, spec)
            got = kernel_frames(states, maps, counts, spec)
            if not torch.equal(got, want):
                bad = (got != want).any(-1).nonzero()
                e, t, r, c = bad[0].tolist()
                pytest.fail(f"maps {with_maps}, layers {name}: {len(bad)} pixels differ, first at episode {e} frame {t} row {r} column {c}: "
                            f"kernel {got[e, t, r, c].tolist()}, definition {want[e, t, r, c].tolist()}")


def test_kernel_equals_the_definition_on_every_reference_heading():
    states, maps, counts = rc.heading_tables()
    spec = rd.RenderSpec(size=64, n_agents=3)
    assert torch.equal(kernel_frames(states, maps, counts, spec), rd.render_episodes_torch(states, maps, counts, spec))


def test_int64_counts_and_a_fresh_output_are_accepted():
    states, maps, counts = rc.case_tables(3, 15, 7, True)
    spec = rd.RenderSpec(size=36, n_agents=3)
    got = rd.render_episodes(dev(states), dev(maps), counts.to(torch.int64).cuda(), spec)
    assert got.is_cuda and torch.equal(got.cpu(), rd.render_episodes_torch(states, maps, counts, spec))


# ---- 2. one full-length case ------------------------------------------------------------------------------------------------

def full_length_tables():
    R = 201
    g = rc.golden_states("flight_n3_am0_s0_a1", stride=1)[:R]
    states = torch.stack([g, rc.composed_rows(3, 15, R)], 0).contiguous()
    gm = rc.golden_maps()
    maps = torch.stack([gm[torch.arange(R) // 21], gm[(torch.arange(R) // 13) % len(gm)]], 0).contiguous()
    return states, maps, torch.tensor([R, 120], dtype=torch.int32)


def test_full_length_flight_episodes_equal_the_definition_on_the_same_device():
    states, maps, counts = (dev(t) for t in full_length_tables())
    spec = rd.RenderSpec(size=256, n_agents=3)
    out = torch.full((2, 201, 256, 256, 3), 0xAB, dtype=torch.uint8, device="cuda")
    rd.render_episodes(states, maps, counts, spec, out=out)
    want = rd.render_episodes_torch(states, maps, counts, spec)
    assert want.is_cuda and torch.equal(out, want)
    assert torch.equal(out[1, 119], out[1, 200]) and not torch.equal(out[1, 118], out[1, 119])


def test_output_offsets_past_two_gib():
    """E = 4 episodes of 180 frames at W = 1024 are 2.26e9 bytes: the last episode's frames, written past 2^31, equal the
    same episode drawn alone."""
    R, W = 180, 1024
    g = rc.golden_states("easy_n3_am0_s0_a1", stride=1)[:R]
    states = dev(torch.stack([g, g.flip(0), g, g.flip(0)], 0))
    counts = torch.tensor([R, R, 7, 50], dtype=torch.int32).cuda()
    spec = rd.RenderSpec(size=W, n_agents=3)
    frames = rd.render_episodes(states, None, counts, spec)
    assert frames.numel() > 2 ** 31
    alone = rd.render_episodes(states[3:].contiguous(), None, counts[3:].contiguous(), spec)
    assert torch.equal(frames[3], alone[0])
    small = rd.render_episodes_torch(states[3:, :3].contiguous(), None, counts[3:], spec)
    assert torch.equal(frames[3, :3], small[0])


# ---- 3. two calls give equal bytes, and a call never synchronises ------------------------------------------------------------

def test_two_calls_give_equal_bytes_without_synchronising():
    states, maps, counts = (dev(t) for t in rc.case_tables(5, 15, 7, True))
    spec = rd.RenderSpec(size=64, n_agents=5)
    rd.render_episodes(states, maps, counts, spec)   # the spec's palette and lookup table reach the device here, once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = rd.render_episodes(states, maps, counts, spec)
        b = rd.render_episodes(states, maps, counts.to(torch.int64), spec)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(a, b)


# ---- 4. env.render_frames ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant, B", [("flight_easy", 8), ("flight", 4)])
def test_env_render_frames_draws_the_current_state(variant, B):
    args = cs.make_env_args(variant, n_agents=3)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 31)
    g = torch.Generator().manual_seed(3)
    for _ in range(6):
        env.step(torch.randint(0, 3, (B, 3), generator=g, dtype=torch.int32))
    states = env.get_state().cpu().reshape(B, 1, -1)
    maps = env.get_obs()[:, 0, :env.cells].cpu().reshape(B, 1, -1).contiguous() if env.flight else None
    spec = rd.RenderSpec(size=64, view_range=args.view_range, map_size=args.map_size, n_agents=3, trail=False)
    want = rd.render_episodes_torch(states, maps, torch.ones(B, dtype=torch.int32), spec)[:, 0]
    got = env.render_frames(size=64)
    assert got.is_cuda and got.shape == (B, 64, 64, 3) and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), want)
    if env.flight:   # the map shows: the same states without it give other frames
        assert not torch.equal(want, rd.render_episodes_torch(states, None, torch.ones(B, dtype=torch.int32), spec)[:, 0])
    some = env.render_frames(envs=[2, 0], size=64)
    assert torch.equal(some.cpu(), want[[2, 0]])
    big = env.render_frames(envs=torch.tensor([1]), spec=rd.RenderSpec.for_env(env, 128, bar=False))
    assert big.shape == (1, 128, 128, 3)


def test_single_env_adapter_render_frame():
    e = cs.FlightSearchEnvEasy(cs.make_env_args("flight_easy", n_agents=3), cs.default_circle_dict(), seed=5)
    e.step([0, 1, 2])
    pic = e.render_frame(size=32)
    assert isinstance(pic, np.ndarray) and pic.shape == (32, 32, 3) and pic.dtype == np.uint8
    state = torch.from_numpy(e.get_state().astype(np.float32)).reshape(1, 1, -1)
    spec = rd.RenderSpec(size=32, n_agents=3, trail=False)
    assert np.array_equal(pic, rd.render_episodes_torch(state, None, torch.ones(1, dtype=torch.int32), spec)[0, 0].numpy())


# ---- 5. Runner.replay on a shipped checkpoint -------------------------------------------------------------------------------

def test_runner_replay_draws_a_greedy_batch_of_a_shipped_checkpoint(tmp_path):
    d = np.load(os.path.join(GOLDEN, "trained_easy3_qmix.npz"))
    B, W, m = 4, 64, 15
    args = cs.make_env_args("flight_easy", n_agents=3, agent_mode=int(d["agent_mode"]))
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + 11)
    cs.apply_env_info(args, env)
    args.alg = "qmix"
    cs.get_mixer_args(args, seed=17)
    args.buffer_size, args.batch_size = 2 * B, 4
    args.model_dir, args.result_dir = str(tmp_path / "model") + "/", str(tmp_path / "result") + "/"
    r = rn.Runner(env, args)
    # the checkpoint in the reference's file names (policy/qmix.py:189-196): the shipped agent network, a mixer of the right shape
    rnn = {k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w_")}
    torch.save(rnn, os.path.join(r.model_path, "7_rnn_net_params.pkl"))
    torch.save(r.learner.eval_qmix_net.state_dict(), os.path.join(r.model_path, "7_qmix_net_params.pkl"))
    with pytest.raises(FileNotFoundError):
        r.replay(8)
    frames, targets_find, episode_reward, steps = r.replay(7, size=W)
    T = env.time_limit
    assert frames.is_cuda and frames.shape == (B, T + 1, W, W, 3) and frames.dtype == torch.uint8
    assert os.path.getsize(os.path.join(r.result_path, "replay_7.gif")) > 0
    for k in ("fc1.weight", "rnn.weight_hh"):
        assert torch.equal(r.learner.eval_rnn.state_dict()[k].cpu(), rnn[k])
    assert torch.equal(targets_find, env.target_find) and torch.equal(steps.to(torch.int32), env.time_step)
    assert torch.equal(episode_reward, env.total_reward.to(torch.float32))
    assert int(targets_find.max()) > 0   # the trained policy finds targets
    last = frames[:, T].cpu().numpy()
    spec = rd.RenderSpec(size=W, n_agents=3)
    for b in range(B):
        green = math.ceil(int(targets_find[b]) * W / m)
        assert (last[b, :4, :green] == np.array(spec.bar_on, dtype=np.uint8)).all(), b
        assert (last[b, :4, green:] == np.array(spec.bar_off, dtype=np.uint8)).all(), b
    two, *_ = r.replay(7, episodes=2, size=32, path=str(tmp_path / "two.gif"))
    assert two.shape == (2, T + 1, 32, 32, 3) and os.path.exists(str(tmp_path / "two.gif"))
