"""GPU test of exact resume (Runner.save_state / load_state): three epochs, a state file, a NEW env with other seeds and a new
Runner that loads it, three more epochs -- against six epochs in one go.  evaluate_cycle = 3 puts an evaluation, which draws
from every env's stream, right after the resume point.  The uninterrupted run is made twice and its spread is the tolerance,
as in tests/test_gpu_runner.py::test_runner_equals_the_hand_written_loop: bitwise when the two agree."""
import os

import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import runner as rn

pytestmark = pytest.mark.gpu
ARGS_FN = {"qmix": cs.get_mixer_args, "dop": cs.get_dop_args, "reinforce": cs.get_reinforce_args}
N_AGENTS, EPOCHS, HALF = 3, 6, 3


def make_runner(alg, env_name, B, root, seed0=101, **over):
    args = cs.make_env_args(env_name, n_agents=N_AGENTS)
    env = cs.BatchedFlightEnv(args, batch=B, seeds=np.arange(B, dtype=np.uint32) + seed0)
    cs.apply_env_info(args, env)
    args.alg = alg
    ARGS_FN[alg](args, seed=17)
    args.n_episodes, args.train_steps, args.batch_size, args.buffer_size = 1, 1, 32, 2 * B
    args.evaluate_cycle, args.save_cycle, args.evaluate_epoch = 3, 4, B
    args.model_dir, args.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
    for k, v in over.items():
        setattr(args, k, v)
    return rn.Runner(env, args)


def flat(prefix, obj, out):
    """Every tensor / number of a nested state_dict under a dotted name."""
    if isinstance(obj, dict):
        for k, v in obj.items():
            flat(f"{prefix}.{k}", v, out)
    elif isinstance(obj, (list, tuple)):
        for k, v in enumerate(obj):
            flat(f"{prefix}.{k}", v, out)
    elif torch.is_tensor(obj):
        out[prefix] = obj.detach().clone()
    elif isinstance(obj, (int, float, bool)):
        out[prefix] = torch.tensor(float(obj), dtype=torch.float64)


def outcome(r):
    learner = {}
    flat("learner", rn.learner_state(r.learner), learner)
    ring = None if r.buffer is None else {k: v[:r.buffer.current_size].clone() for k, v in r.buffer.buffers.items()}
    return dict(learner=learner, ring=ring, cursor=None if r.buffer is None else (r.buffer.current_idx, r.buffer.current_size),
                eps=r.schedule.values.clone(), evals=list(zip(r.win_rates, r.episode_rewards, r.targets_find)),
                packed=r.agents.packed.clone(), records=r.env.snapshot().records, calls=r.agents.calls,
                counts=(r.epoch, r.train_steps))


def max_diff(a, b):
    assert sorted(a) == sorted(b)
    return max((a[k].double() - b[k].double()).abs().max().item() if a[k].numel() else 0.0 for k in a)


@pytest.mark.parametrize("alg, env_name, B, over", [("qmix", "flight_easy", 16, {}), ("dop", "flight_easy", 16, {}),
                                                     ("reinforce", "flight_easy", 16, {}),
                                                     ("qmix", "flight", 8, dict(compact_episodes=True))],
                         ids=["qmix-easy", "dop-easy", "reinforce-easy", "qmix-flight-compact"])
def test_a_resumed_run_equals_the_uninterrupted_one(alg, env_name, B, over, tmp_path):
    whole = []
    for k in range(2):
        r = make_runner(alg, env_name, B, str(tmp_path / f"w{k}"), **over)
        r.run(0, n_epoch=EPOCHS)
        whole.append(outcome(r))
    spread = max_diff(whole[0]["learner"], whole[1]["learner"])
    # the interrupted run
    root = str(tmp_path / "r")
    first = make_runner(alg, env_name, B, root, **over)
    first.run(0, n_epoch=HALF)
    assert (first.epoch, first.train_steps) == (HALF, HALF)
    path = str(tmp_path / "state.pt")
    first.save_state(path)
    del first
    second = make_runner(alg, env_name, B, root, seed0=40000, **over)   # other seeds: every env takes its record
    assert not torch.equal(second.env.snapshot().records[:, 640:], whole[0]["records"][:, 640:])
    second.load_state(path)
    assert (second.epoch, second.train_steps) == (HALF, HALF)
    second.run(0, n_epoch=EPOCHS)
    got, want = outcome(second), whole[0]
    assert got["counts"] == want["counts"] == (EPOCHS, EPOCHS) and got["calls"] == want["calls"]
    d = max_diff(got["learner"], want["learner"])
    print(f"{alg} {env_name}: spread of two uninterrupted runs {spread:g}, resumed against uninterrupted {d:g}")
    assert d <= spread, (d, spread)
    assert got["cursor"] == want["cursor"]
    assert torch.equal(got["eps"], want["eps"])   # one subtraction per executed step: exact, whatever the learner's rounding
    if spread == 0:
        assert torch.equal(got["packed"].view(torch.int32), want["packed"].view(torch.int32))
        if want["ring"] is not None:
            for k, v in want["ring"].items():
                assert torch.equal(got["ring"][k], v), k
        assert got["evals"] == want["evals"]
        assert torch.equal(got["records"], want["records"])
