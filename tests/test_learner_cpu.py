"""CPU tests of the QMIX learner (cooperative-search_amd/learner.py) against the reference's own learn step, recorded by
tests/golden/gen_learn.py: the torch unroll (the reference's per-step loop over the same modules) on the CPU reproduces the
reference's initial parameters, gradients, pre-clip norm, Adam step, soft update and checkpoint files; the C ABI and the torch
op layer carry the recurrence entry points."""
import os

import numpy as np
import pytest
import torch

from cooperative_search_amd import _lib
from cooperative_search_amd.learner import QMixLearner
from learn_util import learner_args, load_fixture, record


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def named_params(learner, which="eval"):
    rnn, mix = (learner.eval_rnn, learner.eval_qmix_net) if which == "eval" else (learner.target_rnn, learner.target_qmix_net)
    out = {f"rnn.{k}": p for k, p in rnn.named_parameters()}
    out.update({f"qmix.{k}": p for k, p in mix.named_parameters()})
    return out


def load_params(learner, ev, tg):
    with torch.no_grad():
        for which, vals in (("eval", ev), ("target", tg)):
            for k, p in named_params(learner, which).items():
                p.copy_(torch.from_numpy(vals[k]))


def check_grads(learner, want, norm_want, bar):
    """Per tensor: |dg| <= bar * max(|g|, 1e-3 |g_all|); tensors without a recorded gradient have none here either."""
    have = {k: p.grad for k, p in named_params(learner).items()}
    g_all = float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in want.values())))
    assert set(k for k, g in have.items() if g is not None) == set(want), "parameters with a gradient differ"
    for k, w in want.items():
        g = have[k].detach().cpu().double().numpy()
        d = float(np.linalg.norm((g - w).ravel()))
        floor = max(float(np.linalg.norm(w.ravel())), 1e-3 * g_all)
        assert d <= bar * floor, (k, d, floor)
    assert abs(float(learner.last_grad_norm) - norm_want) <= bar * norm_want
    for name in ("V", "hyper_b1", "hyper_b2"):   # unused by the mixer's output: never a gradient
        assert all(p.grad is None for p in getattr(learner.eval_qmix_net, name).parameters())


def check_step(learner, fx, bar):
    """One learn step from the recorded initial state against the reference's first step."""
    meta, batch, init, steps = fx
    lr, tau = meta["args"]["lr"], meta["args"]["tau"]
    before = {k: p.detach().cpu().clone() for k, p in named_params(learner, "target").items()}
    learner.learn({k: v.copy() for k, v in batch.items()})
    check_grads(learner, record(steps[0], "grad"), float(steps[0]["grad_norm"]), bar)
    want_eval, grads = record(steps[0], "eval"), record(steps[0], "grad")
    for k, p in named_params(learner).items():
        have = p.detach().cpu().double().numpy()
        w = want_eval[k].astype(np.float64)
        if k not in grads:
            assert np.array_equal(have, w), k   # no gradient: the parameter never moves
            continue
        g = np.abs(grads[k])
        big = g >= 1e-3 * g.max()
        # Adam's first step is ~lr * sign(g): where the gradient is at noise level its sign may flip
        assert np.abs(have - w)[big].max(initial=0.0) <= 1e-6, k
        assert np.abs(have - w)[~big].max(initial=0.0) <= 2 * lr, k
    for k, p in named_params(learner, "target").items():
        e = named_params(learner)[k].detach().cpu().double()
        want = tau * e + (1 - tau) * before[k].double()
        assert float((p.detach().cpu().double() - want).abs().max()) <= 1e-6, k


def test_initial_parameters_are_the_references(fx):
    meta, _, init, _ = fx
    lr = QMixLearner(learner_args(meta), device="cpu", unroll="torch")
    for which in ("eval", "target"):
        for k, p in named_params(lr, which).items():
            assert np.array_equal(p.detach().numpy(), init[k]), (which, k)
    names = {id(p): k for k, p in named_params(lr).items()}
    assert meta["eval_parameters"] == [names[id(p)] for p in lr.eval_parameters]   # the order clip_grad_norm_ sums in


@pytest.mark.parametrize("k", [0, 1])
def test_gradients_match_the_reference(fx, k):
    meta, batch, init, steps = fx
    lr = QMixLearner(learner_args(meta), device="cpu", unroll="torch")
    if k == 0:
        load_params(lr, init, init)
    else:
        load_params(lr, record(steps[k - 1], "eval"), record(steps[k - 1], "target"))
    lr.learn({key: v.copy() for key, v in batch.items()})
    check_grads(lr, record(steps[k], "grad"), float(steps[k]["grad_norm"]), 1e-6)


def test_one_learn_step_matches_the_reference(fx):
    meta = fx[0]
    check_step(QMixLearner(learner_args(meta), device="cpu", unroll="torch"), fx, 1e-6)


def test_checkpoints_use_the_reference_names_and_round_trip(fx, tmp_path):
    meta = fx[0]
    args = learner_args(meta, model_dir=str(tmp_path) + "/")
    lr = QMixLearner(args, device="cpu", unroll="torch")
    lr.learn({key: v.copy() for key, v in fx[1].items()})
    lr.save_model(7)
    assert lr.model_dir == str(tmp_path) + "/" + meta["model_dir"][len(meta["args"]["model_dir"]):]
    files = sorted(os.listdir(lr.model_dir))
    assert files == sorted(f.format(num=7) for f in meta["files"])
    for m, fn in (("qmix", "7_qmix_net_params.pkl"), ("rnn", "7_rnn_net_params.pkl")):
        sd = torch.load(os.path.join(lr.model_dir, fn), map_location="cpu", weights_only=True)
        assert {k: list(v.shape) for k, v in sd.items()} == meta["state_dicts"][m]
    other = QMixLearner(learner_args(meta, seed=meta["args"]["seed"] + 1), device="cpu", unroll="torch")
    other.load_model(os.path.join(lr.model_dir, "7_rnn_net_params.pkl"), os.path.join(lr.model_dir, "7_qmix_net_params.pkl"))
    for which in ("eval", "target"):
        got = named_params(other, which)
        for k, p in named_params(lr).items():
            assert torch.equal(got[k], p), (which, k)


def test_recurrence_ops_are_registered_and_refuse_cpu_tensors():
    ops = _lib.torch_ops()
    assert hasattr(ops, "gru_seq_forward") and hasattr(ops, "gru_seq_backward")
    T, R = 2, 3
    w, b = torch.zeros(192, 64), torch.zeros(192)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gru_seq_forward(w, b, torch.zeros(T, R, 192), None, T, R, torch.zeros(T, R, 64), None)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.gru_seq_backward(w, torch.zeros(T, R, 64), torch.zeros(T, R, 64), None, torch.zeros(T, R, 4, 64), T, R,
                             torch.zeros(T, R, 192), torch.zeros(T, R, 192), None)
    L = _lib.load()
    for name in ("cs_gru_seq_forward", "cs_gru_seq_backward", "cs_learn_last_error"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    # host-side argument checks: no launch, the error names the entry point
    rc = L.cs_gru_seq_forward(None, None, None, None, 0, 0, None, None, None)
    assert rc != 0 and b"cs_gru_seq_forward" in L.cs_learn_last_error()
    rc = L.cs_gru_seq_backward(None, None, None, None, None, 0, 0, None, None, None, None)
    assert rc != 0 and b"cs_gru_seq_backward" in L.cs_learn_last_error()
