"""GPU tests of the QMIX learner: the recurrence kernels (csrc/gru_seq.h) against fp64 torch, the fused learner against the
reference's recorded learn step and against the torch unroll, and the whole loop collect -> store -> sample -> learn -> act."""
import numpy as np
import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd.learner import GRUSequence, QMixLearner, get_mixer_args
from learn_util import GOLDEN, learner_args, load_fixture, record
from test_learner_cpu import check_grads, named_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 64


def weights(kind, gen):
    """(w_ih, b_ih, w_hh, b_hh) fp64 on the device: torch's default GRUCell init, or a shipped checkpoint's."""
    if kind == "random":
        k = 1.0 / np.sqrt(H)
        return [(torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1).mul_(k).to(DEV)
                for shape in ((3 * H, H), (3 * H,), (3 * H, H), (3 * H,))]
    z = np.load(f"{GOLDEN}/trained_{kind}.npz")
    return [torch.from_numpy(z[f"w_rnn.{k}"].astype(np.float64)).to(DEV) for k in ("weight_ih", "bias_ih", "weight_hh", "bias_hh")]


def gru_step(gi, h, w_hh, b_hh):
    """One torch.nn.GRUCell step with gi = W_ih x + b_ih given: rows of gi [..., 192] and h [..., 64]."""
    gh = h @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return (1 - z) * n + z * h


def gru_fp64(gi, w_hh, b_hh, h0):
    """torch.nn.GRUCell's recurrence with gi given for all t (autograd-capable; fp64 when its inputs are)."""
    h = h0 if h0 is not None else gi.new_zeros(gi.shape[1], H)
    out = []
    for t in range(gi.shape[0]):
        h = gru_step(gi[t], h, w_hh, b_hh)
        out.append(h)
    return torch.stack(out, 0)


def inputs(kind, R, T, seed, with_h0=True):
    gen = torch.Generator().manual_seed(seed)
    w_ih, b_ih, w_hh, b_hh = weights(kind, gen)
    x = torch.relu(torch.randn(T, R, H, generator=gen, dtype=torch.float64)).to(DEV)   # fc1's ReLU outputs
    gi = (x @ w_ih.t() + b_ih).float()                                                   # what the learner hands over: fp32
    h0 = (torch.rand(R, H, generator=gen, dtype=torch.float64) * 1.8 - 0.9).to(DEV).float() if with_h0 else None
    return gi, w_hh.float(), b_hh.float(), h0


@pytest.mark.parametrize("kind", ["random", "easy3_qmix", "flight3_qmix"])
@pytest.mark.parametrize("R", [1, 15, 96, 160, 3000])
@pytest.mark.parametrize("T", [1, 7, 200])
def test_forward_matches_fp64_grucell(kind, R, T):
    """Every step of the kernel's unroll is an fp64 GRUCell step of its own h_{t-1} to 2e-5 (the policy kernel's bar per step).
    The free-running trajectory is compared with the fp64 one too, but a 200-step unroll with trained weights amplifies rounding:
    fp32 torch itself drifts from fp64 by up to ~1e-4 there, and the kernel's per-step rounding (split-fp16 products, hardware
    sigmoid) is carried the same way (measured: at most 4.2x fp32 torch's drift, R = 15 with the easy3 weights).  So the bar of the
    trajectory is 2e-5 or eight times fp32 torch's own drift on the same data, whichever is larger."""
    gi, w_hh, b_hh, h0 = inputs(kind, R, T, seed=R * 1000 + T, with_h0=(R % 2 == 0))
    with torch.no_grad():
        got = GRUSequence.apply(gi, w_hh, b_hh, h0)
        torch.cuda.synchronize()
        assert got.shape == (T, R, H) and torch.isfinite(got).all()
        g64, w64, b64 = gi.double(), w_hh.double(), b_hh.double()
        first = h0.double().unsqueeze(0) if h0 is not None else g64.new_zeros(1, R, H)
        step = gru_step(g64, torch.cat([first, got.double()[:-1]], 0), w64, b64)
        assert float((got.double() - step).abs().max()) <= 2e-5
        want = gru_fp64(g64, w64, b64, None if h0 is None else h0.double())
        drift32 = float((gru_fp64(gi, w_hh, b_hh, h0).double() - want).abs().max())
        assert float((got.double() - want).abs().max()) <= max(2e-5, 8 * drift32), drift32


def test_fp64_statement_is_torch_grucell():
    """gru_fp64 (the yardstick above) is torch.nn.GRUCell: the same weights through the stock cell, x and W_ih explicit."""
    gen = torch.Generator().manual_seed(9)
    w_ih, b_ih, w_hh, b_hh = weights("easy3_qmix", gen)
    cell = torch.nn.GRUCell(H, H).double().to(DEV)
    with torch.no_grad():
        for p, v in ((cell.weight_ih, w_ih), (cell.bias_ih, b_ih), (cell.weight_hh, w_hh), (cell.bias_hh, b_hh)):
            p.copy_(v)
        x = torch.relu(torch.randn(7, 33, H, generator=gen, dtype=torch.float64)).to(DEV)
        h, out = torch.zeros(33, H, dtype=torch.float64, device=DEV), []
        for t in range(7):
            h = cell(x[t], h)
            out.append(h)
        want = torch.stack(out, 0)
        got = gru_fp64(x @ w_ih.t() + b_ih, w_hh, b_hh, None)
    assert float((got - want).abs().max()) <= 1e-12


def rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("R", [1, 15, 96, 160, 3000])
@pytest.mark.parametrize("T", [1, 7, 200])
def test_backward_matches_fp64_autograd_and_is_deterministic(R, T):
    kind = "random" if R % 2 else "easy3_qmix"
    gi, w_hh, b_hh, h0 = inputs(kind, R, T, seed=7 * R + T)
    scale = 1e-5 if R in (15, 160) else 1.0   # gradients have no natural scale: the kernel must not care
    dH = torch.randn(T, R, H, generator=torch.Generator().manual_seed(R + T)).to(DEV) * scale

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (gi, w_hh, b_hh, h0)]
        GRUSequence.apply(*leaves).backward(dH)
        torch.cuda.synchronize()
        return [t.grad for t in leaves]

    got = run()
    again = run()
    for a, b in zip(got, again):
        assert torch.equal(a, b)   # no atomics, fixed grid: bit-identical runs
    leaves = [t.double().requires_grad_(True) for t in (gi, w_hh, b_hh, h0)]
    gru_fp64(*leaves).backward(dH.double())
    for name, a, leaf in zip(("dgi", "dW_hh", "db_hh", "dh0"), got, leaves):
        assert torch.isfinite(a).all(), name
        assert rel(a, leaf.grad) <= 1e-4, (name, rel(a, leaf.grad))


def test_backward_without_h0_and_bad_arguments():
    gi, w_hh, b_hh, _ = inputs("random", 40, 5, seed=3, with_h0=False)
    leaves = [t.clone().requires_grad_(True) for t in (gi, w_hh, b_hh)]
    dH = torch.randn(5, 40, H, device=DEV)
    GRUSequence.apply(*leaves, None).backward(dH)
    ref = [t.double().requires_grad_(True) for t in (gi, w_hh, b_hh)]
    gru_fp64(*ref, None).backward(dH.double())
    for a, b in zip(leaves, ref):
        assert rel(a.grad, b.grad) <= 1e-4
    ops = cs.lib.torch_ops()
    with pytest.raises(RuntimeError, match="gi"):
        ops.gru_seq_forward(w_hh, b_hh, gi[:, :39].contiguous(), None, 5, 40, torch.empty(5, 40, H, device=DEV), None)


# k_gru_seq_bwd scales every block of 16 rows by its own power of two (from the block's largest |dH| over all t; m == 0 leaves
# the scale at 1).  The tests above scale the whole tensor by one factor and judge one norm per tensor, which the largest block
# dominates; these judge dgi and dh0 -- the kernel's own outputs; dW_hh and db_hh are torch sums across the blocks -- block by
# block.

def kernel_backward(gi, w_hh, b_hh, h0, dH):
    """(dgi, dh0) of GRUSequence for dH: the two outputs of the backward kernel that belong to a block's own rows."""
    lgi, lh0 = gi.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    GRUSequence.apply(lgi, w_hh, b_hh, lh0).backward(dH)
    torch.cuda.synchronize()
    return lgi.grad, lh0.grad


def test_backward_scales_every_block_of_rows_on_its_own():
    """Five blocks whose dH are unit normal draws times 2^-100, 2^-40, 1, 2^40 and 2^100 in ONE launch: each block's dgi and dh0
    rows to 1e-4 relative Frobenius (the bar of the tests above, per block) of fp64 autograd with the same dH.
    Measured on an MI355X: dgi 2.3e-7 to 2.7e-7 and dh0 2.2e-7 to 3.3e-7 in every block, whatever its exponent."""
    R, T = 80, 7
    gi, w_hh, b_hh, h0 = inputs("easy3_qmix", R, T, seed=83)
    exps = (-100, -40, 0, 40, 100)
    assert R == 16 * len(exps)
    factor = torch.tensor([2.0 ** k for k in exps], dtype=torch.float64).repeat_interleave(16)[None, :, None]
    dH64 = (torch.randn(T, R, H, generator=torch.Generator().manual_seed(84), dtype=torch.float64) * factor).to(DEV)
    dH = dH64.float()
    assert torch.isfinite(dH).all() and all(dH[:, 16 * b:16 * b + 16].any() for b in range(len(exps)))   # float32 holds 2^+-100
    dgi, dh0 = kernel_backward(gi, w_hh, b_hh, h0, dH)
    leaves = [t.double().requires_grad_(True) for t in (gi, w_hh, b_hh, h0)]
    gru_fp64(*leaves).backward(dH.double())   # the same dH: float32 -> float64 is exact
    want_dgi, want_dh0 = leaves[0].grad, leaves[3].grad
    assert torch.isfinite(dgi).all() and torch.isfinite(dh0).all()
    errs = []
    for b, k in enumerate(exps):
        rows = slice(16 * b, 16 * b + 16)
        assert float(want_dgi[:, rows].norm()) > 0 and float(want_dh0[rows].norm()) > 0
        errs.append((k, rel(dgi[:, rows], want_dgi[:, rows]), rel(dh0[rows], want_dh0[rows])))
    print("gru backward, per block (exponent, dgi, dh0):", ", ".join(f"(2^{k}: {a:.2e}, {c:.2e})" for k, a, c in errs))
    for k, a, c in errs:
        assert a <= 1e-4 and c <= 1e-4, (k, a, c)


def test_backward_of_an_all_zero_block_is_zero_and_leaves_its_neighbours_alone():
    """R = 40 (blocks of 16, 16 and 8 rows), dH of rows 16..31 zero at every t: that block's dgi and dh0 are exactly zero (the
    m == 0 path: scale 1), and the other two blocks are bit-identical to a launch in which rows 16..31 carry dH of their own --
    no block reads another's rows."""
    R, T = 40, 5
    gi, w_hh, b_hh, h0 = inputs("easy3_qmix", R, T, seed=85)
    dH = torch.randn(T, R, H, generator=torch.Generator().manual_seed(86)).to(DEV)
    holed = dH.clone()
    holed[:, 16:32] = 0.0
    dgi_full, dh0_full = kernel_backward(gi, w_hh, b_hh, h0, dH)
    dgi, dh0 = kernel_backward(gi, w_hh, b_hh, h0, holed)
    assert not dgi[:, 16:32].any() and not dh0[16:32].any()
    assert dgi_full[:, 16:32].any() and dh0_full[16:32].any()
    for rows in (slice(0, 16), slice(32, 40)):
        assert torch.equal(dgi[:, rows], dgi_full[:, rows]) and torch.equal(dh0[rows], dh0_full[rows])
        assert dgi[:, rows].any() and dh0[rows].any()


def test_backward_of_all_zero_dH_is_all_zero():
    """A whole launch of zeros (R = 15: one partial block): every gradient is zero and finite, nothing divides by the block's m."""
    R, T = 15, 5
    gi, w_hh, b_hh, h0 = inputs("easy3_qmix", R, T, seed=87)
    leaves = [t.clone().requires_grad_(True) for t in (gi, w_hh, b_hh, h0)]
    GRUSequence.apply(*leaves).backward(torch.zeros(T, R, H, device=DEV))
    for name, leaf in zip(("dgi", "dW_hh", "db_hh", "dh0"), leaves):
        assert torch.isfinite(leaf.grad).all() and not leaf.grad.any(), name


# ---- the fused learner ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def to_dev(batch):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in batch.items()}


def load_params(learner, ev, tg):
    with torch.no_grad():
        for which, vals in (("eval", ev), ("target", tg)):
            for k, p in named_params(learner, which).items():
                p.copy_(torch.from_numpy(vals[k]).to(DEV))


@pytest.mark.parametrize("k", [0, 1])
def test_fused_learner_gradients_match_the_reference(fx, k):
    meta, batch, init, steps = fx
    lr = QMixLearner(learner_args(meta), device=DEV, unroll="fused")
    if k == 0:
        load_params(lr, init, init)
    else:
        load_params(lr, record(steps[k - 1], "eval"), record(steps[k - 1], "target"))
    b = to_dev(batch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = lr.learn(b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss)
    check_grads(lr, record(steps[k], "grad"), float(steps[k]["grad_norm"]), 1e-4)


def test_fused_learner_step_matches_the_reference(fx):
    meta, batch, init, steps = fx
    lr = QMixLearner(learner_args(meta), device=DEV, unroll="fused")
    tau, step_lr = meta["args"]["tau"], meta["args"]["lr"]
    before = {k: p.detach().clone().double() for k, p in named_params(lr, "target").items()}
    b = to_dev(batch)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        lr.learn(b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_grads(lr, record(steps[0], "grad"), float(steps[0]["grad_norm"]), 1e-4)
    want_eval, grads = record(steps[0], "eval"), record(steps[0], "grad")
    for k, p in named_params(lr).items():
        have, w = p.detach().cpu().double().numpy(), want_eval[k].astype(np.float64)
        if k not in grads:
            assert np.array_equal(have, w), k
            continue
        g = np.abs(grads[k])
        big = g >= 1e-3 * g.max()
        assert np.abs(have - w)[big].max(initial=0.0) <= 1e-6, k
        assert np.abs(have - w)[~big].max(initial=0.0) <= 2 * step_lr, k
    for k, p in named_params(lr, "target").items():
        want = tau * named_params(lr)[k].detach().double() + (1 - tau) * before[k]
        assert float((p.detach().double() - want).abs().max()) <= 1e-6, k


def replay(env_name, n, E, episodes, seed):
    args = cs.make_env_args(env_name, n_agents=n)
    env = cs.BatchedFlightEnv(args, batch=episodes)
    cs.apply_env_info(args, env)
    get_mixer_args(args, seed=seed)
    rb = cs.DeviceReplayBuffer(args, episodes)
    g = torch.Generator(DEV).manual_seed(seed)
    cs.EpisodeCollector(env).generate_episodes(policy=cs.random_policy(g), into=rb)
    return args, rb, g


@pytest.mark.parametrize("env_name,n,E", [("flight_easy", 3, 32), ("flight_easy", 5, 32), ("flight", 3, 4)])
def test_fused_and_torch_learners_agree_over_20_steps(env_name, n, E):
    args, rb, g = replay(env_name, n, E, episodes=64 if env_name == "flight_easy" else 8, seed=11)
    batches = [rb.sample(E, generator=g) for _ in range(20)]
    fused = QMixLearner(args, device=DEV, unroll="fused")
    ref = QMixLearner(args, device=DEV, unroll="torch")
    lf = torch.stack([fused.learn(b) for b in batches]).cpu()
    lt = torch.stack([ref.learn(b) for b in batches]).cpu()
    assert torch.isfinite(lf).all() and torch.isfinite(lt).all()
    assert float(((lf - lt).abs() / lt.abs()).max()) <= 1e-3, (lf, lt)


def test_collect_store_sample_learn_act():
    """The whole loop on the device: FusedAgents acting with the learner's eval network -> replay -> learn -> load_weights."""
    B, E = 64, 32
    args = cs.make_env_args("flight_easy", n_agents=3)
    env = cs.BatchedFlightEnv(args, batch=B)
    cs.apply_env_info(args, env)
    get_mixer_args(args, seed=5)
    learner = QMixLearner(args, device=DEV)
    agents = cs.FusedAgents(args, B, net=learner.eval_rnn, seed=1)
    rb = cs.DeviceReplayBuffer(args, 2 * B)
    col = cs.EpisodeCollector(env)
    col.generate_episodes(agents=agents, epsilon=0.5, evaluate=False, into=rb)
    g = torch.Generator(DEV).manual_seed(2)

    def q_of_first_step():
        env.reset(init=True)
        agents.init_hidden()
        obs = env.get_obs().clone()
        agents.choose_action(obs, evaluate=True, want_q=True)
        return agents.q.clone(), obs

    q0, _ = q_of_first_step()
    losses = [learner.learn(rb.sample(E, generator=g)) for _ in range(3)]
    agents.load_weights()
    q1, obs = q_of_first_step()
    with torch.no_grad():   # the agents act with exactly the learner's network
        x = torch.cat([obs, torch.zeros(B, 3, 3, device=DEV), torch.eye(3, device=DEV).expand(B, 3, 3)], 2).reshape(B * 3, -1)
        q_ref, _ = learner.eval_rnn(x, torch.zeros(B * 3, H, device=DEV))
    col.generate_episodes(agents=agents, epsilon=0.5, evaluate=False, into=rb)
    losses.append(learner.learn(rb.sample(E, generator=g)))
    assert all(bool(torch.isfinite(x)) for x in losses)
    assert torch.isfinite(q1).all() and not torch.equal(q0, q1)
    assert float((q1.reshape(B * 3, -1) - q_ref).abs().max()) <= 1e-4
