"""CPU tests of the map-once episode format (replay.COMPACT_KEYS): the two conversions are inverses,
the compact ring walks the dense ring's slots, the learners' torch unrolls compute on a compact batch what they compute on its
expansion, the Runner's call schedule does not depend on the format, and the new entry points refuse bad arguments before
touching a device."""
import contextlib
import ctypes as C
import os
import types

import pytest
import torch

import cooperative_search_amd as cs
from cooperative_search_amd import _lib
from cooperative_search_amd import runner as rn
from cooperative_search_amd.collector import assemble_episodes_torch
from cooperative_search_amd.learner import DOPLearner, QMixLearner, ReinforceLearner
from cooperative_search_amd.replay import (COMPACT_KEYS, KEYS, CompactReplayBuffer, DeviceReplayBuffer, compact_from_dense,
                                           expand_compact)

CELLS, TARGETS, A = 2500, 15, 3


def tables(lengths, T, n, seed=0, dtype=torch.float32):
    """Step-major tables of len(lengths) episodes as the flight kernels leave them: one map per (step, env), the agents' own 4
    floats = state[4i..4i+3], terminated from step L - 1 on (L > T: the episode never terminates)."""
    g = torch.Generator().manual_seed(seed)
    B, S = len(lengths), 4 * n + 3 * TARGETS
    m = torch.rand(T + 1, B, CELLS, generator=g, dtype=dtype)
    s = torch.rand(T + 1, B, S, generator=g, dtype=dtype) * 2 - 1
    o = torch.cat([m[:, :, None, :].expand(T + 1, B, n, CELLS), s[..., :4 * n].reshape(T + 1, B, n, 4)], 3).contiguous()
    u = torch.randint(0, A, (T, B, n), generator=g)
    r = torch.randint(-3, 111, (T, B), generator=g).to(dtype)
    term = torch.arange(T)[:, None] >= (torch.as_tensor(lengths) - 1)[None, :]
    return m, s, o, u, r, term


def dense_batch(lengths, T, n, seed=0, dtype=torch.float32):
    m, s, o, u, r, term = tables(lengths, T, n, seed, dtype)
    d = assemble_episodes_torch(o, s, u, r, term, A)
    return {k: v.to(dtype) for k, v in d.items()}


def assert_same(a, b, keys):
    assert set(a) == set(keys) and set(b) == set(keys)
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


# ---- the format --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("lengths", [[1], [6], [7], [9], [1, 6, 7, 3, 9, 2]], ids=["1", "T-1", "T", "never", "mix"])
def test_the_two_conversions_are_inverses(lengths, n):
    T = 7
    d = dense_batch(lengths, T, n, seed=len(lengths) + n)
    c = compact_from_dense(d)
    assert tuple(c) == COMPACT_KEYS
    assert c["map"].shape == (len(lengths), T + 1, CELLS) and c["s_full"].shape == (len(lengths), T + 1, 4 * n + 3 * TARGETS)
    assert_same(expand_compact(c, n, A), d, KEYS)
    assert_same(compact_from_dense(expand_compact(c, n, A)), c, COMPACT_KEYS)
    for e, L in enumerate(min(L, T) for L in lengths):   # rows t <= L hold data (a uniform map is never all zero), the rest is zero
        assert (c["map"][e, :L + 1] != 0).any(dim=-1).all() and (c["s_full"][e, :L + 1] != 0).any(dim=-1).all()
        assert (c["map"][e, L + 1:] == 0).all() and (c["s_full"][e, L + 1:] == 0).all()
        assert c["padded"][e, :, 0].tolist() == [0.0] * L + [1.0] * (T - L)
    narrow = expand_compact(c, n, A, wide=False)
    assert set(narrow) == set(KEYS) - {"o", "o_next"}
    for k in narrow:
        assert torch.equal(narrow[k], d[k]), k


# ---- the ring ----------------------------------------------------------------------------------------------------------------

def ring_args(n=3, T=4, env="flight"):
    return types.SimpleNamespace(env=env, n_actions=A, n_agents=n, state_shape=4 * n + 3 * TARGETS, obs_shape=4, episode_limit=T,
                                 conv=env == "flight", map_size=50)


def test_compact_ring_walks_the_dense_ring():
    args, size, T, n = ring_args(), 16, 4, 3
    dense, comp = DeviceReplayBuffer(args, size, device="cpu"), CompactReplayBuffer(args, size, device="cpu")
    twin_d, twin_c = DeviceReplayBuffer(args, size, device="cpu"), CompactReplayBuffer(args, size, device="cpu")
    assert tuple(comp.buffers) == COMPACT_KEYS and comp.keys == COMPACT_KEYS and dense.keys == KEYS
    for step, k in enumerate([3, 5, 8, 7, 16, 2, 16, 1]):   # 3 + 5 + 8: an exact fill; 7: from the un-wrapped cursor; 16: a whole ring
        d = dense_batch([1 + (j * 3 + step) % (T + 2) for j in range(k)], T, n, seed=step)
        dense.store_episode(d)
        comp.store_episode(compact_from_dense(d))
        assert twin_d._get_storage_idx(inc=k).tolist() == twin_c._get_storage_idx(inc=k).tolist()
        assert (comp.current_idx, comp.current_size) == (dense.current_idx, dense.current_size) == (twin_c.current_idx, twin_c.current_size)
        filled = dense.current_size
        got = expand_compact({key: v[:filled] for key, v in comp.buffers.items()}, n, A)
        for key in KEYS:
            assert torch.equal(got[key], dense.buffers[key][:filled]), (step, key)
        for kk in (1, min(3, filled), filled):
            assert comp.can_sample(kk) and comp.latest_indices(kk) == dense.latest_indices(kk)
            assert_same(expand_compact(comp.sample_latest(kk), n, A), dense.sample_latest(kk), KEYS)
        assert not comp.can_sample(filled + 1)
        g1, g2 = torch.Generator().manual_seed(step), torch.Generator().manual_seed(step)
        assert_same(expand_compact(comp.sample(6, generator=g1), n, A), dense.sample(6, generator=g2), KEYS)
        assert torch.equal(g1.get_state(), g2.get_state())   # the same use of the generator
    for rb in (dense, comp):   # inc > size is refused by both, with the cursor untouched
        before = (rb.current_idx, rb.current_size)
        with pytest.raises(ValueError, match="cannot store 17"):
            rb._get_storage_idx(inc=17)
        assert (rb.current_idx, rb.current_size) == before


def test_compact_ring_is_for_flight_only():
    with pytest.raises(ValueError, match="flight_easy"):
        CompactReplayBuffer(ring_args(env="flight_easy"), 8, device="cpu")


def test_ring_bytes_per_episode_are_the_derived_ones():
    """DESIGN.md section 12's table: float32, T = 200, 15 targets."""
    for n, dense_bytes, compact_bytes in ((3, 12136800, 2060628), (5, 20178400, 2068660)):
        args = ring_args(n=n, T=200)
        for cls, want in ((DeviceReplayBuffer, dense_bytes), (CompactReplayBuffer, compact_bytes)):
            rb = cls(args, 1, device="cpu")
            assert sum(v.numel() * v.element_size() for v in rb.buffers.values()) == want


# ---- the learners ------------------------------------------------------------------------------------------------------------

ARGS_FN = {"qmix": cs.get_mixer_args, "dop": cs.get_dop_args, "reinforce": cs.get_reinforce_args}
LEARNER = {"qmix": QMixLearner, "dop": DOPLearner, "reinforce": ReinforceLearner}
NETS = {"qmix": ("eval_rnn", "target_rnn", "eval_qmix_net", "target_qmix_net"),
        "dop": ("actor", "eval_critic", "target_critic", "eval_mixer_net", "target_mixer_net"), "reinforce": ("eval_rnn",)}


def learner_args(alg, n, T):
    a = cs.make_env_args("flight", n_agents=n)
    assert all(getattr(a, k) == v for k, v in cs.FusedAgents.CONV_HYPER.items())
    a.n_actions, a.state_shape, a.obs_shape, a.episode_limit = A, 4 * n + 3 * TARGETS, 4, T
    a.last_action, a.reuse_network, a.alg = True, True, alg
    ARGS_FN[alg](a, seed=11)
    return a


def grads_after_learn(alg, n, T, batch, max_len, dtype, unroll="torch", device="cpu", guard=None):
    """(loss(es), {"<net>.<parameter>": gradient}) of one learn call of a fresh learner (the constructor seeds torch, so two
    learners of the same arguments start from identical weights); guard: a context manager around the call."""
    lr = LEARNER[alg](learner_args(alg, n, T), device=device, unroll=unroll)
    for m in NETS[alg]:
        getattr(lr, m).to(dtype)
    extra = () if alg == "qmix" else (0.3,)
    with (guard() if guard else contextlib.nullcontext()):
        loss = lr.learn(batch, max_len, 0, *extra)
    loss = torch.stack([l.double() for l in loss]) if isinstance(loss, tuple) else loss.double().reshape(1)
    grads = {f"{m}.{k}": p.grad.double() for m in NETS[alg] for k, p in getattr(lr, m).named_parameters() if p.grad is not None}
    return loss, grads


def rel_frobenius(a, b):
    return float((a - b).norm() / b.norm())


def compare_learn_on(alg, n, T, c, d, max_len, dtype, bar, unroll="torch", device="cpu", guard=None):
    """One learn on the compact batch c against one on its expansion d, identical initial weights: the loss(es), every
    parameter's gradient and all gradients together within `bar`, relative Frobenius.  A parameter without a gradient in one
    run has none in the other.  Every figure is printed before the assertion."""
    loss_c, g_c = grads_after_learn(alg, n, T, c, max_len, dtype, unroll, device, guard)
    loss_d, g_d = grads_after_learn(alg, n, T, d, max_len, dtype, unroll, device, guard)
    assert sorted(g_c) == sorted(g_d) and any(k.endswith("conv.0.weight") for k in g_d)
    figures = {"loss": rel_frobenius(loss_c, loss_d),
               "all": rel_frobenius(torch.cat([g_c[k].flatten() for k in sorted(g_d)]), torch.cat([g_d[k].flatten() for k in sorted(g_d)]))}
    figures.update({k: rel_frobenius(g_c[k], g_d[k]) for k in g_d})
    worst = max(figures, key=figures.get)
    print(f"{alg} n={n} max_len={max_len} {dtype} {unroll}: worst {worst} {figures[worst]:.3e}, all {figures['all']:.3e}, "
          f"loss {figures['loss']:.3e}")
    assert figures[worst] <= bar, (worst, figures[worst])


def compare_learn(alg, n, max_len, dtype, bar):
    T = 6
    d = dense_batch([2, 6, 9, 4], T, n, seed=n, dtype=dtype)
    compare_learn_on(alg, n, T, compact_from_dense(d), d, max_len, dtype, bar)


@pytest.mark.parametrize("max_len", [None, 4])
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_learn_on_a_compact_batch_equals_learn_on_its_expansion_float64(alg, n, max_len):
    """1e-12: the map-once restatement of the conv front end differs from the dense one by ~1e-15 in float64 (the sum over
    the agents' identical maps moves from the weight gradient's reduction to the broadcast's backward)."""
    compare_learn(alg, n, max_len, torch.float64, 1e-12)


@pytest.mark.parametrize("max_len", [None, 4])
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_learn_on_a_compact_batch_equals_learn_on_its_expansion_float32(alg, n, max_len):
    """1e-4: the project's pin for two unrolls of one learner in float32."""
    compare_learn(alg, n, max_len, torch.float32, 1e-4)


def test_qmix_and_reinforce_never_build_the_dense_observations(monkeypatch):
    """No tensor with an n * cells wide row: the widest thing learn may touch is the map itself."""
    n, T = 3, 5
    c = compact_from_dense(dense_batch([2, 5, 7], T, n))
    seen = []
    real_cat = torch.cat

    def spy(tensors, *a, **k):
        out = real_cat(tensors, *a, **k)
        seen.append(tuple(out.shape))
        return out
    monkeypatch.setattr(torch, "cat", spy)
    for alg in ("qmix", "reinforce"):
        lr = LEARNER[alg](learner_args(alg, n, T), device="cpu", unroll="torch")
        lr.learn(c, None, 0, *(() if alg == "qmix" else (0.3,)))
    assert seen and all(shape[-1] < CELLS for shape in seen), [s for s in seen if s[-1] >= CELLS]


# ---- the Runner --------------------------------------------------------------------------------------------------------------

class Recorder:
    """The recording stubs of tests/test_runner_cpu.py (collector, ring, agents, learner writing one trace), format-aware: the
    episodes they hand out carry the keys of the format the Runner asked for."""

    def __init__(self, args, T, batch=1):
        self.trace, self.args, self.batch, self.T = [], args, batch, T
        self.env = types.SimpleNamespace(batch=batch, device=torch.device("cpu"))
        self.formats = set()
        rec = self

        class Buffer:
            current_size = 0

            def sample(self, size):
                rec.trace.append(["sample", int(size)])
                return rec.episode(size)

        class Collector:
            def generate_episodes(self, agents=None, evaluate=True, episode_num=None, into=None, compact=False, **kw):
                assert agents is rec.agents and not evaluate and not kw
                rec.formats.add(bool(compact))
                rec.trace.append(["generate_episode", episode_num])
                if into is not None:
                    rec.trace.append(["store", rec.batch])
                    into.current_size += rec.batch
                    return None, None, None, None
                return rec.episode(rec.batch), None, None, None

            def evaluate(self, policy, batches=1):
                rec.trace.append(["evaluate", int(batches)])
                return 0.0, -3.0, 2.0

        class Learner:
            def learn(self, batch, max_episode_len=None, train_step=0, *epsilon):
                assert max_episode_len is None
                assert tuple(batch) == (COMPACT_KEYS if args.compact_episodes else KEYS)
                rec.trace.append(["learn", int(train_step), len(epsilon) == 1, int(batch["u"].shape[0])])

            def save_model(self, idx):
                rec.trace.append(["save", int(idx)])
                open(os.path.join(args.model_dir + rn.run_name(args), f"{idx}_rnn_net_params.pkl"), "w").close()

        class Agents:
            syncs = 0

            def sync_weights(self):
                self.syncs += 1

            def check_weights(self):
                pass

            def policy(self, epsilon=0.0, evaluate=True):
                return None

        self.buffer, self.collector, self.learner, self.agents = Buffer(), Collector(), Learner(), Agents()
        self.schedule = types.SimpleNamespace(values=torch.full((batch,), 0.5, dtype=torch.float64))

    def episode(self, k):
        return {key: torch.zeros(k, self.T, 1) for key in (COMPACT_KEYS if self.args.compact_episodes else KEYS)}

    def runner(self, **kw):
        parts = dict(learner=self.learner, agents=self.agents, schedule=self.schedule, collector=self.collector, buffer=self.buffer)
        parts.update(kw)
        return rn.Runner(self.env, self.args, **parts)


def run_args(alg, root, compact, **over):
    a = learner_args(alg, 3, 4)
    a.n_epoch, a.n_episodes, a.train_steps, a.batch_size, a.buffer_size = 7, 2, 2, 3, 8
    a.evaluate_cycle, a.save_cycle, a.evaluate_epoch = 3, 2, 2
    a.model_dir, a.result_dir = os.path.join(root, "model") + "/", os.path.join(root, "result") + "/"
    if compact is not None:
        a.compact_episodes = compact
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_runner_schedule_does_not_depend_on_the_format(alg, tmp_path):
    traces = {}
    for compact in (None, False, True):
        args = run_args(alg, str(tmp_path / str(compact)), compact)
        rec = Recorder(args, 4)
        rec.runner().run(0)
        assert args.compact_episodes is bool(compact)                       # RUN_DEFAULTS: off unless asked for
        assert rec.formats == {bool(compact)}
        traces[compact] = (rec.trace, rec.agents.syncs)
    assert traces[None] == traces[False] == traces[True]
    assert any(ev[0] == "save" for ev in traces[True][0]) and any(ev[0] == "learn" for ev in traces[True][0])


def test_runner_builds_the_ring_of_the_format(tmp_path):
    for compact, cls in ((False, DeviceReplayBuffer), (True, CompactReplayBuffer)):
        args = run_args("qmix", str(tmp_path / str(compact)), compact)
        r = Recorder(args, 4).runner(buffer=None)
        assert type(r.buffer) is cls and r.buffer.size == args.buffer_size and r.buffer.device.type == "cpu"
    easy = run_args("qmix", str(tmp_path / "easy"), True, env="flight_easy", conv=False)
    with pytest.raises(ValueError, match="flight_easy"):
        Recorder(easy, 4).runner(buffer=None)
    vdn = run_args("qmix", str(tmp_path / "v"), True)
    vdn.alg = "vdn"
    with pytest.raises(ValueError, match="vdn"):                             # the refusals stay
        rn.Runner(types.SimpleNamespace(batch=1, device="cpu"), vdn)


# ---- the C ABI and the torch ops ----------------------------------------------------------------------------------------------

def test_new_entries_are_declared_exported_and_registered():
    L = _lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "coopsearch.h")).read()
    for name in ("cs_collect_flight", "cs_store_episodes_compact"):
        assert name in _lib.EXPORTS and hasattr(L, name) and f"int {name}(" in hdr
    assert L.cs_abi_version() == _lib.ABI_VERSION == 7
    ops = _lib.torch_ops()
    assert hasattr(ops, "collect_flight") and hasattr(ops, "store_episodes_compact")


@pytest.mark.parametrize("null", [5, 6, 7, 8, 9, 11])
def test_store_episodes_compact_argument_errors_return_before_any_launch(null):
    """No GPU here: the fake pointers are never dereferenced."""
    L = _lib.load()
    ptrs = [C.c_void_p(4096 * (k + 1)) for k in range(6)]
    co = _lib.CsCompactOut(*[4096 * (k + 10) for k in range(6)])
    argv = [4, 5, 3, CELLS, 57] + ptrs[:5] + [None, C.byref(co), None]
    if null == 11:
        co.s_full = None
    else:
        argv[null] = None
    assert L.cs_store_episodes_compact(*argv) == -2   # CS_E_ARG
    assert L.cs_episodes_last_error().startswith(b"cs_store_episodes_compact")
    assert L.cs_store_episodes_compact(0, 5, 3, CELLS, 57, *ptrs[:5], None, C.byref(co), None) == -2


def test_collect_flight_refuses_missing_tables_and_the_ops_refuse_cpu_tensors():
    L = _lib.load()
    cfg = _lib.CsConfig()
    p = C.c_void_p(4096)
    head = [C.byref(cfg), p] + [p] * 10 + [5, 0, None, 0, 0, 0, 0] + [p] * 4
    assert L.cs_collect_flight(*head, None, p, None) == -2 and L.cs_last_error().startswith(b"cs_collect_flight")
    assert L.cs_collect_flight(*head, p, None, None) == -2
    assert L.cs_collect_flight(*head, C.c_void_p(4100), p, None) == -2 and b"16-byte" in L.cs_last_error()
    ops = _lib.torch_ops()
    T, B, n = 3, 2, 3
    m, s, u, r, term = (torch.zeros(T + 1, B, CELLS), torch.zeros(T + 1, B, 57), torch.zeros(T, B, n, dtype=torch.int64),
                        torch.zeros(T, B), torch.zeros(T, B, dtype=torch.uint8))
    outs = [torch.zeros(B, T + 1, CELLS), torch.zeros(B, T + 1, 57), torch.zeros(B, T, n, 1)] + [torch.zeros(B, T, 1) for _ in range(3)]
    with pytest.raises(RuntimeError, match="coopsearch"):
        ops.store_episodes_compact(m, s, u, r, term, None, outs)
