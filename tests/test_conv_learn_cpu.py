"""CPU tests of the learners' conv front end on the project's own kernels (`conv_impl`): the new entry
points are declared, exported and bound; the learners take `conv_impl` and refuse it, with the reason, where the kernels cannot
run; and the default ("torch") is the code as it was."""
import ctypes as C
import os
import re

import pytest
import torch

from cooperative_search_amd import _lib, learner as ln
from cooperative_search_amd import runner as rn
from test_compact_cpu import LEARNER, NETS, compact_from_dense, dense_batch, learner_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cs_policy_conv_features_backward", "cs_policy_conv_features_backward_scratch")


def test_header_declares_the_new_symbols_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, "include", "coopsearch.h")).read()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTS
    assert re.search(r"#define CS_ABI_VERSION\s+7\b", header) and _lib.ABI_VERSION == 7


def test_library_exports_the_new_symbols_with_argument_types():
    L = _lib.load()
    assert L.cs_abi_version() == 7
    for name in NEW:
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int
    # argument errors are reported before anything touches a device
    floats = C.c_int64(-1)
    assert L.cs_policy_conv_features_backward_scratch(0, C.byref(floats)) != 0
    assert b"n_maps" in L.cs_policy_last_error()
    assert L.cs_policy_conv_features_backward(*([None] * 7), 2500, 1, *([None] * 8), 0, None) != 0
    assert b"cs_policy_conv_features_backward" in L.cs_policy_last_error()


def test_torch_op_layer_registers_the_new_ops():
    ops = _lib.torch_ops()
    assert hasattr(ops, "policy_conv_features_backward") and hasattr(ops, "policy_conv_features_backward_scratch")
    w = [torch.zeros(s) for s in ((4, 1, 4, 4), (4,), (1, 4, 3, 3), (1,), (16, 576), (16,))]
    with pytest.raises(RuntimeError, match="must be on"):   # CPU tensors are refused, not dereferenced
        ops.policy_conv_features_backward(*w, torch.zeros(1, 2500), 2500, 1, torch.zeros(1, 16), *[torch.zeros_like(x) for x in w],
                                          torch.zeros(16))


def test_conv_features_is_an_autograd_function():
    assert issubclass(ln.ConvFeatures, torch.autograd.Function)
    assert ln.CONV_IMPLS == ("torch", "hip")


@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_learners_accept_conv_impl_and_refuse_it_with_the_reason(alg):
    cls = LEARNER[alg]
    assert cls(learner_args(alg, 3, 6), device="cpu", unroll="torch", conv_impl="torch").conv_impl == "torch"
    assert cls(learner_args(alg, 3, 6), device="cpu", unroll="torch").conv_impl == "torch"
    with pytest.raises(ValueError, match="conv_impl must be"):
        cls(learner_args(alg, 3, 6), device="cpu", unroll="torch", conv_impl="miopen")
    with pytest.raises(ValueError, match="unroll='fused'"):
        cls(learner_args(alg, 3, 6), device="cuda", unroll="torch", conv_impl="hip")
    with pytest.raises(ValueError, match="GPU"):
        cls(learner_args(alg, 3, 6), device="cpu", unroll="fused", conv_impl="hip")
    other = learner_args(alg, 3, 6)
    other.kernel_size_1 = 6
    with pytest.raises(ValueError, match="kernel_size_1"):   # (refused before the device is touched)
        cls(other, device="cuda", unroll="fused", conv_impl="hip")
    easy = learner_args(alg, 3, 6)
    easy.conv = False
    with pytest.raises(ValueError, match="conv front end"):
        cls(easy, device="cuda", unroll="fused", conv_impl="hip")


def test_runner_passes_args_conv_impl_to_the_learner(monkeypatch):
    seen = []

    class Stop(Exception):
        pass

    def fake(args, device, **kw):
        seen.append(kw)
        raise Stop
    monkeypatch.setitem(rn.LEARNERS, "qmix", fake)
    for value, want in ((None, "torch"), ("hip", "hip")):
        args = learner_args("qmix", 3, 6)
        if value is not None:
            args.conv_impl = value
        with pytest.raises(Stop):
            rn.Runner(type("Env", (), {"batch": 1, "device": "cpu"})(), args)
        assert seen[-1] == {"conv_impl": want}


@pytest.mark.parametrize("alg", ["qmix", "dop", "reinforce"])
def test_conv_impl_torch_is_the_default_bit_for_bit(alg):
    """One learn (unroll="torch", CPU) from equal weights on a dense and on a map-once batch: every parameter of every network
    is equal bit for bit with and without the argument."""
    n, T = 3, 6
    d = dense_batch([2, 6, 9, 4], T, n, seed=3)
    for batch in (d, compact_from_dense(d)):
        after = []
        for kw in ({}, {"conv_impl": "torch"}):
            lr = LEARNER[alg](learner_args(alg, n, T), device="cpu", unroll="torch", **kw)
            lr.learn(batch, None, 0, *(() if alg == "qmix" else (0.3,)))
            after.append({f"{m}.{k}": v for m in NETS[alg] for k, v in getattr(lr, m).state_dict().items()})
        assert after[0].keys() == after[1].keys() and any(k.endswith("conv.0.weight") for k in after[0])
        for k in after[0]:
            assert torch.equal(after[0][k], after[1][k]), k
