"""The grid policies' definitions against their own record (tests/golden/grid_defs.npz, written by tests/golden/gen_grid_defs.py):
the recorded states go through `coverage_actions_torch`, `belief_actions_torch` (walk and evade, `moved` alternating),
`local_coverage_actions_torch` (comm_range -1, 0, 4), `plan_actions_torch`, `sweep_episodes_torch` and `label_episodes_torch` again,
and every action, score, plan, grid and stored position must equal the record exactly.  The kernels are tested bit for bit against
these definitions; this is what holds the definitions themselves in place."""
import importlib.util
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def replayed():
    """(the record, what the definitions give today for the recorded states), both {name: array}; computed once."""
    spec = importlib.util.spec_from_file_location("gen_grid_defs", os.path.join(GOLDEN, "gen_grid_defs.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    before = torch.get_num_threads()
    torch.set_num_threads(1)   # the tensors are small: the thread pool only costs time on them
    try:
        with np.load(os.path.join(GOLDEN, "grid_defs.npz")) as z:
            want = {k: z[k] for k in z.files}
        return want, gen.record(list(torch.from_numpy(want["states"])))
    finally:
        torch.set_num_threads(before)


def test_the_record_is_complete(replayed):
    want, got = replayed
    assert sorted(want) == sorted(got) and len(want) == 33
    assert want["states"].shape == (6, 4, 17) and want["states"].dtype == np.float32


@pytest.mark.parametrize("family", ["coverage", "belief_walk", "belief_evade", "local_inf", "local_0", "local_4", "plan", "sweep",
                                    "label_coverage", "label_belief"])
def test_definitions_reproduce_the_record_exactly(replayed, family):
    want, got = replayed
    names = [k for k in want if k.startswith(family + "_")]
    assert names
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k
