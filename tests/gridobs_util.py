"""Shared by the grid-observation tests (gridobs.py, csrc/gridobs.h): grids in the states the kernels must
read correctly, a plain-Python statement of one probe sum, and the float64 twin of the grid student's forward."""
import numpy as np
import torch

from cooperative_search_amd import baseline as bl
from cooperative_search_amd import belief as be
from cooperative_search_amd import gridobs as go
from cooperative_search_amd import motion as mo
from imitate_util import KEEP, state_rows

# (n, side, view_range, lookahead): one agent; the env's shape; lookahead 0 with five agents; everything at its maximum (the whole
# map under every probe, eight agents: 128 probes); a 7 x 7 map with view_range 0 (fewer cells than threads, empty boxes); a
# full-size map with the far ring well off it (every outer probe clamped at a wall)
FEATURE_CASES = [(1, 50, 7, 7), (3, 50, 7, 7), (5, 50, 7, 0), (8, 64, 64, 64), (2, 7, 0, 7), (3, 64, 7, 64)]


def rows(B, n, S, seed, spoil=False):
    """float32 [B, S]: one state row per env (imitate_util.state_rows with T = 1)."""
    return state_rows(B, 1, n, S, seed, spoil=spoil)[:, 0].contiguous()


def grids(kind, state, n, side, vr, look, seed=0):
    """int32 [B, side * side] in one of the states a caller can hand over: "fresh"; "coverage" / "belief": flown for three steps
    by that filter's definition on random rows, the last of them `state`; "cap": CAP everywhere; "wild": cells above CAP, below 0
    and at both int32 ends among ordinary ones."""
    B, cells = int(state.shape[0]), side * side
    grid = torch.full((B, cells), bl.FRESH, dtype=torch.int32)
    if kind == "fresh":
        return grid
    if kind == "cap":
        return torch.full((B, cells), be.CAP, dtype=torch.int32)
    if kind == "wild":
        rng = np.random.RandomState(100 + seed)
        g = rng.randint(0, be.CAP + 1, size=(B, cells)).astype(np.int64)
        bad = np.array([-1, -(1 << 31), (1 << 31) - 1, be.CAP + 1, 1 << 24, -be.CAP], dtype=np.int64)
        hit = rng.rand(B, cells) < 0.2
        g[hit] = bad[rng.randint(0, len(bad), size=int(hit.sum()))]
        return torch.from_numpy(g.astype(np.int32))
    S = int(state.shape[1])
    steps = [rows(B, n, S, 50 + seed + k) for k in range(2)] + [state]
    prev = torch.zeros(B, 8, 2, dtype=torch.int32)
    model = be.BeliefModel.from_motion(mo.TargetMotion(mode="evade", speed=1.0, sense=5.0), side)
    for k, row in enumerate(steps):
        if kind == "coverage":
            bl.coverage_actions_torch(row, grid, n, side, vr, KEEP, 8, look)
        else:
            be.belief_actions_torch(row, grid, prev, n, side, vr, KEEP, model, 1 if k else 0, look)
    return grid


def probe_sum_python(state_row, grid_row, i, k, n, side, vr, look):
    """sum_k of agent i in plain Python integers, from the module docstring's text: the one place the probe geometry is written
    a second time."""
    X, Y, h = (int(v[0, i]) for v in bl.quantise(state_row.view(1, -1), n, side))
    ct, st = bl.trig_tables()
    hp = (h + go.REL[k % 8]) % 36
    d16 = go.DIST[k // 8] * 16 * look
    px = min(max(X + ((d16 * ct[hp]) >> 14), 0), 16 * side)
    py = min(max(Y + ((d16 * st[hp]) >> 14), 0), 16 * side)
    total, R2 = 0, (16 * vr) ** 2
    g = grid_row.tolist()
    for ix in range(side):
        for iy in range(side):
            if (16 * ix + 8 - px) ** 2 + (16 * iy + 8 - py) ** 2 <= R2:
                total += min(max(g[ix * side + iy], 0), be.CAP)
    return total


def same_bits(a, b):
    """torch.equal on the int32 views of two float32 tensors (so that -0.0 and +0.0, or two NaNs, cannot pass for each other)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the grid student's forward ------------------------------------------------------------------------------------------------------

FORWARD_SEED = 11   # chosen on the CPU (test_gridobs_cpu.py): the float64 twin alone leaves >= 90 % of the rows a top-2 gap above 1e-3


def forward_case(args, n, B, steps=6, seed=FORWARD_SEED):
    """An AgentRNN of the grid student's width with weights scaled by 3 (test_gpu_policy.py's case) and `steps` steps of inputs:
    features float32 [steps, B, n, 16] in the range the kernel produces (0 .. 1.2 on a fresh map at view_range 7), obs float32
    [steps, B, n, 4] in -1..1 -> (net, features, obs)."""
    import cooperative_search_amd as cs
    torch.manual_seed(seed)
    net = cs.AgentRNN(cs.rnn_input_shape(args) + go.PROBES, args)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    g = torch.Generator().manual_seed(seed + 1)
    feats = torch.rand(steps, B, n, go.PROBES, generator=g) * 1.2
    obs = torch.rand(steps, B, n, 4, generator=g) * 2 - 1
    return net, feats, obs


def twin_of(net, dtype):
    """A copy of the module in `dtype` on the CPU."""
    import copy
    return copy.deepcopy(net).to("cpu", dtype)


def twin_step(m, feat, obs, last, h, n, A):
    """One step of the module `m` on rows [features | obs | one-hot(last action, -1 = none) | one-hot(agent id)]: feat [B, n, 16],
    obs [B, n, 4], last int64 [B, n], h [B * n, 64] -> (q [B * n, A], h' [B * n, 64]) in m's dtype."""
    dtype = m.fc1.weight.dtype
    B = int(feat.shape[0])
    onehot = torch.nn.functional.one_hot(last.clamp(min=0), A).to(dtype) * (last >= 0).unsqueeze(2).to(dtype)
    ids = torch.eye(n, dtype=dtype).expand(B, n, n)
    x = torch.cat([feat.to(dtype), obs.to(dtype), onehot, ids], 2).reshape(B * n, -1)
    with torch.no_grad():
        return m(x, h.to(dtype))


def clear_fraction(q):
    """The share of rows of q [rows, A] whose top-2 gap exceeds 1e-3, and the mask."""
    top2 = q.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3
    return float(clear.double().mean()), clear
