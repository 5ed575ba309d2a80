#!/usr/bin/env python3
"""Record what the grid policies' DEFINITIONS compute, call by call, as tests/golden/grid_defs.npz.

The definitions (`coverage_actions_torch`, `belief_actions_torch`, `local_coverage_actions_torch`, `plan_actions_torch`,
`sweep_episodes_torch`, `label_episodes_torch`) are the bit-exact statements the kernels are tested against; this fixture holds the
definitions themselves in place.  tests/test_grid_defs_cpu.py replays the recorded states through them and asserts equality, so a
rewrite that shares code between them cannot move a bit unnoticed.  Regenerate it only from a commit whose definitions are known
good, and say which one in the commit message:

    python tests/golden/gen_grid_defs.py

The inputs: flight_easy's constants (detect_prob 0.9, regrow 8) on a map shrunk to side 12 with view_range 3, 3 agents, B = 4
envs, six consecutive calls from fresh grids.  Envs 0 and 1 are a seeded random walk that runs past the walls; env 2 keeps agent 0
in the far corner heading into it (its three look-ahead points clamp to one point: a three-way tie, at a wall) and agent 1 on a
wall; env 3 keeps agents 0 and 1 on one pose.  The file needs no GPU and reads nothing outside the repository.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from cooperative_search_amd import _lib  # noqa: E402
from cooperative_search_amd import baseline as bl  # noqa: E402
from cooperative_search_amd import belief as be  # noqa: E402
from cooperative_search_amd import imitate as im  # noqa: E402
from cooperative_search_amd import local as lc  # noqa: E402
from cooperative_search_amd import motion as mo  # noqa: E402
from cooperative_search_amd import plan as pl  # noqa: E402
from cooperative_search_amd import sweep as sw  # noqa: E402

SIDE, VR, N, B, CALLS, TAIL = 12, 3, 3, 4, 6, 5
KEEP = bl.keep_of(0.9)
COMMS = (-1, 0, 4)
DEPTH, STRIDE, DISCOUNT = 2, 2, 230
LENS = (6, 4, 0, 5)   # the live rows of the four episodes for sweep_episodes_torch and label_episodes_torch
MODELS = {"walk": mo.TargetMotion(mode="walk", speed=0.8, every=2), "evade": mo.TargetMotion(mode="evade", speed=1.3, every=2, sense=4.0)}


def pose(X, Y, k):
    """(xn, yn, cos, sin) float32 of a quantised position (sub-units of 1/16 cell) and a heading index of 0..35."""
    a = np.float32(k * math.pi / 18)
    return [X / (8.0 * SIDE) - 1.0, Y / (8.0 * SIDE) - 1.0, float(np.cos(a, dtype=np.float32)), float(np.sin(a, dtype=np.float32))]


def states():
    """CALLS state rows float32 [B, 4 N + TAIL] (module docstring)."""
    g = torch.Generator().manual_seed(20)
    pos = torch.rand(B, N, 2, generator=g, dtype=torch.float64) * 2 - 1
    k = torch.randint(0, 36, (B, N), generator=g)
    out = []
    for t in range(CALLS):
        k = (k + torch.randint(-1, 2, (B, N), generator=g)) % 36
        k = torch.where((pos.abs() > 1.2).any(-1), (k + 18) % 36, k)
        ang = (k.to(torch.float64) * (math.pi / 18)).to(torch.float32)
        c, s = torch.cos(ang), torch.sin(ang)
        pos = pos + (2.0 / SIDE) * torch.stack([c, s], -1).to(torch.float64)   # one cell per call, not stopped by the walls
        ag = torch.cat([pos.to(torch.float32), c[..., None], s[..., None]], -1)
        ag[2, 0] = torch.tensor(pose(16 * SIDE, 16 * SIDE, 4 + t % 2))          # the far corner, heading into it
        ag[2, 1] = torch.tensor(pose(0, 16 * (3 + t), 9))                        # along the x = 0 wall
        ag[3, 1] = ag[3, 0]                                                      # two agents on one pose
        out.append(torch.cat([ag.reshape(B, 4 * N), torch.rand(B, TAIL, generator=g)], 1).to(torch.float32).contiguous())
    return out


def fresh(*shape):
    return torch.full(shape, bl.FRESH, dtype=torch.int32)


def record(rows=None):
    """{name: array}: the inputs (rows: the CALLS state rows, default `states()`) and, per call, everything each definition
    returns or updates."""
    rows = states() if rows is None else rows
    out = {"states": torch.stack(rows), "lens": torch.tensor(LENS, dtype=torch.int32)}
    ties, walls = {}, {}

    def note(name, scores, state):
        top = scores.max(-1, keepdim=True).values
        ties[name] = ties.get(name, False) or bool(((scores == top).sum(-1) >= 2).any())
        X, Y = bl.quantise_positions(state, N, SIDE)
        walls[name] = walls.get(name, False) or bool(((X == 0) | (X == 16 * SIDE) | (Y == 0) | (Y == 16 * SIDE)).any())

    def stack(name, calls):
        for key in calls[0]:
            out[f"{name}_{key}"] = torch.stack([c[key] for c in calls])

    grid, calls, plans = fresh(B, SIDE * SIDE), [], []
    for s in rows:
        a, sc = bl.coverage_actions_torch(s, grid, N, SIDE, VR, KEEP, return_scores=True)
        calls.append({"actions": a, "scores": sc, "grid": grid.clone()})
        note("coverage", sc, s)
        # the planner reads the grid coverage left (its tie is checked below: it returns the winner's score only)
        pa, pp, ps = pl.plan_actions_torch(s, grid, N, SIDE, VR, DEPTH, STRIDE, DISCOUNT, return_plans=True)
        plans.append({"actions": pa, "plans": pp, "scores": ps})
    stack("coverage", calls)
    stack("plan", plans)

    for mode, motion in MODELS.items():
        model = be.BeliefModel.from_motion(motion, SIDE)
        grid, prev, calls = fresh(B, SIDE * SIDE), torch.zeros(B, _lib.MAX_AGENTS, 2, dtype=torch.int32), []
        for t, s in enumerate(rows):
            a, sc = be.belief_actions_torch(s, grid, prev, N, SIDE, VR, KEEP, model, t % 2, return_scores=True)
            calls.append({"actions": a, "scores": sc, "grid": grid.clone(), "prev": prev.clone()})
            note(f"belief_{mode}", sc, s)
        stack(f"belief_{mode}", calls)

    for comm in COMMS:
        grids, calls = fresh(B, N, SIDE * SIDE), []
        for s in rows:
            a, sc = lc.local_coverage_actions_torch(s, grids, N, SIDE, VR, KEEP, comm, return_scores=True)
            calls.append({"actions": a, "scores": sc, "grids": grids.clone()})
            note(f"local_{comm}", sc, s)
        stack("local_" + ("inf" if comm < 0 else str(comm)), calls)

    episodes = out["states"].transpose(0, 1).contiguous()   # [E = B, T = CALLS, S]
    res = sw.sweep_episodes_torch(episodes, out["lens"], N, SIDE, VR)
    out.update(sweep_first=res.first, sweep_new_cells=res.new_cells, sweep_seen_cells=res.seen_cells)
    experts = {"coverage": im.ExpertParams(im.COVERAGE, N, SIDE, VR, KEEP),
               "belief": im.ExpertParams(im.BELIEF, N, SIDE, VR, KEEP, model=be.BeliefModel.from_motion(MODELS["evade"], SIDE),
                                         every=2, moving=1)}
    for name, params in experts.items():
        labels, grid_out, prev_out = im.label_episodes_torch(episodes, out["lens"], params)
        out.update({f"label_{name}_labels": labels, f"label_{name}_grid": grid_out})
        if prev_out is not None:
            out[f"label_{name}_prev"] = prev_out

    # every policy meets a tie between two actions and an agent at a wall at least once; checked, not eyeballed
    for name in ties:
        assert ties[name], f"{name}: no call has two actions sharing the top score"
        assert walls[name], f"{name}: no call has an agent at a wall"
    # the planner: env 2's corner agent cannot leave the corner, so every one of its 9 sequences sweeps the same disc and scores
    # the same; the lowest sequence (0) must have won each time
    X, Y = bl.quantise_positions(rows[0], N, SIDE)
    assert (int(X[2, 0]), int(Y[2, 0])) == (16 * SIDE, 16 * SIDE)
    one = pl.plan_actions_torch(rows[0][2:3, :4].contiguous(), fresh(1, SIDE * SIDE), 1, SIDE, VR, 1, STRIDE, DISCOUNT, return_plans=True)
    two = pl.plan_actions_torch(rows[0][2:3, :4].contiguous(), fresh(1, SIDE * SIDE), 1, SIDE, VR, DEPTH, STRIDE, DISCOUNT, return_plans=True)
    assert int(one[2]) == int(two[2]) and int(two[1]) == 0, "plan: the corner agent's sequences do not tie"
    assert bool((out["plan_plans"][:, 2, 0] == 0).all())
    return {k: v.numpy() for k, v in out.items()}


if __name__ == "__main__":
    torch.set_num_threads(1)
    path = os.path.join(HERE, "grid_defs.npz")
    np.savez_compressed(path, **record())
    print(path, os.path.getsize(path), "bytes")
