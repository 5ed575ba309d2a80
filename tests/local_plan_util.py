"""Shared by tests/test_local_plan_cpu.py and tests/test_gpu_local_plan.py: the shapes and ranges both files use, and the planner on
private grids restated per env and per agent with links, claim points and claimed discs in plain Python integers (only the lone
agent's search is plan.plan_actions_torch, which tests/test_plan_cpu.py holds against a brute force)."""
import torch

from cooperative_search_amd import plan as pl
from local_util import disc, landed, random_grids, walk

SHAPES = [(3, 3, 50, 7), (2, 8, 64, 7), (5, 2, 7, 2)]      # B, n, side, view_range
PARAMS = [(4, 3, 230), (2, 4, 256)]                        # depth, stride, discount
MIXED = {(3, 3, 50): 15, (2, 8, 64): 20, (5, 2, 7): 3, (65, 5, 50): 20, (1, 1, 50): 10}   # a range that links some pairs and not others


def inputs(B, n, side):
    """Row 0 of walk(B, n, 1, seed 5) and random_grids(B, 1, side, 3) repeated over the agents."""
    return walk(B, n, 1, 5)[0], random_grids(B, 1, side, 3).expand(B, n, side * side).contiguous()


def points_by_hand(X, Y, h, s, side, depth, stride):
    """The `depth` segment end points of sequence s from pose (X, Y, h), in plain Python integers."""
    sx, sy = pl.step_tables()
    out = []
    for d in range(depth):
        turn = pl.TURN[(s // 3 ** (depth - 1 - d)) % 3]
        for _ in range(stride):
            h = (h + turn) % 36
            X = min(max(X + sx[h], 0), 16 * side)
            Y = min(max(Y + sy[h], 0), 16 * side)
        out.append((X, Y))
    return out


def by_hand(state, grids, n, side, vr, depth, stride, discount, comm):
    """(actions, plans, scores) int64 [B, n]: env by env and agent by agent, the lone agent's search on its own grid with the discs
    zeroed that the linked agents before it claimed."""
    from cooperative_search_amd import baseline as bl
    B = state.shape[0]
    pos = landed(state, n, side)
    head = bl.quantise(state, n, side)[2]
    out = torch.zeros(3, B, n, dtype=torch.int64)
    for b in range(B):
        claims = []
        for i in range(n):
            W = grids[b, i].clamp(0, pl.CAP).clone()
            for j in range(i):
                dx, dy = pos[b][i][0] - pos[b][j][0], pos[b][i][1] - pos[b][j][1]
                if comm < 0 or dx * dx + dy * dy < (16 * comm) ** 2:
                    W[claims[j]] = 0
            row = state[b:b + 1, 4 * i:4 * i + 4].contiguous()
            a, p, s = pl.plan_actions_torch(row, W.unsqueeze(0), 1, side, vr, depth, stride, discount, return_plans=True)
            out[0, b, i], out[1, b, i], out[2, b, i] = a[0, 0], p[0, 0], s[0, 0]
            mask = torch.zeros(side * side, dtype=torch.bool)
            for px, py in points_by_hand(pos[b][i][0], pos[b][i][1], int(head[b, i]), int(p[0, 0]), side, depth, stride):
                mask |= disc(px, py, side, vr)
            claims.append(mask)
    return out[0], out[1], out[2]
