"""Shared by tests/test_local_forecast_cpu.py and tests/test_gpu_local_forecast.py: the shapes, parameters, `moves` patterns and inputs
both files use, the two definitions of local_forecast.py computed ONCE per case (cached, never modified), and both restated per env
and per agent in plain Python: the heard agents listed from the bits, forecast.forecast_torch on the compacted positions, the claimed
discs zeroed in every level (only the lone agent's forecast and search are forecast.py's, which tests/test_forecast_cpu.py pins)."""
import functools

import torch

from cooperative_search_amd import baseline as bl
from cooperative_search_amd import forecast as fc
from cooperative_search_amd import local_forecast as lf
from cooperative_search_amd import plan as pl
from local_belief_util import model, random_heard, random_prev
from local_plan_util import MIXED, PARAMS, SHAPES, points_by_hand
from local_util import disc, landed, walk

CAP = pl.CAP
PARAMS3 = PARAMS + [(5, 2, 200)]          # depth, stride, discount; depth 5 at side 64 is the 85 KB LDS path
SENSE = {50: 10.0, 64: 10.0, 7: 2.0}      # the evaders' sensing radius in cells, per side
# all ones; a zero first (level 0 is a copy of the clamped grid); one with MAX_STRIDE; a single level
MOVES = [(1, 1, 1, 1), (0, 1, 2, 0, 1), (1, pl.MAX_STRIDE, 1), (2,)]


def moves_for(depth):
    """The `moves` a plan test forecasts its stacks with: a zero first from depth 3 on, never all zero."""
    return ((1, 2) if depth < 3 else (0, 1, 2, 1, 1))[:depth]


def mdl(side, mode="evade"):
    return model(mode=mode, speed=1.0, sense=SENSE[side], side=side)


def extreme_grids(B, n, side, seed):
    """int32 [B, n, side * side]: a grid of its own per agent, densities in 0..2^17 with an eighth of the cells below 0 and an
    eighth above 2^19 (up to 2^31 - 1): both are read clamped."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, n, side * side)
    grids = torch.randint(0, 2 ** 17 + 1, shape, generator=g, dtype=torch.int32)
    kind = torch.rand(shape, generator=g)
    low = torch.randint(-2 ** 31, 0, shape, generator=g, dtype=torch.int64).to(torch.int32)
    high = torch.randint(CAP + 1, 2 ** 31, shape, generator=g, dtype=torch.int64).to(torch.int32)
    grids = torch.where(kind < 0.125, low, torch.where(kind > 0.875, high, grids))
    grids[:, :, 0], grids[:, :, -1] = -1, 2 ** 31 - 1
    return grids


@functools.lru_cache(maxsize=None)
def forecast_inputs(B, n, side):
    """(grids, prev, heard): extreme grids, prev beyond +-2^15, heard over all 32 bits.  Shared: never modified."""
    return extreme_grids(B, n, side, 11), random_prev(B, side, 12), random_heard(B, 13)


@functools.lru_cache(maxsize=None)
def forecast_case(B, n, side, moves, mode="evade"):
    """(grids, prev, heard, stacks): the inputs and the definition's forecast of them."""
    grids, prev, heard = forecast_inputs(B, n, side)
    return grids, prev, heard, lf.local_forecast_torch(grids, prev, heard, n, side, mdl(side, mode), moves)


def spoil(stacks, seed):
    """A copy with one cell in sixteen below 0 or above 2^19: a stack is read clamped."""
    g = torch.Generator().manual_seed(seed)
    kind = torch.rand(stacks.shape, generator=g)
    out = torch.where(kind < 1 / 32, torch.full_like(stacks, -3), torch.where(kind > 31 / 32, torch.full_like(stacks, 2 ** 31 - 1), stacks))
    return out.contiguous()


@functools.lru_cache(maxsize=None)
def plan_inputs(B, n, side, depth):
    """(state, stacks): row 0 of walk(B, n, 1, seed 5) and the forecast of forecast_inputs with moves_for(depth), spoilt."""
    return walk(B, n, 1, 5)[0], spoil(forecast_case(B, n, side, moves_for(depth))[3], 14)


@functools.lru_cache(maxsize=None)
def plan_case(B, n, side, vr, depth, stride, discount, comm):
    """(state, stacks, (actions, plans, scores)): the inputs and the definition's decision on them."""
    state, stacks = plan_inputs(B, n, side, depth)
    return state, stacks, lf.local_plan_forecast_actions_torch(state, stacks, n, side, vr, depth, stride, discount, comm, return_plans=True)


def heard_list(word, i, n):
    """The agents agent i knows of, from the bits of its heard word, in plain Python."""
    return [j for j in range(n) if j == i or (int(word) >> j) & 1]


def forecast_by_hand(grids, prev, heard, n, side, model_, moves):
    """stacks int32 [B, n, L, cells]: env by env and agent by agent, forecast_torch on the compacted positions of the heard agents with
    n_agents = their number."""
    B = grids.shape[0]
    out = torch.zeros(B, n, len(moves), side * side, dtype=torch.int32)
    for b in range(B):
        for i in range(n):
            known = heard_list(heard[b, i], i, n)
            pos = torch.zeros(1, 8, 2, dtype=torch.int32)
            pos[0, :len(known)] = prev[b, known]
            out[b, i] = fc.forecast_torch(grids[b:b + 1, i], pos, len(known), side, model_, moves)[0]
    return out


def plan_by_hand(state, stacks, n, side, vr, depth, stride, discount, comm):
    """(actions, plans, scores) int64 [B, n]: env by env and agent by agent, the lone agent's search on its own levels with the discs
    zeroed, in every level, that the linked agents before it claimed."""
    B = state.shape[0]
    pos = landed(state, n, side)
    head = bl.quantise(state, n, side)[2]
    out = torch.zeros(3, B, n, dtype=torch.int64)
    for b in range(B):
        claims = []
        for i in range(n):
            W = stacks[b, i].clamp(0, CAP).clone()
            for j in range(i):
                dx, dy = pos[b][i][0] - pos[b][j][0], pos[b][i][1] - pos[b][j][1]
                if comm < 0 or dx * dx + dy * dy < (16 * comm) ** 2:
                    W[:, claims[j]] = 0
            row = state[b:b + 1, 4 * i:4 * i + 4].contiguous()
            a, p, s = fc.plan_forecast_actions_torch(row, W.unsqueeze(0), 1, side, vr, depth, stride, discount, return_plans=True)
            out[0, b, i], out[1, b, i], out[2, b, i] = a[0, 0], p[0, 0], s[0, 0]
            mask = torch.zeros(side * side, dtype=torch.bool)
            for px, py in points_by_hand(pos[b][i][0], pos[b][i][1], int(head[b, i]), int(p[0, 0]), side, depth, stride):
                mask |= disc(px, py, side, vr)
            claims.append(mask)
    return out[0], out[1], out[2]


__all__ = ["CAP", "MIXED", "MOVES", "PARAMS3", "SENSE", "SHAPES", "extreme_grids", "forecast_by_hand", "forecast_case", "forecast_inputs",
           "heard_list", "mdl", "moves_for", "plan_by_hand", "plan_case", "plan_inputs", "spoil"]
