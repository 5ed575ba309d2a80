"""Shared by tests/test_local_belief_cpu.py and tests/test_gpu_local_belief.py: motion models, the state tensors of
LocalBeliefAgents (local_belief.py, csrc/local_belief.h) and the definition run over a sequence of calls.  The state rows are
local_util's."""
import torch

from cooperative_search_amd import belief as be
from cooperative_search_amd import local_belief as lb
from cooperative_search_amd import motion as mo
from local_util import KEEP

CAP = be.CAP
FAR = -(1 << 15)   # where identity D parks an agent that was not heard: farther than any sense16 from every cell centre


def model(mode="evade", speed=1.0, sense=10.0, side=50):
    return be.BeliefModel.from_motion(mo.TargetMotion(mode=mode, speed=speed, sense=sense), side)


def moved_at(t):
    """The targets stand still before the first call of a sequence and move before every later one."""
    return 1 if t > 0 else 0


def random_prev(B, side, seed):
    """int32 [B, 8, 2]: positions on the map, a quarter of them off it (beyond the +-2^15 clamp too)."""
    g = torch.Generator().manual_seed(seed)
    prev = torch.randint(0, 16 * side + 1, (B, 8, 2), generator=g, dtype=torch.int32)
    off = torch.randint(-40000, 40000, (B, 8, 2), generator=g, dtype=torch.int32)
    return torch.where(torch.rand(B, 8, 1, generator=g) < 0.25, off, prev)


def random_heard(B, seed):
    """int32 [B, 8] over all 32 bits: garbage above bit n - 1, own bits set or not."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31, (B, 8), generator=g, dtype=torch.int64).to(torch.int32)


def own_bits(B):
    """int32 [B, 8]: every agent heard itself alone."""
    return (1 << torch.arange(8, dtype=torch.int32)).expand(B, 8).contiguous()


def run_definition(states, grids, prev, heard, n, side, vr, mdl, comm, moved=moved_at, lookahead=None):
    """The definition over consecutive calls from (grids, prev, heard), none of them modified -> [(grids, prev, heard, actions), ...]
    after each call.  moved: a function of the call index."""
    g, p, h, out = grids.clone(), prev.clone(), heard.clone(), []
    for t, s in enumerate(states):
        a = lb.local_belief_actions_torch(s, g, p, h, n, side, vr, KEEP, mdl, moved(t), comm, lookahead)
        out.append((g.clone(), p.clone(), h.clone(), a))
    return out
