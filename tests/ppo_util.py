"""Shared by the PPO learner's CPU and GPU tests: NumPy statements of cs_gae (csrc/ppo.h), the data they run on, the cases of
the loss kernel with their float64 yardstick, and the learner's namespace."""
import types

import numpy as np
import torch

from cooperative_search_amd.learner import get_ppo_args, ppo_policy_loss_torch


def gae_f32(r, term, pad, v, vn, gamma, lam):
    """csrc/ppo.h's evaluation order in NumPy float32, one operation at a time -> (adv, ret) [E, T]."""
    f = np.float32
    r, term, pad, v, vn = (x.astype(f) for x in (r, term, pad, v, vn))
    g = f(gamma)
    gl = g * f(lam)
    c, m = f(1) - term, f(1) - pad
    T = r.shape[1]
    adv = np.zeros_like(r)
    acc = None
    for t in range(T - 1, -1, -1):
        delta = (r[:, t] + (g * vn[:, t]) * c[:, t]) - v[:, t]
        acc = delta * m[:, t] if t == T - 1 else (delta + (gl * acc) * c[:, t]) * m[:, t]
        adv[:, t] = acc
    return adv, (adv + v) * m


def gae_f64(r, term, pad, v, vn, gamma, lam):
    """The same formulas in float64."""
    r, term, pad, v, vn = (x.astype(np.float64) for x in (r, term, pad, v, vn))
    c, m = 1 - term, 1 - pad
    T = r.shape[1]
    adv = np.zeros_like(r)
    acc = np.zeros(r.shape[0])
    for t in range(T - 1, -1, -1):
        delta = r[:, t] + gamma * vn[:, t] * c[:, t] - v[:, t]
        acc = (delta + gamma * lam * acc * c[:, t]) * m[:, t]
        adv[:, t] = acc
    return adv, (adv + v) * m


def gae_case(E, T, seed):
    """Data shaped like the returns kernel's test: random integer rewards, episodes of random length with a padded tail, some
    terminated (terminated = 1 on their last step and, as the collector writes them, on the padding), others cut at their
    length; values ~ N(0, 20).  Rewards and values also sit on the padded steps (garbage there)."""
    rng = np.random.RandomState(seed)
    r = rng.randint(-3, 6, size=(E, T)).astype(np.float32)
    v = (rng.randn(E, T) * 20).astype(np.float32)
    vn = (rng.randn(E, T) * 20).astype(np.float32)
    lengths = rng.randint(1, T + 1, size=E)
    lengths[rng.rand(E) < 0.3] = T
    live = np.arange(T)[None, :] < lengths[:, None]
    ends = rng.rand(E) < 0.5
    term = np.where(live, 0.0, 1.0).astype(np.float32)
    term[ends, lengths[ends] - 1] = 1.0
    return r, term, (~live).astype(np.float32), v, vn


CLIP = 0.2
# (E, T, n): R = E T n = 1, 45, 70, 195, 1080 rows -- a partial wavefront, a partial block, several blocks; each with epsilon in
# EPSILONS and the entropy coefficient in BETAS.  UNAVAILABLE: the shape whose live rows lose actions.  SEED was
# checked on the CPU: loss_case's conditions hold with it for every case.
LOSS_SHAPES = [(1, 1, 1), (3, 5, 3), (2, 7, 5), (5, 13, 3), (9, 40, 3)]
EPSILONS, BETAS = (0.0, 0.3), (0.0, 0.01)
UNAVAILABLE = (5, 13, 3)
SEED = 0
A = 3
# The other row widths k_ppo_loss<A> is instantiated for (ppo_launch, csrc/policy.hip: 2 .. 8): the smallest, the two next to the
# tested 3, the largest; on a partial block and on several wavefronts, with the entropy term on.  loss_case's conditions depend on
# the draw, so every (A, shape, epsilon) has its own seed: the smallest one for which they hold, found on the CPU
# (test_learner_ppo_cpu.test_loss_twin_in_float32_matches_float64_at_every_width checks them again).  With A = 2 the rows that lose
# an action keep one: p = 1, entropy 0, log p = 0 -- the edge of the kernel's p_a > 0 guards.
WIDTHS = (2, 4, 5, 8)
WIDTH_SHAPES = [(3, 5, 3), (5, 13, 3)]
WIDTH_BETA = 0.01
WIDTH_SEEDS = {   # (A, (E, T, n), epsilon): seed
    (2, (3, 5, 3), 0.0): 1, (2, (3, 5, 3), 0.3): 2, (2, (5, 13, 3), 0.0): 0, (2, (5, 13, 3), 0.3): 19,
    (4, (3, 5, 3), 0.0): 0, (4, (3, 5, 3), 0.3): 1, (4, (5, 13, 3), 0.0): 0, (4, (5, 13, 3), 0.3): 0,
    (5, (3, 5, 3), 0.0): 0, (5, (3, 5, 3), 0.3): 2, (5, (5, 13, 3), 0.0): 1, (5, (5, 13, 3), 0.3): 0,
    (8, (3, 5, 3), 0.0): 1, (8, (3, 5, 3), 0.3): 1, (8, (5, 13, 3), 0.0): 0, (8, (5, 13, 3), 0.3): 0,
}
WIDTH_CASES = [(A_, E, T, n, eps) for A_ in WIDTHS for (E, T, n) in WIDTH_SHAPES for eps in EPSILONS]


def loss_inputs(E, T, n, unavailable, seed, A=A):
    """float64 CPU tensors of one case: logits ~ N(0, 1.5); episodes of random length (padded rows: avail all zero, garbage
    logits / old_logp / adv); `unavailable`: a third of the live rows lose one action other than the one taken; old_logp: the
    log-probability of u under logits perturbed by N(0, 0.6) (filled in by loss_case, which knows epsilon).  A: the row width
    (with A = 3 the draws are the ones the existing cases have always had)."""
    rng = np.random.RandomState(1000 + seed)
    logits = rng.randn(E, T, n, A) * 1.5
    lengths = rng.randint(1, T + 1, size=E)
    if E > 1:
        lengths[0] = T
    live = (np.arange(T)[None, :] < lengths[:, None])
    u = rng.randint(0, A, size=(E, T, n, 1))
    avail = np.ones((E, T, n, A))
    if unavailable:
        drop = (u[..., 0] + 1 + rng.randint(0, A - 1, size=(E, T, n))) % A   # never the action taken
        hit = rng.rand(E, T, n) < 1 / 3
        e, t, k = np.nonzero(hit)
        avail[e, t, k, drop[e, t, k]] = 0.0
    avail *= live[:, :, None, None]
    adv = rng.randn(E, T)
    noise = rng.randn(E, T, n, A) * 0.6
    garbage = rng.randn(E, T, n) * 3
    t64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return dict(logits=t64(logits), avail=t64(avail), u=torch.from_numpy(u), adv=t64(adv), mask=t64(live.astype(np.float64)),
                noise=t64(noise), garbage=t64(garbage), unavailable=unavailable)


def twin(x, dtype, epsilon, beta):
    """ppo_policy_loss_torch on the CPU in `dtype` -> (loss, stats [4], dlogits, outside-the-clip-range count), float64."""
    c = lambda k: x[k].to(dtype)
    logits = c("logits").clone().requires_grad_(True)
    loss, stats = ppo_policy_loss_torch(logits, c("avail"), x["u"], c("old_logp"), c("adv"), c("mask"), CLIP, beta, epsilon)
    loss.backward()
    live_rows = float(x["mask"].sum()) * logits.shape[2]
    return loss.detach().double(), stats.double(), logits.grad.double(), int(round(float(stats[2]) * live_rows))


def loss_case(E, T, n, epsilon, beta, A=A, seed=None):
    """One case (LOSS_SHAPES x EPSILONS x BETAS at A = 3, seed SEED; WIDTH_CASES at WIDTH_BETA with the seed WIDTH_SEEDS names;
    `seed` overrides either: the search for those seeds) with its float64 yardstick, after asserting from that yardstick that (a) each of
    the four classes (advantage sign x ratio inside / outside the clip range) holds at least 10 % of the live rows (the one-row case
    is exempt) and (b) no live row's ratio lies within 1e-4 of 1 +- CLIP: float32 then decides every row's branch as float64
    does and no row needs to be left out."""
    from cooperative_search_amd.learner import action_prob, log_pi_taken
    unavailable = (E, T, n) == UNAVAILABLE
    if seed is None:
        seed = SEED if A == 3 else WIDTH_SEEDS[(A, (E, T, n), epsilon)]
    x = loss_inputs(E, T, n, unavailable, seed, A)
    m3 = x["mask"].reshape(E, T, 1).expand(E, T, n)
    old = log_pi_taken(action_prob(x["logits"] + x["noise"], x["avail"], epsilon), x["u"], m3)
    x["old_logp"] = torch.where(m3 > 0, old, x["garbage"])
    logp = log_pi_taken(action_prob(x["logits"], x["avail"], epsilon), x["u"], m3)
    ratio = torch.exp(logp - x["old_logp"])
    live = m3 > 0
    assert float(torch.minimum((ratio - (1 - CLIP)).abs(), (ratio - (1 + CLIP)).abs())[live].min()) > 1e-4
    if E * T * n > 1:
        outside = (ratio < 1 - CLIP) | (ratio > 1 + CLIP)
        pos = (x["adv"] > 0).reshape(E, T, 1).expand(E, T, n)
        for sign in (pos, ~pos):
            for where in (outside, ~outside):
                assert float((sign & where & live).sum()) >= 0.1 * float(live.sum()), (E, T, n, seed)
    if unavailable:
        assert bool(((x["avail"].sum(-1) < A) & live).any())
    x["want"] = twin(x, torch.float64, epsilon, beta)
    return x


def rel_err(got, want):
    """Relative Frobenius error."""
    return float((got.double() - want).norm() / want.norm())


def ppo_args(env_fields, seed, **over):
    """The learner's namespace: env fields (a dict or a namespace) + get_ppo_args + overrides."""
    a = types.SimpleNamespace(**(env_fields if isinstance(env_fields, dict) else vars(env_fields)))
    get_ppo_args(a, seed=seed)
    a.alg = "ppo"
    for k, v in over.items():
        setattr(a, k, v)
    return a
