#!/usr/bin/env python3
"""Time per learn step on one GPU: the fused learner (GRUSequence: one launch for the whole forward recurrence, one for its
backward; for DOP and REINFORCE also one cs_episode_returns launch for the returns) against the reference's per-step unroll over
the same modules (unroll="torch"; for DOP it includes the reference's O(T^2) lambda-return).  --alg: qmix (QMixLearner, the
default), dop (DOPLearner), reinforce (ReinforceLearner, here on sampled batches) or ppo (PPOLearner with its defaults: four
epochs per learn; flight_easy with 3 agents at E = 32 and 256 only, and cs_ppo_loss alone -- forward and backward of
PPOPolicyLoss -- against ppo_policy_loss_torch on the same rows).

Cases: flight_easy with 3 and 5 agents at E = 32, 256, 1024 sampled episodes, and flight with 3 agents at E = 32; T = 200 (the
full episode limit, as the reference learns).  The replay buffer is filled by EpisodeCollector with random actions, batches are
drawn by DeviceReplayBuffer.sample with a fixed generator, and each learn() is timed with HIP events after warm-up steps.
Prints ONE JSON line.

    python tools/learn_bench.py [--alg qmix|dop|reinforce|ppo] [--warmup 2] [--steps 5] [--quick] [--impl both|fused|torch]
                                [--max-episode-len N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("flight_easy", 3, 32), ("flight_easy", 3, 256), ("flight_easy", 3, 1024),
         ("flight_easy", 5, 32), ("flight_easy", 5, 256), ("flight_easy", 5, 1024), ("flight", 3, 32)]


ALGS = {"qmix": ("QMixLearner", "get_mixer_args"), "dop": ("DOPLearner", "get_dop_args"),
        "reinforce": ("ReinforceLearner", "get_reinforce_args"), "ppo": ("PPOLearner", "get_ppo_args")}
PPO_CASES = [("flight_easy", 3, 32), ("flight_easy", 3, 256)]


def time_learns(learner, batches, warmup, max_episode_len=None):
    import torch
    for b in batches[:warmup]:
        learner.learn(b, max_episode_len)
    torch.cuda.synchronize()
    ms = []
    for b in batches[warmup:]:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        learner.learn(b, max_episode_len)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return sorted(ms)[len(ms) // 2], min(ms)


def run_case(env_name, n, E, warmup, steps, impls=("fused", "torch"), alg="qmix", max_episode_len=None):
    import torch
    import cooperative_search_amd as cs
    learner_cls, args_fn = (getattr(cs, name) for name in ALGS[alg])
    args = cs.make_env_args(env_name, n_agents=n)
    B = E if env_name == "flight_easy" else 2 * E
    env = cs.BatchedFlightEnv(args, batch=B)
    cs.apply_env_info(args, env)
    args_fn(args, seed=1)
    rb = cs.DeviceReplayBuffer(args, B)
    g = torch.Generator("cuda").manual_seed(3)
    cs.EpisodeCollector(env).generate_episodes(policy=cs.random_policy(g), into=rb)
    batches = [rb.sample(E, generator=g) for _ in range(warmup + steps)]
    out = dict(env=env_name, n_agents=n, E=E, T=min(args.episode_limit, max_episode_len or args.episode_limit))
    for impl in impls:
        learner = learner_cls(args, device="cuda", unroll=impl)
        med, best = time_learns(learner, batches, warmup, max_episode_len)
        out[f"{impl}_ms"], out[f"{impl}_min_ms"] = round(med, 3), round(best, 3)
        del learner
    if len(impls) == 2:
        out["speedup"] = round(out["torch_ms"] / out["fused_ms"], 1)
    del rb, env, batches
    torch.cuda.empty_cache()
    return out


def time_ppo_loss(E, T=200, n=3, A=3, warmup=3, steps=10):
    """PPOPolicyLoss (cs_ppo_loss: one pass + a one-block reduction; backward = one multiply) against ppo_policy_loss_torch
    (autograd over action_prob / log_pi_taken), forward and backward, on the same random rows."""
    import torch
    from cooperative_search_amd.learner import PPOPolicyLoss, ppo_policy_loss_torch
    g = torch.Generator("cuda").manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    logits, avail = rnd(E, T, n, A).requires_grad_(True), torch.ones(E, T, n, A, device="cuda")
    u = torch.randint(0, A, (E, T, n, 1), device="cuda", generator=g)
    old_logp, adv, mask = torch.log_softmax(rnd(E, T, n, A), -1).gather(3, u).squeeze(3), rnd(E, T), torch.ones(E, T, device="cuda")
    inv_count = 1 / (n * mask.sum())

    def fused():
        loss, _ = PPOPolicyLoss.apply(logits, avail, u, old_logp, adv, mask, 0.2, 0.01, 0.0, inv_count)
        loss.backward()

    def twin():
        loss, _ = ppo_policy_loss_torch(logits, avail, u, old_logp, adv, mask, 0.2, 0.01, 0.0)
        loss.backward()
    out = dict(E=E, T=T, n_agents=n, rows=E * T * n)
    for name, fn in (("kernel", fused), ("torch", twin)):
        for _ in range(warmup):
            logits.grad = None
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            logits.grad = None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        out[f"{name}_ms"] = round(sorted(ms)[len(ms) // 2], 4)
    out["speedup"] = round(out["torch_ms"] / out["kernel_ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="only flight_easy 3 agents at E = 32")
    ap.add_argument("--impl", choices=("both", "fused", "torch"), default="both",
                    help="time one unroll only (e.g. under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--alg", choices=tuple(ALGS), default="qmix")
    ap.add_argument("--max-episode-len", type=int, default=None, help="learn on the first N steps of every batch")
    a = ap.parse_args()
    import torch
    t0 = time.time()
    cases = CASES[:1] if a.quick else PPO_CASES if a.alg == "ppo" else CASES
    impls = ("fused", "torch") if a.impl == "both" else (a.impl,)
    res = [run_case(*c, a.warmup, a.steps, impls, a.alg, a.max_episode_len) for c in cases]
    head = dict(tool="learn_bench")
    if a.alg != "qmix":   # the default keeps its output as it was
        head["alg"] = a.alg
    if a.alg == "ppo":
        head["ppo_loss"] = [time_ppo_loss(c[2]) for c in cases]
        head["ppo_loss_timer"] = "HIP events around loss forward + backward, median of 10"
    print(json.dumps(dict(head, device=torch.cuda.get_device_name(0), warmup=a.warmup, steps=a.steps,
                          timer="HIP events around learn(), median of the timed steps", cases=res,
                          wall_s=round(time.time() - t0, 1))))


if __name__ == "__main__":
    main()
