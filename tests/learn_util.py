"""The QMIX learner fixture (tests/golden/learn_easy3*.npz, written by tests/golden/gen_learn.py): batch rebuild and loaders."""
import json
import os
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("o", "u", "s", "r", "o_next", "s_next", "avail_u", "avail_u_next", "u_onehot", "padded", "terminated")


def rebuild_batch(z, n_actions):
    """The 11 keys of a sampled batch (common/rollout.py:66-132 padding) from the compact form: o_full / s_full [E][T+1][...]
    (obs / state of every step and of the step after the last), u [E][T][n], r / term [E][T], lengths [E].  u comes back as
    int64, everything else as float32 -- the types the learner converts them to."""
    o_full, s_full, lengths = z["o_full"], z["s_full"], z["lengths"]
    E, T = int(o_full.shape[0]), int(o_full.shape[1]) - 1
    live = (np.arange(T)[None, :] < lengths[:, None])                       # [E][T]
    lv = live.astype(np.float32)
    o = o_full[:, :T] * lv[:, :, None, None]
    s = s_full[:, :T] * lv[:, :, None]
    o_next = o_full[:, 1:] * lv[:, :, None, None]
    s_next = s_full[:, 1:] * lv[:, :, None]
    u = np.where(live[:, :, None], z["u"].astype(np.int64), 0)
    onehot = np.eye(n_actions, dtype=np.float32)[u] * lv[:, :, None, None]
    avail = np.broadcast_to(lv[:, :, None, None], onehot.shape).astype(np.float32)
    term = np.where(live, z["term"].astype(np.float32), 1.0).astype(np.float32)
    return {"o": o.astype(np.float32), "u": u[..., None], "s": s.astype(np.float32),
            "r": (z["r"] * lv)[..., None].astype(np.float32), "o_next": o_next.astype(np.float32),
            "s_next": s_next.astype(np.float32), "avail_u": avail, "avail_u_next": avail.copy(), "u_onehot": onehot,
            "padded": (1.0 - lv)[..., None], "terminated": term[..., None]}


def load_fixture():
    """(meta dict, the 11-key batch, initial eval parameters {"rnn.<name>" / "qmix.<name>": array}, [per-step records])."""
    z = np.load(os.path.join(GOLDEN, "learn_easy3.npz"))
    meta = json.loads(str(z["meta"]))
    batch = rebuild_batch(z, meta["args"]["n_actions"])
    init = {k[len("init_"):]: z[k] for k in z.files if k.startswith("init_")}
    steps = []
    for k in range(meta["steps"]):
        s = np.load(os.path.join(GOLDEN, f"learn_easy3_step{k}.npz"))
        steps.append({key: s[key] for key in s.files})
    return meta, batch, init, steps


def learner_args(meta, **over):
    """The learner's namespace: the env fields and get_mixer_args values the fixture was recorded with."""
    a = dict(meta["args"])
    a.update(env=meta["env"], n_agents=meta["n_agents"], agent_mode=meta["agent_mode"], target_num=meta["target_num"],
             target_mode=meta["target_mode"], map_size=50)
    a.update(over)
    return types.SimpleNamespace(**a)


def record(rec, prefix):
    """{"rnn.<name>" / "qmix.<name>": array} of one prefix (grad / eval / target) of a step record."""
    return {k[len(prefix) + 1:]: v for k, v in rec.items() if k.startswith(prefix + "_") and k != "grad_norm"}
