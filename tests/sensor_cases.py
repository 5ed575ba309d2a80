"""Target positions planted AT the sensor threshold, and a classifier that says what a table of positions really holds.  NumPy
float64 on the CPU, nothing imported from the kernels.  tests/test_sensor_cases_cpu.py asserts, without a GPU, that the planter
fills every class and that the fp32 pre-filter's band covers the fp32 error on all of them;
tests/test_gpu_sensor_edge.py writes the planted targets into real envs and runs every rollout kernel over them.

The sensor test of the simulator (flight_env_easy.py:237), the statement every distance here is judged by, in float64:
    dx = tx - ax;  dy = ty - ay;  in range  iff  dx*dx + dy*dy <= vr*vr
The lane kernels and the pair / octet kernels decide it in fp32 on the normalised coordinates f = float32((v - mid) * inv_half),
d2 = fma(dx, dx, dy * dy), against thr = vr^2 inv_half^2, and trust that verdict only outside thr +- eps32, eps32 = 1e-6 + 4e-6 thr
(cs_configure); inside the band they run the statement above.

Classes of an (agent, target) pair -- `CLASSES`, then the two that nothing is planted for:
  eq        dx*dx + dy*dy == vr*vr, bit for bit
  ulp_in    in range, and out of range at the next float64 tx away from the agent   (the last tx for which the statement is true)
  ulp_out   out of range, and in range at the next float64 tx towards the agent      (the first tx for which it is false)
  band_in   normalised d2 in (thr - eps32, thr): the fp32 verdict must not be trusted   band_out: in (thr, thr + eps32)
  edge_in   normalised d2 in (thr - 2 eps32, thr - eps32]: the fp32 verdict stands and has to be right
  edge_out  in [thr + eps32, thr + 2 eps32)
  under     the target stands at the agent's position, d2 = 0
  wall      a band_in / band_out pair whose target has a coordinate of exactly 0.0 or exactly map_size
  far_in / far_out   everything else
A pair takes the first class of under, eq, ulp_in / ulp_out, wall, band, edge, far that it satisfies."""
import numpy as np

CLASSES = ("eq", "ulp_in", "ulp_out", "band_in", "band_out", "edge_in", "edge_out", "under", "wall")
NAMES = CLASSES + ("far_in", "far_out")
CYCLE = CLASSES + ("wall",)    # wall twice: it can be planted only where an agent stands within view_range of a wall
SLOTS = 16
CONFIGS = [(50, 7), (20, 3), (50, 30), (64, 1)]   # (map_size, view_range): shipped; two of the octet parity test; largest map, smallest range
MARGIN = 1e-6      # a target that is not of class wall or under keeps this distance from the walls
MIN_COS = 0.25     # eq / ulp: |cos| of the direction, so that tx decides the statement
ROUNDS = 120       # angles tried per slot


class Config:
    """The constants of one (map_size, view_range), in the operation order of cs_configure."""

    def __init__(self, map_size, view_range):
        self.map_size, self.view_range = map_size, view_range
        self.L = float(map_size)
        self.vr = float(view_range)
        self.r2 = float(view_range * view_range)
        self.mid = 0.5 * self.L
        self.inv_half = 1.0 / (self.L / 2.0)
        self.thr = self.r2 * self.inv_half * self.inv_half
        self.thr32 = np.float32(self.thr)
        self.eps32 = np.float32(1e-6 + 4e-6 * self.thr)
        self.eps = float(self.eps32)


def statement(tx, ty, ax, ay, r2):
    """The reference's sensor test -> (in range, dx*dx + dy*dy), float64, every operation rounded once."""
    dx = tx - ax
    dy = ty - ay
    s = dx * dx + dy * dy
    return s <= r2, s


# ---- the planter --------------------------------------------------------------------------------------------------------------

def _aim(rng, ax, ay, dist, cfg, need_dx=False):
    """A direction per slot, towards the map centre +- up to 1 rad (any direction once half of the rounds have failed), such that
    the point at `dist` from (ax, ay) keeps MARGIN from every wall.  -> (cos, sin, found)."""
    k = len(ax)
    c, s, ok = np.ones(k), np.zeros(k), np.zeros(k, dtype=bool)
    base = np.arctan2(cfg.mid - ay, cfg.mid - ax)
    for r in range(ROUNDS):
        todo = np.flatnonzero(~ok)
        if todo.size == 0:
            break
        spread = 1.0 if r < ROUNDS // 2 else np.pi
        th = base[todo] + rng.uniform(-spread, spread, todo.size)
        ct, st = np.cos(th), np.sin(th)
        tx, ty = ax[todo] + dist[todo] * ct, ay[todo] + dist[todo] * st
        good = (tx >= MARGIN) & (tx <= cfg.L - MARGIN) & (ty >= MARGIN) & (ty <= cfg.L - MARGIN)
        if need_dx:
            good &= np.abs(ct) >= MIN_COS
        g = todo[good]
        c[g], s[g], ok[g] = ct[good], st[good], True
    return c, s, ok


def _last_true(ax, ay, ty, sgn, cfg):
    """Per slot the last float64 tx, going away from the agent in x (sgn = +-1), for which the statement is true, found by
    bisection over the floats between a tx that is in range and one that is not (the statement is monotone in tx on one side
    of the agent: every rounding is).  -> (tx_in, tx_out, found)."""
    dy = ty - ay
    rem = cfg.r2 - dy * dy
    ok = rem > 0.0
    est = ax + sgn * np.sqrt(np.where(ok, rem, 1.0))
    delta = 1e-9 * cfg.vr / MIN_COS
    lo, hi = est - sgn * delta, est + sgn * delta
    ok &= statement(lo, ty, ax, ay, cfg.r2)[0] & ~statement(hi, ty, ax, ay, cfg.r2)[0] & ((lo - ax) * sgn > 0.0)
    for _ in range(80):
        mid = lo + (hi - lo) * 0.5
        mid = np.where((mid == lo) | (mid == hi), lo, mid)
        v = statement(mid, ty, ax, ay, cfg.r2)[0]
        lo, hi = np.where(v, mid, lo), np.where(v, hi, mid)
    nxt = np.nextafter(lo, lo + sgn)
    ok &= nxt == hi
    return lo, nxt, ok


def plant(P, map_size, view_range, m, seed=0):
    """Targets at the threshold of the agents at P.

    P    float64 [B, n, 2] or [T, B, n, 2]: the positions the agents will have AFTER the step(s); slot j is planted for the
         positions of step j % T
    ->   (tgt float64 [B, 16, 2], plan): every slot below m inside [0, map_size]^2 (the others hold the map's centre);
         plan = dict(cls, agent, step: int64 [B, 16]; cls indexes CLASSES, -1 from slot m on) -- what was AIMED AT; what the
         table really holds is `classify`'s to say.
    Target j of env b is aimed at agent (b + j) % n and takes class CYCLE[(3 b + j) % 10]; a wall slot whose agent stands
    farther than view_range from every wall, and an eq slot for which no angle lands on equality, take another class."""
    cfg = Config(map_size, view_range)
    P = np.asarray(P, dtype=np.float64)
    if P.ndim == 3:
        P = P[None]
    T, B, n = P.shape[:3]
    assert P.shape[3] == 2 and 1 <= m <= SLOTS and np.isfinite(P).all()
    rng = np.random.RandomState(seed)
    b, j = (v.reshape(-1) for v in np.meshgrid(np.arange(B), np.arange(m), indexing="ij"))
    agent, step = (b + j) % n, j % T
    ax, ay = P[step, b, agent, 0], P[step, b, agent, 1]
    want = np.array([CLASSES.index(CYCLE[k]) for k in (3 * b + j) % len(CYCLE)])
    S = b.size
    tx, ty = np.full(S, cfg.mid), np.full(S, cfg.mid)
    done = np.zeros(S, dtype=bool)
    lo_of = {"band_in": -1.0, "band_out": 0.0, "edge_in": -2.0, "edge_out": 1.0}   # normalised d2 in thr + (lo, lo + 1) eps32

    def nd2_in(name, k):
        u = rng.uniform(0.0, 1.0, k)
        return cfg.thr + (lo_of[name] + u) * cfg.eps

    # wall: coordinate `axis` exactly 0.0 or L, the other one at the distance that puts the pair into the band
    idx = np.flatnonzero(want == CLASSES.index("wall"))
    pos = np.stack((ax, ay), 1)
    for turn in range(4):
        todo = idx[~done[idx]]
        if todo.size == 0:
            break
        w = (b[todo] + j[todo] + turn) % 4
        axis, value = w // 2, np.where(w % 2 == 0, 0.0, cfg.L)
        inside = rng.randint(0, 2, todo.size) == 0
        nd2 = np.where(inside, nd2_in("band_in", todo.size), nd2_in("band_out", todo.size))
        gap = value - pos[todo, axis]
        rest = nd2 / (cfg.inv_half * cfg.inv_half) - gap * gap
        other = pos[todo, 1 - axis]
        off = np.sqrt(np.where(rest > 0.0, rest, 0.0))
        toward = np.where(other <= cfg.mid, 1.0, -1.0)
        for sign in (1.0, -1.0):
            o = other + sign * toward * off
            good = (rest > 0.0) & (o >= 0.0) & (o <= cfg.L) & ~done[todo]
            g = todo[good]
            tx[g] = np.where(axis[good] == 0, value[good], o[good])
            ty[g] = np.where(axis[good] == 0, o[good], value[good])
            done[g] = True
    left = idx[~done[idx]]
    want[left] = (b[left] + 2 * j[left]) % (len(CLASSES) - 1)    # any class but wall

    # under
    idx = np.flatnonzero(want == CLASSES.index("under"))
    tx[idx], ty[idx] = np.clip(ax[idx], 0.0, cfg.L), np.clip(ay[idx], 0.0, cfg.L)
    done[idx] = True

    # eq, ulp_in, ulp_out: ty at view_range along a direction, tx from the bisection; eq draws angles until the sum at the last
    # in-range tx equals view_range^2 (ulp_in: until it does not), and becomes ulp_in when none does
    for name in ("eq", "ulp_in", "ulp_out"):
        idx = np.flatnonzero(want == CLASSES.index(name))
        for _ in range(ROUNDS if name == "eq" else 16):
            todo = idx[~done[idx]]
            if todo.size == 0:
                break
            c, s, ok = _aim(rng, ax[todo], ay[todo], np.full(todo.size, cfg.vr), cfg, need_dx=True)
            y = ay[todo] + cfg.vr * s
            x_in, x_out, found = _last_true(ax[todo], ay[todo], y, np.sign(c), cfg)
            ok &= found & (np.minimum(x_in, x_out) >= 0.0) & (np.maximum(x_in, x_out) <= cfg.L)
            if name != "ulp_out":    # (an ulp_in slot whose last in-range tx lands on equality would be one more eq)
                ok &= (statement(x_in, y, ax[todo], ay[todo], cfg.r2)[1] == cfg.r2) == (name == "eq")
            g = todo[ok]
            tx[g], ty[g] = (x_out if name == "ulp_out" else x_in)[ok], y[ok]
            done[g] = True
        left = idx[~done[idx]]
        want[left] = CLASSES.index("ulp_in" if name == "eq" else "under")
        if name != "eq":
            tx[left], ty[left] = np.clip(ax[left], 0.0, cfg.L), np.clip(ay[left], 0.0, cfg.L)
            done[left] = True

    # band and edge: normalised d2 uniform in the class's interval, any admissible direction
    for name in ("band_in", "band_out", "edge_in", "edge_out"):
        idx = np.flatnonzero(want == CLASSES.index(name))
        d = np.sqrt(nd2_in(name, idx.size)) / cfg.inv_half
        c, s, ok = _aim(rng, ax[idx], ay[idx], d, cfg)
        g = idx[ok]
        tx[g], ty[g] = ax[g] + d[ok] * c[ok], ay[g] + d[ok] * s[ok]
        left = idx[~ok]
        want[left] = CLASSES.index("under")
        tx[left], ty[left] = np.clip(ax[left], 0.0, cfg.L), np.clip(ay[left], 0.0, cfg.L)
        done[idx] = True
    assert done.all()

    tgt = np.full((B, SLOTS, 2), cfg.mid)
    tgt[b, j, 0], tgt[b, j, 1] = tx, ty
    assert np.isfinite(tgt).all() and tgt.min() >= 0.0 and tgt.max() <= cfg.L
    plan = {k: np.full((B, SLOTS), -1, dtype=np.int64) for k in ("cls", "agent", "step")}
    plan["cls"][b, j], plan["agent"][b, j], plan["step"][b, j] = want, agent, step
    return tgt, plan


# ---- the classifier -----------------------------------------------------------------------------------------------------------

def fp32_statement(tgt, P, cfg):
    """The kernels' fp32 arithmetic on every (target j, agent i) pair, [B, slots, n]: f = float32((v - mid) inv_half) of both,
    dx, dy their float32 differences, d2 = float32(float64(dx) dx + float64(float32(dy dy))) -- the product of two float32 values
    is exact in float64, so this is fma(dx, dx, dy * dy)."""
    f32, f64 = np.float32, np.float64
    norm = lambda v: ((v - cfg.mid) * cfg.inv_half).astype(f32)
    dx = norm(tgt[:, :, None, 0]) - norm(P[:, None, :, 0])
    dy = norm(tgt[:, :, None, 1]) - norm(P[:, None, :, 1])
    assert dx.dtype == f32 and dy.dtype == f32
    d2 = (dx.astype(f64) * dx.astype(f64) + (dy * dy).astype(f64)).astype(f32)
    return d2


def classify(tgt, P, map_size, view_range, m=SLOTS, eps_scale=1.0):
    """What the table holds: tgt float64 [B, >= m, 2], P float64 [B, n, 2] -> dict of [B, m, n] arrays over the pairs
    (target j, agent i):
      cls       index into NAMES, by plain float64 comparisons (module docstring)
      verdict   the float64 statement;  d2: its left side;  nd2: d2 inv_half^2
      d2_32     the kernels' fp32 left side (fp32_statement)
      lane_band, lane_verdict   the lane kernels' rule: sure = d2_32 - (thr32 - eps32) < 0, maybe = d2_32 - (thr32 + eps32) < 0 by
                sign bit; band = maybe and not sure (these pairs take the fp64 statement), verdict outside it = sure
      pair_band, pair_verdict   the pair / octet kernels' rule: u = d2_32 - thr32; band = |u| <= eps32, verdict = u < 0
    eps_scale scales eps32 in the two rules (0: no band at all), to show what the band is needed for."""
    cfg = Config(map_size, view_range)
    tgt, P = np.asarray(tgt, dtype=np.float64)[:, :m], np.asarray(P, dtype=np.float64)
    tx, ty = tgt[:, :, None, 0], tgt[:, :, None, 1]
    ax, ay = P[:, None, :, 0], P[:, None, :, 1]
    tx, ty, ax, ay = np.broadcast_arrays(tx, ty, ax, ay)
    verdict, d2 = statement(tx, ty, ax, ay, cfg.r2)
    dx = tx - ax
    away = np.where(dx > 0.0, np.inf, -np.inf)
    v_away = statement(np.nextafter(tx, away), ty, ax, ay, cfg.r2)[0]
    v_near = statement(np.nextafter(tx, -away), ty, ax, ay, cfg.r2)[0]
    nd2 = d2 * (cfg.inv_half * cfg.inv_half)
    on_wall = (tx == 0.0) | (tx == cfg.L) | (ty == 0.0) | (ty == cfg.L)
    e = cfg.eps
    cls = np.where(verdict, NAMES.index("far_in"), NAMES.index("far_out"))
    rules = [("edge_in", (nd2 > cfg.thr - 2 * e) & (nd2 <= cfg.thr - e)), ("edge_out", (nd2 >= cfg.thr + e) & (nd2 < cfg.thr + 2 * e)),
             ("band_in", (nd2 > cfg.thr - e) & verdict), ("band_out", (nd2 < cfg.thr + e) & ~verdict)]
    rules.append(("wall", (rules[2][1] | rules[3][1]) & on_wall))
    rules += [("ulp_in", verdict & ~v_away & (dx != 0.0)), ("ulp_out", ~verdict & v_near & (dx != 0.0)),
              ("eq", d2 == cfg.r2), ("under", d2 == 0.0)]
    for name, mask in rules:    # later rules win
        cls = np.where(mask, NAMES.index(name), cls)
    f32 = np.float32
    d2_32 = fp32_statement(tgt, P, cfg)
    eps = f32(cfg.eps32 * f32(eps_scale))
    thr_lo, thr_hi = f32(cfg.thr32 - eps), f32(cfg.thr32 + eps)
    sure, maybe = np.signbit(d2_32 - thr_lo), np.signbit(d2_32 - thr_hi)
    u = d2_32 - cfg.thr32
    assert u.dtype == f32
    return dict(cls=cls, verdict=verdict, d2=d2, nd2=nd2, d2_32=d2_32, lane_band=maybe & ~sure, lane_verdict=sure,
                pair_band=np.abs(u) <= eps, pair_verdict=u < f32(0.0))


def counts(cls, where=None):
    """{class name: number of pairs} of a `cls` array (over the pairs where `where` holds)."""
    c = cls if where is None else cls[where]
    return {name: int((c == k).sum()) for k, name in enumerate(NAMES)}


def aimed(plan, m):
    """Index arrays (b, j, i) of the pairs the planter aimed at: target j of env b and the agent it was planted for."""
    b, j = np.nonzero(plan["cls"][:, :m] >= 0)
    return b, j, plan["agent"][b, j]


def synthetic_positions(B, n, map_size, seed=0):
    """Agent positions float64 [B, n, 2]: the first third of the envs uniform over the map; then, agent by agent in turn, within
    1 of one of the four walls (every fourth of them exactly ON it) with the other coordinate uniform; the last eighth of the
    envs in the corners, within 1 of both walls (every fourth agent exactly in the corner)."""
    rng = np.random.RandomState(seed)
    L = float(map_size)
    P = rng.uniform(0.0, L, (B, n, 2))
    k = 0
    for b in range(B // 3, B):
        for i in range(n):
            gap = 0.0 if (k // 4) % 4 == 3 else rng.uniform(0.0, 1.0)
            wall = k % 4
            if b >= B - B // 8:
                gap2 = 0.0 if (k // 4) % 4 == 3 else rng.uniform(0.0, 1.0)
                P[b, i] = [gap if wall & 1 else L - gap, gap2 if wall & 2 else L - gap2]
            else:
                P[b, i, wall // 2] = gap if wall % 2 == 0 else L - gap
            k += 1
    return P
