"""CPU tests of tests/sensor_cases.py, the planter of (agent, target) pairs at the sensor threshold, and of the bound that
DESIGN.md section 3 states for the fp32 pre-filter of the rollout kernels: outside thr +- eps32 the fp32 verdict is the float64
one.  The planter must fill every class, or tests/test_gpu_sensor_edge.py would pass on empty cases; the bound is the reference
arithmetic's own property, stated in NumPy, and needs no GPU.  Synthetic agent positions: uniform over the map, within 1 of each
wall, on the walls and in the corners."""
import numpy as np
import pytest

import sensor_cases as sc

B, N, M = 64, 5, 16
BAND, EDGE = [sc.NAMES.index(k) for k in ("band_in", "band_out")], [sc.NAMES.index(k) for k in ("edge_in", "edge_out")]


@pytest.fixture(scope="module", params=sc.CONFIGS, ids=lambda c: f"map{c[0]}-range{c[1]}")
def case(request):
    L, vr = request.param
    P = sc.synthetic_positions(B, N, L)
    tgt, plan = sc.plant(P, L, vr, M)
    return dict(L=L, vr=vr, P=P, tgt=tgt, plan=plan, got=sc.classify(tgt, P, L, vr, M), cfg=sc.Config(L, vr))


def test_synthetic_positions_stand_on_the_map_at_the_walls_and_in_the_corners():
    for L, _ in sc.CONFIGS:
        P = sc.synthetic_positions(B, N, L)
        assert P.shape == (B, N, 2) and P.min() >= 0.0 and P.max() <= L
        x, y = P[..., 0], P[..., 1]
        for near in (x <= 1.0, x >= L - 1.0, y <= 1.0, y >= L - 1.0):
            assert near.sum() >= 20
        for on in (x == 0.0, x == L, y == 0.0, y == L):
            assert on.sum() >= 3
        assert (((x == 0.0) | (x == L)) & ((y == 0.0) | (y == L))).sum() >= 1
        assert ((x > 0.1 * L) & (x < 0.9 * L) & (y > 0.1 * L) & (y < 0.9 * L)).sum() >= 40   # away from every wall


def test_every_planted_target_is_a_finite_point_of_the_map(case):
    tgt, L = case["tgt"], case["L"]
    assert tgt.shape == (B, 16, 2) and tgt.dtype == np.float64 and np.isfinite(tgt).all()
    assert tgt.min() >= 0.0 and tgt.max() <= L
    plan = case["plan"]
    b, j = np.nonzero(plan["cls"] >= 0)
    assert b.size == B * M and np.array_equal(plan["agent"][b, j], (b + j) % N)
    # the same table again from the same seed; another table from another
    again, _ = sc.plant(case["P"], L, case["vr"], M)
    other, _ = sc.plant(case["P"], L, case["vr"], M, seed=1)
    assert np.array_equal(again, tgt) and not np.array_equal(other, tgt)


def test_every_class_holds_at_least_50_pairs(case):
    got, cfg = case["got"], case["cfg"]
    b, j, i = sc.aimed(case["plan"], M)
    cls = got["cls"][b, j, i]
    n = sc.counts(cls)
    kept = float((cls == case["plan"]["cls"][b, j]).mean())
    print(f"\nmap {case['L']} range {case['vr']}: " + " ".join(f"{k} {n[k]}" for k in sc.NAMES) + f"; aimed-at class reached {kept:.3f}")
    for name in sc.CLASSES:
        assert n[name] >= 50, (name, n)
    eq = cls == sc.NAMES.index("eq")
    d2 = got["d2"][b, j, i][eq]
    assert np.array_equal(d2.view(np.int64), np.full(d2.size, cfg.r2).view(np.int64)) and d2.size >= 50
    # what the classes mean, restated on the aimed pairs
    tx, ty, ax, ay = case["tgt"][b, j, 0], case["tgt"][b, j, 1], case["P"][b, i, 0], case["P"][b, i, 1]
    v = got["verdict"][b, j, i]
    assert v[eq].all()
    under = cls == sc.NAMES.index("under")
    assert np.array_equal(tx[under], ax[under]) and np.array_equal(ty[under], ay[under]) and v[under].all()
    out = np.where(tx > ax, np.inf, -np.inf)
    last, first = cls == sc.NAMES.index("ulp_in"), cls == sc.NAMES.index("ulp_out")
    assert v[last].all() and not sc.statement(np.nextafter(tx, out), ty, ax, ay, cfg.r2)[0][last].any()
    assert not v[first].any() and sc.statement(np.nextafter(tx, -out), ty, ax, ay, cfg.r2)[0][first].all()
    wall = cls == sc.NAMES.index("wall")
    assert ((tx[wall] == 0.0) | (tx[wall] == cfg.L) | (ty[wall] == 0.0) | (ty[wall] == cfg.L)).all()
    assert v[wall].any() and not v[wall].all()
    for name, lo, hi, inside in (("band_in", -1, 0, True), ("band_out", 0, 1, False), ("edge_in", -2, -1, True), ("edge_out", 1, 2, False)):
        k = cls == sc.NAMES.index(name)
        nd2 = got["nd2"][b, j, i][k]
        assert (nd2 >= cfg.thr + lo * cfg.eps).all() and (nd2 <= cfg.thr + hi * cfg.eps).all() and (v[k] == inside).all(), name


@pytest.mark.parametrize("rule", ["lane", "pair"])
def test_band_pairs_lie_inside_the_fp32_band_and_edge_pairs_outside(case, rule):
    got = case["got"]
    b, j, i = sc.aimed(case["plan"], M)
    cls, band = got["cls"][b, j, i], got[rule + "_band"][b, j, i]
    inside, outside = float(band[np.isin(cls, BAND)].mean()), float(1.0 - band[np.isin(cls, EDGE)].mean())
    print(f"\nmap {case['L']} range {case['vr']} {rule}: band_* inside the fp32 band {inside:.3f}, edge_* outside it {outside:.3f}")
    assert inside >= 0.9 and outside >= 0.9
    for name in ("eq", "ulp_in", "ulp_out"):     # nothing at the threshold itself may be left to fp32
        assert band[cls == sc.NAMES.index(name)].all(), name


@pytest.mark.parametrize("rule", ["lane", "pair"])
def test_outside_the_band_the_fp32_verdict_is_the_float64_one(case, rule):
    """The bound of DESIGN.md section 3, over all B x 16 x n pairs of the table (not only the aimed ones)."""
    got = case["got"]
    trusted = ~got[rule + "_band"]
    assert trusted.sum() >= B * M * N // 2
    assert not (trusted & (got[rule + "_verdict"] != got["verdict"])).any()
    # and the band is what makes it so: without one, fp32 gets pairs of these tables wrong
    bare = sc.classify(case["tgt"], case["P"], case["L"], case["vr"], M, eps_scale=0.0)
    assert (~bare[rule + "_band"] & (bare[rule + "_verdict"] != bare["verdict"])).sum() >= 20


def test_slots_follow_the_steps_of_a_launch():
    """plant([T, B, n, 2]): slot j is planted for the positions of step j % T, and every class still fills over the T tables."""
    L, vr, T = 50, 7, 5
    P = np.stack([sc.synthetic_positions(B, N, L, seed=t) for t in range(T)])
    tgt, plan = sc.plant(P, L, vr, M)
    b, j, i = sc.aimed(plan, M)
    assert np.array_equal(plan["step"][b, j], j % T)
    total = {k: 0 for k in sc.NAMES}
    for t in range(T):
        got = sc.classify(tgt, P[t], L, vr, M)
        k = plan["step"][b, j] == t
        for name, v in sc.counts(got["cls"][b[k], j[k], i[k]]).items():
            total[name] += v
    assert all(total[name] >= 50 for name in sc.CLASSES), total
