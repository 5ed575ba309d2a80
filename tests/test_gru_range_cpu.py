"""CPU companion of tests/test_gpu_gru_range.py: the yardstick is what it claims to be, and every case is what its GPU test needs
it to be -- from fp64 alone, on the fp64 trajectory (the GPU tests assert the same conditions again on the kernel's own)."""
import pytest
import torch

from gru_range_util import (BAD_ROW, BAD_T, F16_MAX, G_MIN, GROWTH_CASES, K_LIMIT, PLANTED, ROW_EXPONENTS, TRAINED, adjoint, bar,
                            block_scale, blocks, fp64_trajectory, gates, growth, growth_case, h_prev_of, nonfinite_case, on_device,
                            rel, rows_case, saturated_case, tiny_case, trained_case)
from test_gpu_learner import gru_fp64, inputs

H = 64


@pytest.mark.parametrize("kind,factor", [("random", 1.0), ("random", 6.5), ("easy3_qmix", 1.0)])
def test_adjoint_statement_is_fp64_autograd(kind, factor):
    """The reference of the GPU tests -- the adjoint recurrence written out, at a given H -- equals autograd of gru_fp64 when H is
    gru_fp64's own trajectory: T = 200, R = 16, to 1e-12 relative (measured: 2e-14)."""
    with on_device("cpu"):
        gi, w_hh, b_hh, h0 = inputs(kind, 16, 200, seed=5)
    w_hh = w_hh * factor
    dH = torch.randn(200, 16, H, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    leaves = [t.double().requires_grad_(True) for t in (gi, w_hh, b_hh, h0)]
    traj = gru_fp64(*leaves)
    traj.backward(dH)
    ours = adjoint(gi, w_hh, b_hh, h0, traj.detach(), dH)
    for name, leaf in zip(("dgi", "dW_hh", "db_hh", "dh0"), leaves):
        assert rel(ours[name], leaf.grad) <= 1e-12, (name, rel(ours[name], leaf.grad))


def on_fp64_trajectory(case):
    gi, w_hh, b_hh, h0, dH = case[:5]
    traj = fp64_trajectory(gi, w_hh, b_hh, h0).float()   # the kernel hands over fp32
    return traj, adjoint(gi, w_hh, b_hh, h0, traj, dH)


@pytest.mark.parametrize("R,factor,seed,kind", GROWTH_CASES)
def test_growth_cases_are_past_the_headroom_and_the_test_has_power(R, factor, seed, kind):
    """A: every full block has G = max_t |dgh_t| / max |dH| >= 4096 (twice the largest headroom of a scale chosen from dH); the
    correct answer is representable (max |dgi| max |dH| < 1e30); and an fp64 recurrence with the once-chosen scale and dgh clipped
    at +-65504 differs from the unclipped one by >= 0.1 in dgi and by >= 10 times the bar at K = 8 with the fp32 twin's error."""
    case = growth_case(R, factor, seed, kind, "cpu")
    gi, w_hh, b_hh, h0, dH = case
    traj, ref = on_fp64_trajectory(case)
    twin = adjoint(gi, w_hh, b_hh, h0, traj, dH, torch.float32)
    emu = adjoint(gi, w_hh, b_hh, h0, traj, dH, clip=True)
    G = growth(ref, dH)
    assert float(ref["dgi"].abs().max()) * float(dH.abs().max()) < 1e30
    for b, g in zip(blocks(R), G):
        if b.stop - b.start < 16:
            continue
        assert g >= G_MIN, G
        power = rel(emu["dgi"][:, b], ref["dgi"][:, b])
        held_to = bar(rel(twin["dgi"][:, b], ref["dgi"][:, b]), K_LIMIT)
        assert power >= 0.1 and power >= 10 * held_to, (power, held_to)


def test_clipped_emulation_is_the_reference_while_nothing_clips():
    """The emulation only differs where dgh * scale passes 65504: on a shipped checkpoint (G < 1023) it IS the reference."""
    case = trained_case("easy3_qmix", "ones", "cpu")
    gi, w_hh, b_hh, h0, dH = case
    traj, ref = on_fp64_trajectory(case)
    assert float((ref["dgh"] * block_scale(dH.double())).abs().max()) < F16_MAX
    emu = adjoint(gi, w_hh, b_hh, h0, traj, dH, clip=True)
    assert torch.equal(emu["dgi"], ref["dgi"]) and torch.equal(emu["dh0"], ref["dh0"])


@pytest.mark.parametrize("kind", TRAINED)
def test_shipped_checkpoints_sit_under_the_headroom_with_same_sign_gradients(kind):
    """B: 16 <= G < 1023 with all-ones dH at T = 200 (measured here: 61, 186, 39): near the headroom, under it."""
    case = trained_case(kind, "ones", "cpu")
    G = growth(on_fp64_trajectory(case)[1], case[4])[0]
    assert 16 <= G < 1023, G
    last = trained_case(kind, "last", "cpu")[4]
    assert not last[:-1].any() and last[-1].all()


def test_rows_case_spans_24_binades_inside_one_block():
    """C: the rows' largest |dH| are 2^0, 2^-8, 2^-16, 2^-24 times the same draw's, four rows each."""
    dH = rows_case("cpu")[4]
    assert dH.shape == (7, 16, H)
    base = torch.randn(7, 16, H, generator=torch.Generator().manual_seed(1021))
    for row in range(16):
        assert torch.equal(dH[:, row], base[:, row] * 2.0 ** ROW_EXPONENTS[row // 4])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_case_plants_one_value_in_the_middle_block(bad):
    """D: three blocks, exactly one non-finite dH, in block 1; the fp64 recurrence keeps it in its row."""
    gi, w_hh, b_hh, h0, dH, holed = nonfinite_case(bad, "cpu")
    assert dH.shape[1] == 48 and torch.isfinite(dH).all()
    where = (~torch.isfinite(holed)).nonzero()
    assert where.tolist() == [[BAD_T, BAD_ROW, 5]] and 16 <= BAD_ROW < 32
    traj = fp64_trajectory(gi, w_hh, b_hh, h0)
    out = adjoint(gi, w_hh, b_hh, h0, traj, holed)
    rows = (~torch.isfinite(out["dgi"])).any(0).any(-1).nonzero().flatten().tolist()
    assert rows == [BAD_ROW] and not torch.isfinite(out["dgi"][BAD_T, BAD_ROW]).all()


def test_tiny_case_reaches_the_exponent_clamp_and_is_not_zero_in_fp32():
    """D: max |dH| = 2^-125, so frexp's exponent is -124 < -120; the fp64 dgi and dh0 survive rounding to fp32."""
    case = tiny_case("cpu")
    dH = case[4]
    assert torch.frexp(dH.abs().max()).exponent.item() == -124
    ref = on_fp64_trajectory(case)[1]
    assert ref["dgi"].float().any() and ref["dh0"].float().any()


def test_saturated_case_plants_every_value_in_every_gate_third():
    """E: +-20, +-90, +-1e4 each once per row and gate third; in fp64 the +-1e4 entries saturate their gate exactly."""
    gi, w_hh, b_hh, h0, dH, planted = saturated_case("cpu")
    for gate in range(3):
        third, mask = gi[..., gate * H:(gate + 1) * H], planted[..., gate * H:(gate + 1) * H]
        assert int(mask[0, 0].sum()) == len(PLANTED)
        assert sorted(third[0, 0][mask[0, 0]].tolist()) == sorted(PLANTED)
    traj = fp64_trajectory(gi, w_hh, b_hh, h0)
    assert torch.isfinite(traj).all()
    r, z, n, _ = gates(gi.double(), w_hh.double(), b_hh.double(), h_prev_of(traj, h0.double()))
    huge = gi.abs() == 1e4
    assert ((r == 0) | (r == 1))[huge[..., :H]].all() and ((z == 0) | (z == 1))[huge[..., H:2 * H]].all()
    assert (n.abs() == 1)[huge[..., 2 * H:]].all()
