"""Cases and yardsticks of the GRU recurrence kernels' range tests (tests/test_gpu_gru_range.py on the GPU,
tests/test_gru_range_cpu.py for the conditions every case must meet, from fp64 alone).

The backward kernel is judged ALONE, on the trajectory the forward produced: with w_hh scaled up the forward recurrence is
chaotic (fp32 torch autograd of forward + backward differs from fp64 by 3e-3 to 0.5 there), so an end-to-end comparison would
say nothing about the adjoint.  `adjoint` is the adjoint recurrence at a GIVEN H, in the dtype of its inputs: fp64 is the
reference, fp32 torch on the same H the twin; `clip=True` is an fp64 emulation of a kernel that scales each block of 16 rows once
(largest |dH| into [32, 64)) and saturates dgh_t at +-65504 on its way into the W_hh product -- the fault the growth cases are
built to catch (the power condition: the emulation must be far outside the bar)."""
import contextlib

import torch

import test_gpu_learner as tgl
from test_gpu_learner import gru_fp64, inputs

H = 64
F16_MAX = 65504.0
FLOOR = 1e-4          # the bar of test_backward_matches_fp64_autograd_and_is_deterministic
K_LIMIT = 8.0         # the factor test_forward_matches_fp64_grucell grants over fp32 drift: the most K may ever be
TRAINED = ("easy3_qmix", "easy3_dop", "flight5_qmix")

# A: (R, factor on w_hh, seed of inputs(), dH pattern).  Chosen on the CPU so that the conditions of test_gru_range_cpu.py hold.
# Measured there (fp64 trajectory): G of the full blocks 1.1e8, 4.1e7, (4.6e7, 5.8e9), (4.8e6, 1.3e8); the clipped emulation is
# 1.0 relative from the unclipped dgi in every block; the fp32 twin 1.4e-6 to 6.9e-6.  (w_hh x 5.5 leaves several blocks under
# 4096 and w_hh x 6 within a factor of 10 of it: the trajectory on the GPU is another one, so the margin has to be wide.)
GROWTH_CASES = [(16, 6.5, 1, "ones"), (16, 6.5, 1, "normal"), (40, 6.5, 1, "ones"), (40, 6.5, 1, "normal")]
G_MIN = 4096.0        # twice the largest headroom of a scale chosen from dH alone (1023 to 2047)


@contextlib.contextmanager
def on_device(dev):
    """test_gpu_learner's builders (`weights`, `inputs`) put their tensors on that module's global DEV, which they look up when
    they are CALLED; the CPU companion runs them with DEV = "cpu" for the length of this block.  This depends on that global
    keeping its name and on the builders not binding it earlier (a default argument, say): if either changes, the CPU tests
    of tests/test_gru_range_cpu.py fail at once with a device error -- give the builders a device parameter then."""
    old, tgl.DEV = tgl.DEV, dev
    try:
        yield
    finally:
        tgl.DEV = old


def blocks(R):
    """The row slices of the kernel's workgroups (16 rows each, the last one partial)."""
    return [slice(r, min(r + 16, R)) for r in range(0, R, 16)]


def pattern(kind, T, R, seed, dev):
    """dH [T, R, 64] fp32: "ones", "normal" (unit normal), "last" (ones at t = T - 1, zero elsewhere)."""
    if kind == "ones":
        return torch.ones(T, R, H, device=dev)
    if kind == "normal":
        return torch.randn(T, R, H, generator=torch.Generator().manual_seed(1000 + seed)).to(dev)
    assert kind == "last"
    dH = torch.zeros(T, R, H, device=dev)
    dH[-1] = 1.0
    return dH


def growth_case(R, factor, seed, kind, dev, T=200):
    """A: torch's default init with w_hh times `factor` -> (gi, w_hh, b_hh, h0, dH), fp32 on dev."""
    with on_device(dev):
        gi, w_hh, b_hh, h0 = inputs("random", R, T, seed)
    return gi, w_hh * factor, b_hh, h0, pattern(kind, T, R, seed, dev)


def trained_case(kind, pat, dev, R=16, T=200):
    """B: a shipped checkpoint's recurrence, same-sign dH."""
    with on_device(dev):
        gi, w_hh, b_hh, h0 = inputs(kind, R, T, seed=11)
    return gi, w_hh, b_hh, h0, pattern(pat, T, R, 11, dev)


ROW_EXPONENTS = (0, -8, -16, -24)


def rows_case(dev, T=7):
    """C: one block whose rows' dH are unit normal times 2^0, 2^-8, 2^-16, 2^-24, four rows each."""
    with on_device(dev):
        gi, w_hh, b_hh, h0 = inputs("easy3_qmix", 16, T, seed=21)
    f = torch.tensor([2.0 ** k for k in ROW_EXPONENTS]).repeat_interleave(4)[None, :, None]
    return gi, w_hh, b_hh, h0, (pattern("normal", T, 16, 21, "cpu") * f).to(dev)


BAD_ROW, BAD_T = 20, 3


def nonfinite_case(bad, dev, R=48, T=5):
    """D: three blocks; `bad` (inf or nan) at row 20 (block 1), t = 3, unit 5.  -> (..., dH clean, dH with the bad value)."""
    with on_device(dev):
        gi, w_hh, b_hh, h0 = inputs("easy3_qmix", R, T, seed=31)
    dH = pattern("normal", T, R, 31, dev)
    holed = dH.clone()
    holed[BAD_T, BAD_ROW, 5] = bad
    return gi, w_hh, b_hh, h0, dH, holed


def tiny_case(dev, R=16, T=7):
    """D: one block with max |dH| = 2^-125 exactly: the scale's exponent clamp (e < -120)."""
    with on_device(dev):
        gi, w_hh, b_hh, h0 = inputs("easy3_qmix", R, T, seed=41)
    d = pattern("normal", T, R, 41, "cpu").double()
    dH = (d / d.abs().max() * 2.0 ** -125).float().to(dev)
    assert float(dH.abs().max()) == 2.0 ** -125
    return gi, w_hh, b_hh, h0, dH


PLANTED = (20.0, -20.0, 90.0, -90.0, 1e4, -1e4)   # +-90: where __expf in the kernel's sigmoid overflows to inf


def saturated_case(dev, R=16, T=7):
    """E: easy3_qmix gi with planted entries of +-20, +-90, +-1e4 in all three gate thirds (every row, every t; units 3 j + gate
    for the j-th value, so each gate third carries each value once per row).  -> (gi, w_hh, b_hh, h0, dH, planted mask of gi)."""
    with on_device(dev):
        gi, w_hh, b_hh, h0 = inputs("easy3_qmix", R, T, seed=51)
    gi = gi.clone()
    mask = torch.zeros_like(gi, dtype=torch.bool)
    for gate in range(3):
        for j, v in enumerate(PLANTED):
            col = gate * H + 7 + 3 * j + gate
            gi[..., col] = v
            mask[..., col] = True
    return gi, w_hh, b_hh, h0, pattern("normal", T, R, 51, dev), mask


def h_prev_of(Hseq, h0):
    first = h0.unsqueeze(0) if h0 is not None else Hseq.new_zeros(1, *Hseq.shape[1:])
    return torch.cat([first, Hseq[:-1]], 0)


def gates(gi, w_hh, b_hh, hp):
    """(r, z, n, gh_n) of every step from gi_t and h_{t-1}, exactly as gru_step forms them."""
    gh = hp @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    return r, z, n, gh[..., 2 * H:]


def block_scale(dH):
    """The power of two per row that puts the largest |dH| of the row's block of 16 (all t) into [32, 64); 1 for a zero block."""
    R = dH.shape[1]
    s = torch.ones(R, dtype=dH.dtype, device=dH.device)
    for b in blocks(R):
        m = float(dH[:, b].abs().max())
        if m > 0:
            s[b] = 2.0 ** (6 - torch.frexp(torch.tensor(m)).exponent.item())
    return s[:, None]


def adjoint(gi, w_hh, b_hh, h0, Hseq, dH, dtype=torch.float64, clip=False):
    """The adjoint recurrence at the given trajectory Hseq, in `dtype` -> dict(dgi, dgh, dh0, dW_hh, db_hh).
        dh = dH_t + carry;  da_n = dh (1 - z)(1 - n^2);  da_r = da_n gh_n r (1 - r);  da_z = dh (h_{t-1} - n) z (1 - z)
        dgi_t = [da_r, da_z, da_n];  dgh_t = [da_r, da_z, da_n r];  carry = dh z + dgh_t W_hh;  dh0 = the last carry."""
    gi, w_hh, b_hh, Hseq, dH = (x.to(dtype) for x in (gi, w_hh, b_hh, Hseq, dH))
    hp = h_prev_of(Hseq, None if h0 is None else h0.to(dtype))
    r, z, n, ghn = gates(gi, w_hh, b_hh, hp)
    T = gi.shape[0]
    scale = block_scale(dH) if clip else None
    carry = torch.zeros_like(dH[0])
    dgi, dgh = torch.empty_like(gi), torch.empty_like(gi)
    for t in range(T - 1, -1, -1):
        dh = dH[t] + carry
        dan = dh * (1 - z[t]) * (1 - n[t] * n[t])
        dar = dan * ghn[t] * (r[t] * (1 - r[t]))
        daz = dh * (hp[t] - n[t]) * (z[t] * (1 - z[t]))
        dgi[t] = torch.cat([dar, daz, dan], -1)
        dgh[t] = torch.cat([dar, daz, dan * r[t]], -1)
        through = dgh[t] if not clip else (dgh[t] * scale).clamp(-F16_MAX, F16_MAX) / scale
        carry = dh * z[t] + through @ w_hh
    flat = dgh.reshape(-1, 3 * H)
    return dict(dgi=dgi, dgh=dgh, dh0=carry, dW_hh=flat.t() @ hp.reshape(-1, H), db_hh=flat.sum(0))


def growth(ref, dH):
    """G = max_t |dgh_t| / max |dH| of every block of rows (inf for a block without dH)."""
    out = []
    for b in blocks(dH.shape[1]):
        m = float(dH[:, b].abs().max())
        out.append(float(ref["dgh"][:, b].abs().max()) / m if m > 0 else float("inf"))
    return out


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def judged(R):
    """(name, tensor key, index) of everything held to the bar: dgi and dh0 per block of rows, dW_hh and db_hh whole."""
    out = []
    for i, b in enumerate(blocks(R)):
        out.append((f"dgi[block {i}]", "dgi", (slice(None), b)))
        out.append((f"dh0[block {i}]", "dh0", (b,)))
    return out + [("dW_hh", "dW_hh", ()), ("db_hh", "db_hh", ())]


def errors(got, ref, twin, R):
    """[(name, err of got, err of the fp32 twin)] against the fp64 reference, relative Frobenius."""
    return [(name, rel(got[k][ix], ref[k][ix]), rel(twin[k][ix], ref[k][ix])) for name, k, ix in judged(R)]


def bar(err_twin, K):
    return max(FLOOR, K * err_twin)


def fp64_trajectory(gi, w_hh, b_hh, h0):
    with torch.no_grad():
        return gru_fp64(gi.double(), w_hh.double(), b_hh.double(), None if h0 is None else h0.double())
