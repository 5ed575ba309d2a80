// cooperative-search_amd/csrc/gru_seq.h -- the T-step GRU recurrence of the QMIX learner, forward and backward, each in ONE
// launch whatever T is (cs_gru_seq_forward / cs_gru_seq_backward, policy.hip).  Included by policy.hip inside its anonymous
// namespace, after policy_dev.h (split-fp16 matrix path, gate nonlinearities).
//
// The reference unrolls its agent network step by step (policy/qmix.py:160-182, network/base_net.py:40-46: fc1 -> ReLU ->
// GRUCell -> fc2 per transition) and autograd walks the same T-step graph backwards: thousands of launches on E*n rows each.
// Everything but the recurrence h_t = GRUCell(x_t, h_{t-1}) is a batched GEMM over all T*R rows (learner.py does those with
// torch); what stays sequential is
//     gh = W_hh h + b_hh,  r = sigma(gi_r + gh_r),  z = sigma(gi_z + gh_z),  n = tanh(gi_n + r * gh_n),  h' = (1 - z) n + z h
// with gi = W_ih x + b_ih precomputed for all t (gate rows ordered [r | z | n], torch.nn.GRUCell), and its adjoint.
//
// Layout (both kernels): a block of 4 wavefronts owns 16 rows for all T steps -- no communication between blocks, no atomics,
// results independent of the grid.  The W_hh fragments of a wavefront are read from the fp32 torch tensor and split ONCE into
// registers (the weights change every learn step: no host packing).  The per-step exchange goes through double-buffered split
// planes in LDS with one barrier per step; the inputs of the next step (gi_{t+1}, or dH_{t-1} and the saved gates) do not
// depend on the recurrence and are loaded one step ahead.
#pragma once

constexpr int G3 = 3 * H;          // gate rows [r | z | n]
constexpr int GST = G3 + 8;        // halves per LDS row of the split dgh planes: rows 400 B apart (100 dwords = 4 mod 32, like HST)
constexpr int GBLOCK = 256;        // 4 wavefronts, 16 rows

struct GruFwdParams {
    const float *w_hh, *b_hh, *gi, *h0;   // [192][64], [192], [T][R][192], [R][64] or null (zeros)
    float *h_out, *saved;                 // [T][R][64]; [T][R][4][64] = (r, z, n, gh_n) or null
    int T, rows;
};

struct GruBwdParams {
    const float *w_hh, *dh_seq, *h_seq, *h0, *saved;   // [192][64], [T][R][64], [T][R][64], [R][64] or null, [T][R][4][64]
    float *dgi, *dgh, *dh0;                            // [T][R][192], [T][R][192], [R][64] or null
    int T, rows;
};

// the B fragment (hi, lo) of 8 fp32 weights of this lane, split here
__device__ __forceinline__ BFrag split_frag(const float (&v)[8]) {
    BFrag f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        _Float16 h, l;
        split_f16(v[j], h, l);
        f.hi[j] = h;
        f.lo[j] = l;
    }
    return f;
}

// Forward.  Wavefront w owns hidden units 16w..16w+15, i.e. gate column tiles w, 4 + w, 8 + w of gh, so it forms h' for its units
// without exchanging gates: per step 3 tiles x 2 k-steps x 3 matrix instructions (split-fp16) = 18 MFMAs, then the gate math of its
// 16 x 16 elements (four rows per lane), and h' goes to LDS (split, for every wavefront's next product) and to H.  The lane keeps
// its own h_{t-1} elements in registers for the blend.  SAVE also writes (r, z, n, gh_n): what the backward needs.
// n uses libm's tanhf, not policy_dev.h's tanhf_ (1 - 2 / (1 + e^2x): ~1e-7 ABSOLUTE error, large relative error near 0): over a
// 200-step unroll with trained weights the per-step errors are carried forward and amplified, and the hardware form roughly
// doubled the drift against fp64.  The sigmoids keep the hardware form: their absolute error is a quarter of exp's relative one.
template <bool SAVE>
__global__ __launch_bounds__(GBLOCK) void k_gru_seq_fwd(GruFwdParams p) {
    __shared__ __attribute__((aligned(16))) _Float16 s_h[2][2][16 * HST];   // [step parity][hi, lo]: h_{t-1}
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int crow = (lane >> 4) * 4, col = 16 * w + (lane & 15);
    const int row0 = 16 * blockIdx.x;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // W_hh rows g*64 + col, k = 32 ks + 8 (lane >> 4) + j: the B operand of gate g, k-step ks (B[k][n] = W_hh[g*64 + n][k])
    BFrag wf[3][2];
#pragma unroll
    for (int g = 0; g < 3; g++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const float *src = p.w_hh + (size_t)(g * H + col) * H + 32 * ks + 8 * (lane >> 4);   // scalar loads: no alignment assumed
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = src[j];
            wf[g][ks] = split_frag(v);
        }
    const float bh[3] = {p.b_hh[col], p.b_hh[H + col], p.b_hh[2 * H + col]};

    size_t rowc[4];   // the lane's four rows, clamped into range for loads (rows past R compute on a copy and store nothing)
    bool valid[4];
    float hp[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = row0 + crow + r;
        valid[r] = row < p.rows;
        rowc[r] = (size_t)(valid[r] ? row : p.rows - 1);
        hp[r] = p.h0 ? p.h0[rowc[r] * H + col] : 0.0f;
        split_store(s_h[0][0], s_h[0][1], (crow + r) * HST + col, hp[r]);
    }
    float gc[3][4], gn[3][4];
    auto fetch = [&](int t, float (&g)[3][4]) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float *src = p.gi + ((size_t)t * p.rows + rowc[r]) * G3 + col;
#pragma unroll
            for (int k = 0; k < 3; k++) g[k][r] = src[k * H];
        }
    };
    fetch(0, gc);
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int r = 0; r < 4; r++) gn[k][r] = 0.0f;
    __syncthreads();

    for (int t = 0; t < p.T; t++) {
        const int cur = t & 1;
        if (t + 1 < p.T) fetch(t + 1, gn);   // block-uniform; first used at the end of the step
        h8 ah[2], al[2];
#pragma unroll
        for (int ks = 0; ks < 2; ks++) load_afrag(s_h[cur][0], s_h[cur][1], 0, ks, lane, ah[ks], al[ks]);
        f32x4 hi[3], lo[3];
#pragma unroll
        for (int g = 0; g < 3; g++) {
            hi[g] = splat4(bh[g]);   // b_hh enters the accumulator
            lo[g] = zero;
        }
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int g = 0; g < 3; g++) mfma_split(ah[ks], al[ks], wf[g][ks], hi[g], lo[g]);   // three independent chains
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float ghr = split_sum(hi[0][r], lo[0][r]), ghz = split_sum(hi[1][r], lo[1][r]), ghn = split_sum(hi[2][r], lo[2][r]);
            const float rg = sigmoidf_(gc[0][r] + ghr), zg = sigmoidf_(gc[1][r] + ghz);
            const float ng = tanhf(__builtin_fmaf(rg, ghn, gc[2][r]));   // libm: see below
            const float hn = __builtin_fmaf(zg, hp[r] - ng, ng);   // (1 - z) n + z h
            split_store(s_h[cur ^ 1][0], s_h[cur ^ 1][1], (crow + r) * HST + col, hn);   // last read before the previous barrier
            if (valid[r]) {
                const size_t tr = (size_t)t * p.rows + rowc[r];
                p.h_out[tr * H + col] = hn;
                if (SAVE) {
                    float *sv = p.saved + tr * 4 * H + col;
                    sv[0] = rg;
                    sv[H] = zg;
                    sv[2 * H] = ng;
                    sv[3 * H] = ghn;
                }
            }
            hp[r] = hn;
        }
        __syncthreads();
        // first use of the next step's gi: here, not earlier (else the compiler waits for the loads right after issuing them)
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                asm volatile("" : "+v"(gn[k][r]));
                gc[k][r] = gn[k][r];
            }
    }
}

// |v| of a finite v, 0 of an inf or a NaN: what the block's scale may look at
__device__ __forceinline__ float finite_abs(float v) {
    const float a = fabsf(v);
    return a < __builtin_inff() ? a : 0.0f;
}
// 2^k as a float, -126 <= k <= 127
__device__ __forceinline__ float pow2f_(int k) { return __int_as_float((127 + k) << 23); }
// largest of a non-negative int over the wavefront, in every lane's hands as a scalar: quads, half rows and rows by DPP (register
// to register, no LDS), then the four rows of 16 lanes through scalar registers
__device__ __forceinline__ int wave_max_nonneg(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
constexpr int NO_EXP = -(1 << 20);   // s_exp of a wavefront whose dgh_t holds no finite non-zero value

// Backward, t = T-1 .. 0.  Wavefront w owns hidden units 16w..16w+15 again: with dh = dH_t + carry it forms the gate adjoints of its
// units (dgi_t = [da_r, da_z, da_n], dgh_t = [da_r, da_z, da_n r]), writes them out and into LDS (split), and after the barrier
// multiplies the whole dgh_t row tile (K = 192) by ITS 16 columns of W_hh: carry = dh z + dgh_t W_hh, output tile w -- the same
// (row, unit) elements the lane owns, so the carry never leaves its registers.  6 k-steps x 3 = 18 MFMAs per step, as two
// independent accumulator pairs (even / odd k-steps).
//
// Scaling: gradients have no natural scale, and the split-fp16 operands keep 22 significant bits only inside fp16's normal range
// and SATURATE at +-65504 (split_f16).  The block therefore runs its recurrence on (true value) * 2^s and multiplies every output
// by 2^-s on its way out; powers of two, so the scaling itself is exact.  s starts at s0, chosen from one pass over the block's
// rows of dH so that the largest finite |dH| lies in [32, 64).  dH alone does not bound what goes through the matrix path: that is
// dgh_t, formed from dH_t 2^s + carry, and the carry can grow along the recurrence by many orders of magnitude (same-sign
// gradients, |W_hh| large).  So s FOLLOWS dgh: in the shadow of step t's MFMAs every wavefront reduces the largest finite
// |dgh_t| and |dh| of its elements (dh too: it is what the carry hands on through dh z when every gate of a step is saturated
// and dgh_t all but vanishes; registers, DPP, no LDS traffic) and publishes its exponent in TRUE units (minus s: an integer, so it
// cannot overflow) in s_exp[t & 1][w]; the barrier of step t - 1 makes the four values visible, and at the end of step t - 1
// the carry is moved by an exact power of two to s = min(s0 + 5, 5 - E_t), E_t that exponent: the largest |dgh| or |dh| of
// two steps earlier lies in [32, 64), which leaves a factor of 1023 for the growth over TWO STEPS (not, as a scale fixed from dH
// would, over the whole recurrence; the lag spares a second barrier per step, the instructions themselves are not free: measured
// +0.14 us per step, 304 -> 333 us per launch at T = 200).  s may rise above s0 when
// the carry decays (dH concentrated on the last steps), but by 2^5 at the most, so dH_t 2^s never exceeds 2048 whatever comes.
// Below the largest value the planes resolve 2^-35 absolutely (the lo plane's subnormal halves): a block has ONE scale, and a row
// much smaller than the block's largest is accurate relative to that row, not to itself.  Non-finite values are left out of both
// maxima, element by element: a row that carries an inf or a NaN keeps it (rows do not mix in the products) and the block's other rows keep their
// scale.  No atomics, nothing depends on the grid.
__global__ __launch_bounds__(GBLOCK) void k_gru_seq_bwd(GruBwdParams p) {
    __shared__ __attribute__((aligned(16))) _Float16 s_g[2][2][16 * GST];   // [step parity][hi, lo]: dgh_t
    __shared__ float s_max[4];
    __shared__ __attribute__((aligned(16))) int s_exp[2][4];   // [step parity][wavefront]: exponent of the wavefront's largest finite |dgh_t|, true units
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int crow = (lane >> 4) * 4, col = 16 * w + (lane & 15);
    const int row0 = 16 * blockIdx.x;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // B[k][n] = W_hh[k][n], k over the 192 gate rows, n = this wavefront's units: lane holds k = 32 ks + 8 (lane >> 4) + j, n = col
    BFrag wf[6];
#pragma unroll
    for (int ks = 0; ks < 6; ks++) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = p.w_hh[(size_t)(32 * ks + 8 * (lane >> 4) + j) * H + col];
        wf[ks] = split_frag(v);
    }

    // the block's scale: largest |dH| over its rows and all t (16 threads per row, four values each)
    {
        float m = 0.0f;
        const int srow = row0 + (threadIdx.x >> 4), k4 = 4 * (threadIdx.x & 15);
        if (srow < p.rows)
            for (int t = 0; t < p.T; t++) {
                const float *v = p.dh_seq + ((size_t)t * p.rows + srow) * H + k4;
                m = fmaxf(m, fmaxf(fmaxf(finite_abs(v[0]), finite_abs(v[1])), fmaxf(finite_abs(v[2]), finite_abs(v[3]))));
            }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        if (lane == 0) s_max[w] = m;
        if (threadIdx.x < 8) (&s_exp[0][0])[threadIdx.x] = NO_EXP;
    }
    __syncthreads();
    const float m = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    int s0 = 0;   // m == 0 (no finite non-zero dH): scale 1
    if (m > 0.0f) {
        int e;
        frexpf(m, &e);          // m = f 2^e, f in [0.5, 1)
        e = e < -120 ? -120 : e;
        s0 = 6 - e;             // -122 .. 126: 2^s0 and 2^-s0 are normal floats
    }
    const int s_cap = min(s0 + 5, 126);
    int s = __builtin_amdgcn_readfirstlane(s0);
    float scale = pow2f_(s), unscale = pow2f_(-s);

    size_t rowc[4];
    bool valid[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = row0 + crow + r;
        valid[r] = row < p.rows;
        rowc[r] = (size_t)(valid[r] ? row : p.rows - 1);
    }
    // inputs of step t: dH_t, the saved (r, z, n, gh_n) and h_{t-1}
    struct StepIn {
        float dh[4], sv[4][4], hp[4];
    };
    auto fetch = [&](int t, StepIn &s) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t tr = (size_t)t * p.rows + rowc[r];
            s.dh[r] = p.dh_seq[tr * H + col];
#pragma unroll
            for (int k = 0; k < 4; k++) s.sv[k][r] = p.saved[(tr * 4 + k) * H + col];
            s.hp[r] = t > 0 ? p.h_seq[(tr - p.rows) * H + col] : (p.h0 ? p.h0[rowc[r] * H + col] : 0.0f);
        }
    };
    StepIn cur, nxt;
    fetch(p.T - 1, cur);
    nxt = cur;
    float carry[4] = {0.f, 0.f, 0.f, 0.f};

    for (int t = p.T - 1; t >= 0; t--) {
        const int buf = t & 1;
        if (t > 0) fetch(t - 1, nxt);   // block-uniform; first used at the end of the step
        float dhz[4], g[4][4];   // g: dgh_t and dh of the lane's elements, kept for the scale's maximum (taken after the barrier)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float dh = __builtin_fmaf(cur.dh[r], scale, carry[r]);   // exact product: scale is a power of two
            const float rg = cur.sv[0][r], zg = cur.sv[1][r], ng = cur.sv[2][r], ghn = cur.sv[3][r];
            const float dn = dh * (1.0f - zg), dz = dh * (cur.hp[r] - ng);
            const float dan = dn * (1.0f - ng * ng);
            const float dar = (dan * ghn) * (rg * (1.0f - rg));
            const float daz = dz * (zg * (1.0f - zg));
            const float dghn = dan * rg;
            dhz[r] = dh * zg;
            g[0][r] = dar;
            g[1][r] = daz;
            g[2][r] = dghn;
            g[3][r] = dh;
            split_store(s_g[buf][0], s_g[buf][1], (crow + r) * GST + col, dar);
            split_store(s_g[buf][0], s_g[buf][1], (crow + r) * GST + H + col, daz);
            split_store(s_g[buf][0], s_g[buf][1], (crow + r) * GST + 2 * H + col, dghn);
            if (valid[r]) {
                const size_t o = ((size_t)t * p.rows + rowc[r]) * G3 + col;
                p.dgi[o] = dar * unscale;
                p.dgi[o + H] = daz * unscale;
                p.dgi[o + 2 * H] = dan * unscale;
                p.dgh[o] = dar * unscale;
                p.dgh[o + H] = daz * unscale;
                p.dgh[o + 2 * H] = dghn * unscale;
            }
        }
        __syncthreads();   // dgh_t complete in s_g[buf] (last read in step t + 2, before the previous barrier)
        const int4 e4 = *reinterpret_cast<const int4 *>(s_exp[buf ^ 1]);   // step t + 1's exponents: read first, used last
        f32x4 hi0 = {dhz[0], dhz[1], dhz[2], dhz[3]}, lo0 = zero, hi1 = zero, lo1 = zero;
#pragma unroll
        for (int ks = 0; ks < 6; ks += 2) {
            h8 ah0, al0, ah1, al1;
            load_afrag<GST>(s_g[buf][0], s_g[buf][1], 0, ks, lane, ah0, al0);
            load_afrag<GST>(s_g[buf][0], s_g[buf][1], 0, ks + 1, lane, ah1, al1);
            mfma_split(ah0, al0, wf[ks], hi0, lo0);
            mfma_split(ah1, al1, wf[ks + 1], hi1, lo1);
        }
        // the scale follows dgh (see above): publish this step's exponent, adopt the one of the step before (visible since the
        // barrier).  All of it here, among the MFMAs, where vector instructions are nearly free -- not before the barrier
        {
            float big = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                asm volatile("" : "+v"(g[0][r]), "+v"(g[1][r]), "+v"(g[2][r]), "+v"(g[3][r]));
                big = fmaxf(fmaxf(big, finite_abs(g[3][r])), fmaxf(fmaxf(finite_abs(g[0][r]), finite_abs(g[1][r])), finite_abs(g[2][r])));
            }
            const int mb = wave_max_nonneg(__float_as_int(big));   // bits of a finite float >= 0: ordered like the floats
            if (lane == 0) s_exp[buf][w] = mb ? (mb >> 23) - 127 - s : NO_EXP;
        }
        const int E = __builtin_amdgcn_readfirstlane(max(max(e4.x, e4.y), max(e4.z, e4.w)));   // NO_EXP at t = T - 1
        const int s_next = E != NO_EXP ? min(s_cap, max(5 - E, -122)) : s;
#pragma unroll
        for (int r = 0; r < 4; r++) carry[r] = ldexpf(split_sum(hi0[r] + hi1[r], lo0[r] + lo1[r]), s_next - s);   // exact: 2^(s' - s)
        s = s_next;
        scale = pow2f_(s);
        unscale = pow2f_(-s);
        // first use of the next step's inputs: here (see the forward)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            asm volatile("" : "+v"(nxt.dh[r]), "+v"(nxt.hp[r]));
#pragma unroll
            for (int k = 0; k < 4; k++) asm volatile("" : "+v"(nxt.sv[k][r]));
        }
        cur = nxt;
    }
    if (p.dh0)
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (valid[r]) p.dh0[rowc[r] * H + col] = carry[r] * unscale;
}
