// cooperative-search_amd/csrc/ppo.h -- the two kernels of the PPO learner (learner.PPOLearner): generalised advantage
// estimation over t in ONE launch (cs_gae) and the clipped surrogate with its entropy bonus, their statistics and the
// gradient with respect to the logits in one pass over the rows (cs_ppo_loss).  Included by policy.hip inside its anonymous
// namespace, after returns.h (RBLOCK).
//
// ---- k_gae -------------------------------------------------------------------------------------------------------------------
// Per episode row, with c = 1 - terminated, m = 1 - padded, v = V(s), v_next = V(s_next) and gl = gamma * lambda, in fp32 with
// every operation rounded once (the library is built with -ffp-contract=off), so a NumPy float32 statement of the same order
// reproduces the kernel bit for bit:
//     delta = (r + (gamma * v_next) * c) - v
//     t = T-1:  A = delta * m            t < T-1:  A = (delta + (gl * A_next) * c) * m
//     ret = (A + v) * m
// With v = v_next = 0 and lambda = 1 this is k_episode_returns<false>'s order: delta = r, A = (r + (gamma * A_next) * c) * m,
// so the advantages ARE REINFORCE's returns, bit for bit (the tests hold the two kernels together).  Padded steps are exactly
// zero (m = 0, finite inputs).  Layout as k_episode_returns: one lane per episode walks t = T-1 .. 0 and loads the inputs of
// step t-1 while step t computes; no atomics, no communication between lanes.
//
// ---- k_ppo_loss --------------------------------------------------------------------------------------------------------------
// One lane per row rho = (episode, step, agent) of R = E*T*n rows; row rho belongs to step rho / n (adv, mask).  The A <= 8
// values of a row live in registers.  Per live row (mask != 0), with s = softmax(logits), N = sum(avail):
//     q_a = avail_a ? (1 - eps) s_a + eps / N : 0       p_a = q_a / sum(q)              (learner.action_prob)
//     logp = log p_u      ratio = exp(logp - old_logp)      surr = min(ratio Adv, clamp(ratio, 1 - k, 1 + k) Adv)
//     H = -sum_a p_a log p_a   (0 log 0 = 0)
// and, for the loss L = inv_count * sum_rows mask * (-surr - beta H), dL/dlogits through the renormalisation, the epsilon mix
// and the softmax:
//     g_p[a] = -[a == u] g ratio / p_u + beta (log p_a + 1) [p_a > 0]      g = Adv where the unclipped term is the active one
//     g_q[b] = avail_b ? (g_p[b] - sum_a g_p[a] p_a) / sum(q) : 0          (1 - k <= ratio <= 1 + k, both ends included, or
//     g_s[b] = (1 - eps) g_q[b]                                             ratio Adv < clamp(ratio) Adv), else 0: what
//     dlogits[c] = mask inv_count s_c (g_s[c] - sum_b g_s[b] s_b)           torch.clamp and torch.minimum send back
// A row with mask == 0 is skipped before any arithmetic (its avail row may be all zeros: N = 0): its dlogits are written as
// zeros, its logp as 0 and it adds nothing to any sum.  The four sums (surr, H, [ratio outside the clip range], old_logp -
// logp; each times mask) are reduced over the wavefront by shuffles in a fixed order, over the block's four wavefronts through
// LDS in index order, and leave the block as ONE partial (4 floats) in the scratch buffer; k_ppo_finish (one block) adds the
// partials -- lane l of a wavefront takes partials l, l + 64, .. in index order, then the 64 lane sums in the same shuffle
// tree -- and scales them by inv_count.  No atomics: the block size is fixed (PPO_BLOCK), so the order of every sum is a
// function of R alone and reruns are bit-identical.
// FULL = false (old_logp null: the learner's no-grad pass) runs the same instructions up to logp and writes logp only, so the
// first epoch's ratio is exp(0) = 1 exactly.
#pragma once

struct GaeParams {
    const float *r, *term, *pad, *v, *v_next;   // [E][T] each
    float *adv, *ret;                           // [E][T]
    int E, T;
    float gamma, lambda;
};

__global__ __launch_bounds__(RBLOCK) void k_gae(GaeParams p) {
    const int e = blockIdx.x * RBLOCK + threadIdx.x;
    if (e >= p.E) return;
    const size_t base = (size_t)e * (size_t)p.T;
    const float *r = p.r + base, *term = p.term + base, *pad = p.pad + base, *v = p.v + base, *vn = p.v_next + base;
    float *adv = p.adv + base, *ret = p.ret + base;
    const float gamma = p.gamma, gl = p.gamma * p.lambda;

    int t = p.T - 1;
    float rt = r[t], tt = term[t], pt = pad[t], vt = v[t], nt = vn[t];
    float acc = 0.0f;
    for (; t >= 0; --t) {
        const float rc = rt, cc = 1.0f - tt, mc = 1.0f - pt, vc = vt, nc = nt;
        if (t > 0) {   // step t-1's inputs, loaded before step t's arithmetic
            rt = r[t - 1];
            tt = term[t - 1];
            pt = pad[t - 1];
            vt = v[t - 1];
            nt = vn[t - 1];
        }
        const float delta = (rc + (gamma * nc) * cc) - vc;
        acc = t == p.T - 1 ? delta * mc : (delta + (gl * acc) * cc) * mc;
        adv[t] = acc;
        ret[t] = (acc + vc) * mc;
    }
}

constexpr int PPO_BLOCK = CS_PPO_BLOCK;   // rows per block = partials' granularity (the caller sizes the scratch buffer by it)
constexpr int PPO_WAVES = PPO_BLOCK / 64;

struct PpoParams {
    const float *logits, *avail;   // [R][A]
    const int64_t *u;              // [R]
    const float *old_logp;         // [R] (FULL)
    const float *adv, *mask;       // [R / n] (adv: FULL)
    const float *eps_dev;          // null: `epsilon`
    const float *inv_count;        // [1] (FULL)
    float *dlogits;                // [R][A] (FULL)
    float *logp_out;               // [R] or null (FULL); [R] (!FULL)
    float *scratch;                // [blocks][4] (FULL)
    long long R;
    int n;
    float clip, beta, epsilon;
};

// the sum of v over the wavefront's 64 lanes, in lane 0: a fixed tree (32, 16, .. 1)
__device__ inline float ppo_wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <int A, bool FULL>
__global__ __launch_bounds__(PPO_BLOCK) void k_ppo_loss(PpoParams p) {
    __shared__ float s_part[PPO_WAVES][4];
    const long long row = (long long)blockIdx.x * PPO_BLOCK + threadIdx.x;
    float sum_surr = 0.0f, sum_ent = 0.0f, sum_clip = 0.0f, sum_kl = 0.0f;
    if (row < p.R) {
        const long long step = row / p.n;
        const float m = p.mask[step];
        float dz[A];
#pragma unroll
        for (int a = 0; a < A; a++) dz[a] = 0.0f;
        float logp = 0.0f;
        if (m != 0.0f) {
            const float eps = p.eps_dev ? p.eps_dev[0] : p.epsilon;
            const float *zr = p.logits + (size_t)row * A, *ar = p.avail + (size_t)row * A;
            const int ui = (int)p.u[row];
            float z[A], av[A], s[A], pr[A], lp[A];
#pragma unroll
            for (int a = 0; a < A; a++) {
                z[a] = zr[a];
                av[a] = ar[a];
            }
            float mx = z[0], N = av[0];
#pragma unroll
            for (int a = 1; a < A; a++) {
                mx = fmaxf(mx, z[a]);
                N += av[a];
            }
            float den = 0.0f;
#pragma unroll
            for (int a = 0; a < A; a++) {
                s[a] = expf(z[a] - mx);
                den += s[a];
            }
            const float mixed = eps / N, keep = 1.0f - eps;
            float S = 0.0f;
#pragma unroll
            for (int a = 0; a < A; a++) {
                s[a] = s[a] / den;
                pr[a] = av[a] != 0.0f ? keep * s[a] + mixed : 0.0f;
                S += pr[a];
            }
            float pu = 0.0f;
#pragma unroll
            for (int a = 0; a < A; a++) {
                pr[a] = pr[a] / S;
                lp[a] = pr[a] > 0.0f ? logf(pr[a]) : 0.0f;
                if (a == ui) {
                    pu = pr[a];
                    logp = pr[a] > 0.0f ? lp[a] : logf(pr[a]);   // an unavailable action taken: log 0, as in torch
                }
            }
            if (FULL) {
                const float adv = p.adv[step], old = p.old_logp[row], inv = p.inv_count[0];
                const float ratio = expf(logp - old);
                const float lo = 1.0f - p.clip, hi = 1.0f + p.clip;
                const float clamped = fminf(fmaxf(ratio, lo), hi);
                const float s1 = ratio * adv, s2 = clamped * adv;
                const bool outside = ratio < lo || ratio > hi;
                const float g = (!outside || s1 < s2) ? adv : 0.0f;
                float ent = 0.0f;
#pragma unroll
                for (int a = 0; a < A; a++) ent -= pr[a] * lp[a];
                sum_surr = fminf(s1, s2) * m;
                sum_ent = ent * m;
                sum_clip = outside ? m : 0.0f;
                sum_kl = (old - logp) * m;
                // back through p = q / sum(q), q = (1 - eps) s + eps / N on the available actions, s = softmax(z)
                float gp[A], dot = 0.0f;
#pragma unroll
                for (int a = 0; a < A; a++) {
                    gp[a] = pr[a] > 0.0f ? p.beta * (lp[a] + 1.0f) : 0.0f;
                    if (a == ui) gp[a] -= g * ratio / pu;
                    dot += gp[a] * pr[a];
                }
                float gs[A], dot_s = 0.0f;
#pragma unroll
                for (int a = 0; a < A; a++) {
                    gs[a] = av[a] != 0.0f ? keep * ((gp[a] - dot) / S) : 0.0f;
                    dot_s += gs[a] * s[a];
                }
                const float w = m * inv;
#pragma unroll
                for (int a = 0; a < A; a++) dz[a] = w * (s[a] * (gs[a] - dot_s));
            }
        }
        if (FULL) {
            float *dr = p.dlogits + (size_t)row * A;
#pragma unroll
            for (int a = 0; a < A; a++) dr[a] = dz[a];
        }
        if (p.logp_out) p.logp_out[row] = logp;
    }
    if (!FULL) return;
    // every lane of the block arrives here: the four sums over the wavefront, then over the block's wavefronts in index order
    sum_surr = ppo_wave_sum(sum_surr);
    sum_ent = ppo_wave_sum(sum_ent);
    sum_clip = ppo_wave_sum(sum_clip);
    sum_kl = ppo_wave_sum(sum_kl);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        s_part[wave][0] = sum_surr;
        s_part[wave][1] = sum_ent;
        s_part[wave][2] = sum_clip;
        s_part[wave][3] = sum_kl;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float acc = s_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < PPO_WAVES; w++) acc += s_part[w][threadIdx.x];
        p.scratch[(size_t)blockIdx.x * 4 + threadIdx.x] = acc;
    }
}

struct PpoFinishParams {
    const float *scratch;     // [blocks][4]
    const float *inv_count;   // [1]
    float *stats;             // [4]: policy loss, mean entropy, clip fraction, mean(old_logp - logp)
    int blocks;
};

// One block of 4 wavefronts, wavefront k sums statistic k.
__global__ __launch_bounds__(256) void k_ppo_finish(PpoFinishParams p) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc = 0.0f;
    for (int b = lane; b < p.blocks; b += 64) acc += p.scratch[(size_t)b * 4 + k];
    acc = ppo_wave_sum(acc);
    if (lane == 0) {
        const float mean = acc * p.inv_count[0];
        p.stats[k] = k == 0 ? -mean : mean;
    }
}
