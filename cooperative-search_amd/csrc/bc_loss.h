// cooperative-search_amd/csrc/bc_loss.h -- the kernel of the imitation learner (imitate.ImitationLearner): the masked
// cross-entropy between the actor's action probabilities and an expert's labels, its statistics and its gradient with respect
// to the logits in one pass over the rows (cs_bc_loss).  Included by policy.hip inside its anonymous namespace, after ppo.h
// (PPO_BLOCK, PPO_WAVES, ppo_wave_sum).  DEFINED by imitate.bc_loss_torch; DESIGN.md section 23.
//
// ---- k_bc_loss ---------------------------------------------------------------------------------------------------------------
// k_ppo_loss's layout: one lane per row rho = (episode, step, agent) of R = E*T*n rows; row rho belongs to step rho / n (mask).
// The A <= 8 values of a row live in registers.  Per live row (mask != 0), with s = softmax(logits) and u the label:
//     q_a = avail_a ? s_a : 0        p_a = q_a / sum(q)                         (learner.action_prob with epsilon = 0)
//     ce = avail_u ? -log p_u : 0    hit = avail_u && u == the lowest a that maximises p_a
//     H = -sum_a p_a log p_a   (0 log 0 = 0)
// and, for the loss L = inv_count * sum_rows mask * ce, the gradient of a masked softmax's cross-entropy in closed form:
//     dlogits[c] = avail_u ? mask inv_count (p_c - [c == u]) : 0      (p_c = 0 on an unavailable action: no gradient there)
// A live row whose label is unavailable -- or lies outside 0..A-1, which no avail row can make available -- adds no loss and no
// gradient and counts as a miss; its entropy is counted.  A row with mask == 0 is skipped before any arithmetic (its avail row
// may be all zeros): its dlogits are written as zeros and it adds nothing to any sum.  The three sums (ce, hit, H; each times
// mask) are reduced as k_ppo_loss reduces its four: over the wavefront by shuffles in a fixed order, over the block's four
// wavefronts through LDS in index order, ONE partial (3 floats) per block in the scratch buffer; k_bc_finish (one block) adds
// the partials -- lane l of a wavefront takes partials l, l + 64, .. in index order, then the 64 lane sums in the same shuffle
// tree -- and scales them by inv_count.  No atomics: the block size is fixed (PPO_BLOCK), so the order of every sum is a
// function of R alone and reruns are bit-identical.
#pragma once

struct BcParams {
    const float *logits, *avail;   // [R][A]
    const int64_t *labels;         // [R]
    const float *mask;             // [R / n]
    const float *inv_count;        // [1]
    float *dlogits;                // [R][A]
    float *scratch;                // [blocks][3]
    long long R;
    int n;
};

template <int A>
__global__ __launch_bounds__(PPO_BLOCK) void k_bc_loss(BcParams p) {
    __shared__ float s_part[PPO_WAVES][3];
    const long long row = (long long)blockIdx.x * PPO_BLOCK + threadIdx.x;
    float sum_ce = 0.0f, sum_hit = 0.0f, sum_ent = 0.0f;
    if (row < p.R) {
        const float m = p.mask[row / p.n];
        float dz[A];
#pragma unroll
        for (int a = 0; a < A; a++) dz[a] = 0.0f;
        if (m != 0.0f) {
            const float *zr = p.logits + (size_t)row * A, *ar = p.avail + (size_t)row * A;
            const long long ul = p.labels[row];
            const int ui = ul >= 0 && ul < A ? (int)ul : -1;
            float z[A], av[A], pr[A];
#pragma unroll
            for (int a = 0; a < A; a++) {
                z[a] = zr[a];
                av[a] = ar[a];
            }
            float mx = z[0];
#pragma unroll
            for (int a = 1; a < A; a++) mx = fmaxf(mx, z[a]);
            float den = 0.0f;
#pragma unroll
            for (int a = 0; a < A; a++) {
                pr[a] = expf(z[a] - mx);
                den += pr[a];
            }
            float S = 0.0f;
#pragma unroll
            for (int a = 0; a < A; a++) {
                pr[a] = av[a] != 0.0f ? pr[a] / den : 0.0f;
                S += pr[a];
            }
            float pu = 0.0f, top = -1.0f, ent = 0.0f;
            int arg = 0;
            bool live = false;   // is the label an available action?
#pragma unroll
            for (int a = 0; a < A; a++) {
                pr[a] = pr[a] / S;
                if (pr[a] > 0.0f) ent -= pr[a] * logf(pr[a]);
                if (pr[a] > top) {   // strict: the lowest index on ties
                    top = pr[a];
                    arg = a;
                }
                if (a == ui) {
                    pu = pr[a];
                    live = av[a] != 0.0f;
                }
            }
            sum_ent = ent * m;
            if (live) {
                const float w = m * p.inv_count[0];
                sum_ce = -logf(pu) * m;
                sum_hit = arg == ui ? m : 0.0f;
#pragma unroll
                for (int a = 0; a < A; a++) dz[a] = w * (pr[a] - (a == ui ? 1.0f : 0.0f));
            }
        }
        float *dr = p.dlogits + (size_t)row * A;
#pragma unroll
        for (int a = 0; a < A; a++) dr[a] = dz[a];
    }
    // every lane of the block arrives here: the three sums over the wavefront, then over the block's wavefronts in index order
    sum_ce = ppo_wave_sum(sum_ce);
    sum_hit = ppo_wave_sum(sum_hit);
    sum_ent = ppo_wave_sum(sum_ent);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        s_part[wave][0] = sum_ce;
        s_part[wave][1] = sum_hit;
        s_part[wave][2] = sum_ent;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float acc = s_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < PPO_WAVES; w++) acc += s_part[w][threadIdx.x];
        p.scratch[(size_t)blockIdx.x * 3 + threadIdx.x] = acc;
    }
}

struct BcFinishParams {
    const float *scratch;     // [blocks][3]
    const float *inv_count;   // [1]
    float *stats;             // [3]: loss, agreement, mean entropy
    int blocks;
};

// One block of 4 wavefronts, wavefront k < 3 sums statistic k.
__global__ __launch_bounds__(256) void k_bc_finish(BcFinishParams p) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (k >= 3) return;
    float acc = 0.0f;
    for (int b = lane; b < p.blocks; b += 64) acc += p.scratch[(size_t)b * 3 + k];
    acc = ppo_wave_sum(acc);
    if (lane == 0) p.stats[k] = acc * p.inv_count[0];
}
