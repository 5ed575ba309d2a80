// cooperative-search_amd/csrc/label.h -- cs_label_episodes: an expert relabels a recorded batch of episodes in ONE launch
// (included by episodes.hip inside its namespace, after belief.h whose bel_* helpers and coverage.h whose cov_* helpers it
// calls).
//
// The labels are DEFINED by imitate.label_episodes_torch, which loops baseline.coverage_actions_torch or
// belief.belief_actions_torch over the rows t = 0..T-1 of s [E][T][S] from a fresh grid; this kernel reproduces its labels, its
// final grid and its final stored positions element for element.  Done with k_coverage_actions / k_belief_actions that is T
// launches, each of which reads and writes the whole grid in HBM; here the expert's grid never leaves LDS until the episode ends.
//
// Layout: one workgroup of 256 threads per EPISODE.  Two LDS arrays of 64 * 64 words (32 KB: four workgroups per CU): G, the
// expert's grid, and W, the working copy of the choose loop -- for the belief expert first the scatter accumulator, as acc is in
// k_belief_actions.  Every thread reads lens[e] once (uniform over the block) and the block walks the live rows in order:
//   quantise   lane i < n keeps agent i's previous position as prev (px, py) and quantises the new one from s[e][t]
//   predict    belief rows with moved = moving && t > 0 && (t - 1) % every == 0: zero W | barrier | bel_scatter G -> W | barrier
//   update     cap (moved) or clamp, and sweep (belief), or regrow and sweep (coverage): -> G and W, every cell once
//   choose     the loop of coverage.h on W; thread 0 writes labels[e][t][i]
// After the loop the rows t >= lens[e] get label 0, and G and the last positions go to grid_out / prev_out (either may be null),
// 16 bytes per lane where the row allows.  No global atomics, no host synchronisation; LDS atomics are bel_spread's only.
//
// What could go wrong in this shape, and why it does not:
//   a barrier inside a diverging branch   every __syncthreads() stands outside any branch on tid, side, expert, moved or the data:
//                                         the two barriers of the predict step are executed on every row, moved or not.  The trip
//                                         count len is the same in all 256 threads: each reads the same word lens[e] (clamped to
//                                         0..T here, whatever the entry point's caller wrote there).
//   a row races with the one before       the choose loop ends on a barrier, so ax, ay, ah, red and pick are free when the next
//                                         row's quantise writes them; px[i] / py[i] are written by the lane that owns ax[i].
//   overflow over many rows               nothing accumulates across rows but G, and G leaves every row bounded as sections 17 and
//                                         20 need it on entry: a coverage cell is clamped to 0..65536 as it is read and the regrowth
//                                         and the sweep keep it there; a belief cell leaves bel_update in 0..CAP = 2^19 (FRESH = 2^16
//                                         is inside), so one row's scatter sums to at most 2^12 * 2^19 = 2^31 < 2^32 wherever it lands.
//   prev at t = 0                         ax, ay start as 0, the definition's fresh prev; a stored position is a quantised one,
//                                         |X| <= 2^15, so belief.h's clamp on reading prev changes nothing.  Slots i >= n stay 0.
//   side^2 < 256 leaves idle threads      they run no loop body and fall through to every barrier.
//   side = 64 fills both arrays           cells = 4096 = each array; every index is < cells (the cell loops) or ci * side + cj with
//                                         ci, cj clamped to 0..side - 1 (bel_spread, cov_box).
//   NaN or huge state floats              cov_quant clamps (NaN to the lower bound), as in the definition; rows t >= lens[e] are
//                                         never read.
//   E * T * S or E * T * n past 2^31      every global index is formed in size_t.
//   unaligned rows                        the 16-byte accesses are taken only where the entry point found base and row pitch
//                                         aligned (svec, vec4, lvec); otherwise words.
constexpr int LABEL_COVERAGE = 0, LABEL_BELIEF = 1;

struct LabelArgs {
    BeliefArgs b;            // b.c: state = s, actions = labels, n, side, S, R, keep, regrow, look16, vec4 (grid_out rows); b.c.grid and
                             // b.prev unused; mode, sense2, dx, dy; b.moved is set per row inside the kernel's own copy
    const int32_t *lens;     // [E]
    int32_t *grid_out;       // [E][side * side] or null
    int32_t *prev_out;       // [E][8][2] or null
    int T, expert, every, moving;
    int svec;                // a state row starts on a 16-byte boundary and S % 4 == 0
    int lvec;                // labels is 16-byte aligned
};

__global__ __launch_bounds__(COV_THREADS) void k_label_episodes(LabelArgs a) {
    __shared__ __attribute__((aligned(16))) int G[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ __attribute__((aligned(16))) unsigned W[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS], px[CS_MAX_AGENTS], py[CS_MAX_AGENTS];
    __shared__ int ox[BEL_HEADINGS], fx[BEL_HEADINGS], oy[BEL_HEADINGS], fy[BEL_HEADINGS];
    __shared__ unsigned red[COV_WAVES][3];
    __shared__ int pick;
    const CoverageArgs &c = a.b.c;
    const int tid = threadIdx.x;
    const size_t e = blockIdx.x;
    const int n = c.n, side = c.side, cells = side * side, T = a.T;
    const unsigned R2 = (unsigned)c.R * (unsigned)c.R;
    const int len = min(max(a.lens[e], 0), T);
    const bool belief = a.expert == LABEL_BELIEF;
    // the cell loops step idx by 256 without dividing: (ix, iy) moves by (256 / side, 256 % side) with one carry
    const int ix0 = tid / side, iy0 = tid - ix0 * side, dix = COV_THREADS / side, diy = COV_THREADS - dix * side;
    // 0. a fresh expert: G = FRESH everywhere, prev zero
    for (int idx = tid; idx < cells; idx += COV_THREADS) G[idx] = 65536;
    if (tid < CS_MAX_AGENTS) {
        ax[tid] = 0;
        ay[tid] = 0;
    }
    if (tid >= 64 && tid < 64 + BEL_HEADINGS) {   // (another wavefront than the agents')
        const int k = tid - 64;
        ox[k] = a.b.dx[k] >> 4;
        fx[k] = a.b.dx[k] & 15;
        oy[k] = a.b.dy[k] >> 4;
        fy[k] = a.b.dy[k] & 15;
    }
    __syncthreads();
    for (int t = 0; t < len; t++) {
        const bool moved = belief && a.moving && t > 0 && (t - 1) % a.every == 0;
        // 1. quantise: lane i owns agent i; its last position becomes prev
        if (tid < n) {
            const float *s = c.state + (e * (size_t)T + (size_t)t) * (size_t)c.S + 4 * tid;
            float s0, s1, s2, s3;
            if (a.svec) {
                const float4 v = *reinterpret_cast<const float4 *>(s);
                s0 = v.x, s1 = v.y, s2 = v.z, s3 = v.w;
            } else {
                s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
            }
            const float half = (float)side / 2.0f;
            const int X = cov_quant((s0 * half + half) * 16.0f, COV_POS_LIM), Y = cov_quant((s1 * half + half) * 16.0f, COV_POS_LIM);
            const int cq = cov_quant(s2 * 16384.0f, COV_TRIG_LIM), sn = cov_quant(s3 * 16384.0f, COV_TRIG_LIM);
            int best = cq * COV_CT[0] + sn * COV_ST[0], h = 0;   // |c CT + s ST| <= 2^29
            for (int k = 1; k < COV_HEADINGS; k++) {
                const int d = cq * COV_CT[k] + sn * COV_ST[k];
                if (d > best) {
                    best = d;
                    h = k;
                }
            }
            px[tid] = ax[tid];
            py[tid] = ay[tid];
            ax[tid] = X;
            ay[tid] = Y;
            ah[tid] = h;
        }
        if (moved)
            for (int idx = tid; idx < cells; idx += COV_THREADS) W[idx] = 0u;
        __syncthreads();
        // 2. predict (belief, moved): every source cell of G scatters its mass into W
        if (moved) {
            int ix = ix0, iy = iy0;
            for (int idx = tid; idx < cells; idx += COV_THREADS) {
                bel_scatter(a.b, W, px, py, ox, fx, oy, fy, ix, iy, G[idx]);
                ix += dix;
                if ((iy += diy) >= side) {
                    iy -= side;
                    ix++;
                }
            }
        }
        __syncthreads();
        // 3. cap or clamp and sweep (belief), regrow and sweep (coverage): -> G and W, every cell once
        {
            int ix = ix0, iy = iy0;
            for (int idx = tid; idx < cells; idx += COV_THREADS) {
                int g;
                if (belief) g = bel_update(a.b, ax, ay, R2, ix, iy, moved ? (long long)W[idx] : (long long)G[idx]);
                else g = cov_update(c, ax, ay, R2, ix, iy, G[idx]);
                G[idx] = g;
                W[idx] = (unsigned)g;
                ix += dix;
                if ((iy += diy) >= side) {
                    iy -= side;
                    ix++;
                }
            }
        }
        __syncthreads();
        // 4. choose, agent by agent; each claims what it chose (coverage.h's loop on W)
        for (int i = 0; i < n; i++) {
            const int X = ax[i], Y = ay[i], h = ah[i];
            unsigned sum[3];
#pragma unroll
            for (int act = 0; act < 3; act++) {
                int qx, qy;
                cov_point(c, X, Y, h, act, qx, qy);
                const CovBox box = cov_box(qx, qy, c.R, side);
                unsigned s = 0;
                for (int bx = tid >> 4; bx < box.w; bx += 16)
                    for (int by = tid & 15; by < box.h; by += 16) {
                        const int ix = box.x0 + bx, iy = box.y0 + by;
                        if (cov_within(ix, iy, qx, qy, R2)) s += W[ix * side + iy];
                    }
                sum[act] = s;
            }
#pragma unroll
            for (int act = 0; act < 3; act++) {
                for (int off = 32; off > 0; off >>= 1) sum[act] += __shfl_down(sum[act], off);
                if ((tid & 63) == 0) red[tid >> 6][act] = sum[act];
            }
            __syncthreads();
            if (tid == 0) {
                unsigned sc[3] = {0u, 0u, 0u};
                for (int w = 0; w < COV_WAVES; w++)
                    for (int act = 0; act < 3; act++) sc[act] += red[w][act];
                int best = 0;
                if (sc[1] > sc[0]) best = 1;
                if (sc[2] > sc[best]) best = 2;
                pick = best;
                c.actions[(e * (size_t)T + (size_t)t) * (size_t)n + i] = best;
            }
            __syncthreads();
            int qx, qy;
            cov_point(c, X, Y, h, pick, qx, qy);
            const CovBox box = cov_box(qx, qy, c.R, side);
            for (int bx = tid >> 4; bx < box.w; bx += 16)
                for (int by = tid & 15; by < box.h; by += 16) {
                    const int ix = box.x0 + bx, iy = box.y0 + by;
                    if (cov_within(ix, iy, qx, qy, R2)) W[ix * side + iy] = 0u;
                }
            __syncthreads();   // (also: red, pick and the agents' arrays are free for the next agent and the next row)
        }
    }
    // 5. rows past the episode's end: label 0 (k0 .. k0 + cnt - 1 of the flat labels; pairs where they are 16-byte aligned)
    {
        const size_t k0 = (e * (size_t)T + (size_t)len) * (size_t)n, cnt = (size_t)(T - len) * (size_t)n;
        int64_t *L = c.actions + k0;
        if (a.lvec) {
            const size_t head = (k0 & 1) != 0 && cnt > 0 ? 1 : 0, pairs = (cnt - head) / 2;
            if (tid == 0 && head) L[0] = 0;
            for (size_t q = tid; q < pairs; q += COV_THREADS) reinterpret_cast<longlong2 *>(L + head)[q] = make_longlong2(0, 0);
            if (tid == 0 && head + 2 * pairs < cnt) L[cnt - 1] = 0;
        } else {
            for (size_t k = tid; k < cnt; k += COV_THREADS) L[k] = 0;
        }
    }
    // 6. the expert's state after the last live row
    if (a.grid_out) {
        int32_t *out = a.grid_out + e * (size_t)cells;
        if (c.vec4)
            for (int q = tid; q < cells / 4; q += COV_THREADS) reinterpret_cast<int4 *>(out)[q] = reinterpret_cast<const int4 *>(G)[q];
        else
            for (int idx = tid; idx < cells; idx += COV_THREADS) out[idx] = G[idx];
    }
    if (a.prev_out && tid < 2 * CS_MAX_AGENTS)   // (ax, ay are 0 where no row wrote them: len == 0, slots >= n)
        a.prev_out[e * (size_t)(2 * CS_MAX_AGENTS) + tid] = (tid & 1) ? ay[tid >> 1] : ax[tid >> 1];
}
