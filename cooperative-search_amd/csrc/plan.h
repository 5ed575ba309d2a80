// cooperative-search_amd/csrc/plan.h -- cs_plan_actions: a receding-horizon sequence search over a base policy's grid, one launch
// per decision (included by episodes.hip inside its namespace, after coverage.h whose cov_* helpers and heading tables it uses;
// DESIGN.md section 21).
//
// The planner is DEFINED by plan.plan_actions_torch (stock torch ops); this kernel reproduces its actions, its plans and its
// scores element for element.  Nothing is floating point but the quantisation of an agent's four state floats (coverage.h's).
// Per agent, in index order: the 3 + 9 + .. + 3^D <= 363 nodes of the turn-sequence tree are walked from the agent's pose, every
// node's gain is the mass of W inside its disc and outside its ancestors' discs, every sequence's score is the discounted sum of
// its D gains, the lowest sequence of the largest score wins and its D discs are zeroed in W.
//
// Layout: one workgroup of 256 threads per env, the shape of k_coverage_actions.  LDS: W (the grid clamped to 0..2^19, 16 KB),
// the node table (one packed word per node: x | y << 11 | h << 22, x and y in 0..1024 after the first clamped step), the gains,
// the 36 step offsets and four 64-bit keys: 19.6 KB in all.  Per agent:
//   a. nodes    thread q walks node q from the agent's pose: (level + 1) * stride steps, at most 40.
//   b. gains    one wavefront per node, the nodes dealt round robin; the lanes cover the clipped bounding box of the disc in 8 x 8
//               tiles and the sum is a wavefront shuffle reduction.  Integer sums: any order gives the same bits.
//   c. scores   thread s < 3^D sums its sequence's D gains times the Q8 weights in 64 bits and packs (score << 8) | (255 - s);
//               the largest key over the block is the largest score and, among equals, the lowest s.  One shuffle reduction per
//               wavefront, four keys through LDS, and every thread reads all four: no second broadcast.
//   d. claim    the block zeroes the D discs of the winner in W (16 x 16 tiles, as coverage.h).
// A barrier follows each of a - d; every one is outside any branch that depends on tid or on the data (the trip counts n and D
// are launch arguments), so all 256 threads reach each of them.  No atomics, no global memory traffic but the one read of the
// grid row and 24 bytes of results per agent, no host synchronisation.
//
// What could go wrong in this shape, and why it does not:
//   a gain or a score overflows     a cell is read as at most 2^19 and a map has at most 2^12 cells: a gain is at most 2^31 and
//                                   fits an unsigned word.  The D gains of one sequence are sums over DISJOINT cells, so together
//                                   they are at most 2^31 and a score, with weights of at most 256, is at most 2^39; a key is below 2^48.
//   a thread with no sequence       tid >= 3^D holds key 0; a real key is at least 255 - 242 = 13, so 0 never wins.
//   the packed node word            needs x, y <= 2047 and h <= 63: after one step both coordinates are clamped to 0..16 side <=
//                                   1024 (stride >= 1 is checked by the entry point, so a node is at least one step from the pose,
//                                   whose own coordinates may be anything in +-2^15) and h < 36.
//   an index leaves W               every cell index is box.x0 + bx, box.y0 + by with the box clipped to 0..side - 1 by cov_box.
//   an index leaves the node table  q < nodes = (3^(D+1) - 3) / 2 <= 363 = the arrays; a sequence's node of level d is
//                                   first_d + s / 3^(D-1-d) < first_d + 3^(d+1).
constexpr int PLAN_MAX_DEPTH = 5;
constexpr int PLAN_MAX_STRIDE = 8;
constexpr int PLAN_MAX_NODES = 363;   // 3 + 9 + 27 + 81 + 243
constexpr int PLAN_CAP = 1 << 19;     // a cell is read as clamp(cell, 0, CAP)
constexpr int PLAN_FAR = 1 << 14;     // an x that is farther than any R <= 2^10 from every cell centre (those are below 2^10)

struct PlanArgs {
    const float *state;
    const int32_t *grid;
    int64_t *actions, *plans, *scores;
    int n, side, S, R, depth, stride, discount;   // S = floats per state row, R = 16 view_range
    int nodes, seqs;                              // (3^(depth+1) - 3) / 2 and 3^depth
    int vec4;                                     // a grid row is a whole number of aligned 16-byte pieces
};

__device__ __forceinline__ void plan_unpack(unsigned v, int &x, int &y) {
    x = (int)(v & 2047u);
    y = (int)((v >> 11) & 2047u);
}

__global__ __launch_bounds__(COV_THREADS) void k_plan_actions(PlanArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned W[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ unsigned node[PLAN_MAX_NODES], gain[PLAN_MAX_NODES];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS];
    __shared__ int sx[COV_HEADINGS], sy[COV_HEADINGS];
    __shared__ unsigned long long red[COV_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x, wave = tid >> 6, lane = tid & 63;
    const int side = a.side, cells = side * side, lim = 16 * side;
    const unsigned R2 = (unsigned)a.R * (unsigned)a.R;
    // 1. quantise: lane i owns agent i (coverage.h's); another wavefront fills the step offsets
    if (tid < a.n) {
        const float *s = a.state + (size_t)b * a.S + 4 * tid;
        const float half = (float)side / 2.0f;
        ax[tid] = cov_quant((s[0] * half + half) * 16.0f, COV_POS_LIM);
        ay[tid] = cov_quant((s[1] * half + half) * 16.0f, COV_POS_LIM);
        const int c = cov_quant(s[2] * 16384.0f, COV_TRIG_LIM), sn = cov_quant(s[3] * 16384.0f, COV_TRIG_LIM);
        int best = c * COV_CT[0] + sn * COV_ST[0], h = 0;   // |c CT + s ST| <= 2^29
        for (int k = 1; k < COV_HEADINGS; k++) {
            const int d = c * COV_CT[k] + sn * COV_ST[k];
            if (d > best) {
                best = d;
                h = k;
            }
        }
        ah[tid] = h;
    }
    if (tid >= 64 && tid < 64 + COV_HEADINGS) {
        sx[tid - 64] = (16 * COV_CT[tid - 64]) >> 14;   // (>> of a negative int is arithmetic on this compiler: it floors)
        sy[tid - 64] = (16 * COV_ST[tid - 64]) >> 14;
    }
    // 2. W = the grid row, clamped
    const int32_t *G = a.grid + (size_t)b * cells;
    if (a.vec4) {
        for (int q = tid; q < cells / 4; q += COV_THREADS) {
            int4 v = reinterpret_cast<const int4 *>(G)[q];
            v.x = min(max(v.x, 0), PLAN_CAP);
            v.y = min(max(v.y, 0), PLAN_CAP);
            v.z = min(max(v.z, 0), PLAN_CAP);
            v.w = min(max(v.w, 0), PLAN_CAP);
            reinterpret_cast<int4 *>(W)[q] = v;
        }
    } else {
        for (int idx = tid; idx < cells; idx += COV_THREADS) W[idx] = (unsigned)min(max(G[idx], 0), PLAN_CAP);
    }
    __syncthreads();
    for (int i = 0; i < a.n; i++) {
        // a. the node table: thread q walks node q from the pose
        for (int q = tid; q < a.nodes; q += COV_THREADS) {
            int d = 0, first = 0, cnt = 3;   // level d holds cnt = 3^(d+1) nodes from index first
            while (q >= first + cnt) {
                first += cnt;
                cnt *= 3;
                d++;
            }
            int j = q - first, div = cnt / 3;   // j: d + 1 base-3 digits, the most significant one the first segment
            int x = ax[i], y = ay[i], h = ah[i];
            for (int e = 0; e <= d; e++) {
                const int act = j / div;
                j -= act * div;
                div = max(div / 3, 1);
                const int turn = act == 1 ? 1 : (act == 2 ? COV_HEADINGS - 1 : 0);
                for (int s = 0; s < a.stride; s++) {
                    h += turn;
                    if (h >= COV_HEADINGS) h -= COV_HEADINGS;
                    x = min(max(x + sx[h], 0), lim);
                    y = min(max(y + sy[h], 0), lim);
                }
            }
            node[q] = (unsigned)x | ((unsigned)y << 11) | ((unsigned)h << 22);
        }
        __syncthreads();
        // b. gains: a wavefront per node
        for (int q = wave; q < a.nodes; q += COV_WAVES) {
            int d = 0, first = 0, cnt = 3;
            while (q >= first + cnt) {
                first += cnt;
                cnt *= 3;
                d++;
            }
            int px, py;
            plan_unpack(node[q], px, py);
            int qx[PLAN_MAX_DEPTH - 1], qy[PLAN_MAX_DEPTH - 1];   // the ancestors, nearest first (unrolled: registers)
            int j = q - first;
#pragma unroll
            for (int e = 0; e < PLAN_MAX_DEPTH - 1; e++) {
                const bool has = e < d;
                cnt /= 3;
                first -= cnt;
                j /= 3;
                plan_unpack(node[has ? first + j : 0], qx[e], qy[e]);
                if (!has) qx[e] = PLAN_FAR;   // no ancestor: a point that no cell is within R of, so the test needs no flag
            }
            const CovBox box = cov_box(px, py, a.R, side);
            unsigned s = 0;
            // all coordinates are in 0..1024 (PLAN_FAR: 2^14), so a difference squares within 2^28 and two squares sum within 2^29
            for (int bx = lane >> 3; bx < box.w; bx += 8) {
                const int ix = box.x0 + bx, cx = 16 * ix + 8;
                const unsigned own = (unsigned)((cx - px) * (cx - px));
                unsigned anc[PLAN_MAX_DEPTH - 1];   // the x part of every test is the same down a column
#pragma unroll
                for (int e = 0; e < PLAN_MAX_DEPTH - 1; e++) anc[e] = (unsigned)((cx - qx[e]) * (cx - qx[e]));
                for (int by = lane & 7; by < box.h; by += 8) {
                    const int iy = box.y0 + by, cy = 16 * iy + 8;
                    bool in = own + (unsigned)((cy - py) * (cy - py)) <= R2;
#pragma unroll
                    for (int e = 0; e < PLAN_MAX_DEPTH - 1; e++) in = in && anc[e] + (unsigned)((cy - qy[e]) * (cy - qy[e])) > R2;
                    if (in) s += W[ix * side + iy];
                }
            }
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
            if (lane == 0) gain[q] = s;
        }
        __syncthreads();
        // c. scores and the packed argmax
        unsigned long long key = 0ull;
        if (tid < a.seqs) {
            unsigned long long sc = 0ull;
            unsigned w = 256u;
            int first = 0, cnt = 3, div = a.seqs / 3;
            for (int d = 0; d < a.depth; d++) {
                sc += (unsigned long long)gain[first + tid / div] * w;
                w = (w * (unsigned)a.discount) >> 8;
                first += cnt;
                cnt *= 3;
                div = max(div / 3, 1);
            }
            key = (sc << 8) | (unsigned long long)(255 - tid);
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_down(key, off);
            key = o > key ? o : key;
        }
        if (lane == 0) red[wave] = key;
        __syncthreads();
        key = red[0];
#pragma unroll
        for (int w = 1; w < COV_WAVES; w++) key = red[w] > key ? red[w] : key;
        const int pick = 255 - (int)(key & 255ull);
        if (tid == 0) {
            a.actions[(size_t)b * a.n + i] = pick / (a.seqs / 3);
            a.plans[(size_t)b * a.n + i] = pick;
            a.scores[(size_t)b * a.n + i] = (int64_t)(key >> 8);
        }
        // d. the winner claims its D discs
        {
            int first = 0, cnt = 3, div = a.seqs / 3;
            for (int d = 0; d < a.depth; d++) {
                int px, py;
                plan_unpack(node[first + pick / div], px, py);
                const CovBox box = cov_box(px, py, a.R, side);
                for (int bx = tid >> 4; bx < box.w; bx += 16)
                    for (int by = tid & 15; by < box.h; by += 16) {
                        const int ix = box.x0 + bx, iy = box.y0 + by;
                        if (cov_within(ix, iy, px, py, R2)) W[ix * side + iy] = 0u;
                    }
                first += cnt;
                cnt *= 3;
                div = max(div / 3, 1);
            }
        }
        __syncthreads();   // (also: node, gain and red are free for the next agent)
    }
}
