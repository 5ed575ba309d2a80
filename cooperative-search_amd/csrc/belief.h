// cooperative-search_amd/csrc/belief.h -- cs_belief_actions: the target-density filter policy, one launch per decision
// (included by episodes.hip inside its namespace, after coverage.h whose cov_* helpers it calls).
//
// The policy is DEFINED by belief.belief_actions_torch (stock torch ops); this kernel reproduces its grid, its stored positions
// and its actions element for element.  As in coverage.h nothing is floating point but the quantisation of an agent's four
// state floats.  A call pushes the density D of unfound targets through the targets' motion model (predict: a scatter), sweeps
// it under the sensors (coverage.h's measurement) and lets the agents choose as coverage.h's do.
//
// Layout: one workgroup of 256 threads per env, the shape of k_coverage_actions.  ONE LDS array acc[64 * 64] (16 KB) is the
// scatter accumulator first and the working grid W afterwards.  Order: zero acc (and quantise) | barrier | scatter | barrier |
// cap, sweep, write grid and W in one pass | barrier | the choose loop of coverage.h.  A thread reads its source cells of grid
// from global memory once (16 bytes per lane where the row allows, coverage.h's test): in the scatter when moved, in the sweep
// pass otherwise.  It scatters with atomicAdd on LDS words; integer adds commute, so the sums do not depend on the order.  No
// global atomics, no host synchronisation; every __syncthreads() is outside any branch that depends on tid, side, moved or the
// data, so all 256 threads reach each of them.
//
// What could go wrong in this shape, and why it does not:
//   a wall cell collects many pieces   the pieces of ONE source sum to at most its d (16 headings x (m = 1) x weights that sum to
//                                      256, or one heading x (m = 16), over 4096) and d <= CAP = 2^19 as it is read, so a whole
//                                      map, wherever it lands, sums to at most 2^12 * 2^19 = 2^31 < 2^32: no accumulator word and
//                                      no footprint score can wrap.  One product, d m wx wy <= 2^19 * 16 * 256 = 2^31, fits too.
//   ux is negative near the low walls  ux is never formed: 16 ix has no low bits, so ux >> 4 = ix + (dx >> 4) and ux & 15 = dx & 15
//                                      (>> of a negative int is arithmetic on this compiler and & is two's complement: floor and
//                                      non-negative remainder, as torch and Python give); the cell index is clamped after.
//   side^2 < 256 leaves idle threads   they run no loop body and fall through to every barrier.
//   side = 64 fills the array          cells = 4096 = the array; every index is ci * side + cj with ci, cj clamped to 0..side - 1.
//   a displacement of several cells, or of the whole map: the destination is clamped to 0..side - 1 per axis BEFORE it indexes,
//                                      so whatever would leave the map lands on wall cells; |dx| <= 1024 is checked by the
//                                      entry point.
//   prev off the map                   read clamped to +-2^15: |ex| <= 2^15 + 1016, the two squares sum below 2^32 (unsigned).
//                                      The 16 dot products are only taken inside sense16 <= 2048: |ex CQ + ey SQ| <= 2^26.
constexpr int BEL_HEADINGS = 16;
constexpr int BEL_CAP = 1 << 19;   // a cell is read as clamp(cell, 0, CAP)

// rint(16384 cos(2 pi k / 16)) and rint(16384 sin(2 pi k / 16)), k = 0..15, from motion's CX / CY (belief.heading_tables)
__constant__ int BEL_CQ[BEL_HEADINGS] = {16384, 15137, 11585, 6270, 0, -6270, -11585, -15137, -16384, -15137, -11585, -6270, 0, 6270, 11585, 15137};
__constant__ int BEL_SQ[BEL_HEADINGS] = {0, 6270, 11585, 15137, 16384, 15137, 11585, 6270, 0, -6270, -11585, -15137, -16384, -15137, -11585, -6270};

struct BeliefArgs {
    CoverageArgs c;    // state, grid, actions, n, side, S, R, keep, look16, vec4 (regrow unused)
    int32_t *prev;     // [B][8][2]
    int mode, moved;
    unsigned sense2;   // sense16^2
    int dx[BEL_HEADINGS], dy[BEL_HEADINGS];
};

// the four pieces of d * m along heading (ox, fx, oy, fy) = (dx >> 4, dx & 15, dy >> 4, dy & 15) from cell (ix, iy)
__device__ __forceinline__ void bel_spread(unsigned *acc, int side, int ix, int iy, unsigned dm, int ox, int fx, int oy, int fy) {
    const int i0 = min(max(ix + ox, 0), side - 1), i1 = min(max(ix + ox + 1, 0), side - 1);
    const int j0 = min(max(iy + oy, 0), side - 1), j1 = min(max(iy + oy + 1, 0), side - 1);
    const unsigned wx0 = 16u - (unsigned)fx, wx1 = (unsigned)fx, wy0 = 16u - (unsigned)fy, wy1 = (unsigned)fy;
    unsigned p;   // a piece of 0 (fx or fy 0, or a small d) adds nothing: skipped
    if ((p = (dm * wx0 * wy0) >> 12) != 0) atomicAdd(&acc[i0 * side + j0], p);
    if ((p = (dm * wx1 * wy0) >> 12) != 0) atomicAdd(&acc[i1 * side + j0], p);
    if ((p = (dm * wx0 * wy1) >> 12) != 0) atomicAdd(&acc[i0 * side + j1], p);
    if ((p = (dm * wx1 * wy1) >> 12) != 0) atomicAdd(&acc[i1 * side + j1], p);
}

// the prediction of one source cell: where its mass d goes
__device__ __forceinline__ void bel_scatter(const BeliefArgs &a, unsigned *acc, const int *px, const int *py, const int *ox, const int *fx,
                                            const int *oy, const int *fy, int ix, int iy, int g) {
    const unsigned d = (unsigned)min(max(g, 0), BEL_CAP);
    if (d == 0) return;
    const int side = a.c.side;
    if (a.mode == CS_MOTION_EVADE) {
        unsigned best = 0xffffffffu;
        int bex = 0, bey = 0;
        for (int i = 0; i < a.c.n; i++) {   // the nearest agent inside the radius, lowest index on ties
            const int ex = 16 * ix + 8 - px[i], ey = 16 * iy + 8 - py[i];
            const unsigned d2 = (unsigned)abs(ex) * (unsigned)abs(ex) + (unsigned)abs(ey) * (unsigned)abs(ey);
            if (d2 <= a.sense2 && d2 < best) {
                best = d2;
                bex = ex;
                bey = ey;
            }
        }
        if (best != 0xffffffffu) {   // (d2 <= sense2 <= 2^22: never the sentinel)
            int top = bex * BEL_CQ[0] + bey * BEL_SQ[0], k = 0;
            for (int q = 1; q < BEL_HEADINGS; q++) {   // the heading that leads away fastest, lowest index on ties
                const int s = bex * BEL_CQ[q] + bey * BEL_SQ[q];
                if (s > top) {
                    top = s;
                    k = q;
                }
            }
            bel_spread(acc, side, ix, iy, d * 16u, ox[k], fx[k], oy[k], fy[k]);
            return;
        }
    }
#pragma unroll 1
    for (int k = 0; k < BEL_HEADINGS; k++) bel_spread(acc, side, ix, iy, d, ox[k], fx[k], oy[k], fy[k]);
}

// cap (when predicted) or clamp (when read from the grid), then the sweep of the n sensor discs, for one cell
__device__ __forceinline__ int bel_update(const BeliefArgs &a, const int *ax, const int *ay, unsigned R2, int ix, int iy, long long v) {
    v = min(max(v, 0ll), (long long)BEL_CAP);
    bool seen = false;
    for (int i = 0; i < a.c.n; i++) seen = seen || cov_within(ix, iy, ax[i], ay[i], R2);
    if (seen) v = (v * a.c.keep) >> 16;
    return (int)v;
}

__global__ __launch_bounds__(COV_THREADS) void k_belief_actions(BeliefArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned acc[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS], px[CS_MAX_AGENTS], py[CS_MAX_AGENTS];
    __shared__ int ox[BEL_HEADINGS], fx[BEL_HEADINGS], oy[BEL_HEADINGS], fy[BEL_HEADINGS];
    __shared__ unsigned red[COV_WAVES][3];
    __shared__ int pick;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int side = a.c.side, cells = side * side;
    const unsigned R2 = (unsigned)a.c.R * (unsigned)a.c.R;
    // 1. quantise: lane i owns agent i, reads its stored position and stores the new one; the accumulator is zeroed
    if (tid < a.c.n) {
        const float *s = a.c.state + (size_t)b * a.c.S + 4 * tid;
        const float half = (float)side / 2.0f;
        const int X = cov_quant((s[0] * half + half) * 16.0f, COV_POS_LIM), Y = cov_quant((s[1] * half + half) * 16.0f, COV_POS_LIM);
        const int c = cov_quant(s[2] * 16384.0f, COV_TRIG_LIM), sn = cov_quant(s[3] * 16384.0f, COV_TRIG_LIM);
        int best = c * COV_CT[0] + sn * COV_ST[0], h = 0;   // |c CT + s ST| <= 2^29
        for (int k = 1; k < COV_HEADINGS; k++) {
            const int d = c * COV_CT[k] + sn * COV_ST[k];
            if (d > best) {
                best = d;
                h = k;
            }
        }
        ax[tid] = X;
        ay[tid] = Y;
        ah[tid] = h;
        int32_t *p = a.prev + ((size_t)b * CS_MAX_AGENTS + tid) * 2;
        px[tid] = min(max(p[0], -32768), 32768);
        py[tid] = min(max(p[1], -32768), 32768);
        p[0] = X;
        p[1] = Y;
    }
    if (tid >= 64 && tid < 64 + BEL_HEADINGS) {   // (another wavefront than the agents')
        const int k = tid - 64;
        ox[k] = a.dx[k] >> 4;
        fx[k] = a.dx[k] & 15;
        oy[k] = a.dy[k] >> 4;
        fy[k] = a.dy[k] & 15;
    }
    if (a.moved)
        for (int idx = tid; idx < cells; idx += COV_THREADS) acc[idx] = 0u;
    __syncthreads();
    // 2. predict: every source cell scatters its mass into acc
    int32_t *G = a.c.grid + (size_t)b * cells;
    if (a.moved) {
        if (a.c.vec4) {
            for (int q = tid; q < cells / 4; q += COV_THREADS) {
                const int4 v = reinterpret_cast<const int4 *>(G)[q];
                int ix = (4 * q) / side, iy = 4 * q - ix * side;
                const int *e = reinterpret_cast<const int *>(&v);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    bel_scatter(a, acc, px, py, ox, fx, oy, fy, ix, iy, e[k]);
                    if (++iy == side) {
                        iy = 0;
                        ix++;
                    }
                }
            }
        } else {
            for (int idx = tid; idx < cells; idx += COV_THREADS) {
                const int ix = idx / side, iy = idx - ix * side;
                bel_scatter(a, acc, px, py, ox, fx, oy, fy, ix, iy, G[idx]);
            }
        }
    }
    __syncthreads();
    // 3. cap and sweep: acc (or, when nothing moved, G) -> G and W = acc, every cell once
    if (a.c.vec4) {
        for (int q = tid; q < cells / 4; q += COV_THREADS) {
            int4 v;
            if (a.moved) v = reinterpret_cast<const int4 *>(acc)[q];
            else v = reinterpret_cast<const int4 *>(G)[q];
            int ix = (4 * q) / side, iy = 4 * q - ix * side;
            int *e = reinterpret_cast<int *>(&v);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                // an accumulator word is unsigned (up to 2^31): widen it as such; a grid word is signed
                e[k] = bel_update(a, ax, ay, R2, ix, iy, a.moved ? (long long)(unsigned)e[k] : (long long)e[k]);
                if (++iy == side) {
                    iy = 0;
                    ix++;
                }
            }
            reinterpret_cast<int4 *>(G)[q] = v;
            reinterpret_cast<int4 *>(acc)[q] = v;
        }
    } else {
        for (int idx = tid; idx < cells; idx += COV_THREADS) {
            const int ix = idx / side, iy = idx - ix * side;
            const int g = bel_update(a, ax, ay, R2, ix, iy, a.moved ? (long long)acc[idx] : (long long)G[idx]);
            G[idx] = g;
            acc[idx] = (unsigned)g;
        }
    }
    __syncthreads();
    // 4. choose, agent by agent; each claims what it chose (coverage.h's loop on W = acc)
    const unsigned *W = acc;
    for (int i = 0; i < a.c.n; i++) {
        const int X = ax[i], Y = ay[i], h = ah[i];
        unsigned sum[3];
#pragma unroll
        for (int act = 0; act < 3; act++) {
            int qx, qy;
            cov_point(a.c, X, Y, h, act, qx, qy);
            const CovBox box = cov_box(qx, qy, a.c.R, side);
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
            a.c.actions[(size_t)b * a.c.n + i] = best;
        }
        __syncthreads();
        int qx, qy;
        cov_point(a.c, X, Y, h, pick, qx, qy);
        const CovBox box = cov_box(qx, qy, a.c.R, side);
        for (int bx = tid >> 4; bx < box.w; bx += 16)
            for (int by = tid & 15; by < box.h; by += 16) {
                const int ix = box.x0 + bx, iy = box.y0 + by;
                if (cov_within(ix, iy, qx, qy, R2)) acc[ix * side + iy] = 0u;
            }
        __syncthreads();   // (also: red and pick are free for the next agent)
    }
}
