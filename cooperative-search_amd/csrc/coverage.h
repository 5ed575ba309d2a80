// cooperative-search_amd/csrc/coverage.h -- cs_coverage_actions: the greedy coverage baseline, one launch per decision
// (included by episodes.hip inside its namespace).
//
// The policy is DEFINED by baseline.coverage_actions_torch (stock torch ops); this kernel reproduces its actions and its belief
// grid element for element.  Nothing here is floating point but the quantisation of an agent's four state floats (each operation
// rounded once, round-half-even): positions become integers in sub-units of 1/16 cell (a cell centre at 16 i + 8), headings an
// index into the 36 headings of the env, and everything after is integer arithmetic that cannot overflow: |position| <= 2^15
// bounds what is squared (uint32), a belief is at most 2^16 (a cell is clamped to 0..65536 as it is read) and a footprint at
// most side^2 = 2^12 cells (uint32 sums), and the one product that can reach 2^32 is taken in 64 bits.
//
// Layout: one workgroup of 256 threads per env, the working grid W in LDS (16 KB: eight workgroups per CU, the wavefront limit).
// The belief grid G is read once and written once, 16 bytes per lane where the row allows; the regrowth and the sweep happen
// on the way and the result goes to G and to W.  Then the agents decide in index order: the block sums W over the bounding box
// of each of the three candidate footprints (in 16 x 16 tiles: a box larger than the block takes several, never truncated),
// the three sums are reduced by wavefront shuffles and then through LDS in wavefront order, thread 0 decides, and after a
// barrier the block zeroes the chosen footprint in W.  No atomics, no host synchronisation.
constexpr int COV_THREADS = 256;
constexpr int COV_WAVES = COV_THREADS / 64;
constexpr int COV_HEADINGS = 36;
constexpr float COV_POS_LIM = 32768.0f;    // |quantised position| <= 2^15 sub-units (the map is at most 2^10 wide)
constexpr float COV_TRIG_LIM = 16384.0f;   // |quantised cos / sin| <= 2^14

// rint(16384 cos(k pi / 18)) and rint(16384 sin(k pi / 18)), k = 0..35 (baseline.trig_tables computes the same in double)
__constant__ int COV_CT[COV_HEADINGS] = {16384,  16135,  15396,  14189,  12551,  10531,  8192,  5604,  2845,  0,      -2845,  -5604,
                                         -8192,  -10531, -12551, -14189, -15396, -16135, -16384, -16135, -15396, -14189, -12551, -10531,
                                         -8192,  -5604,  -2845,  0,      2845,   5604,   8192,  10531, 12551, 14189,  15396,  16135};
__constant__ int COV_ST[COV_HEADINGS] = {0,      2845,   5604,   8192,   10531,  12551,  14189, 15396, 16135, 16384,  16135,  15396,
                                         14189,  12551,  10531,  8192,   5604,   2845,   0,     -2845, -5604, -8192,  -10531, -12551,
                                         -14189, -15396, -16135, -16384, -16135, -15396, -14189, -12551, -10531, -8192, -5604,  -2845};

struct CoverageArgs {
    const float *state;
    int32_t *grid;
    int64_t *actions;
    int n, side, S, R, keep, regrow, look16;   // R = 16 view_range, look16 = 16 lookahead (sub-units)
    int vec4;                                  // a grid row is a whole number of aligned 16-byte pieces
};

// rint(v) as an int in [-lim, lim]; NaN gives -lim (both comparisons fail the same way in the definition)
__device__ __forceinline__ int cov_quant(float v, float lim) {
    const float r = rintf(v);
    return (int)(r >= -lim ? (r <= lim ? r : lim) : -lim);
}

// is the centre of cell (ix, iy) within R of (px, py)?  |px|, |py| <= 2^15 + 2^10: the squares fit 32 unsigned bits
__device__ __forceinline__ bool cov_within(int ix, int iy, int px, int py, unsigned R2) {
    const unsigned adx = (unsigned)abs(16 * ix + 8 - px), ady = (unsigned)abs(16 * iy + 8 - py);
    return adx * adx + ady * ady <= R2;
}

// the cells whose centre can lie within R of a point: x0 .. x0 + w - 1 by y0 .. y0 + h - 1, inside the map (w or h may be 0)
struct CovBox {
    int x0, y0, w, h;
};

__device__ __forceinline__ CovBox cov_box(int px, int py, int R, int side) {
    // 16 i + 8 >= p - R  <=>  i >= ceil((p - R - 8) / 16);  16 i + 8 <= p + R  <=>  i <= floor((p + R - 8) / 16)  (>> floors)
    const int x0 = max((px - R + 7) >> 4, 0), x1 = min((px + R - 8) >> 4, side - 1);
    const int y0 = max((py - R + 7) >> 4, 0), y1 = min((py + R - 8) >> 4, side - 1);
    return {x0, y0, max(x1 - x0 + 1, 0), max(y1 - y0 + 1, 0)};
}

// the look-ahead point of an agent at (X, Y) with heading index h that takes action act (the env's coding: 1 is + pi / 18)
__device__ __forceinline__ void cov_point(const CoverageArgs &a, int X, int Y, int h, int act, int &px, int &py) {
    int hp = h + (act == 1 ? 1 : (act == 2 ? COV_HEADINGS - 1 : 0));
    if (hp >= COV_HEADINGS) hp -= COV_HEADINGS;
    const int lim = 16 * a.side;
    px = min(max(X + ((a.look16 * COV_CT[hp]) >> 14), 0), lim);
    py = min(max(Y + ((a.look16 * COV_ST[hp]) >> 14), 0), lim);
}

// regrowth, then the sweep of the n sensor discs, for one cell
__device__ __forceinline__ int cov_update(const CoverageArgs &a, const int *ax, const int *ay, unsigned R2, int ix, int iy, int g) {
    long long v = min(max(g, 0), 65536);   // a cell outside 0..65536 is read as the nearer bound
    v += (65536 - v) >> a.regrow;
    bool seen = false;
    for (int i = 0; i < a.n; i++) seen = seen || cov_within(ix, iy, ax[i], ay[i], R2);
    if (seen) v = (v * a.keep) >> 16;
    return (int)v;
}

__global__ __launch_bounds__(COV_THREADS) void k_coverage_actions(CoverageArgs a) {
    __shared__ __attribute__((aligned(16))) int W[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS];
    __shared__ unsigned red[COV_WAVES][3];
    __shared__ int pick;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int side = a.side, cells = side * side;
    const unsigned R2 = (unsigned)a.R * (unsigned)a.R;
    // 1. quantise: lane i owns agent i
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
    __syncthreads();
    // 2. + 3. regrow and sweep: G -> G and W, every cell once
    int32_t *G = a.grid + (size_t)b * cells;
    if (a.vec4) {
        for (int q = tid; q < cells / 4; q += COV_THREADS) {
            int4 v = reinterpret_cast<const int4 *>(G)[q];
            int ix = (4 * q) / side, iy = 4 * q - ix * side;
            int *e = reinterpret_cast<int *>(&v);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                e[k] = cov_update(a, ax, ay, R2, ix, iy, e[k]);
                if (++iy == side) {
                    iy = 0;
                    ix++;
                }
            }
            reinterpret_cast<int4 *>(G)[q] = v;
            reinterpret_cast<int4 *>(W)[q] = v;
        }
    } else {
        for (int idx = tid; idx < cells; idx += COV_THREADS) {
            const int ix = idx / side, iy = idx - ix * side;
            const int g = cov_update(a, ax, ay, R2, ix, iy, G[idx]);
            G[idx] = g;
            W[idx] = g;
        }
    }
    __syncthreads();
    // 4. choose, agent by agent; each claims what it chose
    for (int i = 0; i < a.n; i++) {
        const int X = ax[i], Y = ay[i], h = ah[i];
        unsigned acc[3];
#pragma unroll
        for (int act = 0; act < 3; act++) {
            int px, py;
            cov_point(a, X, Y, h, act, px, py);
            const CovBox box = cov_box(px, py, a.R, side);
            unsigned s = 0;
            for (int bx = tid >> 4; bx < box.w; bx += 16)   // 16 x 16 tiles of the box: no division, a 15 x 15 box is one pass
                for (int by = tid & 15; by < box.h; by += 16) {
                    const int ix = box.x0 + bx, iy = box.y0 + by;
                    if (cov_within(ix, iy, px, py, R2)) s += (unsigned)W[ix * side + iy];
                }
            acc[act] = s;
        }
#pragma unroll
        for (int act = 0; act < 3; act++) {
            for (int off = 32; off > 0; off >>= 1) acc[act] += __shfl_down(acc[act], off);
            if ((tid & 63) == 0) red[tid >> 6][act] = acc[act];
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
            a.actions[(size_t)b * a.n + i] = best;
        }
        __syncthreads();
        int px, py;
        cov_point(a, X, Y, h, pick, px, py);
        const CovBox box = cov_box(px, py, a.R, side);
        for (int bx = tid >> 4; bx < box.w; bx += 16)
            for (int by = tid & 15; by < box.h; by += 16) {
                const int ix = box.x0 + bx, iy = box.y0 + by;
                if (cov_within(ix, iy, px, py, R2)) W[ix * side + iy] = 0;
            }
        __syncthreads();   // (also: red and pick are free for the next agent)
    }
}
