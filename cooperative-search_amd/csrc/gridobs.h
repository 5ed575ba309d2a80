// cooperative-search_amd/csrc/gridobs.h -- cs_grid_features and cs_feature_episodes: sixteen floats per agent that summarise the grid
// of a coverage.h / belief.h policy, per decision and for a recorded batch of episodes (included by episodes.hip inside its namespace,
// after label.h).
//
// The features are DEFINED by gridobs.grid_features_torch and gridobs.feature_episodes_torch (stock torch ops, integer after the one
// quantisation); both kernels reproduce them bit for bit.  Probe k = 8 ring + b of an agent at (X, Y) with heading index h lies
// GO_DIST[ring] look-ahead distances along heading (h + GO_REL[b]) % 36, clamped to the map: coverage.h's cov_point for ring 0 and
// b = 0..2.  sum_k is the sum of clamp(cell, 0, CAP) over the cells whose centre lies within R of the probe (cov_within), and the
// feature is float(sum_k >> 8) * 2^-15.  A whole map sums to at most 2^12 * 2^19 = 2^31 (uint32), sum_k >> 8 <= 2^23 is exact in
// float32 and the scale is a power of two: there is nothing to round.  No team-mate claims: every agent reads the same grid.
//
// k_grid_features: one workgroup of 256 threads per env.  Lane i < n quantises agent i (k_coverage_actions' step 1) | barrier |
// the 16 n probes are dealt to the four wavefronts, probe k to wavefront k % 4; a wavefront walks its probe's cov_box in 4 x 16
// tiles, 64 cells at a time, reading the grid from global memory (the filter's launch has just written it: it is in L2), reduces by
// shuffles and lane 0 stores the float.  One barrier; none in the probe loop, whose trip counts differ between wavefronts.
//
// k_feature_episodes: k_label_episodes' walk (label.h: G and W in LDS, one workgroup per episode) with the probe sums taken on G
// between the update and the choose loop.  What could go wrong in this shape, and why it does not:
//   a barrier in a branch on `labels`     labels is a kernel argument: all 256 threads of every workgroup see the same pointer, so
//                                         either all of them run the choose loop (which ends on a barrier) or all of them take the one
//                                         barrier that stands in its place.  Every other __syncthreads() stands where label.h's do.
//   the probes race with the next row     the probes READ G, ax, ay and ah.  The next row's quantise writes ax, ay, ah and its update
//                                         writes G; both come after the barrier that ends this row (the choose loop's last, or the one
//                                         in its place).  The choose loop itself writes W, red and pick only: G is not touched by it.
//   the probes race with the update       the barrier that ends step 3 stands between the last write of G and the first probe read.
//   E * T * S or E * T * n * 16 past 2^31 every global index is formed in size_t.
//   unaligned rows                        16-byte accesses are taken only where the entry point found base and row pitch aligned
//                                         (svec, vec4, lvec, fvec); otherwise words.  A features row is 16 n floats from an index that
//                                         is a multiple of 16, so fvec needs the base alone.
//   side^2 < 256 leaves idle threads      they run no loop body and fall through to every barrier; the probe loop is dealt by
//                                         wavefront and a wavefront without a probe runs none.
//   side = 64 fills both arrays           as in label.h; a probe reads G[ix * side + iy] with (ix, iy) inside cov_box: 0..side - 1.
//   view_range = 0                        R = 0: only a cell whose centre IS the probe counts; cov_box is that one cell or empty (w or
//                                         h 0, no loop body runs) and the sum is that cell or 0.
//   view_range = 64                       R = 1024: the box is the whole map, 64 passes of 64 cells; the sum is at most 2^31.
//   lookahead = 0                         all sixteen probes of an agent are its own clamped position: sixteen equal features.
//   probes clamped at the walls           go_point clamps to 0..16 side as cov_point does; 3 * 1024 * 16384 < 2^31 before the shift.
//   NaN or huge state floats              cov_quant clamps (NaN to the lower bound): |X| <= 2^15, the probe is clamped to the map
//                                         after the offset is added, so cov_within's squares fit.  Rows t >= lens[e] are never
//                                         read; their features are written as +0.0f.
constexpr int GO_PROBES = 16;   // per agent
__constant__ int GO_REL[8] = {0, 1, 35, 4, 32, 9, 27, 18};   // bearings relative to the heading, in steps of pi / 18
__constant__ int GO_DIST[2] = {1, 3};                        // ring distances in look-ahead units

struct GridObsArgs {
    const float *state;     // [B][S]
    const int32_t *grid;    // [B][side * side], read only
    float *feat;            // [B][n][16]
    int n, side, S, R, look16;
};

// probe q = 8 ring + b of an agent at (X, Y) with heading index h
__device__ __forceinline__ void go_point(int X, int Y, int h, int q, int look16, int side, int &px, int &py) {
    int hp = h + GO_REL[q & 7];
    if (hp >= COV_HEADINGS) hp -= COV_HEADINGS;
    const int d16 = GO_DIST[q >> 3] * look16, lim = 16 * side;   // <= 3 * 1024
    px = min(max(X + ((d16 * COV_CT[hp]) >> 14), 0), lim);
    py = min(max(Y + ((d16 * COV_ST[hp]) >> 14), 0), lim);
}

// the sum of clamp(cell, 0, CAP) over the footprint of (px, py), by one wavefront; the result is valid in lane 0
template <class GridPtr>
__device__ __forceinline__ unsigned go_probe_sum(GridPtr G, int side, int R, unsigned R2, int px, int py, int lane) {
    const CovBox box = cov_box(px, py, R, side);
    unsigned s = 0;
    for (int bx = lane >> 4; bx < box.w; bx += 4)
        for (int by = lane & 15; by < box.h; by += 16) {
            const int ix = box.x0 + bx, iy = box.y0 + by;
            if (cov_within(ix, iy, px, py, R2)) s += (unsigned)min(max((int)G[ix * side + iy], 0), BEL_CAP);
        }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    return s;
}

__device__ __forceinline__ float go_feature(unsigned sum) { return (float)(sum >> 8) * 0x1p-15f; }

__global__ __launch_bounds__(COV_THREADS) void k_grid_features(GridObsArgs a) {
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int side = a.side;
    const unsigned R2 = (unsigned)a.R * (unsigned)a.R;
    // 1. quantise: lane i owns agent i
    if (tid < a.n) {
        const float *s = a.state + b * (size_t)a.S + 4 * tid;
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
    // 2. the probes, one wavefront each
    const int32_t *G = a.grid + b * (size_t)(side * side);
    const int lane = tid & 63;
    for (int k = tid >> 6; k < GO_PROBES * a.n; k += COV_WAVES) {
        const int i = k >> 4, q = k & 15;
        int px, py;
        go_point(ax[i], ay[i], ah[i], q, a.look16, side, px, py);
        const unsigned s = go_probe_sum(G, side, a.R, R2, px, py, lane);
        if (lane == 0) a.feat[b * (size_t)(GO_PROBES * a.n) + k] = go_feature(s);
    }
}

struct FeatArgs {
    LabelArgs l;    // as k_label_episodes takes it; l.b.c.actions = labels, which may be null here
    float *feat;    // [E][T][n][16]
    int fvec;       // feat is 16-byte aligned
};

__global__ __launch_bounds__(COV_THREADS) void k_feature_episodes(FeatArgs fa) {
    __shared__ __attribute__((aligned(16))) int G[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ __attribute__((aligned(16))) unsigned W[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS], px[CS_MAX_AGENTS], py[CS_MAX_AGENTS];
    __shared__ int ox[BEL_HEADINGS], fx[BEL_HEADINGS], oy[BEL_HEADINGS], fy[BEL_HEADINGS];
    __shared__ unsigned red[COV_WAVES][3];
    __shared__ int pick;
    const LabelArgs &a = fa.l;
    const CoverageArgs &c = a.b.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t e = blockIdx.x;
    const int n = c.n, side = c.side, cells = side * side, T = a.T;
    const unsigned R2 = (unsigned)c.R * (unsigned)c.R;
    const int len = min(max(a.lens[e], 0), T);
    const bool belief = a.expert == LABEL_BELIEF;
    const bool labels = c.actions != nullptr;   // a kernel argument: the same in every thread
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
        // 3b. the probes on G, one wavefront each (k_grid_features' step 2; G holds 0..CAP here, the clamp changes nothing)
        {
            float *F = fa.feat + (e * (size_t)T + (size_t)t) * (size_t)(GO_PROBES * n);
            for (int k = tid >> 6; k < GO_PROBES * n; k += COV_WAVES) {
                const int i = k >> 4, q = k & 15;
                int qx, qy;
                go_point(ax[i], ay[i], ah[i], q, c.look16, side, qx, qy);
                const unsigned s = go_probe_sum(G, side, c.R, R2, qx, qy, lane);
                if (lane == 0) F[k] = go_feature(s);
            }
        }
        if (!labels) {
            __syncthreads();   // (in place of the choose loop's last: ax, ay, ah and G are free for the next row)
            continue;
        }
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
    // 5. rows past the episode's end: features +0.0f, labels 0
    {
        const size_t k0 = (e * (size_t)T + (size_t)len) * (size_t)(GO_PROBES * n), cnt = (size_t)(T - len) * (size_t)(GO_PROBES * n);
        float *F = fa.feat + k0;   // (k0 and cnt are multiples of 16 floats)
        if (fa.fvec)
            for (size_t q = tid; q < cnt / 4; q += COV_THREADS) reinterpret_cast<float4 *>(F)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        else
            for (size_t k = tid; k < cnt; k += COV_THREADS) F[k] = 0.0f;
    }
    if (labels) {
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
