// cooperative-search_amd/csrc/localobs.h -- cs_local_grid_features and cs_local_feature_episodes: sixteen floats per agent that summarise
// the agent's OWN private grid of a local.h / local_belief.h policy, per decision and for a recorded batch of episodes (included by
// episodes.hip inside its namespace, after local_belief.h and gridobs.h, whose device helpers it calls).
//
// The features are DEFINED by localobs.local_grid_features_torch and localobs.local_feature_episodes_torch (stock torch ops, integer
// after the one quantisation); both kernels reproduce them bit for bit.  Row i of the features is gridobs.h's row i taken on
// grids[b][i]: probe points from agent i's pose (go_point), sums of clamp(cell, 0, CAP) over agent i's grid (go_probe_sum),
// float(sum >> 8) * 2^-15 (go_feature).  Nothing here is a new formula; what is new is which grid a probe reads.
//
// k_local_grid_features: k_grid_features with probe k of agent i = k >> 4 reading grids + (b n + i) cells.  One workgroup of 256
// threads per env, one barrier after the quantise, one wavefront per probe, no LDS beyond the agents' 96 bytes.
//
// k_local_feature_episodes: one workgroup of 256 threads per EPISODE walks the live rows in order.  The n private grids do not go
// into LDS (local.h's header has the arithmetic: 128 KB at n = 8); they live in a caller-provided workspace int32 [E][n][cells],
// which the kernel fills with 65536 itself and which IS grids_out after the last live row.  Per live row:
//   quantise   lane i < n keeps agent i's previous position as prev (px, py, LDS) and quantises the new one
//   | barrier |
//   links      lane i < n keeps adj[i] as was[i] (the `heard` of local_belief.h, read with bits >= n dropped and the own bit set) and
//              forms the new adj[i] by local.h's strict 64-bit test
//   | barrier |
//   predict    belief rows with moved(t) only: local_belief.h's n rounds through ONE 16 KB accumulator: zero | barrier | masked
//              scatter of D_j from the workspace | barrier | cap, own sweep, store S_j over D_j | barrier
//   merge      local.h's pass: a thread holds its cells of all n grids before it stores any.  Coverage runs cov_update with one
//              agent on the way in; belief without a move runs bel_update's clamp and the own sweep in registers
//   | barrier |
//   probes     the 16 n probes on M_i, read back from the workspace, one wavefront each
//   choose     if labels: local.h's loop (claims as two integers per earlier agent in registers, tested geometrically, red
//              double-buffered on the agent's parity, one barrier per agent); otherwise the one barrier that stands in its place
// After the loop the feature and label rows past len are zeroed as k_feature_episodes does it, and prev_out / heard_out are written
// when asked for.  What it moves per live row: every cell of n grids read once and written once (twice on a moved belief row),
// plus the footprints of the probes and of the choose loop, which were stored by this workgroup a moment ago and sit in L2.
//
// What could go wrong in this shape, and why it does not:
//   a barrier in a divergent branch       len (one word lens[e], clamped to 0..T), labels (a kernel argument), moved(t) (of t and kernel
//                                         arguments), expert, n and side are the same in all 256 threads.  The predict rounds stand in
//                                         `if (moved)` and in a loop over j < n: both block-uniform; inside a round every thread passes
//                                         all three barriers whether or not it owns a cell.  The choose loop's barrier is one per agent
//                                         for every thread; without labels every thread takes the one barrier in its place.  No barrier
//                                         stands in a branch on tid or on the data.
//   visibility between rows               the next row's scatter and merge read workspace cells that OTHER threads of this workgroup
//                                         stored in this row (a thread's cells differ between the fill, the cap pass and the merge only
//                                         in which thread owns them, not across workgroups: episode e's workspace is touched by
//                                         workgroup e alone).  Every row ends on a __syncthreads() (the choose loop's last, or the one
//                                         in its place): a workgroup-scope release (every store of the wave has left: vmcnt(0)), the
//                                         barrier, and a workgroup-scope acquire; the waves of a workgroup share one CU and its
//                                         write-through L1, which is what local.h relies on for its choose stage.  The fill of step 0
//                                         is followed by a barrier in the same way.
//   the probes read a half-merged grid    the barrier that ends the merge stands between the last store of M_i and the first probe
//                                         load, and nothing writes the workspace again until the row has ended: the choose loop reads
//                                         it, red and registers only.
//   the probes race with the next row     they read ax, ay, ah; the next row's quantise writes them after the row-ending barrier.
//   the accumulator is reused             across rounds as in local_belief.h (the third barrier of a round stands between the cap pass
//                                         and the next zeroing) and across rows (the last round's third barrier, then at least the
//                                         merge's and the row-ending barrier, before the next moved row zeroes it).
//   S_j is stored over D_j                as in local_belief.h: the second barrier of the round stands between the last load of D_j
//                                         and the first store of S_j; round j touches grid j only.
//   the merge is in place                 as in local.h: a thread loads cell c of all n grids into registers and only then stores.
//   the minimum's start                   CAP + 1 for belief, 65537 for coverage: above every cell the expert can hold; adj[i] has bit
//                                         i, so S_i always enters and the start is never stored.
//   2^31                                  an accumulator word, a score and a probe sum are unsigned sums of at most 2^12 cells of at
//                                         most CAP = 2^19 (coverage: 2^16): at most 2^31.  sum >> 8 <= 2^23 is exact in float32.
//   was has garbage bits                  it cannot: was[i] is made from this kernel's own adj[i] (0 before the first row), masked
//                                         to bits < n with the own bit set, as local_belief.h reads heard.
//   the link test wraps                   local.h's: the differences are widened to long long BEFORE they are squared.
//   side^2 < 256 leaves idle threads      they run no loop body and fall through to every barrier; a wavefront without a probe
//                                         runs none.
//   side 64 fills the accumulator         cells = 4096 = the array; every index is ci * side + cj with ci, cj clamped to 0..side - 1.
//   rows are unaligned at side 7          agent i's row of episode e starts (e n + i) * 49 words behind the workspace: the 16-byte path
//                                         is taken only when cells % 4 == 0 AND the workspace is 16-byte aligned (vec4, decided by the
//                                         entry point); then every row of every agent is aligned.  svec, lvec and fvec as in gridobs.h.
//   register arrays                       v[], cx[] and cy[] are indexed by unrolled loop counters only (a run-time i is matched by
//                                         `if (j == i)` inside an unrolled loop): scratch 0.  The heading loop of the scatter stays
//                                         rolled (lbel_scatter's #pragma unroll 1).
//   E * n * cells, E * T * S, E * T * n * 16 past 2^31   every global index is formed in size_t.
//   NaN or huge state floats              cov_quant clamps (NaN to the lower bound): |X| <= 2^15, the probe is clamped to the map after
//                                         the offset is added.  Rows t >= lens[e] are never read; their features are +0.0f, labels 0.
struct LocalGridObsArgs {
    const float *state;      // [B][S]
    const int32_t *grids;    // [B][n][side * side], read only
    float *feat;             // [B][n][16]
    int n, side, S, R, look16;
};

__global__ __launch_bounds__(COV_THREADS) void k_local_grid_features(LocalGridObsArgs a) {
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int side = a.side, cells = side * side;
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
    // 2. the probes, one wavefront each; probe k of agent i reads agent i's grid
    const int lane = tid & 63;
    for (int k = tid >> 6; k < GO_PROBES * a.n; k += COV_WAVES) {
        const int i = k >> 4, q = k & 15;
        const int32_t *G = a.grids + (b * (size_t)a.n + (size_t)i) * (size_t)cells;
        int px, py;
        go_point(ax[i], ay[i], ah[i], q, a.look16, side, px, py);
        const unsigned s = go_probe_sum(G, side, a.R, R2, px, py, lane);
        if (lane == 0) a.feat[b * (size_t)(GO_PROBES * a.n) + k] = go_feature(s);
    }
}

struct LocalFeatArgs {
    LabelArgs l;          // as k_label_episodes takes it; l.b.c.actions = labels, which may be null; l.grid_out = the workspace
                          // [E][n][side * side], REQUIRED; l.b.c.vec4: every row of every agent of the workspace is aligned
    float *feat;          // [E][T][n][16]
    int32_t *heard_out;   // [E][8] or null
    long long C2;         // (16 comm_range)^2, or -1: unlimited
    int fvec;             // feat is 16-byte aligned
};

__global__ __launch_bounds__(COV_THREADS) void k_local_feature_episodes(LocalFeatArgs fa) {
    __shared__ __attribute__((aligned(16))) unsigned acc[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS], px[CS_MAX_AGENTS], py[CS_MAX_AGENTS];
    __shared__ unsigned was[CS_MAX_AGENTS], adj[CS_MAX_AGENTS];   // whom agent i heard on the previous row, and hears now
    __shared__ int ox[BEL_HEADINGS], fx[BEL_HEADINGS], oy[BEL_HEADINGS], fy[BEL_HEADINGS];
    __shared__ unsigned red[2][COV_WAVES][3];
    const LabelArgs &a = fa.l;
    const CoverageArgs &c = a.b.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t e = blockIdx.x;
    const int n = c.n, side = c.side, cells = side * side, T = a.T;
    const unsigned R2 = (unsigned)c.R * (unsigned)c.R;
    const int len = min(max(a.lens[e], 0), T);
    const bool belief = a.expert == LABEL_BELIEF;
    const bool labels = c.actions != nullptr;   // a kernel argument: the same in every thread
    int32_t *G = a.grid_out + e * (size_t)n * (size_t)cells;
    CoverageArgs one = c;   // cov_update with one agent: the regrowth and the sweep of that agent's disc alone
    one.n = 1;
    BeliefArgs oneb = a.b;   // bel_update with one agent: the clamp and the sweep of that agent's disc alone
    oneb.c.n = 1;
    // 0. n fresh grids: FRESH everywhere; prev and heard zero
    if (c.vec4)
        for (int q = tid; q < (n * cells) / 4; q += COV_THREADS) reinterpret_cast<int4 *>(G)[q] = make_int4(65536, 65536, 65536, 65536);
    else
        for (int idx = tid; idx < n * cells; idx += COV_THREADS) G[idx] = 65536;
    if (tid < CS_MAX_AGENTS) {
        ax[tid] = 0;
        ay[tid] = 0;
        adj[tid] = 0u;
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
        __syncthreads();
        // 2. links: lane i keeps the mask of the previous row as `heard` and forms the mask of those agent i hears now (local.h's test)
        if (tid < n) {
            was[tid] = (adj[tid] & ((1u << n) - 1u)) | (1u << tid);
            unsigned m = 1u << tid;
            for (int j = 0; j < n; j++) {
                const long long dx = (long long)ax[tid] - (long long)ax[j], dy = (long long)ay[tid] - (long long)ay[j];
                if (fa.C2 < 0 || dx * dx + dy * dy < fa.C2) m |= 1u << j;
            }
            adj[tid] = m;
        }
        __syncthreads();
        // 3. predict (belief, moved: the same in every thread), agent after agent through the one accumulator: D_j -> S_j, in place
        if (moved)
            for (int j = 0; j < n; j++) {
                int32_t *Gj = G + (size_t)j * cells;
                for (int idx = tid; idx < cells; idx += COV_THREADS) acc[idx] = 0u;
                __syncthreads();
                {
                    const unsigned mask = was[j];
                    if (c.vec4) {
                        for (int q = tid; q < cells / 4; q += COV_THREADS) {
                            const int4 v = reinterpret_cast<const int4 *>(Gj)[q];
                            int ix = (4 * q) / side, iy = 4 * q - ix * side;
                            const int *w = reinterpret_cast<const int *>(&v);
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                lbel_scatter(a.b, acc, px, py, mask, ox, fx, oy, fy, ix, iy, w[k]);
                                if (++iy == side) {
                                    iy = 0;
                                    ix++;
                                }
                            }
                        }
                    } else {
                        for (int idx = tid; idx < cells; idx += COV_THREADS) {
                            const int ix = idx / side, iy = idx - ix * side;
                            lbel_scatter(a.b, acc, px, py, mask, ox, fx, oy, fy, ix, iy, Gj[idx]);
                        }
                    }
                }
                __syncthreads();
                if (c.vec4) {
                    for (int q = tid; q < cells / 4; q += COV_THREADS) {
                        int4 v = reinterpret_cast<const int4 *>(acc)[q];
                        int ix = (4 * q) / side, iy = 4 * q - ix * side;
                        int *w = reinterpret_cast<int *>(&v);
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            w[k] = bel_update(oneb, ax + j, ay + j, R2, ix, iy, (long long)(unsigned)w[k]);   // (an accumulator word is unsigned)
                            if (++iy == side) {
                                iy = 0;
                                ix++;
                            }
                        }
                        reinterpret_cast<int4 *>(Gj)[q] = v;
                    }
                } else {
                    for (int idx = tid; idx < cells; idx += COV_THREADS) {
                        const int ix = idx / side, iy = idx - ix * side;
                        Gj[idx] = bel_update(oneb, ax + j, ay + j, R2, ix, iy, (long long)acc[idx]);
                    }
                }
                __syncthreads();
            }
        // 4. merge (local.h's pass): a thread holds its cells of all n grids before it stores any of them.  Coverage regrows and sweeps
        // on the way in; belief clamps and sweeps on the way in when nothing moved (a moved row's S_j is in the workspace already)
        const int far = belief ? BEL_CAP + 1 : 65537;
        if (c.vec4) {
            for (int q = tid; q < cells / 4; q += COV_THREADS) {
                const int ix0 = (4 * q) / side, iy0 = 4 * q - ix0 * side;
                int4 v[CS_MAX_AGENTS];
#pragma unroll
                for (int j = 0; j < CS_MAX_AGENTS; j++) {
                    v[j] = make_int4(0, 0, 0, 0);
                    if (j < n) {
                        v[j] = reinterpret_cast<const int4 *>(G + (size_t)j * cells)[q];
                        if (!moved) {
                            int *w = reinterpret_cast<int *>(&v[j]);
                            int ix = ix0, iy = iy0;
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                w[k] = belief ? bel_update(oneb, ax + j, ay + j, R2, ix, iy, (long long)w[k])
                                              : cov_update(one, ax + j, ay + j, R2, ix, iy, w[k]);
                                if (++iy == side) {
                                    iy = 0;
                                    ix++;
                                }
                            }
                        }
                    }
                }
                for (int i = 0; i < n; i++) {   // (adj[i] holds bit i: the minimum starts above every cell and takes in S_i itself)
                    const unsigned m = adj[i];
                    int4 r = make_int4(far, far, far, far);
#pragma unroll
                    for (int j = 0; j < CS_MAX_AGENTS; j++)
                        if ((m >> j) & 1u) {   // (bits at and above n are never set)
                            r.x = min(r.x, v[j].x);
                            r.y = min(r.y, v[j].y);
                            r.z = min(r.z, v[j].z);
                            r.w = min(r.w, v[j].w);
                        }
                    reinterpret_cast<int4 *>(G + (size_t)i * cells)[q] = r;
                }
            }
        } else {
            for (int idx = tid; idx < cells; idx += COV_THREADS) {
                const int ix = idx / side, iy = idx - ix * side;
                int v[CS_MAX_AGENTS];
#pragma unroll
                for (int j = 0; j < CS_MAX_AGENTS; j++) {
                    v[j] = 0;
                    if (j < n) {
                        v[j] = G[(size_t)j * cells + idx];
                        if (!moved)
                            v[j] = belief ? bel_update(oneb, ax + j, ay + j, R2, ix, iy, (long long)v[j])
                                          : cov_update(one, ax + j, ay + j, R2, ix, iy, v[j]);
                    }
                }
                for (int i = 0; i < n; i++) {
                    const unsigned m = adj[i];
                    int r = far;
#pragma unroll
                    for (int j = 0; j < CS_MAX_AGENTS; j++)
                        if ((m >> j) & 1u) r = min(r, v[j]);
                    G[(size_t)i * cells + idx] = r;
                }
            }
        }
        __syncthreads();   // the probes and the choose stage read cells that other threads of this workgroup have just stored
        // 5. the probes on M_i, one wavefront each (k_local_grid_features' step 2)
        {
            float *F = fa.feat + (e * (size_t)T + (size_t)t) * (size_t)(GO_PROBES * n);
            for (int k = tid >> 6; k < GO_PROBES * n; k += COV_WAVES) {
                const int i = k >> 4, q = k & 15;
                int qx, qy;
                go_point(ax[i], ay[i], ah[i], q, c.look16, side, qx, qy);
                const unsigned s = go_probe_sum((const int32_t *)(G + (size_t)i * cells), side, c.R, R2, qx, qy, lane);
                if (lane == 0) F[k] = go_feature(s);
            }
        }
        if (!labels) {
            __syncthreads();   // (in place of the choose loop's: ax, ay, ah, adj and the workspace are free for the next row)
            continue;
        }
        // 6. choose, agent by agent, on M_i less the claims agent i has heard: local.h's loop
        int cx[CS_MAX_AGENTS], cy[CS_MAX_AGENTS];
#pragma unroll
        for (int j = 0; j < CS_MAX_AGENTS; j++) cx[j] = cy[j] = 0;
        for (int i = 0; i < n; i++) {
            const int X = ax[i], Y = ay[i], h = ah[i];
            const unsigned heard = adj[i] & ((1u << i) - 1u);
            const int32_t *M = G + (size_t)i * cells;
            unsigned sum[3];
#pragma unroll
            for (int act = 0; act < 3; act++) {
                int qx, qy;
                cov_point(c, X, Y, h, act, qx, qy);
                const CovBox box = cov_box(qx, qy, c.R, side);
                unsigned s = 0;
                for (int bx = tid >> 4; bx < box.w; bx += 16)   // 16 x 16 tiles of the box, as in coverage.h
                    for (int by = tid & 15; by < box.h; by += 16) {
                        const int ix = box.x0 + bx, iy = box.y0 + by;
                        if (cov_within(ix, iy, qx, qy, R2)) {
                            bool claimed = false;
#pragma unroll
                            for (int j = 0; j < CS_MAX_AGENTS - 1; j++)   // (agent 7 is heard by nobody: all decide before it)
                                if ((heard >> j) & 1u) claimed = claimed || cov_within(ix, iy, cx[j], cy[j], R2);
                            if (!claimed) s += (unsigned)M[ix * side + iy];
                        }
                    }
                sum[act] = s;
            }
            unsigned(*part)[3] = red[i & 1];   // double-buffered on the agent's parity: one barrier per agent (local.h)
#pragma unroll
            for (int act = 0; act < 3; act++) {
                for (int off = 32; off > 0; off >>= 1) sum[act] += __shfl_down(sum[act], off);
                if (lane == 0) part[tid >> 6][act] = sum[act];
            }
            __syncthreads();   // (the last agent's is the row-ending barrier)
            unsigned sc[3] = {0u, 0u, 0u};
            for (int w = 0; w < COV_WAVES; w++)
                for (int act = 0; act < 3; act++) sc[act] += part[w][act];
            int best = 0;
            if (sc[1] > sc[0]) best = 1;
            if (sc[2] > sc[best]) best = 2;
            if (tid == 0) c.actions[(e * (size_t)T + (size_t)t) * (size_t)n + i] = best;
            int qx, qy;
            cov_point(c, X, Y, h, best, qx, qy);
#pragma unroll
            for (int j = 0; j < CS_MAX_AGENTS; j++)
                if (j == i) {
                    cx[j] = qx;
                    cy[j] = qy;
                }
        }
    }
    // 7. rows past the episode's end: features +0.0f, labels 0 (k_feature_episodes' step 5)
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
    // 8. the expert's positions and link masks after the last live row (0 where no row wrote them: len == 0, slots >= n); the grids
    // are where they are
    if (a.prev_out && tid < 2 * CS_MAX_AGENTS) a.prev_out[e * (size_t)(2 * CS_MAX_AGENTS) + tid] = (tid & 1) ? ay[tid >> 1] : ax[tid >> 1];
    if (fa.heard_out && tid < CS_MAX_AGENTS) fa.heard_out[e * (size_t)CS_MAX_AGENTS + tid] = (int32_t)adj[tid];
}
