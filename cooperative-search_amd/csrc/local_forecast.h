// cooperative-search_amd/csrc/local_forecast.h -- cs_local_belief_forecast and cs_local_plan_forecast_actions: every agent's private
// density predicted along the planning horizon with the team-mates it hears, and the sequence search of local_plan.h scored on it
// (included by episodes.hip inside its namespace, after forecast.h, whose ForecastArgs and fc_plan_lds_bytes it uses with belief.h's
// bel_* helpers, coverage.h's cov_* helpers and plan.h's PlanArgs / plan_unpack, and after local_plan.h, whose LocalPlanArgs it takes;
// DESIGN.md section 29).
//
// Both are DEFINED in local_forecast.py (stock torch ops, integer after the one quantisation): local_forecast_torch and
// local_plan_forecast_actions_torch.  The kernels reproduce them bit for bit.
//
// k_local_belief_forecast: k_belief_forecast's shape, one workgroup of 256 threads per (env, agent), blockIdx.x = b n + i, two LDS
// arrays of 64 * 64 words (32 KB).  Row b n + i of grids is agent i's grid; rows (b n + i) levels .. of stacks are its levels.  The
// prologue reads heard[b][i] -- every thread the same word -- as (heard & ((1 << n) - 1)) | (1 << i), and lane j < n with its bit
// set stores prev[b][j], clamped to +-2^15, into slot popcount(mask below bit j) of the LDS position list: the heard agents in index
// order, compacted.  The move loop is forecast.h's, with bel_scatter looping over the popcount(mask) listed agents (an args copy whose
// n is the count).  Per move: zero acc | barrier | scatter src -> acc | barrier | cap acc, swap | barrier.  The trip counts (levels,
// moves[d]) are launch arguments and the count is the same in every thread, so every barrier is outside any branch on tid, side or
// the data and all 256 threads reach each of them.  LDS atomics as belief.h (integer adds commute), no global atomics.
//
// What could go wrong in this shape, and why it does not:
//   an accumulator word wraps        forecast.h's bound: every source word is at most CAP = 2^19, a whole map sums to at most 2^31.
//   heard has garbage bits           bits at and above n are dropped and the own bit is set before anything is done with the word: a
//                                    slot is popcount of at most n - 1 bits, below 8 = the list; the count is 1..n, and every slot
//                                    below it is written (by the lane of the bit that counts it) before the first barrier.
//   the list is in another order     slot = the number of heard agents with a lower index: index order, so bel_scatter's lowest-index
//                                    tie rule picks what heard_prev's list makes predict_torch pick.
//   walk mode                        bel_scatter reads no position: the mask plays no part, as in the definition.
//   an index leaves the arrays       cells <= 4096 = an array; bel_spread clamps every destination to 0..side - 1 per axis.
//   prev off the map                 read clamped to +-2^15, belief.h's bound on the squares.
//   B * n * levels * cells past 2^31 the row index is a size_t from the start (blockIdx.x widened), and so is every offset.
//   the 16-byte paths                row r of grids starts r cells words in, row r levels of stacks r levels cells words in: both are
//                                    whole 16-byte pieces when cells % 4 == 0 and the base is aligned; one flag for each side
//                                    (vec_in, vec_out), decided by the entry point as for forecast.h.
//
// k_local_plan_forecast_actions: k_local_plan_actions with W holding `depth` levels.  One workgroup of 256 threads per env.  All its
// LDS is one dynamic region carved as k_plan_forecast_actions carves it -- four 64-bit keys, W (depth * level_words words, level_words
// = cells rounded up to a multiple of 4), the node and gain tables, the poses, the step offsets -- plus adj[8] and the claim table of
// 40 packed points: 3.5 KB + 4 depth level_words bytes, 43 KB at side 50 and depth 4, 85.4 KB at side 64 and depth 5.  Above 64 KB
// the entry point raises the kernel's dynamic-LDS limit first.  Per agent i:
//   load     W = agent i's `depth` levels, clamped (16 bytes per lane when every row is aligned and cells % 4 == 0: the levels are
//            then contiguous on both sides; otherwise level by level at level_words pitch)                         | barrier
//   claims   the block zeroes the depth discs of every heard j < i in EVERY level of W; thread q walks node q       | barrier
//   b.       gains: a wavefront per node, a node of level d summed over W[d] (forecast.h's b)                       | barrier
//   c.       scores, the packed key, the reduction (plan.h's c)                                                     | barrier
//   store    thread 0 writes the three results; thread d < depth packs the winner's point of level d into claim[i][d].
// There is no stage d, for local_plan.h's reason: W is reloaded for the next agent and the claim is replayed by those who hear it.
// The order of phases and every barrier are local_plan.h's, and so is the reason why the node walk shares the claims' phase.
//
// What could go wrong in this shape, and why it does not (beyond local_plan.h's list, which holds per level):
//   W at level_words pitch           a cell of level l is W[l * level_words + ix * side + iy], l < depth, ix * side + iy < cells <=
//                                    level_words: below depth * level_words = the words carved for W.  The 16-byte load writes
//                                    depth * cells / 4 pieces, and takes that path only when cells == level_words.  At side 7 the
//                                    three pad words of a level (49 .. 51) are never written and never read.
//   the claim table index            claim[j * PLAN_MAX_DEPTH + d], j < i < n <= 8, d < depth <= 5: below 40 = the words carved
//                                    for it.  Written by thread d after barrier c of agent j, read after the load barrier of an
//                                    agent > j.
//   the carve is misaligned          every part is a multiple of 16 bytes (32, 4 * 4k, 4 * 364 * 2, 4 * 24, 4 * 72, 4 * 8, 4 * 40).
//   more LDS than a launch is given  the entry point computes lfc_plan_lds_bytes, the same expression the kernel's carve adds up to.
//   the link test wraps              local.h's test: the differences are widened to long long BEFORE they are squared.
//   B * n * depth * cells past 2^31  the row index is formed in size_t.
struct LocalForecastArgs {
    ForecastArgs f;         // f.b.c.n: the team's n; f.grid: [B][n][cells]; f.pos: prev [B][8][2]; f.stack: [B][n][levels][cells]
    const int32_t *heard;   // [B][8]
};

__global__ __launch_bounds__(COV_THREADS) void k_local_belief_forecast(LocalForecastArgs la) {
    __shared__ __attribute__((aligned(16))) unsigned buf0[CS_MAX_MAP * CS_MAX_MAP], buf1[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int px[CS_MAX_AGENTS], py[CS_MAX_AGENTS];
    __shared__ int ox[BEL_HEADINGS], fx[BEL_HEADINGS], oy[BEL_HEADINGS], fy[BEL_HEADINGS];
    const ForecastArgs &a = la.f;
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;   // b n + i
    const int n = a.b.c.n, side = a.b.c.side, cells = side * side;
    const size_t b = row / (size_t)n;
    const int i = (int)(row - b * (size_t)n);
    // whom agent i heard: the same word in every thread
    const unsigned mask = ((unsigned)la.heard[b * CS_MAX_AGENTS + i] & ((1u << n) - 1u)) | (1u << i);
    if (tid < n && ((mask >> tid) & 1u)) {   // the heard agents, compacted in index order
        const int slot = __popc(mask & ((1u << tid) - 1u));
        const int32_t *p = a.pos + (b * CS_MAX_AGENTS + tid) * 2;
        px[slot] = min(max(p[0], -32768), 32768);
        py[slot] = min(max(p[1], -32768), 32768);
    }
    if (tid >= 64 && tid < 64 + BEL_HEADINGS) {   // (another wavefront than the agents')
        const int k = tid - 64;
        ox[k] = a.b.dx[k] >> 4;
        fx[k] = a.b.dx[k] & 15;
        oy[k] = a.b.dy[k] >> 4;
        fy[k] = a.b.dy[k] & 15;
    }
    // F_{-1}: agent i's grid row, clamped
    const int32_t *G = a.grid + row * (size_t)cells;
    if (a.vec_in) {
        for (int q = tid; q < cells / 4; q += COV_THREADS) {
            int4 v = reinterpret_cast<const int4 *>(G)[q];
            v.x = min(max(v.x, 0), BEL_CAP);
            v.y = min(max(v.y, 0), BEL_CAP);
            v.z = min(max(v.z, 0), BEL_CAP);
            v.w = min(max(v.w, 0), BEL_CAP);
            reinterpret_cast<int4 *>(buf0)[q] = v;
        }
    } else {
        for (int idx = tid; idx < cells; idx += COV_THREADS) buf0[idx] = (unsigned)min(max(G[idx], 0), BEL_CAP);
    }
    __syncthreads();
    BeliefArgs known = a.b;   // bel_scatter loops the listed agents only
    known.c.n = __popc(mask);
    unsigned *src = buf0, *acc = buf1;
    int32_t *out = a.stack + row * (size_t)a.levels * (size_t)cells;
    for (int d = 0; d < a.levels; d++) {
        for (int m = 0; m < a.moves[d]; m++) {
            for (int idx = tid; idx < cells; idx += COV_THREADS) acc[idx] = 0u;
            __syncthreads();
            for (int idx = tid; idx < cells; idx += COV_THREADS) {
                const int ix = idx / side, iy = idx - ix * side;
                bel_scatter(known, acc, px, py, ox, fx, oy, fy, ix, iy, (int)src[idx]);
            }
            __syncthreads();
            for (int idx = tid; idx < cells; idx += COV_THREADS) acc[idx] = min(acc[idx], (unsigned)BEL_CAP);
            unsigned *t = src;
            src = acc;
            acc = t;
            __syncthreads();
        }
        if (a.vec_out) {
            for (int q = tid; q < cells / 4; q += COV_THREADS) reinterpret_cast<int4 *>(out)[q] = reinterpret_cast<const int4 *>(src)[q];
        } else {
            for (int idx = tid; idx < cells; idx += COV_THREADS) out[idx] = (int32_t)src[idx];
        }
        out += cells;
    }
}

constexpr int LFC_EXTRA_WORDS = CS_MAX_AGENTS + CS_MAX_AGENTS * PLAN_MAX_DEPTH;   // adj, claim

// bytes of dynamic LDS of k_local_plan_forecast_actions: k_plan_forecast_actions', adj and the claim table
__host__ __device__ constexpr size_t lfc_plan_lds_bytes(int depth, int level_words) {
    return fc_plan_lds_bytes(depth, level_words) + 4 * (size_t)LFC_EXTRA_WORDS;
}

// la.p.grid is the stacks [B][n][depth][cells]; level_words = cells rounded up to a multiple of 4
__global__ __launch_bounds__(COV_THREADS) void k_local_plan_forecast_actions(LocalPlanArgs la, int level_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lfc_lds[];
    const PlanArgs &a = la.p;
    unsigned long long *red = reinterpret_cast<unsigned long long *>(lfc_lds);   // [COV_WAVES]
    unsigned *W = reinterpret_cast<unsigned *>(lfc_lds + 32);                       // [depth][level_words]
    unsigned *node = W + a.depth * level_words, *gain = node + 364;
    int *ax = reinterpret_cast<int *>(gain + 364), *ay = ax + CS_MAX_AGENTS, *ah = ay + CS_MAX_AGENTS;
    int *sx = ah + CS_MAX_AGENTS, *sy = sx + COV_HEADINGS;
    unsigned *adj = reinterpret_cast<unsigned *>(sy + COV_HEADINGS), *claim = adj + CS_MAX_AGENTS;   // [8], [8][PLAN_MAX_DEPTH]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t b = blockIdx.x;
    const int n = a.n, side = a.side, cells = side * side, lim = 16 * side;
    const unsigned R2 = (unsigned)a.R * (unsigned)a.R;
    // 1. quantise: lane i owns agent i (coverage.h's); another wavefront fills the step offsets
    if (tid < n) {
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
    if (tid >= 64 && tid < 64 + COV_HEADINGS) {
        sx[tid - 64] = (16 * COV_CT[tid - 64]) >> 14;   // (>> of a negative int is arithmetic on this compiler: it floors)
        sy[tid - 64] = (16 * COV_ST[tid - 64]) >> 14;
    }
    __syncthreads();
    // 2. links: lane i forms the mask of those agent i hears (local.h's test: 64-bit, strict, the own bit apart from it)
    if (tid < n) {
        unsigned m = 1u << tid;
        for (int j = 0; j < n; j++) {
            const long long dx = (long long)ax[tid] - (long long)ax[j], dy = (long long)ay[tid] - (long long)ay[j];
            if (la.C2 < 0 || dx * dx + dy * dy < la.C2) m |= 1u << j;
        }
        adj[tid] = m;
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {
        // load: W = agent i's `depth` levels, clamped (every thread is past its last read of W: barrier b of the agent before)
        const int32_t *G = a.grid + (b * (size_t)n + (size_t)i) * (size_t)a.depth * (size_t)cells;
        if (a.vec4) {   // cells % 4 == 0: level_words == cells, the levels are contiguous on both sides
            for (int q = tid; q < a.depth * cells / 4; q += COV_THREADS) {
                int4 v = reinterpret_cast<const int4 *>(G)[q];
                v.x = min(max(v.x, 0), PLAN_CAP);
                v.y = min(max(v.y, 0), PLAN_CAP);
                v.z = min(max(v.z, 0), PLAN_CAP);
                v.w = min(max(v.w, 0), PLAN_CAP);
                reinterpret_cast<int4 *>(W)[q] = v;
            }
        } else {
            for (int d = 0; d < a.depth; d++)
                for (int idx = tid; idx < cells; idx += COV_THREADS) W[d * level_words + idx] = (unsigned)min(max(G[d * cells + idx], 0), PLAN_CAP);
        }
        __syncthreads();
        // claims: the discs of the winning sequences of the linked agents that decided before agent i, in every level
        const unsigned heard = adj[i] & ((1u << i) - 1u);
        for (int j = 0; j < i; j++) {
            if (!((heard >> j) & 1u)) continue;   // (block-uniform: adj[i] is the same word in every thread)
            for (int d = 0; d < a.depth; d++) {
                int px, py;
                plan_unpack(claim[j * PLAN_MAX_DEPTH + d], px, py);
                const CovBox box = cov_box(px, py, a.R, side);
                for (int bx = tid >> 4; bx < box.w; bx += 16)
                    for (int by = tid & 15; by < box.h; by += 16) {
                        const int ix = box.x0 + bx, iy = box.y0 + by;
                        if (cov_within(ix, iy, px, py, R2))
                            for (int l = 0; l < a.depth; l++) W[l * level_words + ix * side + iy] = 0u;
                    }
            }
        }
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
        // b. gains: a wavefront per node, summed over the node's own level of W
        for (int q = wave; q < a.nodes; q += COV_WAVES) {
            int d = 0, first = 0, cnt = 3;
            while (q >= first + cnt) {
                first += cnt;
                cnt *= 3;
                d++;
            }
            const unsigned *Wd = W + d * level_words;
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
                    if (in) s += Wd[ix * side + iy];
                }
            }
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
            if (lane == 0) gain[q] = s;
        }
        __syncthreads();
        // c. scores and the packed argmax (plan.h's)
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
            a.actions[b * (size_t)n + i] = pick / (a.seqs / 3);
            a.plans[b * (size_t)n + i] = pick;
            a.scores[b * (size_t)n + i] = (int64_t)(key >> 8);
        }
        // store: thread d keeps the winner's point of level d (node d of the sequence: first_d + pick / 3^(D-1-d)) for those who hear it
        if (tid < a.depth) {
            int first = 0, cnt = 3, div = a.seqs / 3;
            for (int d = 0; d < tid; d++) {
                first += cnt;
                cnt *= 3;
                div = max(div / 3, 1);
            }
            claim[i * PLAN_MAX_DEPTH + tid] = node[first + pick / div] & ((1u << 22) - 1u);
        }
        // (no barrier here: the next writes of W, red, gain and node stand behind the load barrier of the next agent or later, and
        // the claim is read behind it too)
    }
}
