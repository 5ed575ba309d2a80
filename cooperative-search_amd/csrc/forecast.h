// cooperative-search_amd/csrc/forecast.h -- cs_belief_forecast and cs_plan_forecast_actions: the density predicted along the
// planning horizon, and the sequence search scored on it (included by episodes.hip inside its namespace, after belief.h whose
// bel_* helpers and plan.h whose PlanArgs / plan_unpack it uses).
//
// Both are DEFINED in forecast.py (stock torch ops, all integer): forecast.forecast_torch and
// forecast.plan_forecast_actions_torch.  The kernels reproduce them element for element.
//
// k_belief_forecast: one workgroup of 256 threads per env, the shape of k_belief_actions.  Two LDS arrays of 64 * 64 words
// (32 KB): `src` holds the density of the level reached so far, `acc` is the scatter accumulator; they swap after every move.
// Level d is moves[d] prediction steps (belief.h's bel_scatter, the agents held at pos) beyond level d - 1, capped at 2^19 as
// each move ends, and is written to stack[b][d] when its moves are done (16 bytes per lane where the rows allow).  Per move:
// zero acc | barrier | scatter src -> acc | barrier | cap acc, swap | barrier.  The trip counts (levels, moves[d]) are launch
// arguments, so every barrier is outside any branch on tid, side or the data and all 256 threads reach each of them.  LDS
// atomics as belief.h (integer adds commute), no global atomics, no host synchronisation.
//
// What could go wrong in this shape, and why it does not:
//   an accumulator word wraps        every source word is at most CAP = 2^19 (the grid is clamped as it is read, a predicted level
//                                    is capped before it becomes a source), so belief.h's bound holds for every move: a whole
//                                    map sums to at most 2^31.
//   a level without moves            moves[d] = 0 runs no move and writes src again: a copy of the level before (of the clamped
//                                    grid for d = 0).
//   an index leaves the arrays       cells <= 4096 = an array; bel_spread clamps every destination to 0..side - 1 per axis.
//   pos off the map                  read clamped to +-2^15, belief.h's bound on the squares.
//   the 16-byte paths                the read needs cells % 4 == 0 and an aligned grid, the write cells % 4 == 0 and an aligned
//                                    stack (then every level's row is aligned too); each has its own flag.
//
// k_plan_forecast_actions: k_plan_actions with W holding `depth` levels: a node of level d sums its gain over W[d], and the
// winner's D discs are zeroed in EVERY level.  All its LDS is one dynamic region, carved in 16-byte multiples: four 64-bit keys,
// W (depth * cells words, cells rounded up to a multiple of 4 so that every level starts 16-byte aligned), the node and gain
// tables, the poses and the step offsets: 3.3 KB + 4 depth cells bytes, 43 KB at side 50 and depth 4, 85 KB at side 64 and
// depth 5.  Above 64 KB the entry point raises the kernel's dynamic-LDS limit first (a CU has 160 KB).  The bounds of plan.h
// hold per level: a gain is at most 2^31, the D gains of a sequence are over disjoint cells, a score is at most 2^39.
constexpr int FC_MAX_LEVELS = PLAN_MAX_DEPTH;
constexpr int FC_TABLE_WORDS = 2 * 364 + 3 * CS_MAX_AGENTS + 2 * COV_HEADINGS;   // node, gain (363 rounded up), ax ay ah, sx sy

struct ForecastArgs {
    BeliefArgs b;          // c.n, c.side, mode, sense2, dx, dy (the rest unused)
    const int32_t *grid;   // [B][cells]
    const int32_t *pos;    // [B][8][2]
    int32_t *stack;        // [B][levels][cells]
    int levels, moves[FC_MAX_LEVELS];
    int vec_in, vec_out;   // a grid row / a stack row is a whole number of aligned 16-byte pieces
};

__global__ __launch_bounds__(COV_THREADS) void k_belief_forecast(ForecastArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned buf0[CS_MAX_MAP * CS_MAX_MAP], buf1[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int px[CS_MAX_AGENTS], py[CS_MAX_AGENTS];
    __shared__ int ox[BEL_HEADINGS], fx[BEL_HEADINGS], oy[BEL_HEADINGS], fy[BEL_HEADINGS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int side = a.b.c.side, cells = side * side;
    if (tid < a.b.c.n) {
        const int32_t *p = a.pos + ((size_t)b * CS_MAX_AGENTS + tid) * 2;
        px[tid] = min(max(p[0], -32768), 32768);
        py[tid] = min(max(p[1], -32768), 32768);
    }
    if (tid >= 64 && tid < 64 + BEL_HEADINGS) {   // (another wavefront than the agents')
        const int k = tid - 64;
        ox[k] = a.b.dx[k] >> 4;
        fx[k] = a.b.dx[k] & 15;
        oy[k] = a.b.dy[k] >> 4;
        fy[k] = a.b.dy[k] & 15;
    }
    // F_{-1}: the grid row, clamped
    const int32_t *G = a.grid + (size_t)b * cells;
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
    unsigned *src = buf0, *acc = buf1;
    int32_t *out = a.stack + (size_t)b * a.levels * cells;
    for (int d = 0; d < a.levels; d++) {
        for (int m = 0; m < a.moves[d]; m++) {
            for (int idx = tid; idx < cells; idx += COV_THREADS) acc[idx] = 0u;
            __syncthreads();
            for (int idx = tid; idx < cells; idx += COV_THREADS) {
                const int ix = idx / side, iy = idx - ix * side;
                bel_scatter(a.b, acc, px, py, ox, fx, oy, fy, ix, iy, (int)src[idx]);
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

// bytes of dynamic LDS of k_plan_forecast_actions: the keys, `depth` levels of level_words words, the tables
__host__ __device__ constexpr size_t fc_plan_lds_bytes(int depth, int level_words) {
    return 32 + 4 * ((size_t)depth * level_words + FC_TABLE_WORDS);
}

// a.grid is the stack [B][depth][cells]; level_words = cells rounded up to a multiple of 4
__global__ __launch_bounds__(COV_THREADS) void k_plan_forecast_actions(PlanArgs a, int level_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fc_lds[];
    unsigned long long *red = reinterpret_cast<unsigned long long *>(fc_lds);   // [COV_WAVES]
    unsigned *W = reinterpret_cast<unsigned *>(fc_lds + 32);                       // [depth][level_words]
    unsigned *node = W + a.depth * level_words, *gain = node + 364;
    int *ax = reinterpret_cast<int *>(gain + 364), *ay = ax + CS_MAX_AGENTS, *ah = ay + CS_MAX_AGENTS;
    int *sx = ah + CS_MAX_AGENTS, *sy = sx + COV_HEADINGS;
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
    // 2. W = the env's `depth` levels, clamped
    const int32_t *G = a.grid + (size_t)b * a.depth * cells;
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
            a.actions[(size_t)b * a.n + i] = pick / (a.seqs / 3);
            a.plans[(size_t)b * a.n + i] = pick;
            a.scores[(size_t)b * a.n + i] = (int64_t)(key >> 8);
        }
        // d. the winner claims its D discs in every level
        {
            int first = 0, cnt = 3, div = a.seqs / 3;
            for (int d = 0; d < a.depth; d++) {
                int px, py;
                plan_unpack(node[first + pick / div], px, py);
                const CovBox box = cov_box(px, py, a.R, side);
                for (int bx = tid >> 4; bx < box.w; bx += 16)
                    for (int by = tid & 15; by < box.h; by += 16) {
                        const int ix = box.x0 + bx, iy = box.y0 + by;
                        if (cov_within(ix, iy, px, py, R2))
                            for (int l = 0; l < a.depth; l++) W[l * level_words + ix * side + iy] = 0u;
                    }
                first += cnt;
                cnt *= 3;
                div = max(div / 3, 1);
            }
        }
        __syncthreads();   // (also: node, gain and red are free for the next agent)
    }
}
