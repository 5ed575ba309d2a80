// cooperative-search_amd/csrc/local_plan.h -- cs_local_plan_actions: the sequence search of plan.h on n private grids per env under a
// communication range, one launch per decision (included by episodes.hip inside its namespace, after plan.h and local.h, whose cov_*
// helpers, plan_unpack, PlanArgs and constants it uses).
//
// The planner is DEFINED by local_plan.local_plan_actions_torch (stock torch ops, integer after the one quantisation); this kernel
// reproduces its actions, its plans and its scores bit for bit.  Agent i plans on its OWN grid, grids[b][i][ix * side + iy], which is
// only read (every cell as clamp(cell, 0, 2^19)), less the discs of the winning sequences of the agents j < i that it hears: the
// link test is local.h's (adj, a bit mask per agent, symmetric, own bit set), the claim rule is local.h's choose stage, and the
// search -- nodes, gains less the ancestors' discs, Q8 weights, the packed argmax, the action -- is plan.h's stages a to c.
//
// Layout: one workgroup of 256 threads per env.  LDS: plan.h's (W 16 KB, the node and gain tables, the 36 step offsets, four keys)
// plus adj[8] and the claim table, n * depth <= 40 packed points (x | y << 11, plan_unpack's): 19.9 KB, eight workgroups per CU of
// 160 KB, as k_plan_actions.  Lane i < n quantises agent i | barrier | lane i < n forms adj[i] | barrier | then per agent i:
//   load     W = agent i's row, clamped (16 bytes per lane when the entry point found every row aligned)        | barrier
//   claims   the block zeroes in W the depth discs of every j < i with bit j of adj[i] (16 x 16 tiles, as coverage.h);
//   a.       and thread q walks node q from agent i's pose (plan.h's a; it touches the node table only)          | barrier
//   b.       gains: a wavefront per node (plan.h's b)                                                           | barrier
//   c.       scores, the packed key, one shuffle reduction per wavefront, four keys through LDS (plan.h's c)    | barrier
//   store    thread 0 writes the three results; thread d < depth packs the winner's point of level d into claim[i][d].
// plan.h's stage d (zero the winner's discs in W) is gone: W is reloaded for the next agent, and the claim is replayed from the
// table by those who heard it.  Why W is reloaded and not kept: the n rows differ, so there is nothing to keep; why the claims are
// zeroed in W and not tested per cell as local.h does: a gain is summed for up to 363 nodes per agent, each against up to 35
// claim points -- zeroing once per agent is at most 35 discs of work, the per-cell test would be 35 tests in every one of the
// 363 sums.  The node walk shares the claims' phase and not the load's (a deviation from plan.h's order, which walks first):
// thread d < depth reads the winner's nodes AFTER barrier c, while faster threads are already loading the next row; the node
// table may therefore not be written before the next barrier, which is the load's.
//
// Every barrier stands outside any branch that depends on tid or on the data: n, depth, nodes and seqs are launch arguments and
// adj[i] is read from LDS after a barrier, so the trip counts of the claims loop are the same in all 256 threads.  No atomics, no
// host synchronisation, no global memory traffic but n clamped row reads (L2 hits when the base policy's launch just wrote them)
// and 24 bytes of results per agent.  Compiler's report (profiles/kernel_resources.txt, k_local_plan_actions): 63 VGPRs, 16
// SGPRs spilled to the lanes of a VGPR, no VGPR spills, no scratch, 19904 bytes of LDS.  LDS bounds it at eight workgroups (32
// waves) per CU, and 63 VGPRs allow exactly those eight waves per SIMD (512 / 64): k_plan_actions' occupancy, with no register
// to spare.
//
// What could go wrong in this shape, and why it does not:
//   a gain, a score or a key overflows   plan.h's bounds, unchanged: a cell is read as at most 2^19 and a map has at most 2^12 cells,
//                                        so a gain is at most 2^31 and fits an unsigned word; the D gains of a sequence are over
//                                        DISJOINT cells, so a score with weights <= 256 is at most 2^39 and a key is below 2^48.
//                                        Zeroed cells only lower a sum.
//   a thread with no sequence            tid >= 3^D holds key 0; a real key is at least 255 - 242 = 13.
//   the packed node word                 needs x, y <= 2047: after one step both are clamped to 0..16 side <= 1024, and stride >= 1
//                                        is checked by the entry point, so every node is at least one step from the pose (whose own
//                                        coordinates may be anything in +-2^15 and are never packed).  A claim point is a node.
//   the claim table index                claim[j * PLAN_MAX_DEPTH + d], j < i < n <= 8, d < depth <= 5: below 40 = the array.  It
//                                        is written by thread d after barrier c of agent i and read by all after the load barrier
//                                        of an agent > i.  Agent n - 1's claims are stored and never read.
//   a claim is read before it is stored  rows j < i only, each stored an agent ago or more, with at least one barrier between.
//   unaligned rows (side 7, odd agents)  agent i's row of env b starts (b n + i) cells words behind grids_dev.  The 16-byte path is
//                                        taken only when cells % 4 == 0 AND grids_dev is 16-byte aligned (vec4, decided by the
//                                        entry point as for local.h): then every row of every agent is aligned.  At side 7 (49
//                                        cells), or from a base off 16 bytes, the whole launch goes one cell per lane.
//   side^2 < 256, side 1                 idle threads run no loop body and fall through to every barrier.
//   view_range 0                         R = 0: a cell counts, or is zeroed, only if its centre IS the point; cov_box is that cell
//                                        or empty.  All scores may be 0: sequence 0 wins (key 255), action 0.
//   view_range 64                        R = 1024: every box is the whole map; the sums stay within the bounds above.
//   NaN or huge state floats             cov_quant clamps (NaN to the lower bound): |X|, |Y| <= 2^15; the first step clamps to the map.
//   the link test wraps                  clamped positions differ by up to 2^16 per axis and a square reaches 2^32: the differences
//                                        are widened to long long BEFORE they are squared (local.h's test, restated), and compared
//                                        with (16 comm_range)^2 <= 2^22 as long long.  C2 = -1 is unlimited; the test is strict, so
//                                        C2 = 0 links nobody; the own bit is set apart from it.
//   B * n * cells past 2^31              the row index is formed in size_t.
struct LocalPlanArgs {
    PlanArgs p;     // p.grid: [B][n][side * side]; p.vec4: every row of every agent is a whole number of aligned 16-byte pieces
    long long C2;   // (16 comm_range)^2, or -1: unlimited
};

__global__ __launch_bounds__(COV_THREADS) void k_local_plan_actions(LocalPlanArgs la) {
    __shared__ __attribute__((aligned(16))) unsigned W[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ unsigned node[PLAN_MAX_NODES], gain[PLAN_MAX_NODES];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS];
    __shared__ unsigned adj[CS_MAX_AGENTS];
    __shared__ unsigned claim[CS_MAX_AGENTS * PLAN_MAX_DEPTH];
    __shared__ int sx[COV_HEADINGS], sy[COV_HEADINGS];
    __shared__ unsigned long long red[COV_WAVES];
    const PlanArgs &a = la.p;
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
        // load: W = agent i's row, clamped (every thread is past its last read of W: barrier b of the agent before)
        const int32_t *G = a.grid + (b * (size_t)n + (size_t)i) * (size_t)cells;
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
        // claims: the discs of the winning sequences of the linked agents that decided before agent i
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
                        if (cov_within(ix, iy, px, py, R2)) W[ix * side + iy] = 0u;
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
