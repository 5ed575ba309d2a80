// cooperative-search_amd/csrc/local.h -- cs_local_coverage_actions: the coverage baseline under a limited communication range, one
// launch per decision over n private grids per env (included by episodes.hip inside its namespace, after coverage.h; DESIGN.md
// section 25).
//
// The policy is DEFINED by local.local_coverage_actions_torch (stock torch ops, integer after the one quantisation); this kernel
// reproduces its n grids and its actions bit for bit.  Agent i keeps a grid of its own, grids[b][i][ix * side + iy].  Per call: every
// grid regrows and is swept by its OWN agent's disc (cov_update with one agent: S_i); the link test says who hears whom (adj, a bit
// mask per agent, symmetric, own bit set); M_i = min over the linked j of S_j, cell by cell, is written back; then the agents decide
// in index order on M_i less the footprints that the linked agents before them have claimed.
//
// Layout: one workgroup of 256 threads per env.  Lane i < n quantises agent i (k_coverage_actions' step 1) | barrier | lane i < n
// forms adj[i] | barrier | merge: a thread owns a cell (four consecutive cells on the 16-byte path) of ALL n grids | barrier |
// choose: coverage.h's loop over the 16 x 16 tiles of cov_box, reading M_i from global memory.
//
// LDS or L2 for the choose stage -- L2.  k_coverage_actions stages its one grid in LDS because the sweep already holds every cell
// in a register when it stores it, and the claims are then zeroed in that copy.  Here the merge writes n grids; staging them all is
// n * 16 KB of LDS (128 KB at n = 8: one workgroup per CU of 160 KB, four waves where 32 fit), and staging them one at a time is a
// second pass over all cells of M_i (2500 loads at side 50) for a stage that reads only the three footprints of agent i: at view_range
// 7 they overlap almost entirely and hold about 190 distinct cells, under a tenth of the grid.  Those cells were stored by this
// workgroup a moment ago: the vector L1 is write-through, so they sit in this XCD's L2.  The claims need no copy of the grid
// either: a claimed cell is one within R of an earlier agent's chosen point, which is two integers per claim in registers, and the
// sum is taken over "in the footprint and in no heard claim".  So the kernel keeps 224 bytes of LDS (compiler's report:
// profiles/kernel_resources.txt, k_local_coverage_actions: 90 VGPRs, 4 SGPRs spilled to lanes, no VGPR spills, no scratch).
// Registers, not LDS, bound it: 90 VGPRs allow 5 waves per SIMD, five workgroups per CU where k_coverage_actions' 16.5 KB of
// LDS and 30 VGPRs allow eight; the merge holds four cells of eight grids (32 VGPRs) whatever n is.  What it moves: every cell
// of n grids read once and written once, n times k_coverage_actions' grid traffic, plus the footprint reads.
//
// What could go wrong in this shape, and why it does not:
//   the merge is in place                 cell c of M_i depends on cell c of S_0 .. S_n-1 and on nothing else.  The thread that owns c
//                                         loads c from all n grids into registers (the unrolled loop over j), and only then stores
//                                         (the loop over i); no other thread of this or any workgroup touches c of this env.
//                                         Nobody reads a grid that is already merged: before the barrier that ends the stage a
//                                         thread reads only its own cells.
//   the link test wraps                   clamped positions differ by up to 2^16 per axis, a square reaches 2^32: the differences are
//                                         widened to long long BEFORE they are squared, the sum is at most 2^33, and it is compared
//                                         with (16 comm_range)^2 <= 2^22 as long long.  comm_range < 0 is held as C2 = -1 and skips
//                                         the test.  The comparison is strict: C2 = 0 links nobody; the own bit is set apart from it.
//   the choose stage reads stale cells    it loads M_i that other threads of this workgroup stored.  __syncthreads() stands between:
//                                         it is a workgroup-scope release (every store of the wave has left: vmcnt(0)), the barrier,
//                                         and a workgroup-scope acquire, and the waves of a workgroup share one CU and its L1.
//                                         Every later barrier is the choose loop's own; no cell is stored after the merge.
//   trip counts                           W_i is not materialised.  The loops run over cov_box of the candidate's point, in 16 x 16
//                                         tiles as coverage.h's do (a box larger than the block takes several passes, never truncated);
//                                         a claim only decides whether a cell inside that box is added.  The claim points are
//                                         cov_point's, clamped to the map, so cov_within's squares fit as they do for a footprint.
//   16-byte accesses on unaligned rows    agent i's row of env b starts (b n + i) cells words behind grids_dev.  The 16-byte path is
//                                         taken only when cells % 4 == 0 AND grids_dev is 16-byte aligned (vec4, decided by the entry
//                                         point): then EVERY row, of every agent, starts on a multiple of 16 bytes whatever n is (side
//                                         50: 10000 bytes).  At side 7 (49 cells) the rows of the odd agents are not aligned and the
//                                         whole launch goes one cell per lane.
//   dynamic indices into register arrays  v[], cx[] and cy[] are indexed by unrolled loop counters only (a run-time `i` is matched by
//                                         `if (j == i)` inside an unrolled loop), so they stay in registers: scratch 0.
//   barriers in the choose loop           one per agent: red is double-buffered on the agent's parity, so the partial sums of agent
//                                         i + 2 are stored only by threads that have passed agent i + 1's barrier, which every thread
//                                         reaches after it has read agent i's.  Every thread forms the pick from red itself: there is
//                                         no broadcast to wait for.  n, side, R and the boxes are the same in all 256 threads.
//   side^2 < 256, side 1                  idle threads run no loop body and fall through to every barrier; at side 1 the one cell goes
//                                         the scalar way.
//   view_range 0                          R = 0: a cell is swept, or summed, only if its centre IS the point; cov_box is that cell or
//                                         empty.  All three scores may be 0: action 0 (the lowest wins a tie).
//   view_range 64                         R = 1024: the boxes are the whole map, 16 passes of 256 cells at side 64; a score is at most
//                                         2^12 * 2^16 = 2^28 (cells hold 0..65536 after the merge), unsigned.
//   lookahead 0                           the three points are the agent's own clamped position and tie: action 0.
//   B * n * cells past 2^31               every global index is formed in size_t.
//   NaN or huge state floats              cov_quant clamps (NaN to the lower bound): |X| <= 2^15, as in coverage.h.
constexpr int LOC_MAX_COMM = 128;   // cells; the map is at most 64 wide, its diagonal under 91

struct LocalArgs {
    CoverageArgs c;   // c.grid: [B][n][side * side]; c.vec4: every row of every agent is a whole number of aligned 16-byte pieces
    long long C2;     // (16 comm_range)^2, or -1: unlimited
};

__global__ __launch_bounds__(COV_THREADS) void k_local_coverage_actions(LocalArgs la) {
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS];
    __shared__ unsigned adj[CS_MAX_AGENTS];
    __shared__ unsigned red[2][COV_WAVES][3];
    const CoverageArgs &a = la.c;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int n = a.n, side = a.side, cells = side * side;
    const unsigned R2 = (unsigned)a.R * (unsigned)a.R;
    // 1. quantise: lane i owns agent i
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
    __syncthreads();
    // 2. links: lane i forms the mask of those agent i hears (its own bit always; the test is symmetric in i and j)
    if (tid < n) {
        unsigned m = 1u << tid;
        for (int j = 0; j < n; j++) {
            const long long dx = (long long)ax[tid] - (long long)ax[j], dy = (long long)ay[tid] - (long long)ay[j];
            if (la.C2 < 0 || dx * dx + dy * dy < la.C2) m |= 1u << j;
        }
        adj[tid] = m;
    }
    __syncthreads();
    // 3. regrow, own sweep and merge: a thread holds its cells of all n grids before it stores any of them
    int32_t *G = a.grid + b * (size_t)n * (size_t)cells;
    CoverageArgs one = a;   // cov_update with one agent: the regrowth and the sweep of that agent's disc alone
    one.n = 1;
    if (a.vec4) {
        for (int q = tid; q < cells / 4; q += COV_THREADS) {
            const int ix0 = (4 * q) / side, iy0 = 4 * q - ix0 * side;
            int4 v[CS_MAX_AGENTS];
#pragma unroll
            for (int j = 0; j < CS_MAX_AGENTS; j++) {
                v[j] = make_int4(0, 0, 0, 0);
                if (j < n) {
                    v[j] = reinterpret_cast<const int4 *>(G + (size_t)j * cells)[q];
                    int *e = reinterpret_cast<int *>(&v[j]);
                    int ix = ix0, iy = iy0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        e[k] = cov_update(one, ax + j, ay + j, R2, ix, iy, e[k]);
                        if (++iy == side) {
                            iy = 0;
                            ix++;
                        }
                    }
                }
            }
            for (int i = 0; i < n; i++) {   // (adj[i] holds bit i: the minimum starts above every cell and takes in S_i itself)
                const unsigned m = adj[i];
                int4 r = make_int4(65537, 65537, 65537, 65537);
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
                if (j < n) v[j] = cov_update(one, ax + j, ay + j, R2, ix, iy, G[(size_t)j * cells + idx]);
            }
            for (int i = 0; i < n; i++) {
                const unsigned m = adj[i];
                int r = 65537;
#pragma unroll
                for (int j = 0; j < CS_MAX_AGENTS; j++)
                    if ((m >> j) & 1u) r = min(r, v[j]);
                G[(size_t)i * cells + idx] = r;
            }
        }
    }
    __syncthreads();   // the choose stage reads cells that other threads of this workgroup have just stored
    // 4. choose, agent by agent, on M_i less the claims agent i has heard: those of the linked agents before it
    int cx[CS_MAX_AGENTS], cy[CS_MAX_AGENTS];
#pragma unroll
    for (int j = 0; j < CS_MAX_AGENTS; j++) cx[j] = cy[j] = 0;
    for (int i = 0; i < n; i++) {
        const int X = ax[i], Y = ay[i], h = ah[i];
        const unsigned heard = adj[i] & ((1u << i) - 1u);
        const int32_t *M = G + (size_t)i * cells;
        unsigned acc[3];
#pragma unroll
        for (int act = 0; act < 3; act++) {
            int px, py;
            cov_point(a, X, Y, h, act, px, py);
            const CovBox box = cov_box(px, py, a.R, side);
            unsigned s = 0;
            for (int bx = tid >> 4; bx < box.w; bx += 16)   // 16 x 16 tiles of the box, as in coverage.h
                for (int by = tid & 15; by < box.h; by += 16) {
                    const int ix = box.x0 + bx, iy = box.y0 + by;
                    if (cov_within(ix, iy, px, py, R2)) {
                        bool claimed = false;
#pragma unroll
                        for (int j = 0; j < CS_MAX_AGENTS - 1; j++)   // (agent 7 is heard by nobody: all decide before it)
                            if ((heard >> j) & 1u) claimed = claimed || cov_within(ix, iy, cx[j], cy[j], R2);
                        if (!claimed) s += (unsigned)M[ix * side + iy];
                    }
                }
            acc[act] = s;
        }
        unsigned(*part)[3] = red[i & 1];
#pragma unroll
        for (int act = 0; act < 3; act++) {
            for (int off = 32; off > 0; off >>= 1) acc[act] += __shfl_down(acc[act], off);
            if ((tid & 63) == 0) part[tid >> 6][act] = acc[act];
        }
        __syncthreads();
        unsigned sc[3] = {0u, 0u, 0u};
        for (int w = 0; w < COV_WAVES; w++)
            for (int act = 0; act < 3; act++) sc[act] += part[w][act];
        int best = 0;
        if (sc[1] > sc[0]) best = 1;
        if (sc[2] > sc[best]) best = 2;
        if (tid == 0) a.actions[b * (size_t)n + i] = best;
        int px, py;
        cov_point(a, X, Y, h, best, px, py);
#pragma unroll
        for (int j = 0; j < CS_MAX_AGENTS; j++)
            if (j == i) {
                cx[j] = px;
                cy[j] = py;
            }
    }
}
