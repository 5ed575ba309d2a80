// cooperative-search_amd/csrc/local_belief.h -- cs_local_belief_actions: the target-density filter under a limited communication range,
// one launch per decision over n private densities per env (included by episodes.hip inside its namespace, after belief.h and local.h,
// whose device helpers it calls).
//
// The policy is DEFINED by local_belief.local_belief_actions_torch (stock torch ops, integer after the one quantisation); this kernel
// reproduces its n grids, prev, heard and its actions bit for bit.  Agent i keeps a density of its own, grids[b][i][ix * side + iy].
// Per call: when the targets moved, every grid is pushed through the motion model (belief.h's scatter), agent i's evade test seeing
// only the agents in heard[i], the link mask of the PREVIOUS call, at their prev positions; every grid is capped and swept by its OWN
// agent's disc (S_i); M_i = min over the agents linked NOW of S_j, cell by cell, is written back; prev and heard are replaced; the
// agents decide in index order on M_i less the footprints that the linked agents before them have claimed (local.h's choose loop).
//
// Layout: one workgroup of 256 threads per env.  Opening: lane i < n quantises agent i, reads prev[i] and heard[i] into LDS and stores
// the new prev[i] | barrier | lane i < n forms adj[i] (local.h's test) and stores it as the new heard[i] | barrier.  Then eight
// ROUNDS, one per possible agent, through ONE 16 KB accumulator acc[64 * 64]: zero acc | barrier | scatter D_j from global memory
// into acc | barrier | cap, sweep j's own disc, store S_j over D_j in global memory | barrier.  A round does its work only if moved
// and j < n, and passes its three barriers whatever the arguments: no barrier of this kernel stands inside a branch on tid, side,
// moved or the data, and the only one inside a loop over n is the choose loop's, which is local.h's (n is a launch argument, the same
// in every thread).  Then the merge pass of local.h: a thread owns a cell (four on the 16-byte path) of ALL n grids, loads them --
// with moved = 0 it applies bel_update's clamp and the own sweep here, in registers: no accumulator, nothing zeroed, nothing
// scattered -- and stores the n minima | barrier | choose, reading M_i from global memory with the claims in registers.
//
// Resources (compiler's report, profiles/kernel_resources.txt, k_local_belief_actions): 65 VGPRs, 5 SGPRs spilled to lanes, no VGPR
// spills, no scratch, 16960 bytes of LDS.  Registers bound the occupancy: 65 VGPRs are allocated as 72, which allows 7 waves per
// SIMD, seven workgroups per CU, where the 16.6 KB of LDS would allow nine of 160 KB (k_belief_actions: 41 VGPRs, eight;
// k_local_coverage_actions: 90 VGPRs, five).  The merge holds four cells of eight grids (32 VGPRs) whatever n is, as in local.h.
//
// What could go wrong in this shape, and why it does not:
//   acc is reused while a slow wave still reads it   the cap pass of round j reads acc; round j + 1 zeroes it.  The third barrier of a
//                                         round stands between: no thread zeroes before every thread has finished its cap pass.
//   S_j is stored over D_j while another thread still scatters from D_j   the scatter of round j reads D_j from global memory, the cap
//                                         pass stores S_j there.  The second barrier of the round stands between: every source cell
//                                         of D_j has been read (a load's value is in a register before its atomicAdd can issue) by
//                                         the time any thread stores.  Round j touches grid j only: D_k, k > j, is still untouched
//                                         when its round comes, and S_k, k < j, is not read before the merge.
//   the merge reads an S_j that another wave stored   __syncthreads() stands between (the third barrier of the last round): a
//                                         workgroup-scope release (every store of the wave has left: vmcnt(0)), the barrier, and a
//                                         workgroup-scope acquire; the waves of a workgroup share one CU and its write-through L1, as
//                                         local.h says of its choose stage.  The same holds for the choose stage here.
//   the merge is in place                 as in local.h: a thread loads cell c of all n grids into registers (the unrolled loop over j)
//                                         and only then stores the n minima; no other thread touches c of this env.
//   2^31 per accumulator word and per score   a source cell is read as clamp(cell, 0, CAP = 2^19) and its pieces sum to at most its
//                                         value (belief.h), so a full-CAP map of 2^12 cells sums to at most 2^31 wherever it lands: acc
//                                         is unsigned and is widened as unsigned in the cap pass.  A merged cell is at most CAP, a
//                                         footprint at most 2^12 cells: a score is an unsigned sum of at most 2^31.
//   the minimum starts at CAP + 1         not local.h's 65537: a density cell can hold up to CAP, and the start must lie above every
//                                         cell so that an agent that is not heard does not enter the minimum.  adj[i] holds bit i, so
//                                         S_i always enters and the start value is never stored.
//   heard has garbage bits                it is read as (heard[i] & ((1 << n) - 1)) | (1 << i) when it is copied to LDS: a bit at or
//                                         above n can never select a px[] slot that was not written, and the own bit is always set.
//                                         The old masks are in LDS (first barrier) before the second phase overwrites heard[i]; lane i
//                                         alone reads and writes heard[i] and prev[i].
//   the link test wraps                   local.h's: the differences are widened to long long BEFORE they are squared.
//   side^2 < 256                          idle threads run no loop body and fall through to every barrier.
//   side 64 fills acc exactly             cells = 4096 = the array; every index is ci * side + cj with ci, cj clamped to 0..side - 1.
//   rows are unaligned at side 7          agent i's row of env b starts (b n + i) * 49 words behind grids_dev: the 16-byte path is taken
//                                         only when cells % 4 == 0 AND grids_dev is 16-byte aligned (vec4, decided by the entry point);
//                                         then every row of every agent is aligned.  acc is declared 16-byte aligned.
//   register arrays                       v[], cx[] and cy[] are indexed by unrolled loop counters only, so they stay in registers:
//                                         scratch 0.  The heading loop of the scatter stays rolled (#pragma unroll 1): unrolling it
//                                         halves the occupancy and is slower.
//   B * n * cells past 2^31               every global index is formed in size_t.
//   NaN or huge state floats, prev off the map   cov_quant clamps, prev is read clamped to +-2^15, as in belief.h.
struct LocalBeliefArgs {
    BeliefArgs b;      // b.c.grid: [B][n][side * side]; b.c.vec4: every row of every agent is a whole number of aligned 16-byte pieces
    int32_t *heard;    // [B][8]
    long long C2;      // (16 comm_range)^2, or -1: unlimited
};

// bel_scatter with the evade test restricted to the agents in `mask` (bel_scatter's signature takes no mask; everything else is its)
__device__ __forceinline__ void lbel_scatter(const BeliefArgs &a, unsigned *acc, const int *px, const int *py, unsigned mask, const int *ox,
                                             const int *fx, const int *oy, const int *fy, int ix, int iy, int g) {
    const unsigned d = (unsigned)min(max(g, 0), BEL_CAP);
    if (d == 0) return;
    const int side = a.c.side;
    if (a.mode == CS_MOTION_EVADE) {
        unsigned best = 0xffffffffu;
        int bex = 0, bey = 0;
        for (int i = 0; i < a.c.n; i++) {   // the nearest HEARD agent inside the radius, lowest index on ties
            if (!((mask >> i) & 1u)) continue;
            const int ex = 16 * ix + 8 - px[i], ey = 16 * iy + 8 - py[i];
            const unsigned d2 = (unsigned)abs(ex) * (unsigned)abs(ex) + (unsigned)abs(ey) * (unsigned)abs(ey);
            if (d2 <= a.sense2 && d2 < best) {
                best = d2;
                bex = ex;
                bey = ey;
            }
        }
        if (best != 0xffffffffu) {
            int top = bex * BEL_CQ[0] + bey * BEL_SQ[0], k = 0;
            for (int q = 1; q < BEL_HEADINGS; q++) {
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

__global__ __launch_bounds__(COV_THREADS) void k_local_belief_actions(LocalBeliefArgs la) {
    __shared__ __attribute__((aligned(16))) unsigned acc[CS_MAX_MAP * CS_MAX_MAP];
    __shared__ int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS], ah[CS_MAX_AGENTS], px[CS_MAX_AGENTS], py[CS_MAX_AGENTS];
    __shared__ unsigned was[CS_MAX_AGENTS], adj[CS_MAX_AGENTS];   // whom agent i heard at the previous call, and hears now
    __shared__ int ox[BEL_HEADINGS], fx[BEL_HEADINGS], oy[BEL_HEADINGS], fy[BEL_HEADINGS];
    __shared__ unsigned red[2][COV_WAVES][3];
    const BeliefArgs &a = la.b;
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int n = a.c.n, side = a.c.side, cells = side * side;
    const unsigned R2 = (unsigned)a.c.R * (unsigned)a.c.R;
    // 1. quantise: lane i owns agent i, reads its stored position and its old mask and stores the new position
    if (tid < n) {
        const float *s = a.c.state + b * (size_t)a.c.S + 4 * tid;
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
        int32_t *p = a.prev + (b * CS_MAX_AGENTS + tid) * 2;
        px[tid] = min(max(p[0], -32768), 32768);
        py[tid] = min(max(p[1], -32768), 32768);
        p[0] = X;
        p[1] = Y;
        was[tid] = ((unsigned)la.heard[b * CS_MAX_AGENTS + tid] & ((1u << n) - 1u)) | (1u << tid);
    }
    if (tid >= 64 && tid < 64 + BEL_HEADINGS) {   // (another wavefront than the agents')
        const int k = tid - 64;
        ox[k] = a.dx[k] >> 4;
        fx[k] = a.dx[k] & 15;
        oy[k] = a.dy[k] >> 4;
        fy[k] = a.dy[k] & 15;
    }
    __syncthreads();
    // 2. links: lane i forms the mask of those agent i hears now (local.h's test) and stores it for the next call
    if (tid < n) {
        unsigned m = 1u << tid;
        for (int j = 0; j < n; j++) {
            const long long dx = (long long)ax[tid] - (long long)ax[j], dy = (long long)ay[tid] - (long long)ay[j];
            if (la.C2 < 0 || dx * dx + dy * dy < la.C2) m |= 1u << j;
        }
        adj[tid] = m;
        la.heard[b * CS_MAX_AGENTS + tid] = (int32_t)m;
    }
    __syncthreads();
    int32_t *G = a.c.grid + b * (size_t)n * (size_t)cells;
    BeliefArgs one = a;   // bel_update with one agent: the clamp and the sweep of that agent's disc alone
    one.c.n = 1;
    // 3. predict, agent after agent through the one accumulator: D_j -> S_j, in place in global memory
    for (int j = 0; j < CS_MAX_AGENTS; j++) {
        const bool on = a.moved && j < n;   // (the same in every thread; the barriers below are passed either way)
        int32_t *Gj = G + (size_t)(on ? j : 0) * cells;
        if (on)
            for (int idx = tid; idx < cells; idx += COV_THREADS) acc[idx] = 0u;
        __syncthreads();
        if (on) {
            const unsigned mask = was[j];
            if (a.c.vec4) {
                for (int q = tid; q < cells / 4; q += COV_THREADS) {
                    const int4 v = reinterpret_cast<const int4 *>(Gj)[q];
                    int ix = (4 * q) / side, iy = 4 * q - ix * side;
                    const int *e = reinterpret_cast<const int *>(&v);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        lbel_scatter(a, acc, px, py, mask, ox, fx, oy, fy, ix, iy, e[k]);
                        if (++iy == side) {
                            iy = 0;
                            ix++;
                        }
                    }
                }
            } else {
                for (int idx = tid; idx < cells; idx += COV_THREADS) {
                    const int ix = idx / side, iy = idx - ix * side;
                    lbel_scatter(a, acc, px, py, mask, ox, fx, oy, fy, ix, iy, Gj[idx]);
                }
            }
        }
        __syncthreads();
        if (on) {
            if (a.c.vec4) {
                for (int q = tid; q < cells / 4; q += COV_THREADS) {
                    int4 v = reinterpret_cast<const int4 *>(acc)[q];
                    int ix = (4 * q) / side, iy = 4 * q - ix * side;
                    int *e = reinterpret_cast<int *>(&v);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        e[k] = bel_update(one, ax + j, ay + j, R2, ix, iy, (long long)(unsigned)e[k]);   // (an accumulator word is unsigned)
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
                    Gj[idx] = bel_update(one, ax + j, ay + j, R2, ix, iy, (long long)acc[idx]);
                }
            }
        }
        __syncthreads();
    }
    // 4. merge (local.h's pass): a thread holds its cells of all n grids before it stores any of them; when nothing moved the
    // clamp and the own sweep happen here, on the way in
    const bool raw = !a.moved;
    if (a.c.vec4) {
        for (int q = tid; q < cells / 4; q += COV_THREADS) {
            const int ix0 = (4 * q) / side, iy0 = 4 * q - ix0 * side;
            int4 v[CS_MAX_AGENTS];
#pragma unroll
            for (int j = 0; j < CS_MAX_AGENTS; j++) {
                v[j] = make_int4(0, 0, 0, 0);
                if (j < n) {
                    v[j] = reinterpret_cast<const int4 *>(G + (size_t)j * cells)[q];
                    if (raw) {
                        int *e = reinterpret_cast<int *>(&v[j]);
                        int ix = ix0, iy = iy0;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            e[k] = bel_update(one, ax + j, ay + j, R2, ix, iy, (long long)e[k]);
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
                int4 r = make_int4(BEL_CAP + 1, BEL_CAP + 1, BEL_CAP + 1, BEL_CAP + 1);
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
                    if (raw) v[j] = bel_update(one, ax + j, ay + j, R2, ix, iy, (long long)v[j]);
                }
            }
            for (int i = 0; i < n; i++) {
                const unsigned m = adj[i];
                int r = BEL_CAP + 1;
#pragma unroll
                for (int j = 0; j < CS_MAX_AGENTS; j++)
                    if ((m >> j) & 1u) r = min(r, v[j]);
                G[(size_t)i * cells + idx] = r;
            }
        }
    }
    __syncthreads();   // the choose stage reads cells that other threads of this workgroup have just stored
    // 5. choose, agent by agent, on M_i less the claims agent i has heard: local.h's loop
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
            cov_point(a.c, X, Y, h, act, qx, qy);
            const CovBox box = cov_box(qx, qy, a.c.R, side);
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
            if ((tid & 63) == 0) part[tid >> 6][act] = sum[act];
        }
        __syncthreads();
        unsigned sc[3] = {0u, 0u, 0u};
        for (int w = 0; w < COV_WAVES; w++)
            for (int act = 0; act < 3; act++) sc[act] += part[w][act];
        int best = 0;
        if (sc[1] > sc[0]) best = 1;
        if (sc[2] > sc[best]) best = 2;
        if (tid == 0) a.c.actions[b * (size_t)n + i] = best;
        int qx, qy;
        cov_point(a.c, X, Y, h, best, qx, qy);
#pragma unroll
        for (int j = 0; j < CS_MAX_AGENTS; j++)
            if (j == i) {
                cx[j] = qx;
                cy[j] = qy;
            }
    }
}
