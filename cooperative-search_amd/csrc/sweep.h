// cooperative-search_amd/csrc/sweep.h -- cs_sweep_episodes: swept-area accounting of recorded episodes, one launch per batch
// (included by episodes.hip inside its namespace, after coverage.h whose quantisation it shares).
//
// The three outputs are DEFINED by sweep.sweep_episodes_torch (stock torch ops); this kernel reproduces them element for
// element.  Only the quantisation of an agent's position is floating point (cov_quant: each operation rounded once); the sweep
// test is coverage.h's: the centre (16 ix + 8, 16 iy + 8) of a cell lies within R = 16 view_range of an agent.  |position| <=
// 2^15 and a centre <= 2^10, so a squared distance is below 2^32 (uint32), as argued there.
//
// Layout: one workgroup of 256 threads per episode.  Thread `tid` owns the cells tid + 256 k, k < 16 (side <= 64): their `first`
// lives in registers for the whole episode and is written once at the end.  The rows are taken in chunks of SWEEP_CHUNK: the
// block quantises the chunk's (row, agent) positions into LDS (rows at or past the episode's count are never read), and after
// one barrier every wavefront walks the chunk's rows on its own -- each row's two counts are ballots summed per wavefront and
// stored in that wavefront's own LDS column, so nothing is accumulated across chunks and nothing needs clearing.  A second
// barrier ends the chunk: only then are the columns summed and written out (zeros for the rows past the count), and only
// then may the next chunk's positions overwrite the buffer a slower wavefront could still have been reading.  No atomics.
constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_WAVES = SWEEP_THREADS / 64;
constexpr int SWEEP_CHUNK = 64;                                                  // rows per chunk
constexpr int SWEEP_OWN = (CS_MAX_MAP * CS_MAX_MAP + SWEEP_THREADS - 1) / SWEEP_THREADS;   // 16 cells per thread at most

struct SweepArgs {
    const float *states;     // [E][T1][S]
    const int32_t *counts;   // [E]
    int32_t *first;          // [E][side * side]
    int32_t *new_cells;      // [E][T1]
    int32_t *seen_cells;     // [E][T1]
    int n, side, S, T1, R;   // R = 16 view_range (sub-units)
};

__global__ __launch_bounds__(SWEEP_THREADS) void k_sweep_episodes(SweepArgs a) {
    __shared__ int2 pos[SWEEP_CHUNK][CS_MAX_AGENTS];          // quantised (X, Y) of a chunk's rows
    __shared__ int cnt_new[SWEEP_CHUNK][SWEEP_WAVES], cnt_seen[SWEEP_CHUNK][SWEEP_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t e = blockIdx.x;
    const int side = a.side, cells = side * side, n = a.n, T1 = a.T1;
    const int own = (cells + SWEEP_THREADS - 1) / SWEEP_THREADS;   // 1..SWEEP_OWN, the same for every thread
    const unsigned R2 = (unsigned)a.R * (unsigned)a.R;
    const float half = (float)side / 2.0f;
    const int count = min(max(a.counts[e], 0), T1);
    const float *rows = a.states + e * (size_t)T1 * (size_t)a.S;

    int cx[SWEEP_OWN], cy[SWEEP_OWN], first[SWEEP_OWN];   // fully unrolled below: registers
#pragma unroll
    for (int k = 0; k < SWEEP_OWN; k++) {
        const int idx = min(tid + SWEEP_THREADS * k, cells - 1);   // (a cell past the map is masked out below)
        const int ix = idx / side;
        cx[k] = 16 * ix + 8;
        cy[k] = 16 * (idx - ix * side) + 8;
        first[k] = -1;
    }

    for (int t0 = 0; t0 < T1; t0 += SWEEP_CHUNK) {
        const int len = min(SWEEP_CHUNK, T1 - t0);           // rows of this chunk
        const int valid = min(max(count - t0, 0), len);      // of which the episode really has
        for (int q = tid; q < valid * n; q += SWEEP_THREADS) {
            const int r = q / n, i = q - r * n;
            const float *s = rows + (size_t)(t0 + r) * (size_t)a.S + 4 * i;
            pos[r][i] = make_int2(cov_quant((s[0] * half + half) * 16.0f, COV_POS_LIM), cov_quant((s[1] * half + half) * 16.0f, COV_POS_LIM));
        }
        __syncthreads();
        for (int r = 0; r < valid; r++) {
            unsigned seen = 0;   // bit k: cell k of this thread is swept at this row
            for (int i = 0; i < n; i++) {
                const int2 p = pos[r][i];
#pragma unroll
                for (int k = 0; k < SWEEP_OWN; k++)
                    if (k < own) {
                        const unsigned adx = (unsigned)abs(cx[k] - p.x), ady = (unsigned)abs(cy[k] - p.y);
                        seen |= (adx * adx + ady * ady <= R2 ? 1u : 0u) << k;
                    }
            }
            int ns = 0, nn = 0;
#pragma unroll
            for (int k = 0; k < SWEEP_OWN; k++)
                if (k < own) {
                    const bool s = ((seen >> k) & 1u) != 0 && tid + SWEEP_THREADS * k < cells;
                    const bool fresh = s && first[k] < 0;
                    if (fresh) first[k] = t0 + r;
                    ns += __popcll(__ballot(s));
                    nn += __popcll(__ballot(fresh));
                }
            if (lane == 0) {
                cnt_seen[r][wave] = ns;
                cnt_new[r][wave] = nn;
            }
        }
        __syncthreads();
        if (tid < len) {
            int ns = 0, nn = 0;
            if (tid < valid)
                for (int w = 0; w < SWEEP_WAVES; w++) {
                    ns += cnt_seen[tid][w];
                    nn += cnt_new[tid][w];
                }
            a.seen_cells[e * (size_t)T1 + t0 + tid] = ns;
            a.new_cells[e * (size_t)T1 + t0 + tid] = nn;
        }
        // (the next chunk's staging writes pos, which every wavefront has finished reading: they all passed the barrier above;
        // its row loop writes the counters only after the next barrier, which this thread reaches after the reads above)
    }
#pragma unroll
    for (int k = 0; k < SWEEP_OWN; k++)
        if (k < own && tid + SWEEP_THREADS * k < cells) a.first[e * (size_t)cells + tid + SWEEP_THREADS * k] = first[k];
}
