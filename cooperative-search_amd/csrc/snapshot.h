// cooperative-search_amd/csrc/snapshot.h -- cs_snapshot / cs_restore: an env's logical state as one fixed-size record, and back
// (included by coopsearch.hip inside its namespace).
//
// What a record must hide is everything the state blob holds that depends on HOW the env got where it is: how much of the
// MT19937 row the last kernel had twisted ahead of the cursor (cs_layout.ahead_off), the mirror words 624..655, the hit
// tape, the map sweep's pending bits in CS_H_FLAGS and the job records.  A record therefore carries the row in
// cs_mt_canonical's form and none of the derived data; cs_restore rebuilds the derived data for the row it writes -- the
// mirror, ahead = 624 and a hit tape made from THESE words, so that no stored tape of the env's previous stream survives
// (tape_finish checks threshold and word counts, not the stream's identity).
//
// Record (bytes; every section 16-byte aligned, the record a multiple of 16 bytes):
//      0  uint32 [16]     magic, format version, variant, n_agents, n_targets, map_size, 0 ...
//     64  uint32 [16]     the env's CS_H_* words, CS_H_FLAGS bits 1-2 clear, words 12..15 zero
//    128  double [16][2]  targets (rows >= n_targets zero)
//    384  double [8][4]   agents (x, y, yaw, 0; rows >= n_agents zero)
//    640  uint32 [624]    MT19937 row, canonical; the cursor is CS_H_MT_POS above
//   3136  float  [map^2]  flight only: the probability map
constexpr unsigned SNAP_MAGIC = 0x50534343u;   // "CCSP"
constexpr unsigned SNAP_VERSION = 1;
constexpr int SNAP_OFF_HDR = 64, SNAP_OFF_TGT = 128, SNAP_OFF_AGENT = 384, SNAP_OFF_MT = 640, SNAP_OFF_MAP = SNAP_OFF_MT + 4 * MT_N;
static_assert(SNAP_OFF_MAP % 16 == 0, "the map section of a record must be 16-byte aligned");

struct SnapArgs {
    const long long *src;   // cs_snapshot: env of record i; cs_restore: record of entry i (NULL: i)
    const long long *dst;   // cs_restore: env of entry i (NULL: i)
    long long count, n_records;
    size_t rec_bytes;
    int n_agents;
};

__device__ __forceinline__ unsigned snap_head_word(const DevParams &p, int n_agents, int k) {   // (selects, not a table: no scratch)
    return k == 0 ? SNAP_MAGIC : k == 1 ? SNAP_VERSION : k == 2 ? (unsigned)p.variant : k == 3 ? (unsigned)n_agents
         : k == 4 ? (unsigned)p.n_targets : k == 5 ? (unsigned)p.map_size : 0u;
}

// One wavefront per record: env -> record, the state is only read.  An env index out of range gives an all-zero record
// (which cs_restore refuses: no magic).
__global__ __launch_bounds__(64) void k_snapshot(DevParams p, SnapArgs a, unsigned char *out) {
    __shared__ unsigned row[MT_N];
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    unsigned char *rec = out + (size_t)i * a.rec_bytes;
    uint4 *rec4 = reinterpret_cast<uint4 *>(rec);
    unsigned *rw = reinterpret_cast<unsigned *>(rec);
    const long long b = a.src ? a.src[i] : i;
    if (b < 0 || b >= p.B) {   // block-uniform
        for (size_t k = lane; k < a.rec_bytes / 16; k += 64) rec4[k] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const int *h = p.hdr + (size_t)b * CS_H_WORDS;
    if (lane < 16) {
        rw[lane] = snap_head_word(p, a.n_agents, lane);
    } else if (lane < 32) {
        const int k = lane - 16;
        unsigned v = k < 12 ? (unsigned)h[k] : 0u;
        if (k == CS_H_FLAGS) v &= ~(unsigned)(FLAG_DIRTY | FLAG_RESET_PASS);
        rw[lane] = v;
    } else if (lane < 48) {
        const int j = lane - 32;   // target j: one (x, y) pair
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (j < p.n_targets) v = reinterpret_cast<const uint4 *>(p.tgt + (size_t)b * G * 2)[j];
        rec4[SNAP_OFF_TGT / 16 + j] = v;
    } else {
        const int j = lane - 48;   // half j & 1 of agent j >> 1: (x, y) | (yaw, spare)
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((j >> 1) < a.n_agents) {
            v = reinterpret_cast<const uint4 *>(p.agent + (size_t)b * CS_MAX_AGENTS * 4)[j];
            if (j & 1) v.z = v.w = 0u;
        }
        rec4[SNAP_OFF_AGENT / 16 + j] = v;
    }
    // the row in canonical form, as k_mt_canonical makes it
    const unsigned *m = p.mt + (size_t)b * MT_STRIDE;
    for (int k = lane; k < MT_N; k += 64) row[k] = m[k];
    __syncthreads();
    int pos = h[CS_H_MT_POS], ahead = p.ahead[b];
    pos = (unsigned)pos < (unsigned)MT_N ? pos : 0;
    ahead = ahead < 0 ? 0 : ahead;
    while (ahead < MT_N) {   // block-uniform; 64 <= 227 words per round are independent of each other
        const int r = MT_N - ahead < 64 ? MT_N - ahead : 64;
        const int j = wrap624(wrap624(pos + ahead) + lane);
        unsigned nw = 0;
        if (lane < r) nw = mt_mix(row[j], row[wrap624(j + 1)], row[wrap624(j + MT_M)]);
        __syncthreads();
        if (lane < r) row[j] = nw;
        __syncthreads();
        ahead += r;
    }
    for (int k = lane; k < MT_N; k += 64) rw[SNAP_OFF_MT / 4 + k] = row[k];
    if (p.variant == 1) {
        const float4 *src = reinterpret_cast<const float4 *>(p.prob + (size_t)b * p.cells);
        float4 *dst = reinterpret_cast<float4 *>(rec + SNAP_OFF_MAP);
        for (int k = lane; k < p.cells / 4; k += 64) dst[k] = src[k];
    }
}

// What is wrong with entry i of a cs_restore call: 0 nothing, 1 record index out of range, 2 env index out of range, 3 the
// record is not one of this configuration -- its 16 identification words, its cursor, or its unused header words 12..15 --
// (value: the index's low 32 bits, or the first offending uint32 word of the record).
__device__ __forceinline__ int snap_verdict(const DevParams &p, const SnapArgs &a, const unsigned char *records, long long i,
                                            long long &s, long long &d, int &value) {
    s = a.src ? a.src[i] : i;
    d = a.dst ? a.dst[i] : i;
    if (s < 0 || s >= a.n_records) { value = (int)s; return 1; }
    if (d < 0 || d >= p.B) { value = (int)d; return 2; }
    const unsigned *rw = reinterpret_cast<const unsigned *>(records + (size_t)s * a.rec_bytes);
    for (int k = 0; k < 16; k++)
        if (rw[k] != snap_head_word(p, a.n_agents, k)) { value = k; return 3; }
    const unsigned pos = rw[16 + CS_H_MT_POS];
    if (pos >= (unsigned)MT_N || (pos & 1u)) { value = 16 + CS_H_MT_POS; return 3; }   // the cursor indexes the row: never trusted
    for (int k = 12; k < 16; k++)
        if (rw[16 + k] != 0u) { value = 16 + k; return 3; }   // the unused header words of a record are zero
    // (the other CS_H_* words, targets, agents, row and map are the env's state itself: taken as they are)
    return 0;
}

// status = {1, kind, entry, value} of the FIRST refused entry of the call, {0, -1, -1, 0} when there is none.  One workgroup.
__global__ __launch_bounds__(1024) void k_restore_check(DevParams p, SnapArgs a, const unsigned char *records, int32_t *status) {
    __shared__ unsigned long long first;
    if (threadIdx.x == 0) first = ~0ull;
    __syncthreads();
    long long s, d;
    int value;
    for (long long i = threadIdx.x; i < a.count; i += 1024)
        if (snap_verdict(p, a, records, i, s, d, value)) {
            atomicMin(&first, (unsigned long long)i);
            break;   // this thread's later entries are all higher
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (first == ~0ull) {
            status[0] = 0; status[1] = -1; status[2] = -1; status[3] = 0;
        } else {
            const int kind = snap_verdict(p, a, records, (long long)first, s, d, value);
            status[0] = 1; status[1] = kind; status[2] = (int32_t)first; status[3] = value;
        }
    }
}

// One wavefront per entry: record src[i] -> env dst[i], every derived piece rebuilt for the row written.  A refused entry
// leaves its env untouched.
__global__ __launch_bounds__(64) void k_restore(DevParams p, SnapArgs a, const unsigned char *records) {
    __shared__ unsigned row[MT_N];
    const int lane = threadIdx.x;
    long long s, d;
    int value;
    if (snap_verdict(p, a, records, (long long)blockIdx.x, s, d, value)) return;   // block-uniform
    const unsigned char *rec = records + (size_t)s * a.rec_bytes;
    const uint4 *rec4 = reinterpret_cast<const uint4 *>(rec);
    const unsigned *rw = reinterpret_cast<const unsigned *>(rec);
    const int pos = (int)rw[16 + CS_H_MT_POS];
    if (lane < 16) {
        unsigned v = rw[16 + lane];
        if (lane == CS_H_FLAGS) v &= ~(unsigned)(FLAG_DIRTY | FLAG_RESET_PASS);   // nothing pending for the map sweep
        p.hdr[(size_t)d * CS_H_WORDS + lane] = (int)v;
    } else if (lane < 32) {
        reinterpret_cast<uint4 *>(p.tgt + (size_t)d * G * 2)[lane - 16] = rec4[SNAP_OFF_TGT / 16 + lane - 16];
    } else if (lane < 48) {
        reinterpret_cast<uint4 *>(p.agent + (size_t)d * CS_MAX_AGENTS * 4)[lane - 32] = rec4[SNAP_OFF_AGENT / 16 + lane - 32];
    } else if (lane == 48) {
        p.ahead[d] = MT_N;   // canonical: every word of the row is twisted ahead of the cursor
    } else if (lane < 51 && p.variant == 1) {
        *reinterpret_cast<int4 *>(job_ptr(p, lane - 49, (int)d)) = make_int4(0, 0, 0, 0);   // no pending pass in either record
    }
    unsigned *m = p.mt + (size_t)d * MT_STRIDE;
    for (int k = lane; k < MT_N; k += 64) {
        const unsigned w = rw[SNAP_OFF_MT / 4 + k];
        row[k] = w;
        m[k] = w;
        if (k < MT_PAD) m[MT_N + k] = w;
    }
    __syncthreads();
    // the hit tape of THIS row (k_mt_advance's): whatever tape the env's previous stream left is gone
    unsigned *tp = p.tape + (size_t)d * TAPE_STRIDE;
    unsigned long long bm[TAPE_DW / 2];
    row_hits_all(p, row, pos, lane, bm);
    if (lane == 0) {
#pragma unroll
        for (int it = 0; it < TAPE_DW / 2; it++)
            *reinterpret_cast<U2 *>(tp + 2 * it) = U2{(unsigned)(bm[it] & 0xffffffffull), (unsigned)(bm[it] >> 32)};
        *reinterpret_cast<U2 *>(tp + 10) = U2{rw[16 + CS_H_WORDS_LO], rw[16 + CS_H_WORDS_HI]};
        *reinterpret_cast<U2 *>(tp + 12) = U2{(unsigned)(p.detect_K & 0xffffffffull), (unsigned)(p.detect_K >> 32)};
    }
    if (p.variant == 1) {
        const float4 *src = reinterpret_cast<const float4 *>(rec + SNAP_OFF_MAP);
        float4 *dst = reinterpret_cast<float4 *>(p.prob + (size_t)d * p.cells);
        for (int k = lane; k < p.cells / 4; k += 64) dst[k] = src[k];
    }
}
