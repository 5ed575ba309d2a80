// cooperative-search_amd/csrc/motion.h -- k_move_targets: one move of every unfound target of every live env (cs_move_targets).
//
// Included by coopsearch.hip inside its anonymous namespace.  The move is DEFINED by motion.move_targets_torch (stock torch
// ops, fp64, every operation rounded once: no sqrt, no division, no transcendental); this kernel equals it bit for bit, so the
// library's -ffp-contract=off is part of the contract here too.  DESIGN.md section 19 has the text.
//
// Layout: the 16-lane step code's -- 16 lanes per env, lane t owns target slot t: four envs per wavefront, 16 per block of 256
// threads.  A lane reads four header words and the agents of its env (the same addresses across its 16 lanes: one request
// each), its own target, and stores 16 bytes if its target moves.  No atomics, no LDS, no host synchronisation; tgt is the only
// array written.  Per env about 64 + 32 n + 256 bytes are read and at most 256 written: the launch is latency-bound.
#pragma once

constexpr int MOT_HEADINGS = 16;
constexpr int MOT_BLOCK = 256;           // 16 envs

// cos and sin of 2 pi k / 16, k = 0..15, evaluated once in Python doubles: the literals of motion.py (CX, CY), which
// tests/test_motion_cpu.py holds equal to these
__constant__ double MOT_CX[MOT_HEADINGS] = {0x1.0000000000000p+0, 0x1.d906bcf328d46p-1, 0x1.6a09e667f3bcdp-1, 0x1.87de2a6aea964p-2,
                                            0x1.1a62633145c07p-54, -0x1.87de2a6aea962p-2, -0x1.6a09e667f3bccp-1, -0x1.d906bcf328d46p-1,
                                            -0x1.0000000000000p+0, -0x1.d906bcf328d47p-1, -0x1.6a09e667f3bcep-1, -0x1.87de2a6aea96dp-2,
                                            -0x1.a79394c9e8a0ap-53, 0x1.87de2a6aea967p-2, 0x1.6a09e667f3bcbp-1, 0x1.d906bcf328d44p-1};
__constant__ double MOT_CY[MOT_HEADINGS] = {0x0.0p+0, 0x1.87de2a6aea963p-2, 0x1.6a09e667f3bccp-1, 0x1.d906bcf328d46p-1,
                                            0x1.0000000000000p+0, 0x1.d906bcf328d46p-1, 0x1.6a09e667f3bcdp-1, 0x1.87de2a6aea965p-2,
                                            0x1.1a62633145c07p-53, -0x1.87de2a6aea961p-2, -0x1.6a09e667f3bccp-1, -0x1.d906bcf328d44p-1,
                                            -0x1.0000000000000p+0, -0x1.d906bcf328d45p-1, -0x1.6a09e667f3bcep-1, -0x1.87de2a6aea96ep-2};

struct MotionArgs {
    double *tgt;           // [B][16][2], in / out
    const double *agent;   // [B][8][4]
    const int *hdr;        // [B][16]
    long long B, env_offset;
    int n_agents, n_targets, time_limit, mode;
    unsigned persist, seed;
    double speed, sense2, L;   // sense2 = sense * sense, L = map_size
};

__device__ __forceinline__ unsigned mot_fmix(unsigned x) {   // the 32-bit finaliser of MurmurHash3
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ double mot_clamp(double v, double L) {   // min(max(v, 0), L) as two selects: a NaN stays a NaN
    v = v < 0.0 ? 0.0 : v;
    return v > L ? L : v;
}

__global__ __launch_bounds__(MOT_BLOCK) void k_move_targets(MotionArgs a) {
    const long long b = (long long)blockIdx.x * (MOT_BLOCK / 16) + (threadIdx.x >> 4);
    const int j = threadIdx.x & 15;
    if (b >= a.B || j >= a.n_targets) return;
    const int *h = a.hdr + b * CS_H_WORDS;
    const int ts = h[CS_H_TIME_STEP];
    // live on entry (what cs_step with CS_FREEZE_DONE steps) and target j not found yet: everything else keeps its bits
    if ((h[CS_H_FLAGS] & FLAG_WIN) || ts >= a.time_limit || (((unsigned)h[CS_H_FOUND] >> j) & 1u)) return;
    double *t = a.tgt + (b * 16 + j) * 2;
    const double2 p = *reinterpret_cast<const double2 *>(t);

    const unsigned long long g = (unsigned long long)(a.env_offset + b);   // the global env index
    const unsigned words[5] = {(unsigned)g, (unsigned)(g >> 32), (unsigned)h[CS_H_EPISODES], (unsigned)ts / a.persist, (unsigned)j};
    unsigned key = a.seed;
#pragma unroll
    for (int w = 0; w < 5; w++) key = mot_fmix(key ^ words[w]) + 0x9E3779B9u;
    int k = (int)(key >> 28);

    if (a.mode == CS_MOTION_EVADE) {
        const double *ag = a.agent + b * (CS_MAX_AGENTS * 4);
        double best = INFINITY, bdx = 0.0, bdy = 0.0;
        bool seen = false;
        for (int i = 0; i < a.n_agents; i++) {   // the nearest agent inside the radius, lowest index on ties
            const double dx = p.x - ag[4 * i], dy = p.y - ag[4 * i + 1];
            const double d2 = dx * dx + dy * dy;
            if (d2 <= a.sense2 && d2 < best) {
                best = d2, bdx = dx, bdy = dy;
                seen = true;
            }
        }
        if (seen) {   // the heading that leads away fastest, lowest index on ties
            double top = bdx * MOT_CX[0] + bdy * MOT_CY[0];
            k = 0;
#pragma unroll
            for (int q = 1; q < MOT_HEADINGS; q++) {
                const double s = bdx * MOT_CX[q] + bdy * MOT_CY[q];
                if (s > top) top = s, k = q;
            }
        }
    }
    double2 o;
    o.x = mot_clamp(p.x + a.speed * MOT_CX[k], a.L);
    o.y = mot_clamp(p.y + a.speed * MOT_CY[k], a.L);
    *reinterpret_cast<double2 *>(t) = o;
}
