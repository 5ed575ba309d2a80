// cooperative-search_amd/csrc/episodes.hip -- episode batch assembly for the collector / replay buffer (gfx950).
//
// "Next" rows f1 / f2 of SURVEY.md section 8(f).  The reference builds, per episode, eleven [T, ...] arrays with its
// padding rules (common/rollout.py:66-76 and 105-132: steps after termination are zero rows with padded = 1 and
// terminated = 1) and copies them into the replay ring (common/replay_buffer.py:41-61).  The batched collector's
// kernels leave step-major tables ([T+1][B][...] obs / state, [T][B][...] actions / reward / terminated); this file
// turns them into the episode-major, masked, float32 arrays in ONE pass, writing either a fresh [B][T][...] batch or
// straight into the ring slots of a DeviceReplayBuffer.  Pure data movement: HBM-bound.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>

#include <initializer_list>
#include <type_traits>

#include "coopsearch.h"

namespace {

struct EpisodeParams {
    int B, T, n, A, obs_w, state_w;
    const float *o_tab, *s_tab, *r_tab;
    const int64_t *u_tab;
    const uint8_t *term_tab;
    const int64_t *slot;   // destination episode slot of env b (null: b)
    cs_episode_out out;
};

// a step is real if its env had not terminated before it (the batched env freezes finished envs, so `terminated`
// stays 1 once set): real(t, b) = t == 0 || !terminated[t-1][b]
__device__ __forceinline__ bool step_is_real(const EpisodeParams &p, int t, int b) {
    return t == 0 || p.term_tab[(size_t)(t - 1) * p.B + b] == 0;
}

// rows: out[slot][t][:] = real ? tab[t + shift][b][:] : 0 for the wide keys (o, o_next, s, s_next).
// grid (B, T chunks); every thread moves VEC floats at a time along the row.
template <int VEC>
__global__ __launch_bounds__(256) void k_episode_rows(EpisodeParams p, int t_per_block) {
    const int b = blockIdx.x;
    const size_t slot = p.slot ? (size_t)p.slot[b] : (size_t)b;
    const int t0 = blockIdx.y * t_per_block, t1 = min(p.T, t0 + t_per_block);
    const int ow = p.n * p.obs_w, sw = p.state_w;
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const int nt = t1 - t0;
    const V zero = {};
    // (t, column) flattened over the block's threads: a 12-float obs row alone would keep 3 threads busy
    for (int i = threadIdx.x; i < nt * (ow / VEC); i += blockDim.x) {
        const int t = t0 + i / (ow / VEC), c = i % (ow / VEC);
        const bool real = step_is_real(p, t, b);
        const V *src0 = reinterpret_cast<const V *>(p.o_tab + ((size_t)t * p.B + b) * ow);
        const V *src1 = reinterpret_cast<const V *>(p.o_tab + ((size_t)(t + 1) * p.B + b) * ow);
        V v0 = zero, v1 = zero;   // (a select between a loaded value and a constant, not between two addresses)
        if (real) {
            v0 = src0[c];
            v1 = src1[c];
        }
        reinterpret_cast<V *>(p.out.o + (slot * p.T + t) * ow)[c] = v0;
        reinterpret_cast<V *>(p.out.o_next + (slot * p.T + t) * ow)[c] = v1;
    }
    // state rows: wavefront = time step, lane = column (no per-element division)
    for (int tt = threadIdx.x >> 6; tt < nt; tt += 4) {
        const int t = t0 + tt;
        const bool real = step_is_real(p, t, b);
        const float *src0 = p.s_tab + ((size_t)t * p.B + b) * sw, *src1 = p.s_tab + ((size_t)(t + 1) * p.B + b) * sw;
        float *d0 = p.out.s + (slot * p.T + t) * sw, *d1 = p.out.s_next + (slot * p.T + t) * sw;
        for (int c = threadIdx.x & 63; c < sw; c += 64) {
            d0[c] = real ? src0[c] : 0.0f;
            d1[c] = real ? src1[c] : 0.0f;
        }
    }
}

// the narrow keys, one thread per (b, t): u, r, avail_u, avail_u_next, u_onehot, padded, terminated
__global__ __launch_bounds__(256) void k_episode_small(EpisodeParams p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.B * p.T) return;
    const int b = (int)(i / p.T), t = (int)(i % p.T);
    const size_t slot = p.slot ? (size_t)p.slot[b] : (size_t)b, e = slot * p.T + t;
    const bool real = step_is_real(p, t, b);
    const float rf = real ? 1.0f : 0.0f;
    p.out.r[e] = real ? p.r_tab[(size_t)t * p.B + b] : 0.0f;
    p.out.padded[e] = 1.0f - rf;
    p.out.terminated[e] = real ? (p.term_tab[(size_t)t * p.B + b] ? 1.0f : 0.0f) : 1.0f;
    for (int a = 0; a < p.n; a++) {
        const int act = (int)p.u_tab[((size_t)t * p.B + b) * p.n + a];
        p.out.u[e * p.n + a] = real ? (float)act : 0.0f;
        for (int k = 0; k < p.A; k++) {
            const size_t j = (e * p.n + a) * p.A + k;
            p.out.avail_u[j] = rf;        // every action is always available (flight_env_easy.py:184-188)
            p.out.avail_u_next[j] = rf;
            p.out.u_onehot[j] = (real && k == act) ? 1.0f : 0.0f;
        }
    }
}

// ---- the map-once format (cs_store_episodes_compact) -------------------------------------------------
struct CompactParams {
    int B, T, n, cells, state_w;
    const float *map_tab, *s_tab, *r_tab;
    const int64_t *u_tab;
    const uint8_t *term_tab;
    const int64_t *slot;   // destination episode slot of env b (null: b)
    cs_compact_out out;
};

// row t of map / s_full holds data while t <= L (L = the episode's real steps): row 0 always, row t >= 1 iff step t - 1 was
// real (it is that step's o_next / s_next), i.e. iff the env had not terminated before step t - 1
__device__ __forceinline__ bool row_is_live(const CompactParams &p, int t, int b) {
    return t <= 1 || p.term_tab[(size_t)(t - 2) * p.B + b] == 0;
}

// rows: out[slot][t][:] = live ? tab[t][b][:] : 0 for t = 0..T, map and s_full in one pass.  grid (B, row chunks); every
// thread moves VEC floats of a map row at a time (a row is read once and written once: 2 x 10 KB, against the dense
// format's 2n reads and 2n writes of the same bytes).
template <int VEC>
__global__ __launch_bounds__(256) void k_compact_rows(CompactParams p, int t_per_block) {
    const int b = blockIdx.x;
    const size_t slot = p.slot ? (size_t)p.slot[b] : (size_t)b;
    const int rows = p.T + 1;
    const int t0 = blockIdx.y * t_per_block, t1 = min(rows, t0 + t_per_block);
    const int mw = p.cells, sw = p.state_w;
    using V = typename std::conditional<VEC == 4, float4, float>::type;
    const int nt = t1 - t0;
    const V zero = {};
    for (int i = threadIdx.x; i < nt * (mw / VEC); i += blockDim.x) {
        const int t = t0 + i / (mw / VEC), c = i % (mw / VEC);
        V v = zero;   // (a select between a loaded value and a constant, not between two addresses)
        if (row_is_live(p, t, b)) v = reinterpret_cast<const V *>(p.map_tab + ((size_t)t * p.B + b) * mw)[c];
        reinterpret_cast<V *>(p.out.map + (slot * rows + t) * mw)[c] = v;
    }
    // state rows: wavefront = row, lane = column (no per-element division)
    for (int tt = threadIdx.x >> 6; tt < nt; tt += 4) {
        const int t = t0 + tt;
        const bool live = row_is_live(p, t, b);
        const float *src = p.s_tab + ((size_t)t * p.B + b) * sw;
        float *dst = p.out.s_full + (slot * rows + t) * sw;
        for (int c = threadIdx.x & 63; c < sw; c += 64) dst[c] = live ? src[c] : 0.0f;
    }
}

// the narrow keys, one thread per (b, t): u, r, padded, terminated -- k_episode_small's values of the same names
__global__ __launch_bounds__(256) void k_compact_small(CompactParams p) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)p.B * p.T) return;
    const int b = (int)(i / p.T), t = (int)(i % p.T);
    const size_t slot = p.slot ? (size_t)p.slot[b] : (size_t)b, e = slot * p.T + t;
    const bool real = t == 0 || p.term_tab[(size_t)(t - 1) * p.B + b] == 0;
    p.out.r[e] = real ? p.r_tab[(size_t)t * p.B + b] : 0.0f;
    p.out.padded[e] = real ? 0.0f : 1.0f;
    p.out.terminated[e] = real ? (p.term_tab[(size_t)t * p.B + b] ? 1.0f : 0.0f) : 1.0f;
    for (int a = 0; a < p.n; a++) p.out.u[e * p.n + a] = real ? (float)(int)p.u_tab[((size_t)t * p.B + b) * p.n + a] : 0.0f;
}

#include "render.h"   // k_render_episodes: episode rows -> RGB frames (cs_render_episodes)
#include "coverage.h" // k_coverage_actions: the greedy coverage baseline (cs_coverage_actions)
#include "local.h"    // k_local_coverage_actions: the coverage baseline on n private grids under a communication range (cs_local_coverage_actions)
#include "sweep.h"    // k_sweep_episodes: swept-area accounting of recorded episodes (cs_sweep_episodes)
#include "belief.h"   // k_belief_actions: the target-density filter policy for moving targets (cs_belief_actions)
#include "local_belief.h" // k_local_belief_actions: the density filter on n private grids under a communication range (cs_local_belief_actions)
#include "plan.h"     // k_plan_actions: a receding-horizon sequence search over a base policy's grid (cs_plan_actions)
#include "local_plan.h" // k_local_plan_actions: the sequence search on n private grids under a communication range (cs_local_plan_actions)
#include "forecast.h" // k_belief_forecast, k_plan_forecast_actions: the density along the horizon and the search scored on it
#include "local_forecast.h" // k_local_belief_forecast, k_local_plan_forecast_actions: the same on n private grids under a communication range
#include "label.h"    // k_label_episodes: an expert of coverage.h / belief.h relabels a recorded batch in one launch (cs_label_episodes)
#include "gridobs.h"  // k_grid_features, k_feature_episodes: sixteen floats per agent from a policy's grid (cs_grid_features, cs_feature_episodes)
#include "localobs.h" // k_local_grid_features, k_local_feature_episodes: the same from each agent's private grid (cs_local_grid_features, cs_local_feature_episodes)

thread_local char g_eerr[160] = "";

// ---- host helpers of the grid family's entry points (cs_coverage_actions .. cs_feature_episodes) -------------------------------
// A check returns what is wrong (nullptr: nothing) and reads host integers only; `first` keeps the order in which they are listed.
int fail(const char *name, const char *bad) {
    snprintf(g_eerr, sizeof(g_eerr), "%s: %s", name, bad);
    return CS_E_CONFIG;
}

int launched(const char *name) {
    if (hipGetLastError() == hipSuccess) return CS_OK;
    snprintf(g_eerr, sizeof(g_eerr), "%s: kernel launch failed", name);
    return CS_E_LAUNCH;
}

const char *first(std::initializer_list<const char *> checks) {
    for (const char *bad : checks)
        if (bad) return bad;
    return nullptr;
}

const char *bad_agents(int n) { return n < 1 || n > CS_MAX_AGENTS ? "n_agents must be 1..8" : nullptr; }

const char *bad_team(int n, int side, int view_range) {
    return first({bad_agents(n), side < 1 || side > CS_MAX_MAP ? "side must be 1..64" : nullptr,
                  view_range < 0 || view_range > CS_MAX_MAP ? "view_range must be 0..64" : nullptr});
}

const char *bad_cover(int keep, int regrow, int lookahead, int side) {
    return first({keep < 0 || keep > 65536 ? "keep must be 0..65536" : nullptr, regrow < 1 || regrow > 16 ? "regrow must be 1..16" : nullptr,
                  lookahead < 0 || lookahead > side ? "lookahead must be 0..side" : nullptr});
}

const char *bad_plan(int depth, int stride, int discount) {
    return first({depth < 1 || depth > PLAN_MAX_DEPTH ? "depth must be 1..5" : nullptr,
                  stride < 1 || stride > PLAN_MAX_STRIDE ? "stride must be 1..8" : nullptr,
                  discount < 0 || discount > 256 ? "discount must be 0..256" : nullptr});
}

// the motion model's integers (`moved` is cs_belief_actions' alone: 0 elsewhere); its steps come last in every entry point: bad_steps
const char *bad_model(int mode, int moved, int sense16) {
    return first({mode != CS_MOTION_WALK && mode != CS_MOTION_EVADE ? "mode must be CS_MOTION_WALK or CS_MOTION_EVADE" : nullptr,
                  moved != 0 && moved != 1 ? "moved must be 0 or 1" : nullptr,
                  sense16 < 0 || sense16 > 32 * CS_MAX_MAP ? "sense16 must be 0..2048" : nullptr});
}

const char *bad_steps(const int32_t *dx, const int32_t *dy) {
    for (int k = 0; k < 16; k++)
        if (dx[k] < -16 * CS_MAX_MAP || dx[k] > 16 * CS_MAX_MAP || dy[k] < -16 * CS_MAX_MAP || dy[k] > 16 * CS_MAX_MAP)
            return "dx and dy must be -1024..1024";
    return nullptr;
}

const char *bad_width(int state_width, int n) { return state_width < 4 * n ? "state_width must be at least 4 n_agents" : nullptr; }
const char *bad_reserved(int reserved) { return reserved != 0 ? "reserved must be 0" : nullptr; }

// pointers to 4-byte and to 8-byte elements (NULL, where an entry point allows it, is aligned)
const char *misaligned(std::initializer_list<const void *> four, std::initializer_list<const void *> eight) {
    bool bad = false;
    for (const void *q : four) bad = bad || (uintptr_t)q % 4 != 0;
    for (const void *q : eight) bad = bad || (uintptr_t)q % 8 != 0;
    return bad ? "a pointer is not aligned to its element size" : nullptr;
}

int vec4_ok(int cells, const void *rows) { return (cells % 4 == 0 && (uintptr_t)rows % 16 == 0) ? 1 : 0; }

// view_range and lookahead in cells; `rows` is the grid whose alignment decides the vector path (label.h: grid is NULL, rows the output)
CoverageArgs cover_args(const float *state, int32_t *grid, int64_t *actions, int n, int side, int state_width, int view_range, int keep,
                        int regrow, int lookahead, const void *rows) {
    return CoverageArgs{state, grid, actions, n, side, state_width, 16 * view_range, keep, regrow, 16 * lookahead, vec4_ok(side * side, rows)};
}

BeliefArgs belief_args(const CoverageArgs &c, int mode, int sense16, const int32_t *dx, const int32_t *dy) {
    BeliefArgs a{};   // prev NULL, moved 0
    a.c = c;
    a.mode = mode;
    a.sense2 = (unsigned)sense16 * (unsigned)sense16;
    for (int k = 0; k < 16; k++) {
        a.dx[k] = dx[k];
        a.dy[k] = dy[k];
    }
    return a;
}

// cs_label_episodes and cs_feature_episodes: one params struct, one ladder (they differ in their pointers and in `prev_text`)
const char *bad_label(const cs_label_params *p, int E, int T, const void *prev_out, const char *prev_text,
                      std::initializer_list<const void *> four, std::initializer_list<const void *> eight) {
    return first({E < 1 || T < 1 ? "E and T must be >= 1" : nullptr,
                  p->expert != LABEL_COVERAGE && p->expert != LABEL_BELIEF ? "expert must be 0 (coverage) or 1 (belief)" : nullptr,
                  bad_team(p->n_agents, p->side, p->view_range), bad_cover(p->keep, p->regrow, p->lookahead, p->side),
                  bad_width(p->state_width, p->n_agents), bad_model(p->mode, 0, p->sense16), p->every < 1 ? "every must be >= 1" : nullptr,
                  p->moving != 0 && p->moving != 1 ? "moving must be 0 or 1" : nullptr, bad_reserved(p->reserved),
                  p->expert == LABEL_COVERAGE && prev_out ? prev_text : nullptr, misaligned(four, eight), bad_steps(p->dx, p->dy)});
}

LabelArgs label_args(const cs_label_params *p, const float *s, int T, const int32_t *lens, int64_t *labels, int32_t *grid_out,
                     int32_t *prev_out) {
    LabelArgs a{};
    a.b = belief_args(cover_args(s, nullptr, labels, p->n_agents, p->side, p->state_width, p->view_range, p->keep, p->regrow, p->lookahead,
                                 grid_out),
                      p->mode, p->sense16, p->dx, p->dy);
    a.lens = lens;
    a.grid_out = grid_out;
    a.prev_out = prev_out;
    a.T = T;
    a.expert = p->expert;
    a.every = p->every;
    a.moving = p->moving;
    a.svec = (p->state_width % 4 == 0 && (uintptr_t)s % 16 == 0) ? 1 : 0;
    a.lvec = (uintptr_t)labels % 16 == 0 ? 1 : 0;
    return a;
}

// cs_plan_actions (levels: the base policy's grid) and cs_plan_forecast_actions (forecast: the stack of cs_belief_forecast, staged in LDS)
int plan_launch(const char *name, bool forecast, const cs_plan_params *p, const float *state, int B, const int32_t *levels, int64_t *actions,
                int64_t *plans, int64_t *scores, void *stream) {
    if (!p || !state || !levels || !actions || !plans || !scores) return fail(name, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_plan(p->depth, p->stride, p->discount), bad_width(p->state_width, p->n_agents), bad_reserved(p->reserved),
                             misaligned({levels, state}, {actions, plans, scores})});
    if (bad) return fail(name, bad);
    const int cells = p->side * p->side, level_words = (cells + 3) & ~3;
    int seqs = 1;
    for (int d = 0; d < p->depth; d++) seqs *= 3;
    const PlanArgs a{state, levels, actions, plans, scores, p->n_agents, p->side, p->state_width, 16 * p->view_range,
                     p->depth, p->stride, p->discount, (3 * seqs - 3) / 2, seqs, vec4_ok(cells, levels)};
    if (!forecast) {
        hipLaunchKernelGGL(k_plan_actions, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
        return launched(name);
    }
    const size_t lds = fc_plan_lds_bytes(p->depth, level_words);
    // more than 64 KB of dynamic LDS (side 64 with depth 4 or 5) is granted only to a kernel that asked for it
    if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void *>(&k_plan_forecast_actions),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(g_eerr, sizeof(g_eerr), "%s: the device does not grant %zu bytes of LDS", name, lds);
        return CS_E_LAUNCH;
    }
    hipLaunchKernelGGL(k_plan_forecast_actions, dim3((unsigned)B), dim3(COV_THREADS), lds, (hipStream_t)stream, a, level_words);
    return launched(name);
}

}  // namespace

extern "C" {

int cs_store_episodes(int B, int T, int n_agents, int n_actions, int obs_w, int state_w, const float *o_tab_dev,
                      const float *s_tab_dev, const int64_t *u_tab_dev, const float *r_tab_dev, const uint8_t *term_tab_dev,
                      const int64_t *slot_dev, const cs_episode_out *out, void *stream) {
    if (B < 1 || T < 1 || n_agents < 1 || n_actions < 1 || obs_w < 1 || state_w < 1 || !o_tab_dev || !s_tab_dev || !u_tab_dev ||
        !r_tab_dev || !term_tab_dev || !out || !out->o || !out->u || !out->s || !out->r || !out->o_next || !out->s_next ||
        !out->avail_u || !out->avail_u_next || !out->u_onehot || !out->padded || !out->terminated) {
        snprintf(g_eerr, sizeof(g_eerr), "cs_store_episodes: bad argument");
        return CS_E_ARG;
    }
    EpisodeParams p{B, T, n_agents, n_actions, obs_w, state_w, o_tab_dev, s_tab_dev, r_tab_dev, u_tab_dev, term_tab_dev,
                    slot_dev, *out};
    hipStream_t s = (hipStream_t)stream;
    // enough blocks to fill the device even for small B: split T when B alone gives fewer than ~2048 blocks
    int chunks = 1;
    while (B * chunks < 2048 && chunks < T) chunks *= 2;
    const int t_per_block = (T + chunks - 1) / chunks;
    const dim3 grid(B, (T + t_per_block - 1) / t_per_block);
    const bool vec4 = (n_agents * obs_w) % 4 == 0 && ((uintptr_t)o_tab_dev % 16 == 0) && ((uintptr_t)out->o % 16 == 0) &&
                      ((uintptr_t)out->o_next % 16 == 0);
    if (vec4)
        hipLaunchKernelGGL(k_episode_rows<4>, grid, dim3(256), 0, s, p, t_per_block);
    else
        hipLaunchKernelGGL(k_episode_rows<1>, grid, dim3(256), 0, s, p, t_per_block);
    hipLaunchKernelGGL(k_episode_small, dim3((unsigned)(((size_t)B * T + 255) / 256)), dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) {
        snprintf(g_eerr, sizeof(g_eerr), "cs_store_episodes: kernel launch failed");
        return CS_E_LAUNCH;
    }
    return CS_OK;
}

int cs_store_episodes_compact(int B, int T, int n_agents, int cells, int state_w, const float *map_tab_dev,
                              const float *s_tab_dev, const int64_t *u_tab_dev, const float *r_tab_dev,
                              const uint8_t *term_tab_dev, const int64_t *slot_dev, const cs_compact_out *out, void *stream) {
    if (B < 1 || T < 1 || n_agents < 1 || cells < 1 || state_w < 1 || !map_tab_dev || !s_tab_dev || !u_tab_dev || !r_tab_dev ||
        !term_tab_dev || !out || !out->map || !out->s_full || !out->u || !out->r || !out->padded || !out->terminated) {
        snprintf(g_eerr, sizeof(g_eerr), "cs_store_episodes_compact: bad argument");
        return CS_E_ARG;
    }
    CompactParams p{B, T, n_agents, cells, state_w, map_tab_dev, s_tab_dev, r_tab_dev, u_tab_dev, term_tab_dev, slot_dev, *out};
    hipStream_t s = (hipStream_t)stream;
    int chunks = 1;   // as cs_store_episodes: split the rows when B alone gives fewer than ~2048 blocks
    while (B * chunks < 2048 && chunks < T + 1) chunks *= 2;
    const int t_per_block = (T + 1 + chunks - 1) / chunks;
    const dim3 grid(B, (T + 1 + t_per_block - 1) / t_per_block);
    const bool vec4 = cells % 4 == 0 && ((uintptr_t)map_tab_dev % 16 == 0) && ((uintptr_t)out->map % 16 == 0);
    if (vec4)
        hipLaunchKernelGGL(k_compact_rows<4>, grid, dim3(256), 0, s, p, t_per_block);
    else
        hipLaunchKernelGGL(k_compact_rows<1>, grid, dim3(256), 0, s, p, t_per_block);
    hipLaunchKernelGGL(k_compact_small, dim3((unsigned)(((size_t)B * T + 255) / 256)), dim3(256), 0, s, p);
    if (hipGetLastError() != hipSuccess) {
        snprintf(g_eerr, sizeof(g_eerr), "cs_store_episodes_compact: kernel launch failed");
        return CS_E_LAUNCH;
    }
    return CS_OK;
}

int cs_render_episodes(const cs_render_params *p, const float *states_dev, const float *maps_dev, const int32_t *counts_dev,
                       int E, int R, uint8_t *frames_dev, void *stream) {
    const char *bad = nullptr;
    if (!p || !states_dev || !counts_dev || !frames_dev || !p->palette_dev || !p->lut_dev) bad = "a NULL pointer";
    else if (bad_agents(p->n_agents)) bad = bad_agents(p->n_agents);
    else if (p->n_targets < 1 || p->n_targets > CS_MAX_TARGETS) bad = "n_targets must be 1..16";
    else if (p->state_width != 4 * p->n_agents + 3 * p->n_targets) bad = "state_width must be 4 n_agents + 3 n_targets";
    else if (p->size < 16 || p->size > 1024 || p->size % 4 != 0) bad = "size must be a multiple of 4 in 16..1024";
    else if (E < 1 || E > 65535 || R < 1) bad = "E must be 1..65535 and R >= 1";
    else if (p->rv < 0 || p->rv > 32767 || p->rt < 0 || p->rt > 32767 || p->rtr < 0 || p->rtr > 32767 || p->tri_len < 0 ||
             p->tri_len > 16383)
        bad = "a radius is out of range (rv, rt, rtr 0..32767, tri_len 0..16383)";
    else if ((uintptr_t)frames_dev % 4 != 0) bad = "frames_dev must be 4-byte aligned";
    else if (maps_dev && (p->side < 1 || p->side > CS_MAX_MAP || p->map_width != p->side * p->side))
        bad = "side must be 1..64 and map_width side * side";
    if (bad) return fail(__func__, bad);
    auto rgb = [](const uint8_t *c) { return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16); };
    const RenderArgs a{states_dev, maps_dev, counts_dev, frames_dev, p->palette_dev, p->lut_dev, R, p->state_width, p->n_agents,
                       p->n_targets, p->size, maps_dev ? p->side : 0, maps_dev ? p->map_width : 0, p->rv, p->rt, p->rtr, p->tri_len,
                       p->layers, rgb(p->background), rgb(p->sensor_tint), rgb(p->sensor_ring), rgb(p->target), rgb(p->target_found),
                       rgb(p->bar_on), rgb(p->bar_off)};
    const int quads = p->size * p->size / 4;
    hipLaunchKernelGGL(k_render_episodes, dim3((quads + RENDER_THREADS - 1) / RENDER_THREADS, E), dim3(RENDER_THREADS), 0,
                       (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_coverage_actions(const cs_coverage_params *p, const float *state_dev, int B, int32_t *grid_dev, int64_t *actions_dev,
                        void *stream) {
    if (!p || !state_dev || !grid_dev || !actions_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_cover(p->keep, p->regrow, p->lookahead, p->side), bad_width(p->state_width, p->n_agents), bad_reserved(p->reserved),
                             misaligned({grid_dev, state_dev}, {actions_dev})});
    if (bad) return fail(__func__, bad);
    const CoverageArgs a = cover_args(state_dev, grid_dev, actions_dev, p->n_agents, p->side, p->state_width, p->view_range, p->keep,
                                      p->regrow, p->lookahead, grid_dev);
    hipLaunchKernelGGL(k_coverage_actions, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_local_coverage_actions(const cs_local_params *p, const float *state_dev, int B, int32_t *grids_dev, int64_t *actions_dev,
                              void *stream) {
    if (!p || !state_dev || !grids_dev || !actions_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_cover(p->keep, p->regrow, p->lookahead, p->side), bad_width(p->state_width, p->n_agents),
                             p->comm_range < -1 || p->comm_range > LOC_MAX_COMM ? "comm_range must be -1 (unlimited) or 0..128" : nullptr,
                             bad_reserved(p->reserved), misaligned({grids_dev, state_dev}, {actions_dev})});
    if (bad) return fail(__func__, bad);
    // rows are cells words apart, for every agent of every env: all of them are aligned when the base is and cells % 4 == 0
    const LocalArgs a{cover_args(state_dev, grids_dev, actions_dev, p->n_agents, p->side, p->state_width, p->view_range, p->keep,
                                 p->regrow, p->lookahead, grids_dev),
                      p->comm_range < 0 ? -1LL : (long long)(16 * p->comm_range) * (long long)(16 * p->comm_range)};
    hipLaunchKernelGGL(k_local_coverage_actions, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_sweep_episodes(const cs_sweep_params *p, const float *states_dev, const int32_t *counts_dev, int E, int32_t *first_dev,
                      int32_t *new_dev, int32_t *seen_dev, void *stream) {
    if (!p || !states_dev || !counts_dev || !first_dev || !new_dev || !seen_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({E < 1 ? "E must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_width(p->state_width, p->n_agents), p->rows < 1 ? "rows must be >= 1" : nullptr,
                             bad_reserved(p->reserved),
                             misaligned({states_dev, counts_dev, first_dev, new_dev, seen_dev}, {})});
    if (bad) return fail(__func__, bad);
    const SweepArgs a{states_dev, counts_dev, first_dev, new_dev, seen_dev, p->n_agents, p->side, p->state_width, p->rows, 16 * p->view_range};
    hipLaunchKernelGGL(k_sweep_episodes, dim3((unsigned)E), dim3(SWEEP_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_belief_actions(const cs_belief_params *p, const float *state_dev, int B, int32_t *grid_dev, int32_t *prev_dev,
                      int64_t *actions_dev, void *stream) {
    if (!p || !state_dev || !grid_dev || !prev_dev || !actions_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_cover(p->keep, 16, p->lookahead, p->side), bad_width(p->state_width, p->n_agents),
                             bad_model(p->mode, p->moved, p->sense16), bad_reserved(p->reserved),
                             misaligned({grid_dev, prev_dev, state_dev}, {actions_dev}), bad_steps(p->dx, p->dy)});
    if (bad) return fail(__func__, bad);
    BeliefArgs a = belief_args(cover_args(state_dev, grid_dev, actions_dev, p->n_agents, p->side, p->state_width, p->view_range, p->keep,
                                          16, p->lookahead, grid_dev),
                               p->mode, p->sense16, p->dx, p->dy);
    a.prev = prev_dev;
    a.moved = p->moved;
    hipLaunchKernelGGL(k_belief_actions, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_local_belief_actions(const cs_local_belief_params *p, const float *state_dev, int B, int32_t *grids_dev, int32_t *prev_dev,
                            int32_t *heard_dev, int64_t *actions_dev, void *stream) {
    if (!p || !state_dev || !grids_dev || !prev_dev || !heard_dev || !actions_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_cover(p->keep, 16, p->lookahead, p->side), bad_width(p->state_width, p->n_agents),
                             bad_model(p->mode, p->moved, p->sense16),
                             p->comm_range < -1 || p->comm_range > LOC_MAX_COMM ? "comm_range must be -1 (unlimited) or 0..128" : nullptr,
                             bad_reserved(p->reserved), misaligned({grids_dev, prev_dev, heard_dev, state_dev}, {actions_dev}),
                             bad_steps(p->dx, p->dy)});
    if (bad) return fail(__func__, bad);
    // rows are cells words apart, for every agent of every env: all of them are aligned when the base is and cells % 4 == 0
    LocalBeliefArgs a{};
    a.b = belief_args(cover_args(state_dev, grids_dev, actions_dev, p->n_agents, p->side, p->state_width, p->view_range, p->keep, 16,
                                 p->lookahead, grids_dev),
                      p->mode, p->sense16, p->dx, p->dy);
    a.b.prev = prev_dev;
    a.b.moved = p->moved;
    a.heard = heard_dev;
    a.C2 = p->comm_range < 0 ? -1LL : (long long)(16 * p->comm_range) * (long long)(16 * p->comm_range);
    hipLaunchKernelGGL(k_local_belief_actions, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_plan_actions(const cs_plan_params *p, const float *state_dev, int B, const int32_t *grid_dev, int64_t *actions_dev,
                    int64_t *plans_dev, int64_t *scores_dev, void *stream) {
    return plan_launch(__func__, false, p, state_dev, B, grid_dev, actions_dev, plans_dev, scores_dev, stream);
}

int cs_local_plan_actions(const cs_local_plan_params *p, const float *state_dev, int B, const int32_t *grids_dev, int64_t *actions_dev,
                          int64_t *plans_dev, int64_t *scores_dev, void *stream) {
    if (!p || !state_dev || !grids_dev || !actions_dev || !plans_dev || !scores_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_plan(p->depth, p->stride, p->discount), bad_width(p->state_width, p->n_agents),
                             p->comm_range < -1 || p->comm_range > LOC_MAX_COMM ? "comm_range must be -1 (unlimited) or 0..128" : nullptr,
                             bad_reserved(p->reserved), misaligned({grids_dev, state_dev}, {actions_dev, plans_dev, scores_dev})});
    if (bad) return fail(__func__, bad);
    const int cells = p->side * p->side;
    int seqs = 1;
    for (int d = 0; d < p->depth; d++) seqs *= 3;
    // rows are cells words apart, for every agent of every env: all of them are aligned when the base is and cells % 4 == 0
    const LocalPlanArgs a{PlanArgs{state_dev, grids_dev, actions_dev, plans_dev, scores_dev, p->n_agents, p->side, p->state_width,
                                   16 * p->view_range, p->depth, p->stride, p->discount, (3 * seqs - 3) / 2, seqs, vec4_ok(cells, grids_dev)},
                          p->comm_range < 0 ? -1LL : (long long)(16 * p->comm_range) * (long long)(16 * p->comm_range)};
    hipLaunchKernelGGL(k_local_plan_actions, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_belief_forecast(const cs_forecast_params *p, const int32_t *grid_dev, const int32_t *pos_dev, int B, int32_t *stack_dev,
                       void *stream) {
    if (!p || !grid_dev || !pos_dev || !stack_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, 0),
                             p->levels < 1 || p->levels > FC_MAX_LEVELS ? "levels must be 1..5" : nullptr,
                             bad_model(p->mode, 0, p->sense16), bad_reserved(p->reserved),
                             misaligned({grid_dev, pos_dev, stack_dev}, {}), bad_steps(p->dx, p->dy)});
    for (int d = 0; !bad && d < FC_MAX_LEVELS; d++)
        if (p->moves[d] < 0 || p->moves[d] > PLAN_MAX_STRIDE || (d >= p->levels && p->moves[d] != 0))
            bad = "moves must be 0..8, and 0 beyond `levels`";
    if (bad) return fail(__func__, bad);
    const int cells = p->side * p->side;
    ForecastArgs a{};
    a.b = belief_args(CoverageArgs{}, p->mode, p->sense16, p->dx, p->dy);
    a.b.c.n = p->n_agents;
    a.b.c.side = p->side;
    a.grid = grid_dev;
    a.pos = pos_dev;
    a.stack = stack_dev;
    a.levels = p->levels;
    for (int d = 0; d < FC_MAX_LEVELS; d++) a.moves[d] = p->moves[d];
    a.vec_in = vec4_ok(cells, grid_dev);
    a.vec_out = vec4_ok(cells, stack_dev);
    hipLaunchKernelGGL(k_belief_forecast, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_plan_forecast_actions(const cs_plan_params *p, const float *state_dev, int B, const int32_t *stack_dev, int64_t *actions_dev,
                             int64_t *plans_dev, int64_t *scores_dev, void *stream) {
    return plan_launch(__func__, true, p, state_dev, B, stack_dev, actions_dev, plans_dev, scores_dev, stream);
}

int cs_local_belief_forecast(const cs_forecast_params *p, const int32_t *grids_dev, const int32_t *prev_dev, const int32_t *heard_dev,
                             int B, int32_t *stacks_dev, void *stream) {
    if (!p || !grids_dev || !prev_dev || !heard_dev || !stacks_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, 0),
                             p->levels < 1 || p->levels > FC_MAX_LEVELS ? "levels must be 1..5" : nullptr,
                             bad_model(p->mode, 0, p->sense16), bad_reserved(p->reserved),
                             misaligned({grids_dev, prev_dev, heard_dev, stacks_dev}, {}), bad_steps(p->dx, p->dy)});
    for (int d = 0; !bad && d < FC_MAX_LEVELS; d++)
        if (p->moves[d] < 0 || p->moves[d] > PLAN_MAX_STRIDE || (d >= p->levels && p->moves[d] != 0))
            bad = "moves must be 0..8, and 0 beyond `levels`";
    if (!bad && (long long)B * p->n_agents > 0x7fffffffLL) bad = "B * n_agents must fit a launch grid";
    if (bad) return fail(__func__, bad);
    const int cells = p->side * p->side;
    LocalForecastArgs a{};
    a.f.b = belief_args(CoverageArgs{}, p->mode, p->sense16, p->dx, p->dy);
    a.f.b.c.n = p->n_agents;
    a.f.b.c.side = p->side;
    a.f.grid = grids_dev;
    a.f.pos = prev_dev;
    a.f.stack = stacks_dev;
    a.f.levels = p->levels;
    for (int d = 0; d < FC_MAX_LEVELS; d++) a.f.moves[d] = p->moves[d];
    // rows are cells (levels * cells) words apart, for every agent of every env: all of them are aligned when the base is and cells % 4 == 0
    a.f.vec_in = vec4_ok(cells, grids_dev);
    a.f.vec_out = vec4_ok(cells, stacks_dev);
    a.heard = heard_dev;
    hipLaunchKernelGGL(k_local_belief_forecast, dim3((unsigned)B * (unsigned)p->n_agents), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_local_plan_forecast_actions(const cs_local_plan_params *p, const float *state_dev, int B, const int32_t *stacks_dev,
                                   int64_t *actions_dev, int64_t *plans_dev, int64_t *scores_dev, void *stream) {
    if (!p || !state_dev || !stacks_dev || !actions_dev || !plans_dev || !scores_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_plan(p->depth, p->stride, p->discount), bad_width(p->state_width, p->n_agents),
                             p->comm_range < -1 || p->comm_range > LOC_MAX_COMM ? "comm_range must be -1 (unlimited) or 0..128" : nullptr,
                             bad_reserved(p->reserved), misaligned({stacks_dev, state_dev}, {actions_dev, plans_dev, scores_dev})});
    if (bad) return fail(__func__, bad);
    const int cells = p->side * p->side, level_words = (cells + 3) & ~3;
    int seqs = 1;
    for (int d = 0; d < p->depth; d++) seqs *= 3;
    // an agent's levels are depth * cells words apart, for every agent of every env: all of them are aligned when the base is and cells % 4 == 0
    const LocalPlanArgs a{PlanArgs{state_dev, stacks_dev, actions_dev, plans_dev, scores_dev, p->n_agents, p->side, p->state_width,
                                   16 * p->view_range, p->depth, p->stride, p->discount, (3 * seqs - 3) / 2, seqs, vec4_ok(cells, stacks_dev)},
                          p->comm_range < 0 ? -1LL : (long long)(16 * p->comm_range) * (long long)(16 * p->comm_range)};
    const size_t lds = lfc_plan_lds_bytes(p->depth, level_words);
    // more than 64 KB of dynamic LDS (side 64 with depth 4 or 5) is granted only to a kernel that asked for it
    if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void *>(&k_local_plan_forecast_actions),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(g_eerr, sizeof(g_eerr), "%s: the device does not grant %zu bytes of LDS", __func__, lds);
        return CS_E_LAUNCH;
    }
    hipLaunchKernelGGL(k_local_plan_forecast_actions, dim3((unsigned)B), dim3(COV_THREADS), lds, (hipStream_t)stream, a, level_words);
    return launched(__func__);
}

int cs_label_episodes(const cs_label_params *p, const float *s_dev, int E, int T, const int32_t *lens_dev, int64_t *labels_dev,
                      int32_t *grid_out_dev, int32_t *prev_out_dev, void *stream) {
    if (!p || !s_dev || !lens_dev || !labels_dev) return fail(__func__, "a NULL pointer");
    const char *bad = bad_label(p, E, T, prev_out_dev, "prev_out_dev is the belief expert's (the coverage expert keeps no positions)",
                                {s_dev, lens_dev, grid_out_dev, prev_out_dev}, {labels_dev});
    if (bad) return fail(__func__, bad);
    const LabelArgs a = label_args(p, s_dev, T, lens_dev, labels_dev, grid_out_dev, prev_out_dev);
    hipLaunchKernelGGL(k_label_episodes, dim3((unsigned)E), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_grid_features(const cs_grid_params *p, const float *state_dev, int B, const int32_t *grid_dev, float *feat_dev, void *stream) {
    if (!p || !state_dev || !grid_dev || !feat_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_cover(0, 1, p->lookahead, p->side), bad_width(p->state_width, p->n_agents), bad_reserved(p->reserved),
                             misaligned({grid_dev, state_dev, feat_dev}, {})});
    if (bad) return fail(__func__, bad);
    const GridObsArgs a{state_dev, grid_dev, feat_dev, p->n_agents, p->side, p->state_width, 16 * p->view_range, 16 * p->lookahead};
    hipLaunchKernelGGL(k_grid_features, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_feature_episodes(const cs_label_params *p, const float *s_dev, int E, int T, const int32_t *lens_dev, float *feat_dev,
                        int64_t *labels_dev, int32_t *grid_out_dev, int32_t *prev_out_dev, void *stream) {
    if (!p || !s_dev || !lens_dev || !feat_dev) return fail(__func__, "a NULL pointer");
    const char *bad = bad_label(p, E, T, prev_out_dev, "prev_out_dev is the belief filter's (the coverage filter keeps no positions)",
                                {s_dev, lens_dev, feat_dev, grid_out_dev, prev_out_dev}, {labels_dev});
    if (bad) return fail(__func__, bad);
    FeatArgs f{};
    f.l = label_args(p, s_dev, T, lens_dev, labels_dev, grid_out_dev, prev_out_dev);
    f.feat = feat_dev;
    f.fvec = (uintptr_t)feat_dev % 16 == 0 ? 1 : 0;
    hipLaunchKernelGGL(k_feature_episodes, dim3((unsigned)E), dim3(COV_THREADS), 0, (hipStream_t)stream, f);
    return launched(__func__);
}

int cs_local_grid_features(const cs_grid_params *p, const float *state_dev, int B, const int32_t *grids_dev, float *feat_dev,
                           void *stream) {
    if (!p || !state_dev || !grids_dev || !feat_dev) return fail(__func__, "a NULL pointer");
    const char *bad = first({B < 1 ? "B must be >= 1" : nullptr, bad_team(p->n_agents, p->side, p->view_range),
                             bad_cover(0, 1, p->lookahead, p->side), bad_width(p->state_width, p->n_agents), bad_reserved(p->reserved),
                             misaligned({grids_dev, state_dev, feat_dev}, {})});
    if (bad) return fail(__func__, bad);
    const LocalGridObsArgs a{state_dev, grids_dev, feat_dev, p->n_agents, p->side, p->state_width, 16 * p->view_range, 16 * p->lookahead};
    hipLaunchKernelGGL(k_local_grid_features, dim3((unsigned)B), dim3(COV_THREADS), 0, (hipStream_t)stream, a);
    return launched(__func__);
}

int cs_local_feature_episodes(const cs_local_label_params *p, const float *s_dev, const int32_t *lens_dev, int E, int T, float *feat_dev,
                              int64_t *labels_dev, int32_t *grids_dev, int32_t *prev_dev, int32_t *heard_dev, void *stream) {
    if (!p || !s_dev || !lens_dev || !feat_dev || !grids_dev) return fail(__func__, "a NULL pointer");
    cs_label_params q{p->expert, p->n_agents, p->side, p->view_range, p->keep, p->regrow,
                      p->lookahead, p->state_width, p->mode, p->sense16, p->every, p->moving};   // cs_label_params' fields: one ladder
    for (int k = 0; k < 16; k++) {
        q.dx[k] = p->dx[k];
        q.dy[k] = p->dy[k];
    }
    q.reserved = p->reserved;
    const char *bad = first({bad_label(&q, E, T, prev_dev, "prev_dev is the belief filter's (the coverage filter keeps no positions)",
                                       {s_dev, lens_dev, feat_dev, grids_dev, prev_dev, heard_dev}, {labels_dev}),
                             p->comm_range < -1 || p->comm_range > LOC_MAX_COMM ? "comm_range must be -1 (unlimited) or 0..128" : nullptr,
                             p->expert == LABEL_COVERAGE && heard_dev ? "heard_dev is the belief filter's (the coverage filter keeps no masks)"
                                                                     : nullptr});
    if (bad) return fail(__func__, bad);
    // rows of the workspace are cells words apart, for every agent of every episode: all are aligned when the base is and cells % 4 == 0
    LocalFeatArgs f{};
    f.l = label_args(&q, s_dev, T, lens_dev, labels_dev, grids_dev, prev_dev);
    f.feat = feat_dev;
    f.heard_out = heard_dev;
    f.C2 = p->comm_range < 0 ? -1LL : (long long)(16 * p->comm_range) * (long long)(16 * p->comm_range);
    f.fvec = (uintptr_t)feat_dev % 16 == 0 ? 1 : 0;
    hipLaunchKernelGGL(k_local_feature_episodes, dim3((unsigned)E), dim3(COV_THREADS), 0, (hipStream_t)stream, f);
    return launched(__func__);
}

const char *cs_episodes_last_error(void) { return g_eerr; }

// for coopsearch.hip: cs_move_targets takes a cs_config and the state blob, so it lives there, and reports here
__attribute__((visibility("hidden"))) void episodes_set_error(const char *msg) { snprintf(g_eerr, sizeof(g_eerr), "%s", msg); }

}  // extern "C"
