// cooperative-search_amd/csrc/render.h -- cs_render_episodes: the state (and map) rows of E episodes as RGB frames, one launch
// (included by episodes.hip inside its namespace).
//
// The frame is DEFINED by render.render_episodes_torch (stock torch ops); this kernel reproduces it byte for byte.  Nothing here
// is floating point but the quantisation of a row's floats (one add or one multiply, then round-half-even): positions become
// integers in sub-units (U = 16 W across the map, a pixel centre at 16 c + 8), headings integers x 1024, and every disc,
// ring and triangle test is integer arithmetic that cannot overflow -- a box test first bounds what is squared (uint32) or
// multiplied (int64).
//
// Layout: grid (pixel bands, episodes), 256 threads; a thread owns 4 horizontally adjacent pixels -- 12 contiguous output
// bytes, one 3-dword store per frame, 768 contiguous bytes per wavefront -- and walks the R frames of its episode in order with
// the trail bits of its pixels (8 agents x 4 pixels) in one register.  A frame's parameters are the same for the whole
// workgroup: wavefront 0 quantises them into LDS (two buffers in turn: one barrier per frame) and every pixel test reads them
// as broadcasts.  At W = 256 a wavefront is one image row, so the row tests below are wavefront-uniform branches.  Frames at or
// past the episode's count repeat the last real one: its 12 bytes are kept in registers and stored again.
constexpr int RENDER_THREADS = 256;
constexpr float RENDER_POS_LIM = 1048576.0f;   // |quantised position| <= 2^20 sub-units (the image is at most 2^14 wide)

struct RenderArgs {
    const float *states, *maps;
    const int32_t *counts;
    unsigned char *frames;
    const unsigned char *palette, *lut;
    int R, S, n, m, W, side, cells, rv, rt, rtr, L, layers;
    unsigned bg, tint, ring, tgt, tgt_found, bar_on, bar_off;   // r | g << 8 | b << 16
};

struct RenderFrame {   // what one frame's row says, quantised
    int ax[CS_MAX_AGENTS], ay[CS_MAX_AGENTS];   // agent positions, sub-units, y down
    int tri[CS_MAX_AGENTS][6];                  // triangle vertices relative to the position, sub-units x 1024: v0, v1, v2
    int tx[CS_MAX_TARGETS], ty[CS_MAX_TARGETS];
    unsigned found;                             // bit j: target j found
    int k;                                      // how many
};

struct alignas(4) RenderQuad {   // 4 pixels
    unsigned w0, w1, w2;
};

// rint(v) as an int in [-lim, lim]; NaN gives -lim (both comparisons fail the same way in the definition)
__device__ __forceinline__ int render_quant(float v, float lim) {
    const float r = rintf(v);
    return (int)(r >= -lim ? (r <= lim ? r : lim) : -lim);
}

__device__ __forceinline__ unsigned render_rgb(const unsigned char *p) {
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

// (96 tint + 159 dst + 127) / 255 per channel
__device__ __forceinline__ unsigned render_blend(unsigned tint, unsigned dst) {
    unsigned out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const unsigned t = (tint >> (8 * ch)) & 255u, d = (dst >> (8 * ch)) & 255u;
        out |= ((96u * t + 159u * d + 127u) / 255u) << (8 * ch);
    }
    return out;
}

__device__ __forceinline__ void render_stage(const RenderArgs &a, RenderFrame &F, const float *row, int lane) {
    const float s8w = (float)(8 * a.W);
    const int U = 16 * a.W;
    if (lane < a.n) {
        const float *s = row + 4 * lane;
        F.ax[lane] = render_quant((s[0] + 1.0f) * s8w, RENDER_POS_LIM);
        F.ay[lane] = U - render_quant((s[1] + 1.0f) * s8w, RENDER_POS_LIM);
        const int ci = render_quant(s[2] * 1024.0f, 1024.0f), si = render_quant(s[3] * 1024.0f, 1024.0f);
        const int L = a.L, h = L / 2, w = (L * 6) / 10;
        F.tri[lane][0] = L * ci;
        F.tri[lane][1] = -L * si;
        F.tri[lane][2] = -h * ci + w * si;
        F.tri[lane][3] = h * si + w * ci;
        F.tri[lane][4] = -h * ci - w * si;
        F.tri[lane][5] = h * si - w * ci;
    }
    const int j = lane - 16;
    bool f = false;
    if (j >= 0 && j < a.m) {
        const float *s = row + 4 * a.n + 3 * j;
        F.tx[j] = render_quant((s[0] + 1.0f) * s8w, RENDER_POS_LIM);
        F.ty[j] = U - render_quant((s[1] + 1.0f) * s8w, RENDER_POS_LIM);
        f = s[2] > 0.5f;
    }
    const unsigned found = (unsigned)((__ballot(f) >> 16) & 0xffffull);
    if (lane == 0) {
        F.found = found;
        F.k = __popc(found);
    }
}

__global__ __launch_bounds__(RENDER_THREADS) void k_render_episodes(RenderArgs a) {
    __shared__ RenderFrame fr[2];
    __shared__ unsigned lut[256];
    __shared__ unsigned pal[CS_MAX_AGENTS];
    const int tid = threadIdx.x, e = blockIdx.y;
    const int W = a.W, U = 16 * W;
    const int quad = blockIdx.x * RENDER_THREADS + tid;
    const bool live = quad < W * W / 4;
    const int pix = live ? quad * 4 : 0;   // (W is a multiple of 4: the 4 pixels share a row)
    const int r = pix / W, c0 = pix % W;
    const int Y = 16 * r + 8, X0 = 16 * c0 + 8;
    const bool heat = (a.layers & CS_RENDER_HEAT) && a.maps;
    if (heat) lut[tid] = render_rgb(a.lut + 3 * tid);
    if (tid < CS_MAX_AGENTS) pal[tid] = render_rgb(a.palette + 3 * tid);
    int cell[4] = {0, 0, 0, 0};
    if (heat) {
        const int iy = min(max(((U - Y) * a.side) / U, 0), a.side - 1);
#pragma unroll
        for (int k = 0; k < 4; k++) cell[k] = min(max(((X0 + 16 * k) * a.side) / U, 0), a.side - 1) * a.side + iy;
    }
    const int cnt = min(max(a.counts[e], 1), a.R);
    const int tb = max(a.L, a.L / 2 + (a.L * 6) / 10);   // no triangle vertex is further from its agent, per axis
    const unsigned rv2 = (unsigned)a.rv * (unsigned)a.rv, rin2 = (unsigned)((a.rv - 16) * (a.rv - 16));
    const unsigned rt2 = (unsigned)a.rt * (unsigned)a.rt, rtr2 = (unsigned)a.rtr * (unsigned)a.rtr;
    const bool sensor = a.layers & CS_RENDER_SENSOR, trail_on = a.layers & CS_RENDER_TRAIL, targets = a.layers & CS_RENDER_TARGETS;
    const bool agents = a.layers & CS_RENDER_AGENTS, bar = (a.layers & CS_RENDER_BAR) && r < 4;
    unsigned trail = 0;   // bit 4 i + k: pixel k has been within rtr of agent i
    RenderQuad q = {0u, 0u, 0u};
    unsigned char *dst = a.frames + ((size_t)e * a.R * W * W + (size_t)pix) * 3;
    for (int t = 0; t < a.R; t++, dst += (size_t)W * W * 3) {
        if (t < cnt) {   // (block-uniform)
            RenderFrame &F = fr[t & 1];
            if (tid < 64) render_stage(a, F, a.states + ((size_t)e * a.R + t) * a.S, tid);
            __syncthreads();
            if (live) {
                unsigned col[4];
                if (heat) {
                    const float *mp = a.maps + ((size_t)e * a.R + t) * a.cells;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float p = mp[cell[k]];
                        const float pc = p > 0.0f ? (p < 1.0f ? p : 1.0f) : 0.0f;
                        col[k] = lut[(int)rintf(pc * 255.0f)];
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) col[k] = a.bg;
                }
                unsigned fill = 0, ring = 0;       // bit k: pixel k inside a sensor disc / on a sensor ring
                int owner[4] = {-1, -1, -1, -1};   // the last agent whose triangle covers pixel k
                for (int i = 0; i < a.n; i++) {
                    const int dy = Y - F.ay[i], dx0 = X0 - F.ax[i];
                    const unsigned ady = (unsigned)abs(dy);
                    if (ady <= (unsigned)a.rv) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const unsigned adx = (unsigned)abs(dx0 + 16 * k);
                            if (adx <= (unsigned)a.rv) {
                                const unsigned d2 = adx * adx + ady * ady;
                                if (d2 <= rv2) {
                                    fill |= 1u << k;
                                    if (d2 > rin2) ring |= 1u << k;
                                }
                            }
                        }
                    }
                    if (trail_on && ady <= (unsigned)a.rtr) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const unsigned adx = (unsigned)abs(dx0 + 16 * k);
                            if (adx <= (unsigned)a.rtr && adx * adx + ady * ady <= rtr2) trail |= 1u << (4 * i + k);
                        }
                    }
                    if (agents && ady <= (unsigned)tb) {
                        const int *v = F.tri[i];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int dx = dx0 + 16 * k;
                            if ((unsigned)abs(dx) <= (unsigned)tb) {
                                const long long px = 1024ll * dx, py = 1024ll * dy;
                                const long long e0 = (long long)(v[2] - v[0]) * (py - v[1]) - (long long)(v[3] - v[1]) * (px - v[0]);
                                const long long e1 = (long long)(v[4] - v[2]) * (py - v[3]) - (long long)(v[5] - v[3]) * (px - v[2]);
                                const long long e2 = (long long)(v[0] - v[4]) * (py - v[5]) - (long long)(v[1] - v[5]) * (px - v[4]);
                                if ((e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0)) owner[k] = i;
                            }
                        }
                    }
                }
                unsigned unf = 0, fnd = 0;   // bit k: pixel k inside an unfound / a found target's disc
                if (targets) {
                    for (int j = 0; j < a.m; j++) {
                        const unsigned ady = (unsigned)abs(Y - F.ty[j]);
                        if (ady <= (unsigned)a.rt) {
                            const int dx0 = X0 - F.tx[j];
                            unsigned in = 0;
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const unsigned adx = (unsigned)abs(dx0 + 16 * k);
                                if (adx <= (unsigned)a.rt && adx * adx + ady * ady <= rt2) in |= 1u << k;
                            }
                            if ((F.found >> j) & 1u) fnd |= in;
                            else unf |= in;
                        }
                    }
                }
                const int kfound = F.k;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    unsigned c = col[k];
                    if (sensor && ((fill >> k) & 1u)) c = render_blend(a.tint, c);
                    if (trail_on) {
                        unsigned bits = (trail >> k) & 0x11111111u;   // bit 4 i: agent i's trail covers this pixel
                        if (bits) c = pal[(31 - __clz((int)bits)) >> 2];   // the highest agent index wins
                    }
                    if (sensor && ((ring >> k) & 1u)) c = a.ring;
                    if ((unf >> k) & 1u) c = a.tgt;
                    if ((fnd >> k) & 1u) c = a.tgt_found;
                    if (owner[k] >= 0) c = pal[owner[k]];
                    if (bar) c = (c0 + k) * a.m < kfound * W ? a.bar_on : a.bar_off;
                    col[k] = c;
                }
                q.w0 = col[0] | (col[1] << 24);
                q.w1 = (col[1] >> 8) | (col[2] << 16);
                q.w2 = (col[2] >> 16) | (col[3] << 8);
            }
        }
        if (live) *reinterpret_cast<RenderQuad *>(dst) = q;
    }
}
