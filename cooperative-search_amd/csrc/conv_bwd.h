// conv_bwd.h -- the backward pass of the flight conv front end (k_conv_features, policy.hip): the six weight gradients of
// Conv2d(1,4,k=4,s=2) -> ReLU -> Conv2d(4,1,k=3,p=1) -> ReLU -> Linear(576,16), summed over n_maps maps.  Included by policy.hip
// behind k_conv_features (ConvParams, MAPW, C1W, C1P, NPOS, NFEAT, PBLOCK are its names).  No gradient for the maps: data.
//
// * Nothing is saved by the forward.  Both activation planes are recomputed in LDS from the map with k_conv_features' own FMA
//   chains (the conv1 / conv2 blocks below are copies of its code: same tap order, same channel pairing), so the ReLU gates are
//   exactly the ones the forward applied.  The linear layer's output is not needed and is not recomputed.
// * No float atomics.  A persistent workgroup keeps its partial sums in registers over all its maps -- thread (j, sl) the 36
//   entries dlinear.weight[j][sl + 16 i] it alone owns, a strip thread its 37 conv2 and 68 conv1 partials -- reduces the strip
//   partials once at the end (butterfly inside a wavefront, the three wavefronts added in order) and writes one set of
//   CG_FLOATS partial gradients to partial[blockIdx.x].  k_conv_grad_reduce adds the sets in a fixed order.  The grid is a
//   function of the device and n_maps only, so reruns are bit-identical.
// * A map whose 16 dfeat values are all zero (a padded step) contributes nothing and is skipped before it is fetched; the
//   decision is the same for every thread of the workgroup (dfeat row m is read through a uniform address).

// offsets of the six gradients in a partial set (torch layouts: [4][1][4][4], [4], [1][4][3][3], [1], [16][576], [16])
constexpr int CG_C1W = 0, CG_C1B = 64, CG_C2W = 68, CG_C2B = 104, CG_SMALL = 105;   // the 105 values the strip threads share
constexpr int CG_LW = CG_SMALL, CG_LB = CG_LW + NFEAT * NPOS, CG_FLOATS = CG_LB + NFEAT;
constexpr int CG_STRIDE = (CG_FLOATS + 15) / 16 * 16;   // floats between two workgroups' sets
static_assert(CG_FLOATS == 9337, "64 + 4 + 36 + 1 + 9216 + 16");

struct ConvBwdParams {
    ConvParams f;         // weights and maps as the forward takes them (f.feat is not used)
    const float *dfeat;   // [n_maps][16]
    float *partial;       // [gridDim.x][CG_STRIDE]
};

// two workgroups per CU (71 KB of LDS each; <= 256 VGPRs)
__global__ __launch_bounds__(PBLOCK, 2) void k_conv_features_bwd(ConvBwdParams q) {
    using v2f = __attribute__((ext_vector_type(2))) float;
    const ConvParams &p = q.f;
    constexpr int MAPP = 56, C1Q = 40;   // k_conv_features' pitches (its comment on the LDS banks)
    constexpr int DCP = 28;              // floats per row of the dc2 plane ([26][26] used: conv2's padding as a zero border)
    __shared__ __attribute__((aligned(16))) float s_map[MAPW * MAPP];
    __shared__ __attribute__((aligned(16))) float s_c1[2 * C1P * C1Q * 2];
    __shared__ __attribute__((aligned(16))) float s_c2[NPOS];            // transposed: element pos at (pos % 16) * 36 + pos / 16
    __shared__ __attribute__((aligned(16))) float s_dc2[C1P * DCP];
    __shared__ __attribute__((aligned(16))) float s_lw[NFEAT * NPOS];    // linear.weight as it is: [16][576]
    __shared__ v2f s_w1[2][16];
    __shared__ float s_red[3][CG_SMALL];
    const int t = threadIdx.x;
    static_assert(C1CH == 4 && PBLOCK == 256 && C1W % 3 == 0, "192 strip threads = wavefronts 0 .. 2");
    v2f bias1[2], w2[2][9];
    float bias2;
    if (t < 32) s_w1[t >> 4][t & 15] = v2f{p.c1w[(2 * (t >> 4)) * 16 + (t & 15)], p.c1w[(2 * (t >> 4) + 1) * 16 + (t & 15)]};
#pragma unroll
    for (int h = 0; h < 2; h++) bias1[h] = v2f{p.c1b[2 * h], p.c1b[2 * h + 1]};
#pragma unroll
    for (int h = 0; h < 2; h++)   // pair h: input channels h and h + 2
#pragma unroll
        for (int k = 0; k < 9; k++) w2[h][k] = v2f{p.c2w[h * 9 + k], p.c2w[(h + 2) * 9 + k]};
    bias2 = p.c2b[0];
    for (int i = t; i < 2 * C1P * C1Q * 2; i += PBLOCK) s_c1[i] = 0.0f;
    for (int i = t; i < C1P * DCP; i += PBLOCK) s_dc2[i] = 0.0f;
    for (int i = t; i < NFEAT * NPOS; i += PBLOCK) s_lw[i] = p.lw[i];
    const int j = t >> 4, sl = t & 15;
    const bool strip = t < (C1W / 3) * C1W;
    const int ts = strip ? t : 0;
    const int oy = ts / (C1W / 3), ox0 = 3 * (ts % (C1W / 3));

    // the partial sums, on chip over the whole loop
    float g_lw[NPOS / 16], g_lb = 0.0f, g_b2 = 0.0f;
    v2f g_w1[2][16], g_b1[2], g_w2[2][9];   // pairs {channel h, channel h + 2}, as conv2 reads conv1's planes
#pragma unroll
    for (int i = 0; i < NPOS / 16; i++) g_lw[i] = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        g_b1[h] = v2f{0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 16; k++) g_w1[h][k] = v2f{0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 9; k++) g_w2[h][k] = v2f{0.0f, 0.0f};
    }

    for (int m = blockIdx.x; m < p.n_maps; m += gridDim.x) {
        const float *dfp = q.dfeat + (size_t)m * NFEAT;
        float df[NFEAT];
        bool live = false;
#pragma unroll
        for (int jj = 0; jj < NFEAT; jj++) {
            df[jj] = dfp[jj];
            live |= df[jj] != 0.0f;
        }
        if (!live) continue;   // the same for the whole workgroup
        const float dfj = dfp[j];
        if (p.vec4) {
            const float4 *src4 = reinterpret_cast<const float4 *>(p.maps + (size_t)m * p.map_stride);
            for (int chunk = t; chunk < MAPW * MAPW / 4; chunk += PBLOCK) {   // (50 is even: a pair of floats never straddles two rows)
                const float4 v = src4[chunk];
                const int e0 = 4 * chunk, e1 = e0 + 2;
                *reinterpret_cast<v2f *>(s_map + (e0 / MAPW) * MAPP + e0 % MAPW) = v2f{v.x, v.y};
                *reinterpret_cast<v2f *>(s_map + (e1 / MAPW) * MAPP + e1 % MAPW) = v2f{v.z, v.w};
            }
        } else {
            const float *src = p.maps + (size_t)m * p.map_stride;
            for (int i = t; i < MAPW * MAPW; i += PBLOCK) s_map[(i / MAPW) * MAPP + i % MAPW] = src[i];
        }
        __syncthreads();
        if (strip) {   // conv1 + ReLU: k_conv_features' block, unchanged
            v2f acc[3][2];
#pragma unroll
            for (int d = 0; d < 3; d++) {
                acc[d][0] = bias1[0];
                acc[d][1] = bias1[1];
            }
#pragma unroll
            for (int ky = 0; ky < 4; ky++) {
                const v2f *r = reinterpret_cast<const v2f *>(s_map + (2 * oy + ky) * MAPP + 2 * ox0);
                const v2f a0 = r[0], a1 = r[1], a2 = r[2], a3 = r[3];
                const float in[8] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
#pragma unroll
                for (int kx = 0; kx < 4; kx++)
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const v2f w = s_w1[h][ky * 4 + kx];
#pragma unroll
                        for (int d = 0; d < 3; d++) acc[d][h] = __builtin_elementwise_fma(w, v2f{in[2 * d + kx], in[2 * d + kx]}, acc[d][h]);
                    }
            }
#pragma unroll
            for (int d = 0; d < 3; d++) {
                v2f *o = reinterpret_cast<v2f *>(s_c1) + (oy + 1) * C1Q + ox0 + d + 1;
                o[0] = v2f{fmaxf(acc[d][0].x, 0.0f), fmaxf(acc[d][1].x, 0.0f)};
                o[C1P * C1Q] = v2f{fmaxf(acc[d][0].y, 0.0f), fmaxf(acc[d][1].y, 0.0f)};
            }
        }
        __syncthreads();
        if (strip) {   // conv2 + ReLU: k_conv_features' block, unchanged
            v2f acc[3];
#pragma unroll
            for (int d = 0; d < 3; d++) acc[d] = v2f{bias2, 0.0f};
#pragma unroll
            for (int h = 0; h < 2; h++) {
#pragma unroll
                for (int ky = 0; ky < 3; ky++) {
                    v2f w[5];
#pragma unroll
                    for (int c = 0; c < 5; c++) w[c] = reinterpret_cast<const v2f *>(s_c1)[h * C1P * C1Q + (oy + ky) * C1Q + ox0 + c];
#pragma unroll
                    for (int d = 0; d < 3; d++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) acc[d] = __builtin_elementwise_fma(w2[h][ky * 3 + kx], w[d + kx], acc[d]);
                }
            }
#pragma unroll
            for (int d = 0; d < 3; d++) {
                const int pos = oy * C1W + ox0 + d;
                s_c2[(pos & 15) * (NPOS / 16) + (pos >> 4)] = fmaxf(acc[d].x + acc[d].y, 0.0f);
            }
        }
        __syncthreads();
        {   // linear layer: dW[j][pos] += dfeat[j] c2[pos], db[j] += dfeat[j]; dc2[pos] = (c2[pos] > 0) sum_j W[j][pos] dfeat[j]
            const float4 *c2v = reinterpret_cast<const float4 *>(s_c2 + sl * (NPOS / 16));
#pragma unroll
            for (int i = 0; i < NPOS / 16; i += 4) {
                const float4 v = c2v[i / 4];
                g_lw[i] = __builtin_fmaf(dfj, v.x, g_lw[i]);
                g_lw[i + 1] = __builtin_fmaf(dfj, v.y, g_lw[i + 1]);
                g_lw[i + 2] = __builtin_fmaf(dfj, v.z, g_lw[i + 2]);
                g_lw[i + 3] = __builtin_fmaf(dfj, v.w, g_lw[i + 3]);
            }
            g_lb += dfj;
            for (int pos = t; pos < NPOS; pos += PBLOCK) {
                float a = 0.0f;
#pragma unroll
                for (int jj = 0; jj < NFEAT; jj++) a = __builtin_fmaf(s_lw[jj * NPOS + pos], df[jj], a);
                const float c2 = s_c2[(pos & 15) * (NPOS / 16) + (pos >> 4)];
                s_dc2[(pos / C1W + 1) * DCP + pos % C1W + 1] = c2 > 0.0f ? a : 0.0f;
            }
        }
        __syncthreads();
        if (strip) {
            float d2[3];
#pragma unroll
            for (int d = 0; d < 3; d++) d2[d] = s_dc2[(oy + 1) * DCP + ox0 + d + 1];
            g_b2 += (d2[0] + d2[1]) + d2[2];
            // conv2's weights: dW2[c][ky][kx] += dc2[oy][ox] c1[c][oy + ky - 1][ox + kx - 1] (the forward's windows)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int ky = 0; ky < 3; ky++) {
                    v2f w[5];
#pragma unroll
                    for (int c = 0; c < 5; c++) w[c] = reinterpret_cast<const v2f *>(s_c1)[h * C1P * C1Q + (oy + ky) * C1Q + ox0 + c];
#pragma unroll
                    for (int d = 0; d < 3; d++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++)
                            g_w2[h][ky * 3 + kx] = __builtin_elementwise_fma(v2f{d2[d], d2[d]}, w[d + kx], g_w2[h][ky * 3 + kx]);
                }
            // dc1[c][y][x] = (c1[c][y][x] > 0) sum_{ky,kx} W2[c][ky][kx] dc2[y + 1 - ky][x + 1 - kx] at this strip's own positions
            float g[3][5];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 5; c++) g[r][c] = s_dc2[(oy + r) * DCP + ox0 + c];
            v2f dc1[2][3];
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    v2f a = {0.0f, 0.0f};
#pragma unroll
                    for (int ky = 0; ky < 3; ky++)
#pragma unroll
                        for (int kx = 0; kx < 3; kx++) {
                            const float gv = g[2 - ky][d + 2 - kx];
                            a = __builtin_elementwise_fma(w2[h][ky * 3 + kx], v2f{gv, gv}, a);
                        }
                    const v2f c1 = reinterpret_cast<const v2f *>(s_c1)[h * C1P * C1Q + (oy + 1) * C1Q + ox0 + d + 1];
                    dc1[h][d] = v2f{c1.x > 0.0f ? a.x : 0.0f, c1.y > 0.0f ? a.y : 0.0f};
                }
            // conv1: db1[c] += dc1[c][oy][ox], dW1[c][ky][kx] += dc1[c][oy][ox] map[2 oy + ky][2 ox + kx]
#pragma unroll
            for (int h = 0; h < 2; h++) g_b1[h] += (dc1[h][0] + dc1[h][1]) + dc1[h][2];
#pragma unroll
            for (int ky = 0; ky < 4; ky++) {
                const v2f *r = reinterpret_cast<const v2f *>(s_map + (2 * oy + ky) * MAPP + 2 * ox0);
                const v2f a0 = r[0], a1 = r[1], a2 = r[2], a3 = r[3];
                const float in[8] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
#pragma unroll
                for (int kx = 0; kx < 4; kx++)
#pragma unroll
                    for (int h = 0; h < 2; h++)
#pragma unroll
                        for (int d = 0; d < 3; d++)
                            g_w1[h][ky * 4 + kx] = __builtin_elementwise_fma(dc1[h][d], v2f{in[2 * d + kx], in[2 * d + kx]}, g_w1[h][ky * 4 + kx]);
            }
        }
        __syncthreads();   // the next map's staging writes s_map, its conv1 s_c1
    }

    float *P = q.partial + (size_t)blockIdx.x * CG_STRIDE;
#pragma unroll
    for (int i = 0; i < NPOS / 16; i++) P[CG_LW + j * NPOS + sl + 16 * i] = g_lw[i];
    if (sl == 0) P[CG_LB + j] = g_lb;
    // the 105 shared values in their torch order (channel of pair h, half x / y: h, h + 2), one butterfly each
    const int wave = t >> 6, lane = t & 63;
    auto share = [&](int k, float v) __attribute__((always_inline)) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0 && wave < 3) s_red[wave][k] = v;
    };
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int k = 0; k < 16; k++) {
            share(CG_C1W + h * 16 + k, g_w1[h][k].x);
            share(CG_C1W + (h + 2) * 16 + k, g_w1[h][k].y);
        }
        share(CG_C1B + h, g_b1[h].x);
        share(CG_C1B + h + 2, g_b1[h].y);
#pragma unroll
        for (int k = 0; k < 9; k++) {
            share(CG_C2W + h * 9 + k, g_w2[h][k].x);
            share(CG_C2W + (h + 2) * 9 + k, g_w2[h][k].y);
        }
    }
    share(CG_C2B, g_b2);
    __syncthreads();
    if (t < CG_SMALL) P[t] = (s_red[0][t] + s_red[1][t]) + s_red[2][t];
}

// out[k] = sum over the G partial sets, in an order that depends on G alone: workgroup of 64 outputs x 4 slices, slice s adds
// the sets g = s (mod 4) into four interleaved sums (no serial chain longer than G / 16), the slices are added through LDS.
struct ConvReduceParams {
    const float *partial;   // [G][CG_STRIDE]
    int G;
    float *c1w, *c1b, *c2w, *c2b, *lw, *lb;
};

__global__ __launch_bounds__(256) void k_conv_grad_reduce(ConvReduceParams r) {
    __shared__ float s_part[4][64];
    const int o = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + o;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (idx < CG_FLOATS) {
        const float *P = r.partial + idx;
        int g = s;
        for (; g + 12 < r.G; g += 16) {
            a[0] += P[(size_t)g * CG_STRIDE];
            a[1] += P[(size_t)(g + 4) * CG_STRIDE];
            a[2] += P[(size_t)(g + 8) * CG_STRIDE];
            a[3] += P[(size_t)(g + 12) * CG_STRIDE];
        }
        if (g < r.G) a[0] += P[(size_t)g * CG_STRIDE];
        if (g + 4 < r.G) a[1] += P[(size_t)(g + 4) * CG_STRIDE];
        if (g + 8 < r.G) a[2] += P[(size_t)(g + 8) * CG_STRIDE];
    }
    s_part[s][o] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (s == 0 && idx < CG_FLOATS) {
        const float v = (s_part[0][o] + s_part[1][o]) + (s_part[2][o] + s_part[3][o]);
        if (idx < CG_C1B) r.c1w[idx - CG_C1W] = v;
        else if (idx < CG_C2W) r.c1b[idx - CG_C1B] = v;
        else if (idx < CG_C2B) r.c2w[idx - CG_C2W] = v;
        else if (idx < CG_LW) r.c2b[idx - CG_C2B] = v;
        else if (idx < CG_LB) r.lw[idx - CG_LW] = v;
        else r.lb[idx - CG_LB] = v;
    }
}
