// MobileNetV2 inverted-residual kernels on gfx950 (the ReID network of appearance/mobilenetv2.py).
//
// Reference: boxmot/appearance/backbones/mobilenetv2.py ConvBlock (conv + BatchNorm + ReLU6),
// Bottleneck (1x1 expand, depthwise 3x3 stride 1 or 2, linear 1x1 projection, residual) and
// MobileNetV2.featuremaps.  BatchNorms arrive folded.  The projection, conv9 and the unfused
// expand are k_pw of osnet.hip (relu = 2: clamp to [0, 6]); the global mean is k_pool kind 2.
//   k_mb_stem       conv1: 3x3 stride 2 padding 1, 3 -> C0 (1..64) + bias + ReLU6; the input tile
//                   with its halo in LDS, 16 output channels per pass in registers.
//   k_mb_dw         depthwise 3x3, zero padding 1, stride 1 or 2 + bias + ReLU6: the unfused path
//                   and the operator the fused kernel is checked against; planes that fit are
//                   staged in LDS, several small planes to a block.
//   k_mb_expand_dw  relu6(dw3x3_s(relu6(W1 x + b1)) + b2) with the expanded activation held in LDS
//                   only.  A block owns a tile of output pixels and up to 128 mid channels.  Phase
//                   1: the expansion of the tile's input region (the tile plus its one-pixel halo,
//                   clipped to the image) on v_mfma_f32_32x32x2_f32, a wave per 32 channels x 32
//                   region pixels, operands straight from global memory as in k_pw (the pixel axis
//                   is contiguous), + b1, clamp, into LDS as float32.  Region positions outside
//                   the image are never computed: they are the depthwise filter's zero padding
//                   (0, not relu6(b1)) and are zero-filled.  Phase 2: the nine taps from LDS + b2,
//                   clamp, one store per output; 64, 32 or 16 lanes share a channel, whose taps
//                   stay in registers.  A plane whose padded region fits (480 positions) is one
//                   tile, so from the 16 x 8 planes down nothing is computed twice.  Blocks are 8
//                   waves (the two blocks whose LDS fits a CU keep 4 waves on every SIMD).
// NCHW planes, float32 or float16 storage, float32 arithmetic, no atomics.
#include <algorithm>

#include "by_storage.hpp"
#include "common.hpp"
#include "../../include/yolo_tracking_amd.h"

namespace yta {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float relu6(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

// ------------------------------------------------------------------------------------ k_mb_stem
constexpr int MS_TILE = 16, MS_IN = 2 * MS_TILE + 1;   // 33 input rows / columns per tile
constexpr int MS_CMAX = 64;
template <typename T>
__global__ __launch_bounds__(256) void k_mb_stem(const T *x, int H, int W, const float *w,
                                                 const float *b, int C0, T *y, int Ho, int Wo) {
    __shared__ float tile[3][MS_IN][MS_IN + 1];
    __shared__ __attribute__((aligned(16))) float swt[27 * MS_CMAX];   // [27][C0p], zero padded
    const int n = blockIdx.z, t = threadIdx.x;
    const int C0p = (C0 + 15) & ~15;
    const int oy0 = blockIdx.y * MS_TILE, ox0 = blockIdx.x * MS_TILE;
    const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;
    for (int i = t; i < 27 * C0p; i += 256) {
        const int k = i / C0p, co = i - k * C0p;
        swt[i] = co < C0 ? w[co * 27 + k] : 0.f;
    }
    for (int i = t; i < 3 * MS_IN * MS_IN; i += 256) {
        const int c = i / (MS_IN * MS_IN), rem = i - c * MS_IN * MS_IN;
        const int yy = rem / MS_IN, xx = rem - yy * MS_IN;
        const int gy = iy0 + yy, gx = ix0 + xx;
        tile[c][yy][xx] = gy >= 0 && gy < H && gx >= 0 && gx < W
                              ? (float)x[((long long)n * 3 + c) * H * W + (long long)gy * W + gx]
                              : 0.f;
    }
    __syncthreads();
    const int ty = t / MS_TILE, tx = t - ty * MS_TILE;
    const int oy = oy0 + ty, ox = ox0 + tx;
    const bool on = oy < Ho && ox < Wo;
    for (int cb = 0; cb < C0p; cb += 16) {   // block-uniform
        float acc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = cb + q < C0 ? b[cb + q] : 0.f;
#pragma unroll 1
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = tile[c][2 * ty + ky][2 * tx + kx];
                    const float4 *wk = reinterpret_cast<const float4 *>(
                        swt + (c * 9 + ky * 3 + kx) * C0p + cb);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 w4 = wk[q];
                        acc[4 * q] += w4.x * v;
                        acc[4 * q + 1] += w4.y * v;
                        acc[4 * q + 2] += w4.z * v;
                        acc[4 * q + 3] += w4.w * v;
                    }
                }
        if (on)
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (cb + q < C0)
                    y[(((long long)n * C0 + cb + q) * Ho + oy) * Wo + ox] = (T)relu6(acc[q]);
    }
}

// -------------------------------------------------------------------------------------- k_mb_dw
// A block takes ppb consecutive (sample, channel) planes (contiguous in memory).  LDS = true: the
// planes (together at most MD_PX elements) are staged with coalesced loads and every tap comes
// from LDS; otherwise (one larger plane per block) the taps are read from global memory.
constexpr int MD_T = 256, MD_PX = 4096;
template <typename T, bool LDS>
__global__ __launch_bounds__(MD_T) void k_mb_dw(const T *x, const float *w, const float *b, int C,
                                                int H, int W, int s, int Ho, int Wo, int ppb,
                                                long long planes, T *y) {
    __shared__ float in[LDS ? MD_PX : 1];
    const long long pl0 = (long long)blockIdx.x * ppb;
    const int np = (int)(planes - pl0 < ppb ? planes - pl0 : ppb);
    const int HW = H * W, P = Ho * Wo;
    const T *src = x + pl0 * HW;
    if (LDS) {
        for (int i = threadIdx.x; i < np * HW; i += MD_T) in[i] = (float)src[i];
        __syncthreads();
    }
    T *dst = y + pl0 * P;
    // a / d for a < 2^22 (the LDS path: np P <= MD_PX): (a + 0.5) / d rounds to the quotient
    const float inv_p = 1.0f / (float)P, inv_wo = 1.0f / (float)Wo, inv_c = 1.0f / (float)C;
    const int cb = (int)(pl0 % C);
    for (int i = threadIdx.x; i < np * P; i += MD_T) {
        const int j = LDS ? (int)(((float)i + 0.5f) * inv_p) : 0, q = i - j * P;
        const int oy = LDS ? (int)(((float)q + 0.5f) * inv_wo) : q / Wo, ox = q - oy * Wo;
        const int c = cb + j - C * (int)(((float)(cb + j) + 0.5f) * inv_c);
        const float *k = w + c * 9;
        float sum = 0.f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int yy = oy * s + dy - 1;
            if (yy < 0 || yy >= H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int xx = ox * s + dx - 1;
                if (xx < 0 || xx >= W) continue;
                const int at = j * HW + yy * W + xx;
                sum = fmaf(k[dy * 3 + dx], LDS ? in[at] : (float)src[at], sum);
            }
        }
        dst[i] = (T)relu6(sum + b[c]);
    }
}

// ------------------------------------------------------------------------------- k_mb_expand_dw
// v_mfma_f32_32x32x2_f32 operand maps as in k_pw: lane l holds A[l & 31][k = l >> 5] and
// B[k = l >> 5][l & 31]; D register q of lane l is row (q & 3) + 8 (q >> 2) + 4 (l >> 5), column
// l & 31.  A = W1 (k-major [Cin][Cmid]: lanes read along the mid channels), B = x.
constexpr int ME_T = 512;              // 8 waves share a block's LDS: two blocks keep 4 waves on every SIMD
constexpr int ME_KU = 8;              // k-steps (of 2) whose loads are issued together
constexpr int ME_REGION = 480;        // region positions (tile + halo) a block may hold
constexpr int ME_LDS_FLOATS = 16384;  // 64 KiB: e [CT * 32][PTS] + per channel nine taps, b2, b1
constexpr int ME_SW = 11;

struct me_geom {
    int Cin, Cmid, H, W, s, Ho, Wo;
    int TH, TW, IW, PTS, CT, tiles_x;
};

template <typename T>
__global__ __launch_bounds__(ME_T) void k_mb_expand_dw(const T *x, const float *w1,
                                                       const float *b1, const float *wd,
                                                       const float *b2, me_geom g, T *y) {
    extern __shared__ __attribute__((aligned(16))) float me_sm[];
    float *e = me_sm;                          // [CT * 32][PTS] expanded, clamped, float32
    float *sw = me_sm + g.CT * 32 * g.PTS;     // [CT * 32][11]: nine taps, b2, b1
    const int t = threadIdx.x, lane = lane_id(), wv = t / WAVE;
    const int r = lane & 31, h = lane >> 5;
    const int tyi = blockIdx.x / g.tiles_x, txi = blockIdx.x - tyi * g.tiles_x;
    const int c0 = blockIdx.y * g.CT * 32;
    const long long n = blockIdx.z;
    const int nch = min(g.CT * 32, g.Cmid - c0);
    const int oy0 = tyi * g.TH, ox0 = txi * g.TW;
    const int th = min(g.TH, g.Ho - oy0), tw = min(g.TW, g.Wo - ox0);
    const int iy0 = g.s * oy0 - 1, ix0 = g.s * ox0 - 1;
    const int ih = (th - 1) * g.s + 3, iw = (tw - 1) * g.s + 3;
    // the region clipped to the image: only these positions are expanded
    const int cy0 = max(iy0, 0), cy1 = min(iy0 + ih, g.H);
    const int cx0 = max(ix0, 0), cx1 = min(ix0 + iw, g.W);
    const int cw = cx1 - cx0, npix = (cy1 - cy0) * cw;
    if (npix != ih * iw)   // block-uniform: positions outside the image are the filter's zeros
        for (int i = t; i < nch * g.PTS; i += ME_T) e[i] = 0.f;
    for (int i = t; i < nch * ME_SW; i += ME_T) {
        const int cl = i / ME_SW, q = i - cl * ME_SW;
        sw[i] = q < 9 ? wd[(long long)(c0 + cl) * 9 + q] : (q == 9 ? b2 : b1)[c0 + cl];
    }
    __syncthreads();
    // ---- phase 1: e = relu6(W1 x + b1) on the clipped region
    const int ngrp = (npix + 31) / 32, ntile = (nch + 31) / 32;
    const long long HW = (long long)g.H * g.W;
    for (int item = wv; item < ngrp * ntile; item += ME_T / WAVE) {   // wave-uniform
        const int m = item / ngrp, grp = item - m * ngrp;
        const int p = grp * 32 + r;
        const bool p_ok = p < npix;
        const int py = p_ok ? p / cw : 0, px = p_ok ? p - py * cw : 0;
        const int gy = cy0 + py, gx = cx0 + px;
        const T *xp = x + n * g.Cin * HW + (long long)gy * g.W + gx;
        const int co = c0 + m * 32 + r;
        const bool co_ok = co < g.Cmid;
        const float *wp = w1 + (co_ok ? co : 0);
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        for (int k0 = 0; k0 < g.Cin; k0 += 2 * ME_KU) {
            float av[ME_KU], bv[ME_KU];
#pragma unroll
            for (int u = 0; u < ME_KU; ++u) {
                const int k = k0 + 2 * u + h;
                const bool k_ok = k < g.Cin;
                av[u] = co_ok && k_ok ? wp[(long long)k * g.Cmid] : 0.f;
                bv[u] = p_ok && k_ok ? (float)xp[k * HW] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < ME_KU; ++u)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
        }
        if (p_ok) {   // this lane's D column is region pixel p
            const int lp = (gy - iy0) * g.IW + (gx - ix0);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int cl = m * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (cl < nch) e[cl * g.PTS + lp] = relu6(acc[q] + sw[cl * ME_SW + 10]);
            }
        }
    }
    __syncthreads();
    // ---- phase 2: the nine taps from LDS.  G lanes share a channel (a wave takes 64 / G channels
    // at a time: small planes do not idle most of a wave); a lane keeps its channel's taps and
    // bias in registers over its pixels.  q / tw for q < 2^22: (q + 0.5) / tw rounds to the quotient.
    const int npx = th * tw;
    const int gs = npx > 32 ? 6 : (npx > 16 ? 5 : 4), G = 1 << gs;
    const int cpw = WAVE >> gs, sub = lane >> gs, li = lane & (G - 1);
    const float inv_tw = 1.0f / (float)tw;
    const int rs = g.s * g.IW;
    for (int cl = wv * cpw + sub; cl < nch; cl += (ME_T / WAVE) * cpw) {
        float k[10];
#pragma unroll
        for (int q = 0; q < 10; ++q) k[q] = sw[cl * ME_SW + q];
        const float *pl = e + cl * g.PTS;
        T *dst = y + ((n * g.Cmid + c0 + cl) * g.Ho + oy0) * g.Wo + ox0;
        for (int q = li; q < npx; q += G) {
            const int oy = (int)(((float)q + 0.5f) * inv_tw), ox = q - oy * tw;
            const float *p0 = pl + oy * rs + ox * g.s;
            float sum = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) sum = fmaf(k[dy * 3 + dx], p0[dy * g.IW + dx], sum);
            dst[oy * g.Wo + ox] = (T)relu6(sum + k[9]);
        }
    }
}

// Tile of output pixels: the whole plane where its padded region fits, otherwise up to 32 (stride
// 1) or 16 (stride 2) columns and as many rows as fit, both evened out over the plane.
void me_pick(me_geom &g) {
    const int s = g.s;
    auto region = [s](int th, int tw) { return ((th - 1) * s + 3) * ((tw - 1) * s + 3); };
    if (region(g.Ho, g.Wo) <= ME_REGION) {
        g.TH = g.Ho;
        g.TW = g.Wo;
    } else {
        const int twmax = std::min(g.Wo, s == 1 ? 32 : 16);
        const int nx = (g.Wo + twmax - 1) / twmax;
        g.TW = (g.Wo + nx - 1) / nx;
        const int iw = (g.TW - 1) * s + 3;
        const int thmax = std::min(g.Ho, std::max(1, (ME_REGION / iw - 3) / s + 1));
        const int ny = (g.Ho + thmax - 1) / thmax;
        g.TH = (g.Ho + ny - 1) / ny;
    }
    g.IW = (g.TW - 1) * s + 3;
    g.PTS = ((g.TH - 1) * s + 3) * g.IW;
    g.tiles_x = (g.Wo + g.TW - 1) / g.TW;
    g.CT = std::max(1, std::min({4, (g.Cmid + 31) / 32, ME_LDS_FLOATS / (32 * (g.PTS + ME_SW))}));
}

}  // namespace
}  // namespace yta

using namespace yta;

extern "C" {

int yta_mbv2_stem(const void *x, int N, int H, int W, const float *w, const float *b, int C0,
                  int half, void *y, void *stream) {
    YTA_CHECK(x && w && b && y && N > 0 && N <= 65535 && H > 0 && W > 0 && C0 > 0 &&
                  C0 <= MS_CMAX,
              YTA_ERR_INVALID, "bad MobileNetV2 stem arguments (C0 in 1..64)");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const dim3 g((Wo + MS_TILE - 1) / MS_TILE, (Ho + MS_TILE - 1) / MS_TILE, N);
    YTA_CHECK(g.y <= 65535, YTA_ERR_INVALID, "grid too large");
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_mb_stem<T>, g, dim3(256), 0, (hipStream_t)stream, (const T *)x, H, W,
                           w, b, C0, (T *)y, Ho, Wo);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_mbv2_dw3x3(const void *x, const float *w, const float *b, int N, int C, int H, int W,
                   int stride, int half, void *y, void *stream) {
    YTA_CHECK(x && w && b && y && N > 0 && C > 0 && H > 0 && W > 0 &&
                  (stride == 1 || stride == 2) && (long long)H * W <= 0x3fffffffLL,
              YTA_ERR_INVALID, "bad depthwise arguments (stride 1 or 2)");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long long planes = (long long)N * C;
    const bool lds = H * W <= MD_PX;
    const int ppb = lds ? (int)std::min<long long>(planes, MD_PX / (H * W)) : 1;
    const long long blocks = (planes + ppb - 1) / ppb;
    YTA_CHECK(blocks <= 0x7fffffffLL, YTA_ERR_INVALID, "grid too large");
    const dim3 g((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
#define YTA_MD_LAUNCH(L)                                                                        \
    hipLaunchKernelGGL((k_mb_dw<T, L>), g, dim3(MD_T), 0, st, (const T *)x, w, b, C, H, W,      \
                       stride, Ho, Wo, ppb, planes, (T *)y)
        if (lds) YTA_MD_LAUNCH(true);
        else YTA_MD_LAUNCH(false);
#undef YTA_MD_LAUNCH
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_mbv2_expand_dw(const void *x, const float *w1, const float *b1, const float *wdw,
                       const float *b2, int N, int Cin, int Cmid, int H, int W, int stride,
                       int half, void *y, void *stream) {
    YTA_CHECK(x && w1 && b1 && wdw && b2 && y && N > 0 && N <= 65535 && Cin > 0 && Cmid > 0 &&
                  H > 0 && W > 0 && (stride == 1 || stride == 2) &&
                  (long long)H * W <= 0x3fffffffLL,
              YTA_ERR_INVALID, "bad expand + depthwise arguments (stride 1 or 2)");
    me_geom g;
    g.Cin = Cin, g.Cmid = Cmid, g.H = H, g.W = W, g.s = stride;
    g.Ho = (H - 1) / stride + 1, g.Wo = (W - 1) / stride + 1;
    me_pick(g);
    const long long tiles = (long long)g.tiles_x * ((g.Ho + g.TH - 1) / g.TH);
    const int chunks = (Cmid + g.CT * 32 - 1) / (g.CT * 32);
    YTA_CHECK(tiles <= 0x7fffffffLL && chunks <= 65535, YTA_ERR_INVALID, "grid too large");
    const dim3 grid((unsigned)tiles, chunks, N);
    const size_t lds = sizeof(float) * g.CT * 32 * (g.PTS + ME_SW);
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_mb_expand_dw<T>, grid, dim3(ME_T), lds, st, (const T *)x, w1, b1, wdw,
                           b2, g, (T *)y);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

}  // extern "C"
