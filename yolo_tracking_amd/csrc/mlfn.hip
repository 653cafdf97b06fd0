// MLFN (Multi-Level Factorisation Net) kernels on gfx950 (the ReID network of appearance/mlfn.py).
//
// Reference: boxmot/appearance/backbones/mlfn.py MLFNBlock (1x1 reduce, grouped 3x3, factor
// selection, 1x1 recover, residual) and MLFN.forward.  BatchNorms arrive folded.  The 1x1 layers,
// the stem, the max pool and the global means are k_pw / k_stem / k_pool of osnet.hip.
//   k_gconv3x3   fm_conv2 + fm_bn2 + ReLU + the factor selection (mlfn.py:71-82): a grouped 3x3
//                convolution, zero padding 1, stride 1 or 2.  A block owns (sample, group, tile of
//                up to 16 x 16 output pixels).  The tile's input region with its halo (positions
//                outside the image zero-filled) and the group's weights are staged in LDS, up to
//                16 input channels at a time; a thread keeps R (4 or 8) output channels of one
//                pixel in registers, CS (1, 2 or 4) thread slots share a pixel, so a pass covers
//                CS * R <= 32 output channels of the group.  At MLFN's shapes (4 .. 32 channels
//                per group) that is one pass: every input value is read from memory once per
//                group and tile (halo excepted).  Weights sit in LDS as [ci][tap][CS * R] so that
//                a thread's R weights are one or two 16-byte reads, the same address for every
//                lane of a slot.  The block's LDS is sized by what the shape stages.  Epilogue:
//                + bias, ReLU, * scale[sample][group] (channel c belongs to group c / n, NOT
//                c % G).
//   k_fsm        MLFNBlock.fsm (mlfn.py:41-52) on the block input's plane means: three 1x1 layers
//                (ReLU, ReLU, sigmoid), FS_SB samples to a block so that a weight is read once
//                for FS_SB samples; weights k-major, lanes along the output channels, the k
//                range split over the rest of the block's 16 waves and summed in a fixed order.
//   k_subsample  x[:, :, ::s, ::s]: the plane gather ahead of the stride-2 1x1 downsample
//                (mlfn.py:57), which yta_pw_args' single pixel stride cannot express.
//   k_mean2      (a + b) * 0.5, mlfn.py:197.
// NCHW planes, float32 or float16 storage, float32 arithmetic, no atomics.
#include <algorithm>

#include "by_storage.hpp"
#include "common.hpp"
#include "../../include/yolo_tracking_amd.h"

namespace yta {
namespace {

// ---------------------------------------------------------------------------------- k_gconv3x3
constexpr int GC_T = 256;          // threads of the largest block
constexpr int GC_TILE = 16;        // output rows / columns of a tile at most
constexpr int GC_CI = 16;          // input channels staged together at most
constexpr int GC_IN = 6144;        // floats of staged input (24 KiB); 33 x 33 = 1089 per channel
constexpr int GC_COP = 32;         // output channels of a pass at most

struct gc_geom {
    int C, G, n, H, W, s, Ho, Wo;
    int TH, TW, IH, IW, tiles_x;
    int pxs_log2, cs_log2, CI;     // pixel slots and channel slots (powers of two), channel chunk
    int il_log2;                   // staging: lanes along the region's positions (the rest: channels)
    int in_floats;                 // staged input floats, a multiple of 4
    long long scale_stride;
};

template <typename T, int R>
__global__ __launch_bounds__(GC_T) void k_gconv3x3(const T *x, const float *w, const float *b,
                                                   const float *scale, gc_geom g, T *y) {
    extern __shared__ __attribute__((aligned(16))) float gc_sm[];
    float *sx = gc_sm;                       // [ci][IH][IW]
    float *sw = gc_sm + g.in_floats;         // [ci][tap][cop]
    const int t = threadIdx.x, nthr = blockDim.x;
    const int q = t & ((1 << g.pxs_log2) - 1), slot = t >> g.pxs_log2;
    const int tyi = blockIdx.x / g.tiles_x, txi = blockIdx.x - tyi * g.tiles_x;
    const int grp = blockIdx.y;
    const long long nb = blockIdx.z;
    const int oy0 = tyi * g.TH, ox0 = txi * g.TW;
    const int iy0 = g.s * oy0 - 1, ix0 = g.s * ox0 - 1;
    const int TP = g.TH * g.TW, qq = q < TP ? q : 0;
    const int ty = qq / g.TW, tx = qq - ty * g.TW;
    const int oy = oy0 + ty, ox = ox0 + tx;
    const bool on = q < TP && oy < g.Ho && ox < g.Wo;
    const int IP = g.IH * g.IW;
    const float *inp = sx + ty * g.s * g.IW + tx * g.s;
    const int cop_log2 = g.cs_log2 + (R == 8 ? 3 : 2), cop = 1 << cop_log2;
    const long long HW = (long long)g.H * g.W;
    const T *xg = x + (nb * g.C + (long long)grp * g.n) * HW;
    const int il = t & ((1 << g.il_log2) - 1), cl = t >> g.il_log2;
    const int IL = 1 << g.il_log2, CL = nthr >> g.il_log2;
    for (int co0 = 0; co0 < g.n; co0 += cop) {          // block-uniform: one pass for n <= CS * R
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        for (int ci0 = 0; ci0 < g.n; ci0 += g.CI) {     // block-uniform
            const int cic = min(g.CI, g.n - ci0);
            __syncthreads();
            // a position's offset is worked out once and serves the chunk's channels
            for (int i = il; i < IP; i += IL) {
                const int yy = i / g.IW, xx = i - yy * g.IW;
                const int gy = iy0 + yy, gx = ix0 + xx;
                const bool ok = gy >= 0 && gy < g.H && gx >= 0 && gx < g.W;
                const T *src = xg + ci0 * HW + (ok ? (long long)gy * g.W + gx : 0);
                for (int c = cl; c < cic; c += CL) sx[c * IP + i] = ok ? (float)src[c * HW] : 0.f;
            }
            const float *wg = w + (((long long)grp * g.n + co0) * g.n + ci0) * 9;
            for (int i = t; i < (cic * 9) << cop_log2; i += nthr) {
                const int co = i & (cop - 1), k = i >> cop_log2;      // k = c * 9 + tap
                sw[i] = co0 + co < g.n ? wg[(long long)co * g.n * 9 + k] : 0.f;
            }
            __syncthreads();
            for (int c = 0; c < cic; ++c) {
                const float *pl = inp + c * IP;
                const float *wc = sw + ((c * 9) << cop_log2) + slot * R;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const float v = pl[dy * g.IW + dx];
                        const float4 *wk =
                            reinterpret_cast<const float4 *>(wc + ((dy * 3 + dx) << cop_log2));
#pragma unroll
                        for (int r4 = 0; r4 < R / 4; ++r4) {
                            const float4 w4 = wk[r4];
                            acc[4 * r4] = fmaf(w4.x, v, acc[4 * r4]);
                            acc[4 * r4 + 1] = fmaf(w4.y, v, acc[4 * r4 + 1]);
                            acc[4 * r4 + 2] = fmaf(w4.z, v, acc[4 * r4 + 2]);
                            acc[4 * r4 + 3] = fmaf(w4.w, v, acc[4 * r4 + 3]);
                        }
                    }
            }
        }
        if (on) {
            const float sc = scale ? scale[nb * g.scale_stride + grp] : 1.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int ch = co0 + slot * R + r;
                if (ch >= g.n) continue;
                const long long cg = (long long)grp * g.n + ch;
                const float v = fmaxf(acc[r] + b[cg], 0.f) * sc;
                y[((nb * g.C + cg) * g.Ho + oy) * g.Wo + ox] = (T)v;
            }
        }
    }
}

inline int ceil_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// Tile: up to 16 x 16 output pixels, evened out over the plane; pixel slots = the next power of
// two (16 at least); channel slots (1, 2 or 4) fill the block up to 256 threads and 32 channels a
// pass.  Returns the block's LDS bytes: only what this shape stages, so that the small shapes
// keep many blocks on a CU.
template <int R>
size_t gc_pick(gc_geom &g) {
    const int nx = (g.Wo + GC_TILE - 1) / GC_TILE, ny = (g.Ho + GC_TILE - 1) / GC_TILE;
    g.TW = (g.Wo + nx - 1) / nx;
    g.TH = (g.Ho + ny - 1) / ny;
    g.tiles_x = nx;
    g.IH = (g.TH - 1) * g.s + 3;
    g.IW = (g.TW - 1) * g.s + 3;
    g.pxs_log2 = std::max(4, ceil_log2(g.TH * g.TW));
    const int cs = std::min({GC_T >> g.pxs_log2, 1 << ceil_log2((g.n + R - 1) / R), GC_COP / R});
    g.cs_log2 = ceil_log2(cs);                        // cs is a power of two
    g.CI = std::max(1, std::min({g.n, GC_CI, GC_IN / (g.IH * g.IW)}));
    g.il_log2 = std::min(g.pxs_log2 + g.cs_log2, ceil_log2(g.IH * g.IW));
    g.in_floats = (g.CI * g.IH * g.IW + 3) & ~3;
    return sizeof(float) * (size_t)(g.in_floats + g.CI * 9 * (R << g.cs_log2));
}

// ---------------------------------------------------------------------------------------- k_fsm
constexpr int FS_T = 1024;            // 16 waves: the layers are latency-bound reads of the weights
constexpr int FS_SB = 4;              // samples of a block
constexpr int FS_LDS_FLOATS = 16384;  // 64 KiB: FS_SB * (FS_T + cin + f0 + f1)

// One layer for the block's FS_SB samples: out[s][j] = act(bias[j] + sum_k w[k][j] in[s][k]).
// Thread (jl, kp) sums the k = kp, kp + KP, ... terms of output j (lanes along j: coalesced weight
// reads); the KP partial sums meet in LDS and are added in the order of kp.  LAST: sigmoid,
// rounded to T, to the selection buffers; otherwise ReLU into LDS.
template <typename T, bool LAST>
__device__ __forceinline__ void fs_layer(const float *in, int fin, const float *w,
                                         const float *bias, int fout, float *part, float *out,
                                         long long n0, int N, float *sel, long long sel_stride,
                                         T *sel_t, long long sel_t_stride) {
    const int t = threadIdx.x;
    int fp_log2 = 0;
    while ((1 << fp_log2) < fout && fp_log2 < 10) ++fp_log2;
    const int FP = 1 << fp_log2, KP = FS_T >> fp_log2;
    const int jl = t & (FP - 1), kp = t >> fp_log2;
    for (int j0 = 0; j0 < fout; j0 += FP) {      // block-uniform
        const int j = j0 + jl;
        float acc[FS_SB];
#pragma unroll
        for (int s = 0; s < FS_SB; ++s) acc[s] = 0.f;
        if (j < fout) {
#pragma unroll 4
            for (int k = kp; k < fin; k += KP) {
                const float wv = w[(long long)k * fout + j];
#pragma unroll
                for (int s = 0; s < FS_SB; ++s) acc[s] = fmaf(wv, in[s * fin + k], acc[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < FS_SB; ++s) part[((kp * FS_SB + s) << fp_log2) + jl] = acc[s];
        __syncthreads();
        for (int i = t; i < FS_SB << fp_log2; i += FS_T) {
            const int s = i >> fp_log2, j2 = j0 + (i & (FP - 1));
            if (j2 >= fout) continue;
            float v = bias[j2];
            for (int p = 0; p < KP; ++p) v += part[((p * FS_SB + s) << fp_log2) + (i & (FP - 1))];
            if (LAST) {
                if (n0 + s >= N) continue;
                const T r = (T)(1.f / (1.f + expf(-v)));   // rounded to the storage type once
                sel[(n0 + s) * sel_stride + j2] = (float)r;
                if (sel_t) sel_t[(n0 + s) * sel_t_stride + j2] = r;
            } else {
                out[s * fout + j2] = fmaxf(v, 0.f);
            }
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(FS_T) void k_fsm(const T *pooled, int N, int cin, int f0, int f1,
                                              int G, const float *w1, const float *b1,
                                              const float *w2, const float *b2, const float *w3,
                                              const float *b3, float *sel, long long sel_stride,
                                              T *sel_t, long long sel_t_stride) {
    extern __shared__ float fs_sm[];
    float *part = fs_sm;                   // [KP][FS_SB][FP]: FS_SB * FS_T
    float *a = part + FS_SB * FS_T;        // [FS_SB][cin]
    float *h0 = a + FS_SB * cin;           // [FS_SB][f0]
    float *h1 = h0 + FS_SB * f0;           // [FS_SB][f1]
    const long long n0 = (long long)blockIdx.x * FS_SB;
    for (int i = threadIdx.x; i < FS_SB * cin; i += FS_T) {
        const int s = i / cin;
        a[i] = n0 + s < N ? (float)pooled[n0 * cin + i] : 0.f;   // samples are contiguous
    }
    __syncthreads();
    fs_layer<T, false>(a, cin, w1, b1, f0, part, h0, n0, N, sel, sel_stride, sel_t, sel_t_stride);
    fs_layer<T, false>(h0, f0, w2, b2, f1, part, h1, n0, N, sel, sel_stride, sel_t, sel_t_stride);
    fs_layer<T, true>(h1, f1, w3, b3, G, part, nullptr, n0, N, sel, sel_stride, sel_t,
                      sel_t_stride);
}

// ------------------------------------------------------------------------- k_subsample, k_mean2
template <typename T>
__global__ __launch_bounds__(256) void k_subsample(const T *x, int H, int W, int s, int Ho, int Wo,
                                                   long long total, T *y) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long pl = i / (Ho * Wo);
    const int rem = (int)(i - pl * (Ho * Wo));
    const int oy = rem / Wo, ox = rem - oy * Wo;
    y[i] = x[pl * H * W + (long long)oy * s * W + ox * s];
}

template <typename T>
__global__ __launch_bounds__(256) void k_mean2(const T *a, const T *b, long long total, T *y) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) y[i] = (T)(((float)a[i] + (float)b[i]) * 0.5f);
}

template <typename T, int R>
void gc_launch(const void *x, const float *w, const float *b, const float *scale, gc_geom g,
               int N, void *y, hipStream_t st) {
    const size_t lds = gc_pick<R>(g);
    const int tiles = g.tiles_x * ((g.Ho + g.TH - 1) / g.TH);
    hipLaunchKernelGGL((k_gconv3x3<T, R>), dim3(tiles, g.G, N),
                       dim3(1 << (g.pxs_log2 + g.cs_log2)), lds, st, (const T *)x, w, b, scale, g,
                       (T *)y);
}

}  // namespace
}  // namespace yta

using namespace yta;

extern "C" {

int yta_mlfn_gconv3x3(const void *x, const float *w, const float *b, const float *scale,
                      long long scale_stride, int N, int C, int G, int H, int W, int stride,
                      int half, void *y, void *stream) {
    YTA_CHECK(x && w && b && y && N > 0 && N <= 65535 && C > 0 && G > 0 && G <= 65535 &&
                  C % G == 0 && H > 0 && W > 0 && (stride == 1 || stride == 2) &&
                  (long long)H * W <= 0x3fffffffLL && (!scale || scale_stride >= G),
              YTA_ERR_INVALID,
              "bad grouped 3x3 arguments (G divides C, stride 1 or 2, scale stride >= G)");
    gc_geom g;
    g.C = C, g.G = G, g.n = C / G, g.H = H, g.W = W, g.s = stride;
    g.Ho = (H - 1) / stride + 1, g.Wo = (W - 1) / stride + 1;
    g.scale_stride = scale_stride;
    YTA_CHECK((long long)((g.Wo + GC_TILE - 1) / GC_TILE) * ((g.Ho + GC_TILE - 1) / GC_TILE) <=
                  0x7fffffffLL,
              YTA_ERR_INVALID, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    const bool r4 = g.n <= 4;   // 4 accumulators where a group has no more channels
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (r4) gc_launch<T, 4>(x, w, b, scale, g, N, y, st);
        else gc_launch<T, 8>(x, w, b, scale, g, N, y, st);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_mlfn_fsm(const void *pooled, int N, int cin, int f0, int f1, int G, const float *w1,
                 const float *b1, const float *w2, const float *b2, const float *w3,
                 const float *b3, int half, float *sel, long long sel_stride, void *sel_t,
                 long long sel_t_stride, void *stream) {
    YTA_CHECK(pooled && w1 && b1 && w2 && b2 && w3 && b3 && sel && N > 0 && cin > 0 && f0 > 0 &&
                  f1 > 0 && G > 0 && sel_stride >= G && (!sel_t || sel_t_stride >= G),
              YTA_ERR_INVALID, "bad factor selection arguments (strides >= G)");
    const long long floats = (long long)FS_SB * ((long long)FS_T + cin + f0 + f1);
    YTA_CHECK(floats <= FS_LDS_FLOATS, YTA_ERR_INVALID,
              "factor selection layers too wide (cin + f0 + f1 <= 3072)");
    const dim3 g((unsigned)((N + FS_SB - 1) / FS_SB));
    const size_t lds = sizeof(float) * (size_t)floats;
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_fsm<T>, g, dim3(FS_T), lds, st, (const T *)pooled, N, cin, f0, f1, G,
                           w1, b1, w2, b2, w3, b3, sel, sel_stride, (T *)sel_t, sel_t_stride);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_mlfn_subsample(const void *x, int N, int C, int H, int W, int stride, int half, void *y,
                       void *stream) {
    YTA_CHECK(x && y && N > 0 && C > 0 && H > 0 && W > 0 && stride >= 1 &&
                  (long long)H * W <= 0x3fffffffLL,
              YTA_ERR_INVALID, "bad subsample arguments");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long long total = (long long)N * C * Ho * Wo, blocks = (total + 255) / 256;
    YTA_CHECK(blocks <= 0x7fffffffLL, YTA_ERR_INVALID, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_subsample<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T *)x,
                           H, W, stride, Ho, Wo, total, (T *)y);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_mlfn_mean2(const void *a, const void *b, long long count, int half, void *y,
                   void *stream) {
    YTA_CHECK(a && b && y && count > 0 && (count + 255) / 256 <= 0x7fffffffLL, YTA_ERR_INVALID,
              "bad mean arguments");
    const dim3 g((unsigned)((count + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_mean2<T>, g, dim3(256), 0, st, (const T *)a, (const T *)b, count,
                           (T *)y);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

}  // extern "C"
