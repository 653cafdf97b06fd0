// CLIP-ReID ViT kernels on gfx950 (the ReID network of appearance/clip.py).
//
// Reference: boxmot/appearance/backbones/clip/clip/model.py VisionTransformer,
// ResidualAttentionBlock, LayerNorm, QuickGELU (:155-262) and make_model.py:96-122.  Activations are
// row-major (rows, channels) matrices, a token a row; every entry point takes its row strides in
// elements, so it reads or writes a subset of the rows (token 0 of every sample) or of the columns
// (a slot of a wider row) of a buffer.
//   k_linear     y = act(x w^T + bias) (+ res): an LDS-tiled MFMA GEMM.  A block of 4 waves owns a
//                128 x 128 tile of y, a wave 64 x 64 of it as 2 x 2 MFMA tiles of 32 x 32
//                (mfma_f32_32x32x16_f16 with float16 storage, mfma_f32_32x32x2f32 with float32:
//                64 accumulator registers).  x and w are both K-contiguous (w is [Nout][K], a
//                Linear's weight as stored), so both operand tiles are staged the same way: 16-byte
//                pieces global -> registers -> LDS, two LDS buffers, the loads of tile t + 1 issued
//                ahead of the MFMAs of tile t and written behind them, one barrier per tile.  The
//                LDS rows are 80 bytes in float16 (32 k + 8 of padding: a fragment, 8 consecutive
//                k, is one ds_read_b128, and 8 lanes' reads tile the 32 banks) and 17 words in
//                float32 (16 k + 1).  Rows, columns and k past the matrix are staged as zeros;
//                where K, a stride or an address is not a multiple of 16 bytes the pieces are
//                loaded element by element.  Epilogue in float32: + bias, QuickGELU, + res, one
//                rounding to the storage type.  res may be y (each element is read, then written,
//                by the same thread).
//   k_layernorm  (x - mean) / sqrt(var + eps) * gamma + beta over a row: one wave per row, the
//                mean first, then the variance around it (two passes, on the row shifted by its
//                first value), float32.
//   k_tokens     ln_pre(cat(class_embedding, patch rows) + positional_embedding): k_layernorm's
//                row routine on the sum.
//   k_patches    the 16 x 16 patches of NCHW crops as rows in (c, dy, dx) order: the patch
//                embedding is then k_linear with conv1.weight.reshape(width, 768).
//   k_attention  softmax(q k^T / 8) v per (sample, head): K and V of the head in LDS in the
//                storage type (rows padded by 16 bytes: a lane reads its key's row 16 bytes at a
//                time without bank conflicts), a block of 4 waves takes AT_QB queries, a wave one
//                query at a time: lane j scores keys j, j + 64, ... against the query (float32, in
//                LDS), the row maximum and sum are wave reductions, then lane d sums p_j V[j][d]
//                over the keys in order.  A query's result does not depend on which block or wave
//                computed it.  VALU arithmetic: at 129 tokens the two products are 3 % of a
//                block's multiply-adds.
// float32 or float16 storage, float32 arithmetic, no atomics.
#include <algorithm>

#include "by_storage.hpp"
#include "common.hpp"
#include "../../include/yolo_tracking_amd.h"

namespace yta {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------ k_linear
constexpr int LN_T = 256;          // 4 waves, 2 x 2 over the block's tile
constexpr int LN_BM = 128, LN_BN = 128;

template <typename T>
struct lin_cfg;
template <>
struct lin_cfg<_Float16> {
    static constexpr int BK = 32, E = 8, LS = 40;   // k per tile, elements per 16 bytes, LDS row
    typedef f16x8 piece;
};
template <>
struct lin_cfg<float> {
    static constexpr int BK = 16, E = 4, LS = 17;
    typedef f32x4 piece;
};

struct lin_args {
    const void *x, *w, *res;
    const float *bias;
    void *y;
    long long xs, ws, rs, ys;      // row strides in elements
    int M, K, N, act;
    int xvec, wvec;                // the operand can be loaded 16 bytes at a time
};

// One operand's pieces of a k tile: rows r0 .. r0 + 127 (of `rows`), k0 .. k0 + BK - 1.  A tile row
// is 4 pieces, the block's 256 threads take 2 pieces each.
template <typename T>
__device__ __forceinline__ void lin_load(const T *p, long long stride, int rows, int K, int r0,
                                         int k0, bool vec, typename lin_cfg<T>::piece (&v)[2]) {
    constexpr int E = lin_cfg<T>::E;
    typedef typename lin_cfg<T>::piece piece;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = threadIdx.x + i * LN_T, row = r0 + (c >> 2), k = k0 + (c & 3) * E;
        piece q;
#pragma unroll
        for (int e = 0; e < E; ++e) q[e] = (T)0.f;
        if (row < rows && k < K) {
            const T *src = p + (long long)row * stride + k;
            if (vec) {
                q = *reinterpret_cast<const piece *>(src);   // K is a multiple of E: all in range
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (k + e < K) q[e] = src[e];
            }
        }
        v[i] = q;
    }
}

template <typename T>
__device__ __forceinline__ void lin_store(T *s, const typename lin_cfg<T>::piece (&v)[2]) {
    constexpr int E = lin_cfg<T>::E, LS = lin_cfg<T>::LS;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = threadIdx.x + i * LN_T;
        T *d = s + (c >> 2) * LS + (c & 3) * E;
        if constexpr (sizeof(T) == 2) {
            *reinterpret_cast<typename lin_cfg<T>::piece *>(d) = v[i];   // 80-byte rows: aligned
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) d[e] = v[i][e];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(LN_T) void k_linear(lin_args a) {
    constexpr int BK = lin_cfg<T>::BK, LS = lin_cfg<T>::LS;
    typedef typename lin_cfg<T>::piece piece;
    __shared__ __attribute__((aligned(16))) T sm[2][2][LN_BM * LS];   // [buffer][x | w][row][k]
    const T *x = (const T *)a.x, *w = (const T *)a.w;
    const int m0 = blockIdx.y * LN_BM, n0 = blockIdx.x * LN_BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nk = (a.K + BK - 1) / BK;
    piece vx[2], vw[2];
    lin_load<T>(x, a.xs, a.M, a.K, m0, 0, a.xvec, vx);
    lin_load<T>(w, a.ws, a.N, a.K, n0, 0, a.wvec, vw);
    lin_store<T>(sm[0][0], vx);
    lin_store<T>(sm[0][1], vw);
    __syncthreads();
    for (int t = 0; t < nk; ++t) {                       // block-uniform
        const int cur = t & 1;
        if (t + 1 < nk) {
            lin_load<T>(x, a.xs, a.M, a.K, m0, (t + 1) * BK, a.xvec, vx);
            lin_load<T>(w, a.ws, a.N, a.K, n0, (t + 1) * BK, a.wvec, vw);
        }
        const T *sx = sm[cur][0] + (wm + r) * LS, *sw = sm[cur][1] + (wn + r) * LS;
        if constexpr (sizeof(T) == 2) {
            // lane (r, h) holds A[row r][k = 8 h + j] and B[k = 8 h + j][column r], j = 0 .. 7
#pragma unroll
            for (int ks = 0; ks < BK; ks += 16) {
                f16x8 fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = *reinterpret_cast<const f16x8 *>(sx + i * 32 * LS + ks + 8 * h);
                    fb[i] = *reinterpret_cast<const f16x8 *>(sw + i * 32 * LS + ks + 8 * h);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j],
                                                                           0, 0, 0);
            }
        } else {
            // lane (r, h) holds A[row r][k = h] and B[k = h][column r]
#pragma unroll
            for (int ks = 0; ks < BK; ks += 2) {
                float fa[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = sx[i * 32 * LS + ks + h];
                    fb[i] = sw[i * 32 * LS + ks + h];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j],
                                                                         0, 0, 0);
            }
        }
        if (t + 1 < nk) {
            lin_store<T>(sm[cur ^ 1][0], vx);
            lin_store<T>(sm[cur ^ 1][1], vw);
        }
        __syncthreads();
    }
    // accumulator register e of lane (r, h): row (e & 3) + 8 (e >> 2) + 4 h, column r
    const T *res = (const T *)a.res;
    T *y = (T *)a.y;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + j * 32 + r;
        if (n >= a.N) continue;
        const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (m >= a.M) continue;
                float v = acc[i][j][e] + b;
                if (a.act) v = v * (1.f / (1.f + expf(-1.702f * v)));
                if (res) v += (float)res[(long long)m * a.rs + n];
                y[(long long)m * a.ys + n] = (T)v;
            }
    }
}

// -------------------------------------------------------------------- k_layernorm, k_tokens
constexpr int LY_T = 256;          // 4 rows of a block, a wave each

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// One row by one wave: `at(c)` is the row's value at channel c.  Two passes over the row shifted
// by its first value (the differences of nearby floats are exact, so a row of 1000 + noise loses
// nothing to the offset and a constant row gives exactly beta): the mean of the shifted row, then
// the variance around it (biased, as nn.LayerNorm).
template <typename T, typename F>
__device__ __forceinline__ void ln_row(F at, int C, const float *gamma, const float *beta,
                                       float eps, T *y) {
    const int lane = threadIdx.x & 63;
    const float x0 = at(0);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += at(c) - x0;
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = (at(c) - x0) - mean;
        q += d * d;
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    for (int c = lane; c < C; c += 64)
        y[c] = (T)(((at(c) - x0) - mean) * rstd * gamma[c] + beta[c]);
}

template <typename T>
__global__ __launch_bounds__(LY_T) void k_layernorm(const T *x, long long xs, long long M, int C,
                                                    const float *gamma, const float *beta,
                                                    float eps, T *y, long long ys) {
    const long long row = (long long)blockIdx.x * (LY_T / 64) + (threadIdx.x >> 6);
    if (row >= M) return;          // wave-uniform
    const T *xr = x + row * xs;
    ln_row<T>([xr](int c) { return (float)xr[c]; }, C, gamma, beta, eps, y + row * ys);
}

template <typename T>
__global__ __launch_bounds__(LY_T) void k_tokens(const T *pe, long long ps, const float *cls,
                                                 const float *pos, long long N, int G, int C,
                                                 const float *gamma, const float *beta, float eps,
                                                 T *y) {
    const long long row = (long long)blockIdx.x * (LY_T / 64) + (threadIdx.x >> 6);
    const int L = G + 1;
    if (row >= N * L) return;      // wave-uniform
    const long long n = row / L;
    const int l = (int)(row - n * L);
    const float *pr = pos + (long long)l * C;
    if (l == 0) {
        ln_row<T>([cls, pr](int c) { return cls[c] + pr[c]; }, C, gamma, beta, eps, y + row * C);
    } else {
        const T *xr = pe + (n * G + l - 1) * ps;
        ln_row<T>([xr, pr](int c) { return (float)xr[c] + pr[c]; }, C, gamma, beta, eps,
                  y + row * C);
    }
}

// ----------------------------------------------------------------------------------- k_patches
template <typename T>
__global__ __launch_bounds__(256) void k_patches(const T *x, int H, int W, long long total, T *y) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int gw = W >> 4, gh = H >> 4;
    const int col = (int)(i % 768);
    const long long prow = i / 768;
    const int c = col >> 8, dy = (col >> 4) & 15, dx = col & 15;
    const int gx = (int)(prow % gw), gy = (int)((prow / gw) % gh);
    const long long n = prow / ((long long)gw * gh);
    y[i] = x[((n * 3 + c) * H + gy * 16 + dy) * W + gx * 16 + dx];
}

// --------------------------------------------------------------------------------- k_attention
constexpr int AT_T = 256;          // 4 waves
constexpr int AT_QB = 32;          // queries of a block, 8 per wave
constexpr int AT_D = 64;           // head dimension
constexpr int AT_LMAX = 256;       // keys: 4 per lane at most

template <typename T>
struct at_cfg;
template <>
struct at_cfg<float> {
    static constexpr int LS = 68, E = 4;    // row of K / V in elements (64 + 16 bytes), per 16 bytes
    typedef f32x4 piece;
};
template <>
struct at_cfg<_Float16> {
    static constexpr int LS = 72, E = 8;
    typedef f16x8 piece;
};

inline size_t at_lds_bytes(int L, int half) {
    const size_t kv = 2 * (size_t)L * (half ? at_cfg<_Float16>::LS * 2 : at_cfg<float>::LS * 4);
    return kv + (AT_T / 64) * (AT_D + AT_LMAX) * sizeof(float);
}

template <typename T>
__global__ __launch_bounds__(AT_T) void k_attention(const T *qkv, int L, int Lq, int width, T *y) {
    constexpr int LS = at_cfg<T>::LS, E = at_cfg<T>::E;
    typedef typename at_cfg<T>::piece piece;
    extern __shared__ __attribute__((aligned(16))) unsigned char at_sm[];
    T *sk = reinterpret_cast<T *>(at_sm);                    // [L][LS]
    T *sv = sk + (size_t)L * LS;                             // [L][LS]
    float *sq = reinterpret_cast<float *>(sv + (size_t)L * LS);   // [wave][64]
    float *sp = sq + (AT_T / 64) * AT_D;                     // [wave][AT_LMAX]
    const int head = blockIdx.y;
    const long long nb = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T *base = qkv + nb * L * 3 * width + head * AT_D;
    for (int i = threadIdx.x; i < L * AT_D; i += AT_T) {
        const int j = i >> 6, d = i & 63;
        const T *row = base + (long long)j * 3 * width;
        sk[j * LS + d] = row[width + d];
        sv[j * LS + d] = row[2 * width + d];
    }
    __syncthreads();
    float *q = sq + wave * AT_D, *p = sp + wave * AT_LMAX;
    const int q0 = blockIdx.x * AT_QB;
    for (int qi = q0 + wave; qi < min(q0 + AT_QB, Lq); qi += AT_T / 64) {   // wave-uniform
        q[lane] = (float)base[(long long)qi * 3 * width + lane] * 0.125f;   // q / 8: exact
        // a wave's LDS accesses complete in order: the barrier only keeps the compiler from moving
        // the other lanes' reads ahead of this write
        __builtin_amdgcn_wave_barrier();
        float sc[AT_LMAX / 64];
        float mx = -INFINITY;
#pragma unroll
        for (int g = 0; g < AT_LMAX / 64; ++g) {
            const int j = g * 64 + lane;
            sc[g] = -INFINITY;
            if (g * 64 < L) {                                // wave-uniform
                const T *kr = sk + (j < L ? j : 0) * LS;
                float s = 0.f;
#pragma unroll
                for (int d = 0; d < AT_D; d += E) {
                    const piece kk = *reinterpret_cast<const piece *>(kr + d);
#pragma unroll
                    for (int e = 0; e < E; ++e) s = fmaf(q[d + e], (float)kk[e], s);
                }
                if (j < L) sc[g] = s;
                mx = fmaxf(mx, sc[g]);
            }
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int g = 0; g < AT_LMAX / 64; ++g) {
            const int j = g * 64 + lane;
            if (g * 64 < L) {
                const float e = j < L ? expf(sc[g] - mx) : 0.f;
                if (j < L) p[j] = e;
                sum += e;
            }
        }
        const float inv = 1.f / wave_sum(sum);
        __builtin_amdgcn_wave_barrier();
        float o = 0.f;
        for (int j = 0; j < L; ++j) o = fmaf(p[j], (float)sv[j * LS + lane], o);
        y[(nb * Lq + qi) * width + head * AT_D + lane] = (T)(o * inv);
        __builtin_amdgcn_wave_barrier();   // the next query overwrites q and p
    }
}

template <typename T>
int linear_launch(const lin_args &a, hipStream_t st) {
    const dim3 g((unsigned)((a.N + LN_BN - 1) / LN_BN), (unsigned)((a.M + LN_BM - 1) / LN_BM));
    hipLaunchKernelGGL(k_linear<T>, g, dim3(LN_T), 0, st, a);
    return YTA_OK;
}

inline bool vec_ok(const void *p, long long stride, int K, int bytes) {
    const int E = 16 / bytes;
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && stride % E == 0 && K % E == 0;
}

}  // namespace
}  // namespace yta

using namespace yta;

extern "C" {

int yta_clip_linear(const void *x, long long x_stride, const void *w, long long w_stride,
                    const float *bias, const void *res, long long res_stride, int M, int K,
                    int Nout, int act, int half, void *y, long long y_stride, void *stream) {
    YTA_CHECK(x && w && y && M > 0 && K > 0 && Nout > 0 && (act == 0 || act == 1) &&
                  x_stride >= K && w_stride >= K && y_stride >= Nout &&
                  (!res || res_stride >= Nout),
              YTA_ERR_INVALID,
              "bad linear arguments (M, K, Nout > 0, act 0 or 1, strides at least a row)");
    YTA_CHECK((M + LN_BM - 1) / LN_BM <= 65535, YTA_ERR_INVALID, "too many rows for one launch");
    lin_args a;
    a.x = x, a.w = w, a.res = res, a.bias = bias, a.y = y;
    a.xs = x_stride, a.ws = w_stride, a.rs = res_stride, a.ys = y_stride;
    a.M = M, a.K = K, a.N = Nout, a.act = act;
    const int bytes = half ? 2 : 4;
    a.xvec = vec_ok(x, x_stride, K, bytes), a.wvec = vec_ok(w, w_stride, K, bytes);
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) { linear_launch<typename decltype(tag)::type>(a, st); });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_clip_layernorm(const void *x, long long x_stride, long long M, int C, const float *gamma,
                       const float *beta, float eps, int half, void *y, long long y_stride,
                       void *stream) {
    YTA_CHECK(x && y && gamma && beta && M > 0 && C > 0 && x_stride >= C && y_stride >= C &&
                  eps >= 0.f && (M + 3) / 4 <= 0x7fffffffLL,
              YTA_ERR_INVALID, "bad layer norm arguments (strides at least C)");
    const dim3 g((unsigned)((M + LY_T / 64 - 1) / (LY_T / 64)));
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_layernorm<T>, g, dim3(LY_T), 0, st, (const T *)x, x_stride, M, C,
                           gamma, beta, eps, (T *)y, y_stride);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_clip_patches(const void *x, int N, int H, int W, int half, void *y, void *stream) {
    YTA_CHECK(x && y && N > 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0, YTA_ERR_INVALID,
              "bad patch arguments (H and W multiples of 16)");
    const long long total = (long long)N * 3 * H * W, blocks = (total + 255) / 256;
    YTA_CHECK(blocks <= 0x7fffffffLL, YTA_ERR_INVALID, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_patches<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T *)x, H,
                           W, total, (T *)y);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_clip_tokens(const void *patches, long long patch_stride, const float *class_embedding,
                    const float *positional_embedding, int N, int G, int width,
                    const float *gamma, const float *beta, float eps, int half, void *y,
                    void *stream) {
    YTA_CHECK(patches && class_embedding && positional_embedding && gamma && beta && y && N > 0 &&
                  G > 0 && width > 0 && patch_stride >= width && eps >= 0.f,
              YTA_ERR_INVALID, "bad token arguments (patch stride at least width)");
    const long long rows = (long long)N * (G + 1), blocks = (rows + LY_T / 64 - 1) / (LY_T / 64);
    YTA_CHECK(blocks <= 0x7fffffffLL, YTA_ERR_INVALID, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_tokens<T>, dim3((unsigned)blocks), dim3(LY_T), 0, st,
                           (const T *)patches, patch_stride, class_embedding,
                           positional_embedding, (long long)N, G, width, gamma, beta, eps, (T *)y);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_clip_attention(const void *qkv, int N, int L, int width, int head_dim, int Lq, int half,
                       void *y, void *stream) {
    YTA_CHECK(qkv && y && N > 0 && N <= 65535 && L > 0 && width > 0 && Lq > 0 && Lq <= L,
              YTA_ERR_INVALID, "bad attention arguments (0 < Lq <= L, N <= 65535)");
    YTA_CHECK(head_dim == AT_D && width % AT_D == 0 && width / AT_D <= 65535, YTA_ERR_INVALID,
              "attention: the head dimension is 64 and divides width");
    YTA_CHECK(L <= AT_LMAX, YTA_ERR_INVALID, "attention: at most 256 tokens (K and V in LDS)");
    const size_t lds = at_lds_bytes(L, half);
    const dim3 g((unsigned)((Lq + AT_QB - 1) / AT_QB), (unsigned)(width / AT_D), (unsigned)N);
    hipStream_t st = (hipStream_t)stream;
    // the lambda returns the entry point's status: YTA_HIP leaves it on a failed attribute call
    return by_storage(half, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        if (lds > 65536)
            YTA_HIP(hipFuncSetAttribute((const void *)k_attention<T>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)at_lds_bytes(AT_LMAX, half)));
        hipLaunchKernelGGL(k_attention<T>, g, dim3(AT_T), lds, st, (const T *)qkv, L, Lq, width,
                           (T *)y);
        YTA_HIP(hipGetLastError());
        return YTA_OK;
    });
}

}  // extern "C"
