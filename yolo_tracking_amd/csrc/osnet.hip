// OSNet omni-scale block kernels on gfx950 (the ReID network's forward).
//
// Reference: boxmot/appearance/backbones/osnet.py LightConv3x3 (depthwise 3x3 + BatchNorm + ReLU
// after the 1x1) and OSBlock.forward (x2 = gate(x2a) + gate(x2b) + gate(x2c) + gate(x2d), the
// ChannelGate's global average pool).  appearance/osnet.py runs the four branches batched and
// folds every BatchNorm; MIOpen has no fast depthwise path for these shapes (its naive kernel
// took 37 % of the forward), so the two bandwidth-bound steps are written here:
//   k_dw3x3    one (sample, channel) plane per block: depthwise 3x3 (zero padding 1) + bias +
//              ReLU, the output plane routed to one of two tensors (the branch that ends at this
//              depth goes into the block's branch stack, the rest feeds the next depth), and the
//              plane's sum for the channel gate's average pool (float32, block reduction);
//   k_gate_sum x2[n, c] = sum_b stack[n, b, c] * gate[n, b, c] over the four branches.
//   k_pw       every 1x1 convolution (conv1, the branches' pointwise layers, conv3 + downsample
//              + residual, the transition convs, conv5, the fc) as a GEMM on v_mfma_f32_32x32x2_f32:
//              one wave per 32 (output channels) x 32 (pixels) tile, operands straight from
//              global memory (the pixel axis is contiguous: B fragments are coalesced rows), groups,
//              a second input segment (the downsample branch joins conv3's sum), bias, identity
//              residual and ReLU (relu = 1), ReLU6 (relu = 2) or a ReLU on both sides of the
//              residual (relu = 3: MLFN's block end) fused in the epilogue;
//   k_stem     conv 7x7 stride 2 pad 3 (3 -> C0) + bias + ReLU, input tile + halo in LDS,
//              16 output channels per pass in registers, weights broadcast from LDS;
//   k_pool     max 3x3 stride 2 pad 1 / average 2x2 stride 2 / global mean (OSNet's pools);
//   k_gate     ChannelGate's two 1x1 layers on the pooled branch planes (fc1 + ReLU, fc2 +
//              sigmoid), one block per sample;
//   k_instnorm the instance norm of OSNet-IBN / OSNet-AIN (osnet_ain.py OSBlockINin): per-plane
//              statistics in two fixed-order passes over a plane held in LDS, affine, residual and
//              ReLU fused, or (the stem) + ReLU + the 3x3 max pool with only the pooled plane
//              written; k_instnorm_loop for planes that do not fit.
// NCHW planes, float32 or float16 storage, float32 arithmetic.
#include <algorithm>

#include "by_storage.hpp"
#include "common.hpp"
#include "../../include/yolo_tracking_amd.h"

namespace yta {
namespace {

constexpr int DW_T = 256;

template <typename T>
__device__ __forceinline__ float ld(const T *p) { return (float)*p; }

template <typename T>
__global__ __launch_bounds__(DW_T) void k_dw3x3(const T *x, long long xn, long long xc,
                                                 const float *w, const float *b, int C, int H,
                                                 int W, T *yf, long long yfn, int n_first, T *yr,
                                                 long long yrn, float *psum, long long psn) {
    __shared__ float red[DW_T / WAVE];
    const int c = blockIdx.x, n = blockIdx.y;
    const T *src = x + n * xn + c * xc;
    const bool first = c < n_first;
    T *dst = first ? yf + n * yfn + (long long)c * H * W
                   : yr + n * yrn + (long long)(c - n_first) * H * W;
    float k[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) k[q] = w[c * 9 + q];
    const float bias = b[c];
    float acc = 0.f;
    for (int i = threadIdx.x; i < H * W; i += DW_T) {
        const int y = i / W, xx = i - y * W;
        float s = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            const T *row = src + (long long)yy * W;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int xq = xx + dx;
                if (xq < 0 || xq >= W) continue;
                s += k[(dy + 1) * 3 + (dx + 1)] * ld(row + xq);
            }
        }
        const float v = fmaxf(s + bias, 0.f);
        const T o = (T)v;
        dst[i] = o;
        acc += (float)o;
    }
    if (first && psum) {   // the channel gate's average pool reads the stored values
        acc = (float)wave_reduce(RED_SUM, (double)acc);
        if (lane_id() == 0) red[threadIdx.x / WAVE] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int k2 = 0; k2 < DW_T / WAVE; ++k2) s += red[k2];
            psum[n * psn + c] = s;
        }
    }
}

// The same for planes that fit LDS: a block takes ppb consecutive planes of a sample (about 4096
// pixels together, so small late-stage planes do not leave most of a block idle), stages them in
// LDS with coalesced loads and computes every output from LDS; a first-branch plane's sum of its
// stored outputs is reduced in a fixed order (thread partials, waves, then wave 0: deterministic
// gate inputs).
constexpr int DW_LDS_PX = 4096;
template <typename T>
__global__ __launch_bounds__(DW_T) void k_dw3x3_lds(const T *x, long long xn, long long xc,
                                                     const float *w, const float *b, int C, int H,
                                                     int W, int ppb, T *yf, long long yfn,
                                                     int n_first, T *yr, long long yrn,
                                                     float *psum, long long psn) {
    __shared__ float in[DW_LDS_PX];
    __shared__ float red[DW_T / WAVE];
    const int n = blockIdx.y, c0 = blockIdx.x * ppb;
    const int np = C - c0 < ppb ? C - c0 : ppb;
    const int HW = H * W;
    const float invW = 1.0f / (float)W;   // q / W for q < 2^22: (q + 0.5) / W rounds to the quotient
    for (int j = 0; j < np; ++j) {
        const T *src = x + n * xn + (long long)(c0 + j) * xc;
        for (int q = threadIdx.x; q < HW; q += DW_T) in[j * HW + q] = (float)src[q];
    }
    __syncthreads();
    for (int j = 0; j < np; ++j) {
        const int c = c0 + j;
        const float *pl = in + j * HW;
        float k[9];
#pragma unroll
        for (int u = 0; u < 9; ++u) k[u] = w[c * 9 + u];
        const float bias = b[c];
        const bool first = c < n_first;
        T *dst = first ? yf + n * yfn + (long long)c * HW : yr + n * yrn + (long long)(c - n_first) * HW;
        float acc = 0.f;
        for (int q = threadIdx.x; q < HW; q += DW_T) {
            const int y = (int)(((float)q + 0.5f) * invW), xx = q - y * W;
            float s = 0.f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xq = xx + dx;
                    if (xq < 0 || xq >= W) continue;
                    s += k[(dy + 1) * 3 + (dx + 1)] * pl[yy * W + xq];
                }
            }
            const T o = (T)fmaxf(s + bias, 0.f);
            dst[q] = o;
            acc += (float)o;
        }
        if (first && psum) {   // block-uniform
            acc = (float)wave_reduce(RED_SUM, (double)acc);
            if (lane_id() == 0) red[threadIdx.x / WAVE] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                float t = 0.f;
                for (int u = 0; u < DW_T / WAVE; ++u) t += red[u];
                psum[n * psn + c] = t;
            }
            __syncthreads();
        }
    }
}

// x2[n][c][p] = sum_b stack[n][b][c][p] * gate[n][b][c]   (stack: N x 4 x C x P contiguous)
template <typename T>
__global__ __launch_bounds__(256) void k_gate_sum(const T *stack, const T *gate, int C, int P,
                                                  T *out) {
    const int c = blockIdx.x, n = blockIdx.y;
    const long long base = (long long)n * 4 * C;
    float g[4];
#pragma unroll
    for (int br = 0; br < 4; ++br) g[br] = (float)gate[base + br * C + c];
    const T *s0 = stack + (base + c) * P;
    const long long bs = (long long)C * P;
    T *o = out + ((long long)n * C + c) * P;
    for (int p = threadIdx.x; p < P; p += 256) {
        float v = 0.f;
#pragma unroll
        for (int br = 0; br < 4; ++br) v += (float)s0[br * bs + p] * g[br];
        o[p] = (T)v;
    }
}


// ---------------------------------------------------------------------------------------- k_pw
// D[co][p] = sum_k W[co][k] X[k][p] per (sample, group): A = W (f32, row-major [cout_g][K]),
// B = X.  v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][k = l >> 5] and B[k = l >> 5][l & 31];
// D register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31.
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int PW_T = 256;           // 4 waves: 32 channels x 128 pixels per block
constexpr int PW_KU = 8;            // k-steps (of 2) whose loads are issued together

// A wave computes MB 32 x 32 tiles (up to 128 output channels) for its 32 pixels, so each
// X element is read once per 128 output channels.
template <typename T, int MB>
__global__ __launch_bounds__(PW_T) void k_pw(yta_pw_args a) {
    const int lane = lane_id(), wv = threadIdx.x / WAVE;
    const int mt = (a.cout_g + 31) / 32, mg = (mt + MB - 1) / MB;
    const int g = blockIdx.y / mg, co0 = (blockIdx.y - g * mg) * MB * 32;
    const long long n = blockIdx.z;
    const int p0 = (blockIdx.x * (PW_T / WAVE) + wv) * 32;
    if (p0 >= a.P) return;                                   // wave-uniform
    const int K = a.k1 + a.k2;
    const int r = lane & 31, h = lane >> 5;
    const int p = p0 + r;
    const bool p_ok = p < a.P;
    const float *wg = a.w + (long long)g * K * a.cout_g;   // [K][cout_g]: lanes read along co
    bool co_ok[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) co_ok[m] = co0 + 32 * m + r < a.cout_g;
    const T *x1 = (const T *)a.x1 + n * a.x1n + (long long)g * a.k1 * a.x1c + (long long)(p_ok ? p : 0) * a.x1p;
    const T *x2 = a.x2 ? (const T *)a.x2 + n * a.x2n + (long long)(p_ok ? p : 0) * a.x2p : nullptr;
    f32x16 acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[m][q] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 2 * PW_KU) {
        float av[MB][PW_KU], bv[PW_KU];
#pragma unroll
        for (int u = 0; u < PW_KU; ++u) {
            const int k = k0 + 2 * u + h;
#pragma unroll
            for (int m = 0; m < MB; ++m)
                av[m][u] = co_ok[m] && k < K ? wg[(long long)k * a.cout_g + co0 + 32 * m + r] : 0.f;
            float b = 0.f;
            if (p_ok && k < a.k1) b = (float)x1[(long long)k * a.x1c];
            else if (p_ok && k < K) b = (float)x2[(long long)(k - a.k1) * a.x2c];
            bv[u] = b;
        }
#pragma unroll
        for (int u = 0; u < PW_KU; ++u)
#pragma unroll
            for (int m = 0; m < MB; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][u], bv[u], acc[m], 0, 0, 0);
    }
    T *y = (T *)a.y + n * a.yn;
    const T *res = a.res ? (const T *)a.res + n * a.rn : nullptr;
    if (!p_ok) return;   // this lane's D column is pixel p
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int c = co0 + 32 * m + (q & 3) + 8 * (q >> 2) + 4 * h;
            if (c >= a.cout_g) continue;
            const long long ch = (long long)g * a.cout_g + c;
            float v = acc[m][q];
            if (a.bias) v += a.bias[ch];
            if (a.relu == 3) v = fmaxf(v, 0.f);   // mlfn.py:87: the ReLU ahead of the residual
            if (res) v += (float)res[ch * a.rc + (long long)p * a.rp];
            if (a.relu) v = fmaxf(v, 0.f);
            if (a.relu == 2) v = fminf(v, 6.f);   // ReLU6 (MobileNetV2's ConvBlock)
            y[ch * a.yc + (long long)p * a.yp] = (T)v;
        }
}

// --------------------------------------------------------------------------------------- k_stem
// conv1 (osnet.py ConvLayer(3, C0, 7, stride=2, padding=3) + folded BatchNorm + ReLU): a block
// computes a 16 x 16 tile of output pixels; the input tile (3 x 37 x 37 with the halo) sits in
// LDS, each thread keeps the C0 (a multiple of 16, <= 64 per pass) accumulators of its pixel in
// registers and reads every input value once per pass, the weights being uniform across the block
// (scalar loads).  RELU = false: the convolution alone, for the variants whose stem is followed by
// an instance norm (the clamp belongs after the norm there).
constexpr int ST_TILE = 16, ST_IN = 2 * ST_TILE + 5;   // 37 input rows / columns per tile
template <typename T, int CB, bool RELU>
__global__ __launch_bounds__(256) void k_stem(const T *x, int H, int W, const float *w,
                                              const float *b, int C0, T *y, int Ho, int Wo) {
    __shared__ float tile[3][ST_IN][ST_IN + 1];
    extern __shared__ __attribute__((aligned(16))) float swt[];   // [147][C0]
    const int n = blockIdx.z, t = threadIdx.x;
    const int oy0 = blockIdx.y * ST_TILE, ox0 = blockIdx.x * ST_TILE;
    const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
    for (int i = t; i < 147 * C0; i += 256) {
        const int k = i / C0, co = i - k * C0;
        swt[i] = w[co * 147 + k];
    }
    for (int i = t; i < 3 * ST_IN * ST_IN; i += 256) {
        const int c = i / (ST_IN * ST_IN), rem = i - c * ST_IN * ST_IN;
        const int yy = rem / ST_IN, xx = rem - yy * ST_IN;
        const int gy = iy0 + yy, gx = ix0 + xx;
        tile[c][yy][xx] = gy >= 0 && gy < H && gx >= 0 && gx < W
                              ? (float)x[((long long)n * 3 + c) * H * W + (long long)gy * W + gx]
                              : 0.f;
    }
    __syncthreads();
    const int ty = t / ST_TILE, tx = t - ty * ST_TILE;
    const int oy = oy0 + ty, ox = ox0 + tx;
    const bool on = oy < Ho && ox < Wo;
    for (int cb = 0; cb < C0; cb += CB) {   // block-uniform
        float acc[CB];
#pragma unroll
        for (int q = 0; q < CB; ++q) acc[q] = b[cb + q];
#pragma unroll 1
        for (int c = 0; c < 3; ++c)
#pragma unroll 1
            for (int ky = 0; ky < 7; ++ky)
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const float v = tile[c][2 * ty + ky][2 * tx + kx];
                    const float4 *wk = reinterpret_cast<const float4 *>(
                        swt + (c * 49 + ky * 7 + kx) * C0 + cb);
#pragma unroll
                    for (int q = 0; q < CB / 4; ++q) {
                        const float4 w4 = wk[q];
                        acc[4 * q] += w4.x * v;
                        acc[4 * q + 1] += w4.y * v;
                        acc[4 * q + 2] += w4.z * v;
                        acc[4 * q + 3] += w4.w * v;
                    }
                }
        if (on)
#pragma unroll
            for (int q = 0; q < CB; ++q)
                y[(((long long)n * C0 + cb + q) * Ho + oy) * Wo + ox] =
                    (T)(RELU ? fmaxf(acc[q], 0.f) : acc[q]);
    }
}

// --------------------------------------------------------------------------------------- k_pool
// kind 0: max 3x3 stride 2 pad 1 (F.max_pool2d(x, 3, 2, 1)); 1: average 2x2 stride 2
// (F.avg_pool2d(x, 2, 2)); 2: mean over the plane -> y[n][c] (the global average pool, summed in
// float32).  One block per (sample, channel) plane.
template <typename T>
__global__ __launch_bounds__(256) void k_pool(const T *x, int C, int H, int W, int kind, T *y,
                                              int Ho, int Wo) {
    __shared__ float red[256 / WAVE];
    const int c = blockIdx.x, n = blockIdx.y;
    const T *src = x + ((long long)n * C + c) * H * W;
    if (kind == 2) {
        float s = 0.f;
        for (int i = threadIdx.x; i < H * W; i += 256) s += (float)src[i];
        s = (float)wave_reduce(RED_SUM, (double)s);
        if (lane_id() == 0) red[threadIdx.x / WAVE] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            float tot = 0.f;
            for (int k = 0; k < 256 / WAVE; ++k) tot += red[k];
            y[(long long)n * C + c] = (T)(tot / (float)(H * W));
        }
        return;
    }
    T *dst = y + ((long long)n * C + c) * Ho * Wo;
    for (int i = threadIdx.x; i < Ho * Wo; i += 256) {
        const int oy = i / Wo, ox = i - oy * Wo;
        float v;
        if (kind == 0) {
            v = -INFINITY;
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = 2 * oy + dy;
                if (yy < 0 || yy >= H) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = 2 * ox + dx;
                    if (xx < 0 || xx >= W) continue;
                    v = fmaxf(v, (float)src[yy * W + xx]);
                }
            }
        } else {
            const T *q = src + 2 * oy * W + 2 * ox;
            v = (((float)q[0] + (float)q[1]) + ((float)q[W] + (float)q[W + 1])) * 0.25f;
        }
        dst[i] = (T)v;
    }
}

// ------------------------------------------------------------------------------------ k_instnorm
// nn.InstanceNorm2d(affine=True) in eval mode (osnet.py ConvLayer(IN=True) / OSBlock.IN,
// osnet_ain.py OSBlockINin.IN): no running statistics, so every (sample, channel) plane is
// normalised by its own mean and biased variance (eps 1e-5), then gamma[c] x_hat + beta[c], with
// the AIN residual and the ReLU fused.  The statistics cannot be folded into a convolution and are
// not accumulated across blocks: GS threads own a plane (16 or 64 lanes of a wave for the small
// late-stage planes, so a block takes 16 or 4 of them; the whole block up to IN_RESIDENT_PX
// pixels), read it from HBM once into LDS as float32 (16-byte loads where the planes are aligned)
// and make both statistic passes and the write from there.  Two passes, no E[x^2] - mean^2: the
// mean m0 first (clamped into the plane's [min, max], which makes a constant plane exact), then
// s1 = sum(x - m0) and s2 = sum((x - m0)^2) together; s1 / P corrects the float32 mean to first
// order and var = s2 / P - (s1 / P)^2.  Every sum runs in a fixed order (a thread's strided
// elements, xor butterflies inside the wave, the four waves' partials in wave order), without
// atomics: the same input gives the same bits.
constexpr int IN_T = 256;
constexpr int IN_RESIDENT_PX = 8192;   // 32 KiB of LDS: the x1_0 stem plane at 256 x 128 crops
constexpr float IN_EPS = 1e-5f;
enum { IN_SUM = 0, IN_MIN = 1, IN_MAX = 2 };

template <typename T, int V>
struct alignas(sizeof(T) * V) in_vec { T v[V]; };

template <int OP>
__device__ __forceinline__ float in_op(float a, float b) {
    return OP == IN_SUM ? a + b : (OP == IN_MIN ? fminf(a, b) : fmaxf(a, b));
}

// Over the GS lanes of a wave that own a plane (the whole wave for GS = 256): every lane gets the
// same value.
template <int GS, int OP>
__device__ __forceinline__ float in_lanes(float v) {
#pragma unroll
    for (int m = 1; m < (GS < WAVE ? GS : WAVE); m <<= 1) v = in_op<OP>(v, __shfl_xor(v, m, WAVE));
    return v;
}

// The statistics of the plane `get(i)`, i < P, for the GS threads that own it (t: the thread's
// index among them); red: 5 x 4 floats of LDS for the block-wide case.  Block-uniform control
// flow (a group without a plane passes live = false and still meets the barriers); the first
// barrier also publishes what `get` left in LDS during the first pass.
template <int GS, typename Get1, typename Get2>
__device__ __forceinline__ void in_stats(int P, int t, bool live, float (*red)[IN_T / WAVE],
                                         Get1 first_pass, Get2 get, float *mean0, float *dmean,
                                         float *inv_std) {
    const int wv = threadIdx.x / WAVE;
    float s = 0.f, lo = INFINITY, hi = -INFINITY;
    if (live) first_pass(s, lo, hi);
    s = in_lanes<GS, IN_SUM>(s);
    lo = in_lanes<GS, IN_MIN>(lo);
    hi = in_lanes<GS, IN_MAX>(hi);
    if (GS == IN_T && lane_id() == 0) { red[0][wv] = s; red[1][wv] = lo; red[2][wv] = hi; }
    __syncthreads();
    if (GS == IN_T) {
        s = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        lo = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
        hi = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    }
    const float m0 = fminf(fmaxf(s / (float)P, lo), hi);
    float s1 = 0.f, s2 = 0.f;
    if (live)
        for (int i = t; i < P; i += GS) {
            const float d = get(i) - m0;
            s1 += d;
            s2 += d * d;
        }
    s1 = in_lanes<GS, IN_SUM>(s1);
    s2 = in_lanes<GS, IN_SUM>(s2);
    if (GS == IN_T) {
        if (lane_id() == 0) { red[3][wv] = s1; red[4][wv] = s2; }
        __syncthreads();
        s1 = ((red[3][0] + red[3][1]) + red[3][2]) + red[3][3];
        s2 = ((red[4][0] + red[4][1]) + red[4][2]) + red[4][3];
    }
    const float dm = s1 / (float)P;
    const float var = fmaxf(s2 / (float)P - dm * dm, 0.f);
    *mean0 = m0;
    *dmean = dm;
    *inv_std = 1.0f / sqrtf(var + IN_EPS);
}

// Resident planes (P <= IN_RESIDENT_PX): block b owns planes b * (IN_T / GS) ... of the N * C,
// each in its own (P rounded up to 4) floats of dynamic LDS.  POOL: only max_pool2d(3, 2, 1) of
// the normalised plane + ReLU is written, straight from the plane in LDS (the stem: the network's
// largest activation is neither written nor read back).
template <typename T, int GS, bool POOL>
__global__ __launch_bounds__(IN_T) void k_instnorm(const T *x, const T *res, const float *gamma,
                                                   const float *beta, long long planes, int C,
                                                   int P, int vec, int relu, T *y, int H, int W,
                                                   int Ho, int Wo) {
    extern __shared__ __attribute__((aligned(16))) float in_lds[];
    __shared__ float red[5][IN_T / WAVE];
    constexpr int V = 16 / sizeof(T);
    const int g = threadIdx.x / GS, t = threadIdx.x - g * GS;
    const long long pl = (long long)blockIdx.x * (IN_T / GS) + g;
    const bool live = pl < planes;
    float *buf = in_lds + g * ((P + 3) & ~3);
    const T *src = x + pl * P;
    float m0, dm, inv;
    in_stats<GS>(
        P, t, live, red,
        [&](float &s, float &lo, float &hi) {
            if (vec) {
#pragma unroll 4
                for (int i = t * V; i < P; i += GS * V) {
                    const in_vec<T, V> q = *reinterpret_cast<const in_vec<T, V> *>(src + i);
                    float f[V];
#pragma unroll
                    for (int u = 0; u < V; ++u) {
                        f[u] = (float)q.v[u];
                        s += f[u];
                        lo = fminf(lo, f[u]);
                        hi = fmaxf(hi, f[u]);
                    }
#pragma unroll
                    for (int u = 0; u < V; u += 4)
                        *reinterpret_cast<float4 *>(buf + i + u) =
                            make_float4(f[u], f[u + 1], f[u + 2], f[u + 3]);
                }
            } else {
                for (int i = t; i < P; i += GS) {
                    const float f = (float)src[i];
                    buf[i] = f;
                    s += f;
                    lo = fminf(lo, f);
                    hi = fmaxf(hi, f);
                }
            }
        },
        [&](int i) { return buf[i]; }, &m0, &dm, &inv);
    const int c = (int)(pl % C);
    const float sc = live ? gamma[c] * inv : 0.f, bt = live ? beta[c] : 0.f;
    if (POOL) {
        // f(x) = relu(((x - m0) - dm) * sc + bt) is monotone in x, every rounding included (rising
        // for sc >= 0, falling for a negative gamma), so the window's maximum of f is f of the
        // window's largest (smallest) input: one affine step per output, and the plane in LDS is
        // only read.  Taps outside the plane are clamped onto it: a repeated tap changes neither
        // maximum nor minimum.
        if (!live) return;
        T *dst = y + pl * Ho * Wo;
        const float invWo = 1.0f / (float)Wo;   // i / Wo for i < 2^22, as in k_dw3x3_lds
        for (int i = t; i < Ho * Wo; i += GS) {
            const int oy = (int)(((float)i + 0.5f) * invWo), ox = i - oy * Wo;
            const int x1 = 2 * ox, x0 = x1 > 0 ? x1 - 1 : 0, x2 = x1 + 1 < W ? x1 + 1 : W - 1;
            const float *r1 = buf + 2 * oy * W, *r0 = oy > 0 ? r1 - W : r1,
                        *r2 = 2 * oy + 1 < H ? r1 + W : r1;
            const float a[9] = {r0[x0], r0[x1], r0[x2], r1[x0], r1[x1], r1[x2],
                                r2[x0], r2[x1], r2[x2]};
            float mx = a[0], mn = a[0];
#pragma unroll
            for (int u = 1; u < 9; ++u) {
                mx = fmaxf(mx, a[u]);
                mn = fminf(mn, a[u]);
            }
            dst[i] = (T)fmaxf((((sc >= 0.f ? mx : mn) - m0) - dm) * sc + bt, 0.f);
        }
        return;
    }
    if (!live) return;
    T *dst = y + pl * P;
    const T *rs = res ? res + pl * P : nullptr;
    if (vec) {
#pragma unroll 2
        for (int i = t * V; i < P; i += GS * V) {
            in_vec<T, V> r, o;
            if (rs) r = *reinterpret_cast<const in_vec<T, V> *>(rs + i);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                float v = ((buf[i + u] - m0) - dm) * sc + bt;
                if (rs) v += (float)r.v[u];
                if (relu) v = fmaxf(v, 0.f);
                o.v[u] = (T)v;
            }
            *reinterpret_cast<in_vec<T, V> *>(dst + i) = o;
        }
    } else {
        for (int i = t; i < P; i += GS) {
            float v = ((buf[i] - m0) - dm) * sc + bt;
            if (rs) v += (float)rs[i];
            if (relu) v = fmaxf(v, 0.f);
            dst[i] = (T)v;
        }
    }
}

// Planes over IN_RESIDENT_PX: one block per plane, the same arithmetic with the plane read from
// global memory in each of the three passes.
template <typename T>
__global__ __launch_bounds__(IN_T) void k_instnorm_loop(const T *x, const T *res,
                                                        const float *gamma, const float *beta,
                                                        int C, int P, int relu, T *y) {
    __shared__ float red[5][IN_T / WAVE];
    const int t = threadIdx.x;
    const long long pl = blockIdx.x;
    const T *src = x + pl * P;
    float m0, dm, inv;
    in_stats<IN_T>(
        P, t, true, red,
        [&](float &s, float &lo, float &hi) {
            for (int i = t; i < P; i += IN_T) {
                const float f = (float)src[i];
                s += f;
                lo = fminf(lo, f);
                hi = fmaxf(hi, f);
            }
        },
        [&](int i) { return (float)src[i]; }, &m0, &dm, &inv);
    const int c = (int)(pl % C);
    const float sc = gamma[c] * inv, bt = beta[c];
    T *dst = y + pl * P;
    const T *rs = res ? res + pl * P : nullptr;
    for (int i = t; i < P; i += IN_T) {
        float v = (((float)src[i] - m0) - dm) * sc + bt;
        if (rs) v += (float)rs[i];
        if (relu) v = fmaxf(v, 0.f);
        dst[i] = (T)v;
    }
}

// --------------------------------------------------------------------------------------- k_gate
// ChannelGate (osnet.py): pooled = plane sums / P (rounded to T, as the graph's .to(dtype)),
// hidden = relu(W1 pooled + b1), gate = sigmoid(W2 hidden + b2), for the four branches of a
// sample.  Block per sample; mid <= 512, hid <= 64.
template <typename T>
__global__ __launch_bounds__(256) void k_gate(const float *psum, float inv_p, const T *w1,
                                              const T *b1, const T *w2, const T *b2, int mid,
                                              int hid, T *gate) {
    __shared__ float pooled[4 * 512];
    __shared__ float hidden[4 * 64];
    const int n = blockIdx.x;
    for (int i = threadIdx.x; i < 4 * mid; i += 256)
        pooled[i] = (float)(T)(psum[(long long)n * 4 * mid + i] * inv_p);
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * hid; i += 256) {
        const int br = i / hid, j = i - br * hid;
        float s = (float)b1[j];
        for (int k = 0; k < mid; ++k) s += (float)w1[j * mid + k] * pooled[br * mid + k];
        hidden[i] = (float)(T)fmaxf((float)(T)s, 0.f);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * mid; i += 256) {
        const int br = i / mid, c = i - br * mid;
        float s = (float)b2[c];
        for (int j = 0; j < hid; ++j) s += (float)w2[c * hid + j] * hidden[br * hid + j];
        s = (float)(T)s;
        gate[(long long)n * 4 * mid + i] = (T)(1.f / (1.f + expf(-s)));
    }
}
}  // namespace
}  // namespace yta

using namespace yta;

template <bool RELU>
static int stem_launch(const void *x, int N, int H, int W, const float *w, const float *b, int C0,
                       int half, void *y, void *stream) {
    YTA_CHECK(x && w && b && y && N > 0 && H > 0 && W > 0 && C0 > 0 && C0 % 16 == 0,
              YTA_ERR_INVALID, "bad stem arguments (C0 a multiple of 16)");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const dim3 g((Wo + ST_TILE - 1) / ST_TILE, (Ho + ST_TILE - 1) / ST_TILE, N);
    const size_t lds = sizeof(float) * 147 * C0;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((k_stem<T, 16, RELU>), g, dim3(256), lds, (hipStream_t)stream,
                           (const T *)x, H, W, w, b, C0, (T *)y, Ho, Wo);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

// Threads per plane by plane size: 16 lanes up to 128 pixels (the 16 x 8 planes of stage 4 and
// below), a wave up to 512 (stage 3), the block beyond.
template <typename T, bool POOL>
static void instnorm_launch(const void *x, const void *res, const float *gamma, const float *beta,
                            long long planes, int C, int P, int relu, void *y, int H, int W,
                            hipStream_t st) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int V = 16 / (int)sizeof(T);
    const bool al = ((uintptr_t)x | (POOL ? 0 : (uintptr_t)y) | (uintptr_t)res) % 16 == 0;
    const int vec = al && P % V == 0;
    const int gs = P <= 128 ? 16 : (P <= 512 ? 64 : IN_T), ppb = IN_T / gs;
    const dim3 g((unsigned)((planes + ppb - 1) / ppb));
    const size_t lds = sizeof(float) * ppb * ((P + 3) & ~3);
#define YTA_IN_LAUNCH(GS)                                                                       \
    hipLaunchKernelGGL((k_instnorm<T, GS, POOL>), g, dim3(IN_T), lds, st, (const T *)x,         \
                       (const T *)res, gamma, beta, planes, C, P, vec, relu, (T *)y, H, W, Ho,  \
                       Wo)
    if (gs == 16) YTA_IN_LAUNCH(16);
    else if (gs == 64) YTA_IN_LAUNCH(64);
    else YTA_IN_LAUNCH(IN_T);
#undef YTA_IN_LAUNCH
}

extern "C" {

int yta_osnet_dw3x3(const void *x, long long x_n_stride, long long x_c_stride, const float *w,
                    const float *b, int N, int C, int H, int W, int half, void *y_first,
                    long long yf_n_stride, int n_first, void *y_rest, long long yr_n_stride,
                    float *plane_sum, long long ps_n_stride, void *stream) {
    YTA_CHECK(x && w && b && N > 0 && C > 0 && H > 0 && W > 0 && n_first >= 0 && n_first <= C,
              YTA_ERR_INVALID, "bad argument");
    YTA_CHECK((n_first == 0 || y_first) && (n_first == C || y_rest), YTA_ERR_INVALID,
              "null output");
    if (H * W <= DW_LDS_PX) {
        const int ppb = std::max(1, std::min(C, DW_LDS_PX / (H * W)));
        const dim3 gl((C + ppb - 1) / ppb, N);
        by_storage(half, [&](auto tag) {
            using T = typename decltype(tag)::type;
            hipLaunchKernelGGL(k_dw3x3_lds<T>, gl, dim3(DW_T), 0, (hipStream_t)stream,
                               (const T *)x, x_n_stride, x_c_stride, w, b, C, H, W, ppb,
                               (T *)y_first, yf_n_stride, n_first, (T *)y_rest, yr_n_stride,
                               plane_sum, ps_n_stride);
        });
        YTA_HIP(hipGetLastError());
        return YTA_OK;
    }
    const dim3 g(C, N);
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_dw3x3<T>, g, dim3(DW_T), 0, (hipStream_t)stream, (const T *)x,
                           x_n_stride, x_c_stride, w, b, C, H, W, (T *)y_first, yf_n_stride,
                           n_first, (T *)y_rest, yr_n_stride, plane_sum, ps_n_stride);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_osnet_gate_sum(const void *stack, const void *gate, int N, int C, int P, int half,
                       void *out, void *stream) {
    YTA_CHECK(stack && gate && out && N > 0 && C > 0 && P > 0, YTA_ERR_INVALID, "bad argument");
    const dim3 g(C, N);
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_gate_sum<T>, g, dim3(256), 0, (hipStream_t)stream, (const T *)stack,
                           (const T *)gate, C, P, (T *)out);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_osnet_pointwise(const yta_pw_args *args, int half, void *stream) {
    YTA_CHECK(args, YTA_ERR_INVALID, "null argument");
    const yta_pw_args &a = *args;
    YTA_CHECK(a.x1 && a.w && a.y && a.G > 0 && a.cout_g > 0 && a.k1 >= 0 && a.k2 >= 0 &&
                  a.k1 + a.k2 > 0 && a.P > 0 && a.N > 0 && (a.k2 == 0 || a.x2),
              YTA_ERR_INVALID, "bad pointwise arguments");
    const int mt = (a.cout_g + 31) / 32, MB = mt >= 3 ? 4 : mt;
    const dim3 g((a.P + 32 * (PW_T / WAVE) - 1) / (32 * (PW_T / WAVE)),
                 a.G * ((mt + MB - 1) / MB), a.N);
    YTA_CHECK(g.y <= 65535 && g.z <= 65535, YTA_ERR_INVALID, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (MB == 1) hipLaunchKernelGGL((k_pw<T, 1>), g, dim3(PW_T), 0, st, a);
        else if (MB == 2) hipLaunchKernelGGL((k_pw<T, 2>), g, dim3(PW_T), 0, st, a);
        else hipLaunchKernelGGL((k_pw<T, 4>), g, dim3(PW_T), 0, st, a);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_osnet_stem(const void *x, int N, int H, int W, const float *w, const float *b, int C0,
                   int half, void *y, void *stream) {
    return stem_launch<true>(x, N, H, W, w, b, C0, half, y, stream);
}

int yta_osnet_stem_linear(const void *x, int N, int H, int W, const float *w, const float *b,
                          int C0, int half, void *y, void *stream) {
    return stem_launch<false>(x, N, H, W, w, b, C0, half, y, stream);
}

int yta_osnet_instnorm_resident(void) { return IN_RESIDENT_PX; }

int yta_osnet_instnorm(const void *x, const void *res, const float *gamma, const float *beta,
                       int N, int C, int P, int relu, int half, void *y, void *stream) {
    YTA_CHECK(x && gamma && beta && y && N > 0 && C > 0 && P > 0, YTA_ERR_INVALID,
              "bad instance norm arguments");
    const long long planes = (long long)N * C;
    YTA_CHECK(planes <= 0x7fffffffLL, YTA_ERR_INVALID, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        if (P <= IN_RESIDENT_PX)
            instnorm_launch<T, false>(x, res, gamma, beta, planes, C, P, relu, y, 1, P, st);
        else
            hipLaunchKernelGGL(k_instnorm_loop<T>, dim3((unsigned)planes), dim3(IN_T), 0, st,
                               (const T *)x, (const T *)res, gamma, beta, C, P, relu, (T *)y);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_osnet_instnorm_maxpool(const void *x, const float *gamma, const float *beta, int N, int C,
                               int H, int W, int half, void *work, void *y, void *stream) {
    YTA_CHECK(x && gamma && beta && y && N > 0 && C > 0 && H > 0 && W > 0 &&
                  (long long)H * W <= 0x7fffffffLL,
              YTA_ERR_INVALID, "bad instance norm arguments");
    const long long planes = (long long)N * C;
    YTA_CHECK(planes <= 0x7fffffffLL, YTA_ERR_INVALID, "grid too large");
    const int P = H * W;
    if (P > IN_RESIDENT_PX) {
        YTA_CHECK(work, YTA_ERR_INVALID, "plane over the resident bound: work must hold the input");
        const int rc = yta_osnet_instnorm(x, nullptr, gamma, beta, N, C, P, 1, half, work, stream);
        return rc != YTA_OK ? rc : yta_osnet_pool(work, N, C, H, W, 0, half, y, stream);
    }
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        instnorm_launch<T, true>(x, nullptr, gamma, beta, planes, C, P, 1, y, H, W, st);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_osnet_pool(const void *x, int N, int C, int H, int W, int kind, int half, void *y,
                   void *stream) {
    YTA_CHECK(x && y && N > 0 && C > 0 && H > 0 && W > 0 && kind >= 0 && kind <= 2,
              YTA_ERR_INVALID, "bad pool arguments");
    const int Ho = kind == 0 ? (H - 1) / 2 + 1 : H / 2, Wo = kind == 0 ? (W - 1) / 2 + 1 : W / 2;
    YTA_CHECK(kind == 2 || (Ho > 0 && Wo > 0), YTA_ERR_INVALID, "plane too small");
    const dim3 g(C, N);
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_pool<T>, g, dim3(256), 0, (hipStream_t)stream, (const T *)x, C, H, W,
                           kind, (T *)y, Ho, Wo);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_osnet_gate(const float *plane_sum, int N, int mid, int hid, int P, const void *w1,
                   const void *b1, const void *w2, const void *b2, int half, void *gate,
                   void *stream) {
    YTA_CHECK(plane_sum && w1 && b1 && w2 && b2 && gate && N > 0 && mid > 0 && mid <= 512 &&
                  hid > 0 && hid <= 64 && P > 0,
              YTA_ERR_INVALID, "bad gate arguments");
    const float inv = 1.0f / (float)P;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_gate<T>, dim3(N), dim3(256), 0, (hipStream_t)stream, plane_sum, inv,
                           (const T *)w1, (const T *)b1, (const T *)w2, (const T *)b2, mid, hid,
                           (T *)gate);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

}  // extern "C"
