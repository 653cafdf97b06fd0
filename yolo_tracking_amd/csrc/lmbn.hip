// LMBN-n (Lightweight Multi-Branch Network, OSNet backbone) kernels on gfx950: what the ReID
// network of appearance/lmbn.py runs after its OSNet trunk and branches (csrc/osnet.hip).
//
// Reference: boxmot/appearance/backbones/lmbn/lmbn_n.py LMBN_n.forward (:98-132), lmbn/bnneck.py.
//   k_lmbn_pool  the pooling stage (:98-105): per (sample, channel) plane of H x W elements any
//                subset of {max, mean, mean of the upper bin, mean of the lower bin} in one read
//                of the plane.  The bins are AdaptiveAvgPool2d((2, 1))'s: rows [0, ceil(H / 2))
//                and [floor(H / 2), H), which share the middle row of an odd H.  GS lanes (8, 16,
//                32 or 64, by the plane's size) own a plane, so a 256-thread block covers 4 to 32
//                adjacent planes and reads one contiguous run; in a 16-byte aligned tensor a lane
//                loads 16 bytes (4 floats, 8 halves) where the plane size is a multiple of that,
//                else 4 elements, else 1.  The maximum starts from the plane's first element; the
//                sums meet by xor shuffles in a fixed order.
//   k_lmbn_neck  the seven heads (:107-120) and the interleaving stack (:127-131) in one launch:
//                y[n][c * 7 + j] = act_j(sum_k w_j[k][c] x_j[n][k] + b_j[c]), act_j the identity
//                or s_j[c] * relu(.) + t_j[c] (a BatchNorm behind the ReLU, which cannot fold into
//                the weight).  A block owns NK_RT rows x NK_CT channels x all heads: lanes run
//                along the channels (coalesced k-major weight reads), a thread keeps 4 rows, the
//                rows' inputs are staged per k-chunk in LDS as [k][row] (one 16-byte broadcast
//                read per k; rows of 36 words keep that read 16-byte aligned.  The staging write
//                runs its lanes along k for coalesced global reads, so consecutive lanes land 4
//                banks apart: a 4-way conflict on that ds_write_b32, once per chunk and outside
//                the k loop).  The results are staged in LDS as [row][c * 7 + j] (the write has a
//                lane stride of 7 words, coprime with the 32 banks a ds_write_b32 half-wave sees:
//                conflict-free without padding; the read-out is consecutive words) and leave as
//                contiguous runs of 7 * NK_CT elements per row instead of stores 7 elements apart.
// float32 or float16 storage, float32 arithmetic, no atomics.
#include <cstdint>

#include "by_storage.hpp"
#include "common.hpp"
#include "../../include/yolo_tracking_amd.h"

namespace yta {
namespace {

// ---------------------------------------------------------------------------------- k_lmbn_pool
constexpr int LP_T = 256;

// V elements of T as one load: 16 bytes (4 floats, 8 halves) or 8 bytes (4 halves)
template <typename T, int V>
struct lp_vec {
    typedef T type __attribute__((ext_vector_type(V)));
};

struct lp_acc {
    float m, s, su, sl;
    int ub, lb;   // elements below ub are in the upper bin, elements from lb on in the lower one
    __device__ __forceinline__ void add(float v, int i) {
        m = fmaxf(m, v);
        s += v;
        if (i < ub) su += v;
        if (i >= lb) sl += v;
    }
};

template <typename T, int GS, int V>
__global__ __launch_bounds__(LP_T) void k_lmbn_pool(const T *x, long long planes, int H, int W,
                                                    T *mx, T *mean, T *upper, T *lower) {
    const int g = threadIdx.x / GS, t = threadIdx.x - g * GS;
    const long long pl = (long long)blockIdx.x * (LP_T / GS) + g;
    const bool live = pl < planes;          // every lane stays for the shuffles
    const int P = H * W;
    const T *p = x + (live ? pl : 0) * P;
    lp_acc a;
    a.m = (float)p[0];                      // not 0: the planes may be negative throughout
    a.s = a.su = a.sl = 0.f;
    a.ub = ((H + 1) / 2) * W;
    a.lb = (H / 2) * W;
    if (V > 1) {                            // P % V == 0 and x aligned: every plane is aligned
        typedef typename lp_vec<T, V>::type VT;
        const VT *pv = reinterpret_cast<const VT *>(p);
        for (int i = t; i < P / V; i += GS) {
            const VT v = pv[i];
#pragma unroll
            for (int e = 0; e < V; ++e) a.add((float)v[e], V * i + e);
        }
    } else {
        for (int i = t; i < P; i += GS) a.add((float)p[i], i);
    }
#pragma unroll
    for (int m = 1; m < GS; m <<= 1) {
        a.m = fmaxf(a.m, __shfl_xor(a.m, m, GS));
        a.s += __shfl_xor(a.s, m, GS);
        a.su += __shfl_xor(a.su, m, GS);
        a.sl += __shfl_xor(a.sl, m, GS);
    }
    if (live && t == 0) {
        if (mx) mx[pl] = (T)a.m;
        if (mean) mean[pl] = (T)(a.s / (float)P);
        if (upper) upper[pl] = (T)(a.su / (float)a.ub);
        if (lower) lower[pl] = (T)(a.sl / (float)(P - a.lb));
    }
}

// Elements a lane loads at once: 16 bytes where the plane size allows, else 4 elements, else 1.
template <typename T>
int lp_width(const void *x, int P) {
    constexpr int full = 16 / (int)sizeof(T);
    if ((uintptr_t)x % 16) return 1;
    return P % full == 0 ? full : P % 4 == 0 ? 4 : 1;
}

template <typename T, int V>
void lp_launch(const void *x, long long planes, int H, int W, void *mx, void *mean, void *upper,
               void *lower, hipStream_t st) {
    const int units = H * W / V;             // loads a plane takes
    const int gs = units <= 8 ? 8 : units <= 16 ? 16 : units <= 32 ? 32 : 64;
    const int per = LP_T / gs;
    const dim3 g((unsigned)((planes + per - 1) / per));
#define YTA_LP_LAUNCH(GS)                                                                      \
    hipLaunchKernelGGL((k_lmbn_pool<T, GS, V>), g, dim3(LP_T), 0, st, (const T *)x, planes, H, \
                       W, (T *)mx, (T *)mean, (T *)upper, (T *)lower)
    if (gs == 8) YTA_LP_LAUNCH(8);
    else if (gs == 16) YTA_LP_LAUNCH(16);
    else if (gs == 32) YTA_LP_LAUNCH(32);
    else YTA_LP_LAUNCH(64);
#undef YTA_LP_LAUNCH
}

// ---------------------------------------------------------------------------------- k_lmbn_neck
constexpr int NK_T = 256;
constexpr int NK_CT = 32;                 // channels of a block
constexpr int NK_RT = 32;                 // rows of a block: 8 thread rows of 4
constexpr int NK_KC = 128;                // k values staged together
constexpr int NK_XS = NK_RT + 4;          // staged input [k][row], rows padded (16-byte aligned)
constexpr int NK_ROW = YTA_LMBN_HEADS * NK_CT;   // staged results [row][c * 7 + j]

struct nk_heads {
    yta_lmbn_head h[YTA_LMBN_HEADS];
};

template <typename T>
__global__ __launch_bounds__(NK_T) void k_lmbn_neck(nk_heads hs, int N, int C, T *y) {
    __shared__ __attribute__((aligned(16))) float xs[NK_KC * NK_XS];
    __shared__ float os[NK_RT * NK_ROW];
    const int t = threadIdx.x;
    const int cl = t & (NK_CT - 1), rg = t / NK_CT;
    const int c0 = blockIdx.x * NK_CT;
    const long long n0 = (long long)blockIdx.y * NK_RT;
    const int c = c0 + cl < C ? c0 + cl : C - 1;     // loads stay in range; stores are guarded
#pragma unroll 1
    for (int j = 0; j < YTA_LMBN_HEADS; ++j) {
        const yta_lmbn_head &h = hs.h[j];
        const T *xj = (const T *)h.x;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < h.K; k0 += NK_KC) {            // block-uniform
            const int kc = min(NK_KC, h.K - k0);
            __syncthreads();
            for (int i = t; i < NK_RT * NK_KC; i += NK_T) {  // lanes along k: contiguous rows
                const int r = i / NK_KC, kk = i - r * NK_KC;
                xs[kk * NK_XS + r] = (n0 + r < N && kk < kc)
                                         ? (float)xj[(n0 + r) * h.x_stride + k0 + kk] : 0.f;
            }
            __syncthreads();
            const float *wk = h.w + (long long)k0 * C + c;
#pragma unroll 32   // 32 weight loads in flight: the loop is bound by their latency
            for (int kk = 0; kk < kc; ++kk) {
                const float wv = wk[(long long)kk * C];
                const float4 x4 = *reinterpret_cast<const float4 *>(xs + kk * NK_XS + rg * 4);
                acc[0] = fmaf(wv, x4.x, acc[0]);
                acc[1] = fmaf(wv, x4.y, acc[1]);
                acc[2] = fmaf(wv, x4.z, acc[2]);
                acc[3] = fmaf(wv, x4.w, acc[3]);
            }
        }
        const float b = h.bias ? h.bias[c] : 0.f;
        const float sc = h.scale ? h.scale[c] : 1.f, sh = h.shift ? h.shift[c] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[r] + b;
            if (h.relu) v = fmaxf(v, 0.f);
            if (h.scale || h.shift) v = v * sc + sh;
            os[(rg * 4 + r) * NK_ROW + cl * YTA_LMBN_HEADS + j] = v;
        }
    }
    __syncthreads();
    const int run = YTA_LMBN_HEADS * min(NK_CT, C - c0);     // valid elements of a staged row
    for (int i = t; i < NK_RT * NK_ROW; i += NK_T) {
        const int r = i / NK_ROW, q = i - r * NK_ROW;
        if (n0 + r < N && q < run)
            y[(n0 + r) * ((long long)C * YTA_LMBN_HEADS) + (long long)c0 * YTA_LMBN_HEADS + q] =
                (T)os[i];
    }
}

}  // namespace
}  // namespace yta

using namespace yta;

extern "C" {

int yta_lmbn_pool(const void *x, int N, int C, int H, int W, int half, void *mx, void *mean,
                  void *upper, void *lower, void *stream) {
    YTA_CHECK(x && N > 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= 0x3fffffffLL &&
                  (mx || mean || upper || lower),
              YTA_ERR_INVALID, "bad pooling arguments (at least one output)");
    const long long planes = (long long)N * C;
    YTA_CHECK((planes + 3) / 4 <= 0x7fffffffLL, YTA_ERR_INVALID, "grid too large");
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        constexpr int full = 16 / (int)sizeof(T);
        const int v = lp_width<T>(x, H * W);
        if (v == full) lp_launch<T, full>(x, planes, H, W, mx, mean, upper, lower, st);
        else if (v == 4) lp_launch<T, 4>(x, planes, H, W, mx, mean, upper, lower, st);
        else lp_launch<T, 1>(x, planes, H, W, mx, mean, upper, lower, st);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int yta_lmbn_neck(const yta_lmbn_head *heads, int N, int C, int half, void *y, void *stream) {
    YTA_CHECK(heads && y && N > 0 && C > 0 && C <= 0x7fffffff / YTA_LMBN_HEADS, YTA_ERR_INVALID,
              "bad neck arguments");
    nk_heads hs;
    for (int j = 0; j < YTA_LMBN_HEADS; ++j) {
        hs.h[j] = heads[j];
        YTA_CHECK(heads[j].x && heads[j].w && heads[j].K > 0 && heads[j].x_stride >= heads[j].K,
                  YTA_ERR_INVALID, "bad neck head (x, w, K > 0, row stride >= K)");
    }
    const long long rows = ((long long)N + NK_RT - 1) / NK_RT;
    YTA_CHECK(rows <= 65535, YTA_ERR_INVALID, "grid too large");
    const dim3 g((unsigned)((C + NK_CT - 1) / NK_CT), (unsigned)rows);
    hipStream_t st = (hipStream_t)stream;
    by_storage(half, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(k_lmbn_neck<T>, g, dim3(NK_T), 0, st, hs, N, C, (T *)y);
    });
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

}  // extern "C"
