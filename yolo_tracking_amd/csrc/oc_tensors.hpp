// Tensor path of the OC-SORT family (yta_ocsort / yta_deepocsort / yta_hybridsort _update_tensors,
// host protocol: oc_host.hpp): the kernels that bring a frame in and hand its rows back, written
// once for the three engines on their counters type C (OcCounters, DocCounters, HsCounters; the
// fields used are next_id, n_out and n_trk).  bytetrack.hip keeps its own three (k_ingest,
// k_out_offsets_scan, k_pack_rows) on BtCounters, whose live count is a pair.
#pragma once
#include <hip/hip_runtime.h>

namespace yta {

// One launch for everything a frame brings in.  Block 0: the S + 1 detection offsets as the prefix
// sums of the frame's per-stream counts, read straight from the call's page-locked staging (mapped
// host memory, 4 B a stream); cnt[s].next_id from the same staging when the caller passed ID
// counters; and the S x (w, h) image sizes copied from it into a device array, so the cost kernels
// never read mapped host memory.  Blocks 1..: the caller's detection rows (`stride` elements apart,
// of type T) widened exactly into the packed float64 rows the kernels read; a thread takes two
// neighbouring columns of one row (6 is even, so a pair never straddles rows) with two scalar
// loads, which any stride and any element alignment allow, and one 16-B store.  Bytes per
// detection: 6 * sizeof(T) read (plus the stride's padding where lines are shared), 48 written.
constexpr int OC_ING_T = 256;
template <typename T, typename C>
__global__ __launch_bounds__(OC_ING_T) void k_oc_ingest(const T *src, long long stride,
                                                        long long rows, double *dst,
                                                        const int *counts, const long long *nid,
                                                        const int *wh_in, int S, int *off, C *cnt,
                                                        int *wh_out) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        __shared__ int part[OC_ING_T];
        const int per = (S + OC_ING_T - 1) / OC_ING_T, s0 = min(S, t * per), s1 = min(S, s0 + per);
        int sum = 0;
        for (int s = s0; s < s1; ++s) sum += max(counts[s], 0);
        part[t] = sum;
        __syncthreads();
        for (int d = 1; d < OC_ING_T; d <<= 1) {   // inclusive Hillis-Steele scan
            const int v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        int r = part[t] - sum;   // exclusive prefix of this thread's run
        if (t == 0) off[0] = 0;
        for (int s = s0; s < s1; ++s) {
            r += max(counts[s], 0);
            off[s + 1] = r;
            if (nid) cnt[s].next_id = nid[s];
            if (wh_in) {
                wh_out[2 * s] = wh_in[2 * s];
                wh_out[2 * s + 1] = wh_in[2 * s + 1];
            }
        }
        return;
    }
    const long long pairs = rows * 3, step = (long long)(gridDim.x - 1) * OC_ING_T;
    for (long long k = (long long)(blockIdx.x - 1) * OC_ING_T + t; k < pairs; k += step) {
        const long long row = k / 3;
        const T *p = src + row * stride + 2 * (k - row * 3);
        reinterpret_cast<double2 *>(dst)[k] = make_double2((double)p[0], (double)p[1]);
    }
}

// The packed rows' S + 1 offsets from the streams' output counts: one block for any S, each
// thread summing a run of streams, then a block scan.  A count is clamped to [0, cap]: a stream
// with error flags may hold anything.
constexpr int OC_OFFS_T = 1024;
template <typename C>
__global__ __launch_bounds__(OC_OFFS_T) void k_oc_out_offsets(const C *cnt, int S, int cap,
                                                              int *off) {
    __shared__ int part[OC_OFFS_T];
    const int t = threadIdx.x;
    const int per = (S + OC_OFFS_T - 1) / OC_OFFS_T, s0 = min(S, t * per), s1 = min(S, s0 + per);
    int sum = 0;
    for (int s = s0; s < s1; ++s) sum += min(max(cnt[s].n_out, 0), cap);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < OC_OFFS_T; d <<= 1) {   // inclusive Hillis-Steele scan
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int r = part[t] - sum;   // exclusive prefix of this thread's run
    if (t == 0) off[0] = 0;
    for (int s = s0; s < s1; ++s) {
        r += min(max(cnt[s].n_out, 0), cap);
        off[s + 1] = r;
    }
}

// Every stream's output rows (src + s * cap_rows * 8, the engine's own buffer) moved to the
// caller's packed rows at the prefix offsets, with the stream id of each row beside them
// (row_stream, -1 from off[S] to `limit`, the caller's capacity, which no row or id is written
// past), and the stream's live trackers after the frame stored into the call's page-locked staging
// (mapped host memory), where the next calls bound the track capacity without a round trip.  Block
// per stream, 16-B pieces: 64 B read and 64 B written a row, 4 B a row of row_stream.
template <typename C>
__global__ __launch_bounds__(256) void k_oc_pack_rows(const double *src, long long cap_rows,
                                                      const C *cnt, int S, const int *off,
                                                      double *dst, long long limit,
                                                      int *row_stream, int *live) {
    const int s = blockIdx.x, t = threadIdx.x;
    const long long b = off[s];
    const long long n = max(min((long long)off[s + 1], limit) - b, 0LL);
    const double2 *a = reinterpret_cast<const double2 *>(src + s * cap_rows * 8);
    double2 *d = reinterpret_cast<double2 *>(dst + b * 8);
    for (long long k = t; k < n * 4; k += blockDim.x) d[k] = a[k];
    if (row_stream) {
        for (long long r = t; r < n; r += blockDim.x) row_stream[b + r] = s;
        for (long long r = (long long)off[S] + (long long)s * blockDim.x + t; r < limit;
             r += (long long)S * blockDim.x)
            row_stream[r] = -1;
    }
    if (t == 0) live[s] = cnt[s].n_trk;
}

}  // namespace yta
