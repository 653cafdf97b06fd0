// Tensor path of the StrongSORT engine (yta_strongsort_update_tensors, host protocol in
// strongsort.hip): the kernels that bring a frame in and hand its rows back.  They follow
// oc_tensors.hpp's three, on StrongSORT's layout: fixed slabs S x MAXD x 6 in (the engine never
// grows), plain int arrays for the counts (nout / ntrk, which update_device hands to its caller)
// instead of a counters record.
#pragma once
#include <hip/hip_runtime.h>

namespace yta {

// One launch for everything a frame brings in; the only kernel of a frame that reads the call's
// page-locked staging (mapped host memory): `counts` (S) and `offs` (S + 1, their prefix sums,
// taken on the host where the counts are checked against max_dets anyway) and `nid` (S, null when
// the caller passed no ID counters).
// Block 0 copies them to the device: ndet[s], off[0..S] and, for the streams the mask leaves
// active, hdr[s][hdr_next].  The later kernels read only those.
// Blocks 1..: block 1 + s * cps + c widens chunk c of stream s: the caller's rows offs[s] ..
// offs[s + 1] (`stride` elements apart, of type T) exactly into the float64 slab rows
// dets[s][0..m).  A thread takes two neighbouring columns of one row (6 is even, so a pair never
// straddles rows) with two scalar loads, which any stride and any element alignment allow, and
// one 16-B store: the slab is a device allocation and the pair starts at an even element, so the
// store is 16-B aligned.  Bytes per detection: 6 * sizeof(T) read, 48 written; a block of a
// stream that is masked out or has no rows left returns at once.
constexpr int SS_ING_T = 256;
template <typename T>
__global__ __launch_bounds__(SS_ING_T) void k_ss_ingest(const T *src, long long stride,
                                                        const int *counts, const int *offs,
                                                        const long long *nid, const int *active,
                                                        int S, int maxd, int cps, int *ndet,
                                                        int *off, int *hdr, int hdr_n,
                                                        int hdr_next, double *dets) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        for (int s = t; s < S; s += SS_ING_T) {
            ndet[s] = counts[s];
            off[s + 1] = offs[s + 1];
            if (nid && (!active || active[s])) hdr[s * hdr_n + hdr_next] = (int)nid[s];
        }
        if (t == 0) off[0] = 0;
        return;
    }
    const int b = blockIdx.x - 1, s = b / cps, c = b - s * cps;
    if (active && !active[s]) return;
    const int k = c * SS_ING_T + t, m = min(counts[s], maxd);
    if (k >= 3 * m) return;
    const int row = k / 3, cp = k - 3 * row;
    const T *p = src + ((long long)offs[s] + row) * stride + 2 * cp;
    double2 *d = reinterpret_cast<double2 *>(dets + ((long long)s * maxd + row) * 6);
    d[cp] = make_double2((double)p[0], (double)p[1]);
}

// The packed rows' S + 1 offsets from the streams' output counts (k_oc_out_offsets on an int
// array): one block for any S, each thread summing a run of streams, then a block scan.  A count
// is clamped to [0, cap]: a stream with error flags may hold anything.
constexpr int SS_OFFS_T = 1024;
__global__ __launch_bounds__(SS_OFFS_T) void k_ss_out_offsets(const int *nout, int S, int cap,
                                                              int *off) {
    __shared__ int part[SS_OFFS_T];
    const int t = threadIdx.x;
    const int per = (S + SS_OFFS_T - 1) / SS_OFFS_T, s0 = min(S, t * per), s1 = min(S, s0 + per);
    int sum = 0;
    for (int s = s0; s < s1; ++s) sum += min(max(nout[s], 0), cap);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < SS_OFFS_T; d <<= 1) {   // inclusive Hillis-Steele scan
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int r = part[t] - sum;   // exclusive prefix of this thread's run
    if (t == 0) off[0] = 0;
    for (int s = s0; s < s1; ++s) {
        r += min(max(nout[s], 0), cap);
        off[s + 1] = r;
    }
}

// Every stream's output rows (src + s * cap_rows * 8, the engine's own buffer) moved to the
// caller's packed rows at the prefix offsets, with the stream id of each row beside them
// (row_stream, -1 from off[S] to `limit`, the caller's capacity, which no row or id is written
// past), and the stream's track count after the frame stored into the call's page-locked staging
// (mapped host memory), where n_tracks() reads it after the frame's event.  Block per stream,
// 16-B pieces (both buffers are 16-B aligned, the caller's checked by the host): 64 B read and
// 64 B written a row, 4 B a row of row_stream.
__global__ __launch_bounds__(256) void k_ss_pack_rows(const double *src, long long cap_rows,
                                                      const int *ntrk, int S, const int *off,
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
    if (t == 0) live[s] = ntrk[s];
}

}  // namespace yta
