// The tensor path's protocol (yta_*_update_tensors, yta_sof_apply_tensors, yta_ecc_apply_tensors),
// written once for every engine: device tensors in, device tensors out, stream-ordered against the
// caller's stream, no host wait.  The caller's stream hands over to the engine's stream through an
// event, the frame runs there as plain launches, and a second event hands back.  What a call
// copies from host memory travels in a slot of mapped page-locked memory, one per frame in flight,
// guarded by the event recorded after its frame's last launch.  DESIGN §14 describes it.
//
// Host side: FrameSlot / FrameRing (the slots), frame_refuse_capture / frame_hand_in /
// frame_hand_back (the hand-off), tensor_check_args (the trackers' argument checks), tensor_stage
// (device staging that queued frames may outlive) and TrackBound (the track-capacity bound of the
// engines that grow).  Device side: block_run_scan and the three kernels around a tracker's frame,
// k_tp_ingest in front, k_tp_out_offsets and k_tp_pack_rows behind.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "common.hpp"

namespace yta {

// ------------------------------------------------------------------ the slots
// One frame in flight: the two events of its hand-off and one mapped, coherent page-locked block,
// which the engine carves through a view function of its own (8-byte members first).
struct FrameSlot {
    hipEvent_t in = nullptr, done = nullptr;   // caller stream -> engine stream -> caller stream
    void *h = nullptr, *m = nullptr;           // host / device view of the one allocation
    long long seq = -1;                        // enqueue order; -1: never used
    long long gen = -1;                        // the TrackBound::gen the frame belongs to
    std::vector<long long> cum_at;             // TrackBound::cum after the frame was enqueued
};

constexpr size_t FRAME_RING_MAX = 64;   // frames in flight before a call waits for the oldest

struct FrameRing {
    std::vector<FrameSlot *> slots;
    size_t slot_bytes = 0;             // of a slot's block: set by the engine before the first call
    long long seq = 0;
    long long *host_waits = nullptr;   // the engine's count of calls that blocked on the device

    static bool done(const FrameSlot *p) {
        if (p->seq < 0) return true;   // never used
        if (hipEventQuery(p->done) == hipSuccess) return true;
        (void)hipGetLastError();   // hipErrorNotReady
        return false;
    }

    // A slot no queued frame reads, stamped with the next seq: one whose frame has run, else a
    // new one; with FRAME_RING_MAX frames in flight the call waits for the oldest.  `keep` is
    // never handed out (a slot whose contents the engine still reads).
    int acquire(FrameSlot **out, const FrameSlot *keep = nullptr) {
        FrameSlot *p = nullptr, *oldest = nullptr;
        for (FrameSlot *q : slots) {
            if (!q->m || q == keep) continue;   // m null: its allocation failed part way
            if (done(q)) {
                p = q;
                break;
            }
            if (!oldest || q->seq < oldest->seq) oldest = q;
        }
        if (!p && slots.size() >= FRAME_RING_MAX && oldest) {
            ++*host_waits;
            YTA_HIP(hipEventSynchronize(oldest->done));
            p = oldest;
        }
        if (!p) {
            p = new (std::nothrow) FrameSlot();
            YTA_CHECK(p, YTA_ERR_NOMEM, "out of host memory");
            slots.push_back(p);   // owned from here on (release)
            YTA_HIP(hipEventCreateWithFlags(&p->in, hipEventDisableTiming));
            YTA_HIP(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
            YTA_HIP(hipHostMalloc(&p->h, slot_bytes, hipHostMallocMapped | hipHostMallocCoherent));
            YTA_HIP(hipHostGetDevicePointer(&p->m, p->h, 0));
        }
        p->seq = ++seq;
        *out = p;
        return YTA_OK;
    }

    // The newest frame of generation `gen` whose event has completed (null: none).
    const FrameSlot *newest_done(long long gen) const {
        const FrameSlot *k0 = nullptr;
        for (const FrameSlot *p : slots)
            if (p->seq >= 0 && p->gen == gen && (!k0 || p->seq > k0->seq) && done(p)) k0 = p;
        return k0;
    }

    void release() {
        for (FrameSlot *p : slots) {
            if (p->in) (void)hipEventDestroy(p->in);
            if (p->done) (void)hipEventDestroy(p->done);
            if (p->h) (void)hipHostFree(p->h);
            delete p;
        }
        slots.clear();
    }
};

// ------------------------------------------------------------------ the hand-off
// The cross-stream waits must not end up in somebody's graph.
inline int frame_refuse_capture(hipStream_t cs) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(cs, &st) != hipSuccess) (void)hipGetLastError();
    YTA_CHECK(st == hipStreamCaptureStatusNone, YTA_ERR_INVALID, "caller_stream is capturing");
    return YTA_OK;
}

// The engine's stream after everything queued on the caller's so far.
inline int frame_hand_in(FrameSlot *p, hipStream_t cs, hipStream_t es) {
    YTA_HIP(hipEventRecord(p->in, cs));
    YTA_HIP(hipStreamWaitEvent(es, p->in, 0));
    return YTA_OK;
}

// The caller's stream after the frame's last launch: its later work sees the outputs and may free
// or overwrite the inputs.
inline int frame_hand_back(FrameSlot *p, hipStream_t cs, hipStream_t es) {
    YTA_HIP(hipEventRecord(p->done, es));
    YTA_HIP(hipStreamWaitEvent(cs, p->done, 0));
    return YTA_OK;
}

// ------------------------------------------------------------------ the trackers' arguments
// What every tracker's update_tensors refuses before anything is enqueued; *total gets
// sum(det_counts).  D: the engine's embedding width (0: d_feats is not read).  The alignment tests
// refuse only pointers a load of the element type would fault on.
inline int tensor_check_args(const void *e, int S, int D, const void *d_dets, int dtype,
                             long long row_stride, const int *det_counts, const float *d_feats,
                             long long feat_stride, const double *d_rows, long long rows_capacity,
                             const int *d_row_offsets, long long *total_out) {
    YTA_CHECK(e && det_counts && d_row_offsets, YTA_ERR_INVALID, "null argument");
    YTA_CHECK(dtype == YTA_F64 || dtype == YTA_F32 || dtype == YTA_F16, YTA_ERR_INVALID,
              "dtype %d is none of YTA_F64, YTA_F32, YTA_F16", dtype);
    YTA_CHECK(row_stride >= 6, YTA_ERR_INVALID, "row_stride %lld < 6", row_stride);
    long long total = 0;
    for (int s = 0; s < S; ++s) {
        YTA_CHECK(det_counts[s] >= 0, YTA_ERR_INVALID, "det_counts[%d] is negative", s);
        total += det_counts[s];
    }
    YTA_CHECK(total <= 0x7fffffffLL, YTA_ERR_INVALID, "%lld detections in one frame", total);
    const size_t esz = dtype == YTA_F64 ? 8 : dtype == YTA_F32 ? 4 : 2;
    YTA_CHECK(total == 0 || (d_dets && (uintptr_t)d_dets % esz == 0), YTA_ERR_INVALID,
              "d_dets null or not aligned to its element size");
    // every output row is a track matched to or born from one of this frame's detections
    YTA_CHECK(rows_capacity >= total, YTA_ERR_CAPACITY,
              "d_rows holds %lld rows, the call needs sum(det_counts) = %lld", rows_capacity, total);
    YTA_CHECK(total == 0 || (d_rows && (uintptr_t)d_rows % 16 == 0), YTA_ERR_INVALID,
              "d_rows null or not 16-byte aligned");
    YTA_CHECK(D == 0 || total == 0 ||
                  (d_feats && (uintptr_t)d_feats % sizeof(float) == 0 && feat_stride >= D),
              YTA_ERR_INVALID, "d_feats null, misaligned or feat_stride < feat_dim");
    *total_out = total;
    return YTA_OK;
}

// ------------------------------------------------------------------ device staging
// Device staging of at least n elements; an outgrown buffer goes to `retired` and is kept until
// the next host wait (a queued frame may still read it), where tensor_free_retired frees it.
template <typename T>
int tensor_stage(std::vector<void *> &retired, T **buf, long long *cap, long long n,
                 long long floor_n) {
    if (n <= *cap && *buf) return YTA_OK;
    if (*buf) retired.push_back(*buf);
    *buf = nullptr;
    *cap = 0;
    const long long c = std::max(2 * n, floor_n);
    YTA_HIP(hipMalloc((void **)buf, sizeof(T) * (size_t)c));
    *cap = c;
    return YTA_OK;
}

inline void tensor_free_retired(std::vector<void *> &retired) {
    for (void *p : retired) (void)hipFree(p);
    retired.clear();
}

// ------------------------------------------------------------------ the track-capacity bound
// Of the engines that grow (ByteTrack / BoT-SORT, the OC-SORT family): a stream's live tracks after
// a frame are at most its live tracks after some earlier frame plus every detection enqueued for it
// since, this frame's included.  The earlier frame is the newest tensor frame whose event has
// completed (k_tp_pack_rows stored its live counts into the slot), else the last exact host
// counters.  Only the bound is here: what an engine does when it fails (wait, read the exact
// counters, grow) is the engine's.
struct TrackBound {
    std::vector<long long> cum;                   // per stream: detections enqueued so far
    std::vector<long long> base_cum, base_live;   // cum and the live tracks when the host counters
                                                  // were last exact
    bool dirty = false;   // tensor frames enqueued since the host counters were last read
    long long gen = 0;    // bumped whenever the host counters are made exact again

    // The host counters are exact: later frames are bounded from them.  live(s): stream s's.
    template <typename LiveOfStream>
    void rebase(int S, LiveOfStream live) {
        cum.resize(S);
        base_live.resize(S);
        for (int s = 0; s < S; ++s) base_live[s] = live(s);
        base_cum = cum;
    }

    // Whether a frame of `counts` detections keeps every stream within CAP tracks.  live(h, s):
    // stream s's live tracks as the frame of the slot block h left them.
    template <typename LiveOfSlot>
    bool fits(const FrameRing &ring, const int *counts, long long CAP, LiveOfSlot live) const {
        const FrameSlot *k0 = ring.newest_done(gen);
        for (size_t s = 0; s < cum.size(); ++s) {
            const long long from = k0 ? (long long)live(k0->h, (int)s) : base_live[s];
            const long long since = cum[s] - (k0 ? k0->cum_at[s] : base_cum[s]);
            if (from + since + counts[s] > CAP) return false;
        }
        return true;
    }

    // Every tensor frame enqueued so far has run and the host counters have been read.
    void exact() {
        dirty = false;
        ++gen;
    }

    // The frame of slot p, `counts` detections a stream, is about to be enqueued.
    void enqueue(FrameSlot *p, const int *counts) {
        for (size_t s = 0; s < cum.size(); ++s) cum[s] += counts[s];
        p->cum_at = cum;
        p->gen = gen;
        dirty = true;
    }
};

// ------------------------------------------------------------------ device side
// Block scan of per-thread sums (a thread's sum is that of its run of streams): returns the
// exclusive prefix of this thread's run.  `part`: THREADS ints of LDS; every thread of the
// THREADS-wide block calls it.
template <int THREADS>
__device__ __forceinline__ int block_run_scan(int sum, int *part) {
    const int t = threadIdx.x;
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {   // inclusive Hillis-Steele scan
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    return part[t] - sum;
}

// One launch for everything a tracker's frame brings in, on the engine's counters type C (the
// field used is next_id).  Block 0: the S + 1 detection offsets as the prefix sums of the frame's
// per-stream counts, read straight from the call's slot (mapped host memory, 4 B a stream);
// cnt[s].next_id from the same slot when the caller passed ID counters; and, when the caller passed
// image sizes (wh_in; null: none), the S x (w, h) copied from the slot into a device array, so the
// cost kernels never read mapped host memory.  Blocks 1..: the caller's detection rows (`stride`
// elements apart, of type T) widened exactly into the packed float64 rows the kernels read; a
// thread takes two neighbouring columns of one row (6 is even, so a pair never straddles rows) with
// two scalar loads, which any stride and any element alignment allow, and one 16-B store.  Bytes
// per detection: 6 * sizeof(T) read (plus the stride's padding where lines are shared), 48
// written: at most 96.
constexpr int TP_ING_T = 256;
template <typename T, typename C>
__global__ __launch_bounds__(TP_ING_T) void k_tp_ingest(const T *src, long long stride,
                                                        long long rows, double *dst,
                                                        const int *counts, const long long *nid,
                                                        const int *wh_in, int S, int *off, C *cnt,
                                                        int *wh_out) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        __shared__ int part[TP_ING_T];
        const int per = (S + TP_ING_T - 1) / TP_ING_T, s0 = min(S, t * per), s1 = min(S, s0 + per);
        int sum = 0;
        for (int s = s0; s < s1; ++s) sum += max(counts[s], 0);
        int r = block_run_scan<TP_ING_T>(sum, part);
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
    const long long pairs = rows * 3, step = (long long)(gridDim.x - 1) * TP_ING_T;
    for (long long k = (long long)(blockIdx.x - 1) * TP_ING_T + t; k < pairs; k += step) {
        const long long row = k / 3;
        const T *p = src + row * stride + 2 * (k - row * 3);
        reinterpret_cast<double2 *>(dst)[k] = make_double2((double)p[0], (double)p[1]);
    }
}

// The launch of k_tp_ingest for the call's dtype (wh_in / wh_out null: no image sizes).
template <typename C>
int tensor_ingest(hipStream_t es, const void *d_dets, int dtype, long long row_stride,
                  long long rows, double *dst, const int *counts, const long long *nid,
                  const int *wh_in, int S, int *off, C *cnt, int *wh_out) {
    const unsigned grid =
        1u + (unsigned)std::min<long long>(4096, (rows * 3 + TP_ING_T - 1) / TP_ING_T);
    if (dtype == YTA_F64)
        hipLaunchKernelGGL((k_tp_ingest<double, C>), dim3(grid), dim3(TP_ING_T), 0, es,
                           (const double *)d_dets, row_stride, rows, dst, counts, nid, wh_in, S,
                           off, cnt, wh_out);
    else if (dtype == YTA_F32)
        hipLaunchKernelGGL((k_tp_ingest<float, C>), dim3(grid), dim3(TP_ING_T), 0, es,
                           (const float *)d_dets, row_stride, rows, dst, counts, nid, wh_in, S,
                           off, cnt, wh_out);
    else
        hipLaunchKernelGGL((k_tp_ingest<_Float16, C>), dim3(grid), dim3(TP_ING_T), 0, es,
                           (const _Float16 *)d_dets, row_stride, rows, dst, counts, nid, wh_in, S,
                           off, cnt, wh_out);
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

// Stream s's output count out of an engine's counters records: a k_tp_out_offsets accessor.
template <typename C>
struct CountersNOut {
    const C *cnt;
    __device__ int operator()(int s) const { return cnt[s].n_out; }
};

// The packed rows' S + 1 offsets from the streams' output counts (nout(s), a trivially copyable
// accessor): one block for any S, each thread summing a run of streams, then a block scan.  A
// count is clamped to [0, cap]: a stream with error flags may hold anything.  off_host (null:
// none): a mirror in mapped host memory, so a host reader needs no copy.
constexpr int TP_OFFS_T = 1024;
template <typename NOut>
__global__ __launch_bounds__(TP_OFFS_T) void k_tp_out_offsets(NOut nout, int S, int cap, int *off,
                                                              int *off_host) {
    __shared__ int part[TP_OFFS_T];
    const int t = threadIdx.x;
    const int per = (S + TP_OFFS_T - 1) / TP_OFFS_T, s0 = min(S, t * per), s1 = min(S, s0 + per);
    int sum = 0;
    for (int s = s0; s < s1; ++s) sum += min(max(nout(s), 0), cap);
    int r = block_run_scan<TP_OFFS_T>(sum, part);
    if (t == 0) {
        off[0] = 0;
        if (off_host) off_host[0] = 0;
    }
    for (int s = s0; s < s1; ++s) {
        r += min(max(nout(s), 0), cap);
        off[s + 1] = r;
        if (off_host) off_host[s + 1] = r;
    }
}

// Every stream's output rows (src + s * cap_rows * 8, the engine's own buffer) moved to the
// caller's packed rows at the prefix offsets, with the stream id of each row beside them
// (row_stream, -1 from off[S] to `limit`, the caller's capacity, which no row or id is written
// past), and the stream's live-track count after the frame stored into the call's slot (mapped
// host memory) by live(s), an accessor as above, where later calls read it without a round trip.
// Block per stream, 16-B pieces (both buffers are 16-B aligned, the caller's checked by the host):
// 64 B read and 64 B written a row, 4 B a row of row_stream.
template <typename Live>
__global__ __launch_bounds__(256) void k_tp_pack_rows(const double *src, long long cap_rows, int S,
                                                      const int *off, double *dst, long long limit,
                                                      int *row_stream, Live live) {
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
    if (t == 0) live(s);
}

}  // namespace yta
