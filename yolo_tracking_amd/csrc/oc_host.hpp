// Host side shared by the engines (no device code but two accessors of tensor_path.hpp's kernels,
// which the family's tensor path at the end of this file launches).
//
// For every engine: dalloc / DALLOC (tracked device allocations) and grow_pair (a device buffer
// with its page-locked twin).
//
// For the OC-SORT family (ocsort.hip, hybridsort.hip, deepocsort.hip): the host engine skeleton.
// An engine is `struct yta_x : OcEngine<XBuf, yta_x_params>`, XBuf an OcSized<XArgs, XCounters>
// plus the engine's own per-stream staging, and gives the skeleton three members:
//     int alloc(int cap, int maxd, XBuf &b) const   the buffer list and the Args fill
//     std::vector<SlotCopy> slot_arrays(XBuf &n, const XBuf &o) const
//                                                   the per-slot arrays a growth carries over
//     void launch_reset(int s0, int n)              its reset kernel on streams [s0, s0 + n)
// Everything sized by (S, CAP, MAXD) lives in the one XBuf, so a buffer added to alloc() is
// released and carried through a growth without another edit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "common.hpp"
#include "ocsort_common.hpp"
#include "subset.hpp"
#include "tensor_path.hpp"

namespace yta {

// n elements of T on the device, remembered in `allocs` for the owner's release.
template <typename T>
int dalloc(std::vector<void *> &allocs, T **p, long long n) {
    void *q = nullptr;
    if (n <= 0) n = 1;
    hipError_t err = hipMalloc(&q, sizeof(T) * (size_t)n);
    if (err != hipSuccess) {
        set_error("hipMalloc(%lld bytes) failed: %s", (long long)(sizeof(T) * n),
                  hipGetErrorString(err));
        return YTA_ERR_NOMEM;
    }
    allocs.push_back(q);
    *p = static_cast<T *>(q);
    return YTA_OK;
}

// in a function with the owner's `allocs` in scope
#define DALLOC(ptr, n)                         \
    do {                                       \
        int _rc = dalloc(allocs, &(ptr), (n)); \
        if (_rc) return _rc;                   \
    } while (0)

// A device buffer *d and its page-locked twin *h (host_flags) of *cap elements of elem_bytes:
// when `need` outgrows them, both are freed (contents dropped) and allocated anew with new_cap
// elements, the caller's growth rule.
template <typename T>
int grow_pair(T **d, T **h, long long *cap, long long need, size_t elem_bytes, long long new_cap,
              unsigned host_flags = hipHostMallocDefault) {
    if (need <= *cap) return YTA_OK;
    if (*d) (void)hipFree(*d);
    if (*h) (void)hipHostFree(*h);
    *d = *h = nullptr;
    *cap = 0;
    YTA_HIP(hipMalloc((void **)d, elem_bytes * new_cap));
    YTA_HIP(hipHostMalloc((void **)h, elem_bytes * new_cap, host_flags));
    *cap = new_cap;
    return YTA_OK;
}

// ------------------------------------------------------------------ OC-SORT family: the state
// What one (S, CAP, MAXD) owns: the device buffers behind Args, the launch's LDS size and the
// per-stream staging.  Filled by the engine's alloc(), freed by release(), swapped whole by
// oc_reserve.
template <typename ArgsT, typename CountersT>
struct OcSized {
    using Args = ArgsT;
    using Counters = CountersT;
    std::vector<void *> allocs;   // device
    std::vector<void *> pinned;   // page-locked host
    Args a{};                     // a.S, a.CAP, a.MAXD are the sizes
    // The engine's own S * CAP * 8 output rows.  a.out is whatever the last launch wrote to (a
    // caller's buffer after update_device): the host and tensor paths pass this one.
    double *out_own = nullptr;
    size_t lds = 0;
    int *h_off = nullptr, *d_off = nullptr;
    Counters *h_cnt = nullptr;    // the counters as last read (and next_id on its way in)

    template <typename T>
    hipError_t pin(T **p, long long n) {
        void *q = nullptr;
        const hipError_t err = hipHostMalloc(&q, sizeof(T) * (size_t)n, hipHostMallocDefault);
        if (err == hipSuccess) pinned.push_back(q);
        *p = static_cast<T *>(q);
        return err;
    }
    // the pointers dangle afterwards: destroy the object or assign over it
    void release() {
        for (void *p : allocs) (void)hipFree(p);
        for (void *p : pinned) (void)hipHostFree(p);
        allocs.clear();
        pinned.clear();
    }
};

// The tensor path's host state (oc_update_tensors below, protocol: tensor_path.hpp).  A slot
// (oc_slot_view) carries the call's counts, ID counters and image sizes in and the streams' live
// tracker counts back.
struct OcSlotView {
    long long *nid;   // S ID counters in
    int *counts;      // S detection counts in
    int *wh;          // S x (w, h) image sizes in
    int *live;        // S live tracker counts back (k_tp_pack_rows)
};
inline size_t oc_slot_bytes(size_t S) { return S * (8 + 4 + 8 + 4); }
inline OcSlotView oc_slot_view(void *base, size_t S) {
    long long *nid = static_cast<long long *>(base);
    int *counts = reinterpret_cast<int *>(nid + S);
    return {nid, counts, counts + S, counts + 3 * S};
}
struct OcTensorState {
    FrameRing ring;
    TrackBound bound;                    // live tracks: h_cnt's n_trk
    double *det = nullptr;               // float64 staging rows (k_tp_ingest)
    long long det_cap = 0;
    int *off = nullptr;                  // S + 1 detection offsets (k_tp_ingest)
    int *wh = nullptr;                   // S x (w, h) on the device (k_tp_ingest)
    float *feat = nullptr;               // feature rows gathered from a strided tensor
    long long feat_cap = 0;
    std::vector<void *> retired;         // outgrown staging a queued frame may still read: freed
                                         // at the next host wait
    long long stat[4] = {};              // frames, host_waits, reserves, ingest_skipped
};

// Test-only snapshot of the stage-1 matrices (yta_<t>_debug_costs), which later rounds of the
// frame overwrite.  Off unless enabled; when on, the engine's launch calls oc_debug_snapshot after
// its last cost kernel and before its first solver kernel, and every source of the engine's
// debug_sources() is copied device to device on the engine's stream.
struct OcDebugSrc {   // `rows` rows of `width` bytes, `pitch` bytes apart; copied densely
    const void *src;
    size_t width, rows, pitch;
};
// the first five sources of every engine (ODB_BOX: the predicted boxes, 4 doubles per tracker in
// column order), its matrices from ODB_MAT on
enum { ODB_CNT, ODB_ROWS, ODB_SLOT, ODB_ID, ODB_BOX, ODB_MAT };
struct OcDebugCosts {
    bool on = false, taken = false;
    int cap = 0, maxd = 0;        // the engine's sizes when the snapshot was taken
    std::vector<void *> dev;      // one dense copy per source
    std::vector<size_t> bytes;    // their sizes
    void release() {
        for (void *p : dev)
            if (p) (void)hipFree(p);
        dev.clear();
        bytes.clear();
        taken = false;
    }
};

template <typename BufT, typename ParamsT>
struct OcEngine {
    using Buf = BufT;
    int device = 0, S = 0, D = 0;   // D: embedding width (0: none)
    ParamsT prm{};
    hipStream_t stream = nullptr;
    Buf b;
    // detection / feature rows of a host-buffer update: sized by the frame, kept across growth
    double *h_dets = nullptr, *d_det_in = nullptr;
    long long det_cap = 0;
    float *h_feat = nullptr, *d_feat = nullptr;
    long long feat_cap = 0;
    StreamMask mask;   // stream-subset updates (subset.hpp)
    OcTensorState t;   // the tensor path (oc_update_tensors)
    OcDebugCosts dbg;  // the stage-1 snapshot (oc_debug_snapshot), off by default
};

// One per-slot array of a growth: S rows of `bytes` per slot, CAP slots a row.
struct SlotCopy {
    void *dst;
    const void *src;
    size_t bytes;
};

// ------------------------------------------------------------------ counters and errors
template <typename E>
int oc_read_counters(E *e) {
    YTA_HIP(hipMemcpyAsync(e->b.h_cnt, e->b.a.cnt, sizeof(typename E::Buf::Counters) * e->S,
                           hipMemcpyDeviceToHost, e->stream));
    YTA_HIP(host_wait(e->stream));
    // every tensor frame enqueued so far has run: h_cnt is exact again, and nothing reads the
    // staging those frames outgrew
    e->t.bound.exact();
    tensor_free_retired(e->t.retired);
    return YTA_OK;
}

// After tensor frames (oc_update_tensors), which read nothing back: wait for them and bring h_cnt
// up to date, for the entry points that size or report from it.
template <typename E>
int oc_catch_up(E *e) {
    if (!e->t.bound.dirty) return YTA_OK;
    YTA_HIP(hipSetDevice(e->device));
    return oc_read_counters(e);
}

// invalid_bit / invalid_text: an engine's own input-error flag next to the family's four
template <typename E>
int oc_check_errors(E *e, int invalid_bit = 0, const char *invalid_text = "") {
    for (int s = 0; s < e->S; ++s) {
        const int err = e->b.h_cnt[s].err;
        if (err) {
            set_error("stream %d: device error flags 0x%x (%s%s%s%s%s)", s, err,
                      err & ERR_GIOU ? "giou enclosure not positive (iou.py:58 assert) " : "",
                      err & ERR_SOLVER ? "assignment solver failure " : "",
                      err & ERR_TRACK_CAPACITY ? "track capacity exceeded " : "",
                      err & ERR_DET_CAPACITY ? "too many detections " : "",
                      err & invalid_bit ? invalid_text : "");
            return (err & (ERR_TRACK_CAPACITY | ERR_DET_CAPACITY)) ? YTA_ERR_CAPACITY
                   : (err & (ERR_GIOU | invalid_bit))              ? YTA_ERR_INVALID
                                                                   : YTA_ERR_HIP;
        }
    }
    return YTA_OK;
}

// ------------------------------------------------------------------ growth
// The old streams' state into the larger `n`: the engine's per-slot arrays, then the free lists.
template <typename E>
int oc_carry_over(E *e, typename E::Buf &n) {
    using Counters = typename E::Buf::Counters;
    const typename E::Buf &o = e->b;
    const size_t S = e->S, oc = o.a.CAP, nc = n.a.CAP;
    for (const SlotCopy &c : e->slot_arrays(n, o))
        YTA_HIP(hipMemcpy2DAsync(c.dst, nc * c.bytes, c.src, oc * c.bytes, oc * c.bytes, S,
                                 hipMemcpyDeviceToDevice, e->stream));
    // free slots: the old free list, then the new slots [oc, nc) (popped from the end:
    // written so the lowest new slot is used first after the old ones)
    std::vector<int> fl(nc * S), old(oc * S);
    std::vector<Counters> cnt(S);
    hipError_t he = hipMemcpyAsync(old.data(), o.a.free_list, sizeof(int) * oc * S,
                                   hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess)
        he = hipMemcpyAsync(cnt.data(), o.a.cnt, sizeof(Counters) * S, hipMemcpyDeviceToHost,
                            e->stream);
    if (he == hipSuccess) he = host_wait(e->stream);
    if (he == hipSuccess) {
        for (size_t s = 0; s < S; ++s) {
            int k = 0;
            for (int q = (int)nc - 1; q >= (int)oc; --q) fl[s * nc + k++] = q;
            for (int q = 0; q < cnt[s].n_free; ++q) fl[s * nc + k++] = old[s * oc + q];
            cnt[s].n_free = k;
        }
        he = hipMemcpy(n.a.free_list, fl.data(), sizeof(int) * nc * S, hipMemcpyHostToDevice);
        if (he == hipSuccess)
            he = hipMemcpy(n.a.cnt, cnt.data(), sizeof(Counters) * S, hipMemcpyHostToDevice);
    }
    YTA_CHECK(he == hipSuccess, YTA_ERR_HIP, "reserve: %s", hipGetErrorString(he));
    memcpy(n.h_cnt, o.h_cnt, sizeof(Counters) * S);
    return YTA_OK;
}

// Grow capacity (tracks per stream / detections per stream), keeping every stream's state.
template <typename E>
int oc_reserve(E *e, int cap, int maxd) {
    if (cap <= e->b.a.CAP && maxd <= e->b.a.MAXD) return YTA_OK;
    cap = std::max(cap, e->b.a.CAP);
    maxd = std::max(maxd, e->b.a.MAXD);
    int rc = oc_catch_up(e);   // h_cnt goes into the new buffers
    if (rc) return rc;
    YTA_HIP(host_wait(e->stream));
    typename E::Buf n;
    rc = e->alloc(cap, maxd, n);
    if (!rc) rc = oc_carry_over(e, n);
    if (!rc) std::swap(e->b, n);
    n.release();
    return rc;
}

// ------------------------------------------------------------------ the frame protocol
// A host-buffer update is, in this order: oc_begin_frame, oc_stage_dets, the engine's feature
// rows, oc_stage of the offsets and of the engine's per-stream extras, oc_put_next_id, the
// engine's launch, oc_end_frame.

// Pageable `src` to the device buffer `dev` through its page-locked twin `pinned`.
template <typename E>
int oc_stage(E *e, void *dev, void *pinned, const void *src, size_t bytes) {
    memcpy(pinned, src, bytes);
    YTA_HIP(hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, e->stream));
    return YTA_OK;
}

// Validates the offsets, grows the engine to the frame; *total = the frame's detections.
template <typename E>
int oc_begin_frame(E *e, const int *det_offsets, bool have_wh, int out_capacity,
                   long long *total) {
    YTA_HIP(hipSetDevice(e->device));
    {
        const int cu = oc_catch_up(e);   // tensor frames in flight: n_trk below must be exact
        if (cu) return cu;
    }
    const int S = e->S, CAP = e->b.a.CAP, MAXD = e->b.a.MAXD;
    YTA_CHECK(det_offsets[0] == 0, YTA_ERR_INVALID, "det_offsets[0] must be 0");
    YTA_CHECK(have_wh || e->prm.asso_func != 4, YTA_ERR_INVALID, "centroid needs img_wh");
    int need_d = MAXD, need_c = CAP;
    for (int s = 0; s < S; ++s) {
        const int m = det_offsets[s + 1] - det_offsets[s];
        YTA_CHECK(m >= 0, YTA_ERR_INVALID, "det_offsets must be non-decreasing");
        need_d = std::max(need_d, m);
        need_c = std::max(need_c, e->b.h_cnt[s].n_trk + m);
    }
    // every output row is a track matched to or born from one of this frame's detections, so
    // det_offsets[S] rows always suffice; checked before anything moves (the frame is not consumed)
    YTA_CHECK(out_capacity >= det_offsets[S], YTA_ERR_CAPACITY,
              "out holds %d rows, the call needs det_offsets[S] = %d", out_capacity, det_offsets[S]);
    *total = det_offsets[S];
    if (need_d > MAXD || need_c > CAP)
        return oc_reserve(e, need_c > CAP ? std::max(need_c, 2 * CAP) : CAP,
                          need_d > MAXD ? std::max(need_d, 2 * MAXD) : MAXD);
    return YTA_OK;
}

template <typename E>
int oc_stage_dets(E *e, const double *dets, long long total) {
    const int rc = grow_pair(&e->d_det_in, &e->h_dets, &e->det_cap, total, sizeof(double) * 6,
                             std::max<long long>(2 * total, 1024));
    if (rc || !total) return rc;
    return oc_stage(e, e->d_det_in, e->h_dets, dets, sizeof(double) * 6 * total);
}

// Room for `total` feature rows of e->D floats in d_feat / h_feat.
template <typename E>
int oc_grow_feats(E *e, long long total) {
    return grow_pair(&e->d_feat, &e->h_feat, &e->feat_cap, total, sizeof(float) * e->D,
                     std::max<long long>(2 * total, 1024));
}

template <typename E>
int oc_stage_offsets(E *e, const int *det_offsets) {
    return oc_stage(e, e->b.d_off, e->b.h_off, det_offsets, sizeof(int) * (e->S + 1));
}

// The caller's ID counters into the device counters (next_id may be null: keep the device's).
template <typename E>
int oc_put_next_id(E *e, const long long *next_id) {
    using Counters = typename E::Buf::Counters;
    if (!next_id) return YTA_OK;
    for (int s = 0; s < e->S; ++s) e->b.h_cnt[s].next_id = next_id[s];
    YTA_HIP(hipMemcpy2DAsync(&e->b.a.cnt[0].next_id, sizeof(Counters), &e->b.h_cnt[0].next_id,
                             sizeof(Counters), sizeof(long long), e->S, hipMemcpyHostToDevice,
                             e->stream));
    return YTA_OK;
}

// After the launch: counters, ID counters back, device errors, output offsets and rows.
template <typename E>
int oc_end_frame(E *e, long long *next_id, double *out, int out_capacity, int *out_offsets,
                 int invalid_bit = 0, const char *invalid_text = "") {
    const int S = e->S;
    int rc = oc_read_counters(e);
    if (rc) return rc;
    const auto *cnt = e->b.h_cnt;
    if (next_id)   // the device counters have advanced: hand them back even on an error below
        for (int s = 0; s < S; ++s) next_id[s] = cnt[s].next_id;
    rc = oc_check_errors(e, invalid_bit, invalid_text);
    if (rc) return rc;
    long long rows = 0;
    out_offsets[0] = 0;
    for (int s = 0; s < S; ++s) {
        rows += cnt[s].n_out;
        out_offsets[s + 1] = (int)rows;
    }
    YTA_CHECK(rows <= out_capacity, YTA_ERR_CAPACITY, "output needs %lld rows > capacity %d", rows,
              out_capacity);
    YTA_CHECK(rows == 0 || out, YTA_ERR_INVALID, "null out");
    for (int s = 0; s < S; ++s) {
        const int n = cnt[s].n_out;
        if (n)
            YTA_HIP(hipMemcpyAsync(out + (long long)out_offsets[s] * 8,
                                   e->b.out_own + (long long)s * e->b.a.CAP * 8,
                                   sizeof(double) * 8 * n, hipMemcpyDeviceToHost, e->stream));
    }
    YTA_HIP(host_wait(e->stream));
    return YTA_OK;
}

// ------------------------------------------------------------------ stage-1 snapshot (tests)
template <typename E>
int oc_debug_enable(E *e, int on) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    YTA_HIP(hipSetDevice(e->device));
    YTA_HIP(host_wait(e->stream));
    e->dbg.on = on != 0;
    if (!on) e->dbg.release();
    return YTA_OK;
}

// The engine's launch, with e->dbg.on, between its last cost kernel and its first solver kernel.
template <typename E>
int oc_debug_snapshot(E *e) {
    OcDebugCosts &g = e->dbg;
    const std::vector<OcDebugSrc> src = e->debug_sources();
    g.taken = false;
    g.dev.resize(src.size(), nullptr);
    g.bytes.resize(src.size(), 0);
    for (size_t k = 0; k < src.size(); ++k) {
        const size_t need = src[k].width * src[k].rows;
        if (g.bytes[k] != need || !g.dev[k]) {   // first use, or the engine has grown
            if (g.dev[k]) (void)hipFree(g.dev[k]);
            g.dev[k] = nullptr;
            g.bytes[k] = 0;
            YTA_HIP(hipMalloc(&g.dev[k], std::max<size_t>(need, 8)));
            g.bytes[k] = need;
        }
        if (!need) continue;
        if (src[k].rows == 1)
            YTA_HIP(hipMemcpyAsync(g.dev[k], src[k].src, need, hipMemcpyDeviceToDevice, e->stream));
        else
            YTA_HIP(hipMemcpy2DAsync(g.dev[k], src[k].width, src[k].src, src[k].pitch,
                                     src[k].width, src[k].rows, hipMemcpyDeviceToDevice,
                                     e->stream));
    }
    g.cap = e->b.a.CAP;
    g.maxd = e->b.a.MAXD;
    g.taken = true;
    return YTA_OK;
}

// Waits for the engine's stream.  *c: the counters of `stream` as the snapshot took them (n_high
// x n_trk is the matrix); rows: the input row of each matrix row; ids, boxes: the track id and
// the predicted box (x1, y1, x2, y2) of each matrix column (each may be null).
template <typename E>
int oc_debug_head(E *e, int stream, typename E::Buf::Counters *c, int *rows, long long *ids,
                  double *boxes) {
    using Counters = typename E::Buf::Counters;
    YTA_CHECK(e && c, YTA_ERR_INVALID, "null argument");
    YTA_CHECK(stream >= 0 && stream < e->S, YTA_ERR_INVALID, "bad stream %d", stream);
    const OcDebugCosts &g = e->dbg;
    YTA_CHECK(g.on && g.taken, YTA_ERR_INVALID,
              "no stage-1 snapshot: enable debug costs, then update");
    YTA_HIP(hipSetDevice(e->device));
    YTA_HIP(host_wait(e->stream));
    YTA_HIP(hipMemcpy(c, static_cast<const Counters *>(g.dev[ODB_CNT]) + stream, sizeof(Counters),
                      hipMemcpyDeviceToHost));
    YTA_CHECK(c->n_high >= 0 && c->n_high <= g.maxd && c->n_trk >= 0 && c->n_trk <= g.cap,
              YTA_ERR_HIP, "snapshot sizes %d x %d outside %d x %d", c->n_high, c->n_trk, g.maxd,
              g.cap);
    if (rows && c->n_high)
        YTA_HIP(hipMemcpy(rows, static_cast<const int *>(g.dev[ODB_ROWS]) + (size_t)stream * g.maxd,
                          sizeof(int) * c->n_high, hipMemcpyDeviceToHost));
    if (ids && c->n_trk) {
        std::vector<int> slot(c->n_trk);
        std::vector<long long> id(g.cap);
        YTA_HIP(hipMemcpy(slot.data(),
                          static_cast<const int *>(g.dev[ODB_SLOT]) + (size_t)stream * g.cap,
                          sizeof(int) * c->n_trk, hipMemcpyDeviceToHost));
        YTA_HIP(hipMemcpy(id.data(),
                          static_cast<const long long *>(g.dev[ODB_ID]) + (size_t)stream * g.cap,
                          sizeof(long long) * g.cap, hipMemcpyDeviceToHost));
        for (int j = 0; j < c->n_trk; ++j) {
            YTA_CHECK(slot[j] >= 0 && slot[j] < g.cap, YTA_ERR_HIP, "snapshot slot %d", slot[j]);
            ids[j] = id[slot[j]];
        }
    }
    if (boxes && c->n_trk)
        YTA_HIP(hipMemcpy(boxes,
                          static_cast<const double *>(g.dev[ODB_BOX]) + (size_t)stream * g.cap * 4,
                          sizeof(double) * 4 * c->n_trk, hipMemcpyDeviceToHost));
    return YTA_OK;
}

// n elements of source k from element `first` on (after oc_debug_head, which waited); dst may be
// null (nothing is read).
template <typename T, typename E>
int oc_debug_fetch(E *e, int k, long long first, long long n, T *dst) {
    const OcDebugCosts &g = e->dbg;
    if (!dst || n <= 0) return YTA_OK;
    YTA_CHECK((size_t)(first + n) * sizeof(T) <= g.bytes[k], YTA_ERR_HIP,
              "snapshot read past source %d", k);
    YTA_HIP(hipMemcpy(dst, static_cast<const T *>(g.dev[k]) + first, sizeof(T) * n,
                      hipMemcpyDeviceToHost));
    return YTA_OK;
}

// ------------------------------------------------------------------ the tensor path
// yta_<t>_update_tensors: device rows in, device rows out, stream-ordered.  The protocol is
// tensor_path.hpp's: the frame runs on the engine's stream as plain launches (k_tp_ingest, the
// engine's kernels, k_tp_out_offsets, k_tp_pack_rows), and nothing is waited for on the host unless
// the capacity bound below fails.
enum { OTS_FRAMES, OTS_HOST_WAITS, OTS_RESERVES, OTS_INGEST_SKIPPED, OTS_N };

// k_tp_pack_rows' accessor: a stream's live trackers after the frame into the slot.
template <typename C>
struct OcLive {
    const C *cnt;
    int *live;
    __device__ void operator()(int s) const { live[s] = cnt[s].n_trk; }
};

// Capacity before anything is enqueued.  max_dets from the frame's counts.  Track capacity as
// oc_begin_frame bounds it (births are appended before removals, so a stream's list never holds
// more than n_trk + m), through TrackBound.  Only a bound that does not fit waits for the engine
// stream and reads the exact counters; only an exact need that does not fit grows the engine, by
// oc_begin_frame's geometric rule.
template <typename E>
int oc_tensor_capacity(E *e, const int *counts) {
    OcTensorState &t = e->t;
    const int S = e->S, CAP = e->b.a.CAP, MAXD = e->b.a.MAXD;
    auto rebase = [&] { t.bound.rebase(S, [&](int s) { return e->b.h_cnt[s].n_trk; }); };
    if (!t.bound.dirty) rebase();
    int need_d = MAXD;
    for (int s = 0; s < S; ++s) need_d = std::max(need_d, counts[s]);
    if (need_d <= MAXD && t.bound.fits(t.ring, counts, CAP, [S](void *h, int s) {
            return oc_slot_view(h, S).live[s];
        }))
        return YTA_OK;
    ++t.stat[OTS_HOST_WAITS];
    int rc = oc_read_counters(e);
    if (rc) return rc;
    rebase();
    int need_c = CAP;
    for (int s = 0; s < S; ++s)
        need_c = (int)std::max<long long>(need_c, t.bound.base_live[s] + counts[s]);
    if (need_d <= MAXD && need_c <= CAP) return YTA_OK;
    ++t.stat[OTS_RESERVES];
    return oc_reserve(e, need_c > CAP ? std::max(need_c, 2 * CAP) : CAP,
                      need_d > MAXD ? std::max(need_d, 2 * MAXD) : MAXD);
}

// launch(d_dets, d_off, d_feats, d_wh): the engine's frame on e->stream from packed float64 rows,
// the S + 1 device offsets, one feature row per detection row (null: no embeddings) and the
// device image sizes (null: none given), writing e->b.out_own.
template <typename E, typename Launch>
int oc_update_tensors(E *e, void *caller_stream, const void *d_dets, int dtype,
                      long long row_stride, const int *det_counts, const float *d_feats,
                      long long feat_stride, const int *img_wh, const int *d_active,
                      const long long *next_id, double *d_rows, long long rows_capacity,
                      int *d_row_offsets, int *d_row_stream, Launch launch) {
    using Counters = typename E::Buf::Counters;
    long long total = 0;
    int rc = tensor_check_args(e, e ? e->S : 0, e ? e->D : 0, d_dets, dtype, row_stride,
                               det_counts, d_feats, feat_stride, d_rows, rows_capacity,
                               d_row_offsets, &total);
    if (rc) return rc;
    YTA_CHECK(img_wh || e->prm.asso_func != 4, YTA_ERR_INVALID, "centroid needs img_wh");
    YTA_CHECK(!e->dbg.on, YTA_ERR_INVALID,
              "debug costs are on: the tensor path takes no stage-1 snapshot");
    const int S = e->S, D = e->D;
    YTA_HIP(hipSetDevice(e->device));
    const hipStream_t cs = (hipStream_t)caller_stream;
    rc = frame_refuse_capture(cs);
    if (rc) return rc;
    rc = oc_tensor_capacity(e, det_counts);
    if (rc) return rc;
    OcTensorState &t = e->t;
    // float64 rows of 6, 16-byte aligned as the kernels' loads need: read where they are
    const bool in_place = dtype == YTA_F64 && row_stride == 6 && (uintptr_t)d_dets % 16 == 0;
    if (!t.off) {
        YTA_HIP(hipMalloc((void **)&t.off, sizeof(int) * (S + 1)));
        t.ring.slot_bytes = oc_slot_bytes(S);
        t.ring.host_waits = &t.stat[OTS_HOST_WAITS];
    }
    if (!t.wh) YTA_HIP(hipMalloc((void **)&t.wh, sizeof(int) * 2 * S));
    rc = tensor_stage(t.retired, &t.det, &t.det_cap, in_place ? 0 : 6 * total, 6 * 1024);
    if (rc) return rc;
    const bool gather = D > 0 && total > 0 && feat_stride != D;
    if (gather) {
        rc = tensor_stage(t.retired, &t.feat, &t.feat_cap, total * D, 1024LL * D);
        if (rc) return rc;
    }
    FrameSlot *p = nullptr;
    rc = t.ring.acquire(&p);
    if (rc) return rc;
    const OcSlotView hv = oc_slot_view(p->h, S), mv = oc_slot_view(p->m, S);
    memcpy(hv.counts, det_counts, sizeof(int) * S);
    if (next_id) memcpy(hv.nid, next_id, sizeof(long long) * S);
    if (img_wh) memcpy(hv.wh, img_wh, sizeof(int) * 2 * S);
    t.bound.enqueue(p, det_counts);
    ++t.stat[OTS_FRAMES];
    if (in_place) ++t.stat[OTS_INGEST_SKIPPED];
    rc = frame_hand_in(p, cs, e->stream);
    if (rc) return rc;
    rc = tensor_ingest(e->stream, d_dets, dtype, row_stride, in_place ? 0 : total, t.det,
                       mv.counts, next_id ? mv.nid : nullptr, img_wh ? mv.wh : nullptr, S, t.off,
                       e->b.a.cnt, t.wh);
    if (rc) return rc;
    if (gather)
        YTA_HIP(hipMemcpy2DAsync(t.feat, sizeof(float) * D, d_feats, sizeof(float) * feat_stride,
                                 sizeof(float) * D, (size_t)total, hipMemcpyDeviceToDevice,
                                 e->stream));
    e->mask.req_dev = d_active;
    rc = launch(in_place ? (const double *)d_dets : t.det, t.off,
                D > 0 ? (gather ? t.feat : d_feats) : nullptr, img_wh ? t.wh : nullptr);
    e->mask.req_dev = nullptr;
    if (rc) return rc;
    const int CAP = e->b.a.CAP;
    hipLaunchKernelGGL(k_tp_out_offsets<CountersNOut<Counters>>, dim3(1), dim3(TP_OFFS_T), 0,
                       e->stream, CountersNOut<Counters>{e->b.a.cnt}, S, CAP, d_row_offsets,
                       (int *)nullptr);
    hipLaunchKernelGGL(k_tp_pack_rows<OcLive<Counters>>, dim3(S), dim3(256), 0, e->stream,
                       e->b.out_own, (long long)CAP, S, d_row_offsets, d_rows, rows_capacity,
                       d_row_stream, OcLive<Counters>{e->b.a.cnt, mv.live});
    YTA_HIP(hipGetLastError());
    return frame_hand_back(p, cs, e->stream);
}

template <typename E>
int oc_tensor_stats(E *e, long long *out, int n) {
    YTA_CHECK(e && (out || n <= 0), YTA_ERR_INVALID, "null argument");
    for (int k = 0; k < n && k < OTS_N; ++k) out[k] = e->t.stat[k];
    return YTA_OK;
}

// The S per-stream ID counters as the device holds them (waits for the engine's stream).
template <typename E>
int oc_next_ids(E *e, long long *out) {
    YTA_CHECK(e && out, YTA_ERR_INVALID, "null argument");
    YTA_HIP(hipSetDevice(e->device));
    const int rc = oc_read_counters(e);
    if (rc) return rc;
    for (int s = 0; s < e->S; ++s) out[s] = e->b.h_cnt[s].next_id;
    return YTA_OK;
}

// ------------------------------------------------------------------ the small entry points
template <typename E>
int oc_reset(E *e) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    YTA_HIP(hipSetDevice(e->device));
    e->launch_reset(0, e->S);
    YTA_HIP(hipGetLastError());
    YTA_HIP(host_wait(e->stream));
    memset(e->b.h_cnt, 0, sizeof(typename E::Buf::Counters) * e->S);
    e->t.bound.exact();   // exact again: every tensor frame has run and been wiped
    return YTA_OK;
}

template <typename E>
int oc_reset_stream(E *e, int stream) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    YTA_CHECK(stream >= 0 && stream < e->S, YTA_ERR_INVALID, "stream %d outside 0..%d", stream,
              e->S - 1);
    YTA_HIP(hipSetDevice(e->device));
    e->launch_reset(stream, 1);
    YTA_HIP(hipGetLastError());
    YTA_HIP(host_wait(e->stream));
    return oc_read_counters(e);
}

template <typename E>
int oc_destroy(E *e) {
    if (!e) return YTA_OK;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)host_wait(e->stream);
    e->b.release();
    e->mask.release();
    e->dbg.release();
    e->t.ring.release();
    tensor_free_retired(e->t.retired);
    for (void *d : {(void *)e->t.det, (void *)e->t.off, (void *)e->t.wh, (void *)e->t.feat})
        if (d) (void)hipFree(d);
    if (e->h_dets) (void)hipHostFree(e->h_dets);
    if (e->d_det_in) (void)hipFree(e->d_det_in);
    if (e->h_feat) (void)hipHostFree(e->h_feat);
    if (e->d_feat) (void)hipFree(e->d_feat);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return YTA_OK;
}

// The engine's own parameter checks come first; feat_dim is the width the engine will use.
template <typename E, typename Params>
int oc_create(int device, int n_streams, int track_capacity, int max_dets, int feat_dim,
              const Params *params, E **engine) {
    *engine = nullptr;
    int rc = select_device(device);
    if (rc) return rc;
    E *e = new (std::nothrow) E();
    YTA_CHECK(e, YTA_ERR_NOMEM, "out of host memory");
    e->device = device;
    e->S = n_streams;
    e->D = feat_dim;
    e->prm = *params;
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he != hipSuccess) {
        set_error("hipStreamCreate: %s", hipGetErrorString(he));
        delete e;
        return YTA_ERR_HIP;
    }
    rc = e->alloc(track_capacity, max_dets, e->b);
    if (!rc) rc = oc_reset(e);
    if (rc) {
        oc_destroy(e);
        return rc;
    }
    *engine = e;
    return YTA_OK;
}

template <typename E>
int oc_capacity(E *e, int *track_capacity, int *max_dets) {
    YTA_CHECK(e && track_capacity && max_dets, YTA_ERR_INVALID, "null argument");
    *track_capacity = e->b.a.CAP;
    *max_dets = e->b.a.MAXD;
    return YTA_OK;
}

template <typename E>
int oc_sync(E *e, int invalid_bit = 0, const char *invalid_text = "") {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    const int rc = oc_read_counters(e);
    if (rc) return rc;
    return oc_check_errors(e, invalid_bit, invalid_text);
}

template <typename E>
int oc_lap_stats(E *e, long long *stats, int n) {
    YTA_CHECK(e && (stats || n <= 0), YTA_ERR_INVALID, "null argument");
    const int rc = oc_read_counters(e);
    if (rc) return rc;
    long long v[YTA_LAP_STATS] = {};
    for (int s = 0; s < e->S; ++s) {
        const LapStats &l = e->b.h_cnt[s].ls;
        v[0] += l.transposed;
        v[1] += l.uncertified;
        v[2] += l.replays;
        v[3] += l.reduced;
    }
    for (int k = 0; k < n && k < YTA_LAP_STATS; ++k) stats[k] = v[k];
    return YTA_OK;
}

template <typename E>
int oc_hip_stream(E *e, void **stream) {
    YTA_CHECK(e && stream, YTA_ERR_INVALID, "null argument");
    *stream = (void *)e->stream;
    return YTA_OK;
}

// ------------------------------------------------------------------ stream subsets (subset.hpp)
// update_device(): the engine's device-buffer update, run under the device mask d_active.
template <typename E, typename Update>
int oc_update_device_masked(E *e, const int *d_active, Update update_device) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    e->mask.req_dev = d_active;
    const int rc = update_device();
    e->mask.req_dev = nullptr;
    return rc;
}

// The listed streams updated, every other stream untouched.  update(mask, off, nid, full_oo) is
// the engine's full host-buffer update on the S + 1 offsets `off`, the ID counters `nid` (null
// when next_id is) and the S + 1 output offsets `full_oo`; it spreads the engine's own per-stream
// arguments with subset_spread (mask: [S], 1 for a listed stream).
template <typename E, typename Update>
int oc_update_streams(E *e, int n_streams, const int *stream_ids, const int *det_offsets,
                      long long *next_id, int *out_offsets, Update update) {
    YTA_CHECK(e && out_offsets, YTA_ERR_INVALID, "null argument");
    YTA_HIP(hipSetDevice(e->device));
    const int S = e->S;
    std::vector<int> mask, off, full_oo(S + 1, 0);
    int rc = subset_expand(S, n_streams, stream_ids, det_offsets, mask, off);
    if (rc) return rc;
    std::vector<long long> nid(S);
    if (next_id) {   // the skipped streams keep their device counters: read them first
        rc = oc_read_counters(e);
        if (rc) return rc;
        for (int s = 0; s < S; ++s) nid[s] = e->b.h_cnt[s].next_id;
        for (int k = 0; k < n_streams; ++k) nid[stream_ids[k]] = next_id[k];
    }
    e->mask.req_host = mask.data();
    rc = update(mask, off.data(), next_id ? nid.data() : nullptr, full_oo.data());
    e->mask.req_host = nullptr;
    if (next_id)
        for (int k = 0; k < n_streams; ++k) next_id[k] = nid[stream_ids[k]];
    if (rc) return rc;
    subset_compact(n_streams, stream_ids, full_oo, out_offsets);
    return YTA_OK;
}

}  // namespace yta
