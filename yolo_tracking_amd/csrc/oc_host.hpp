// Host side shared by the engines (no device code).
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
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "common.hpp"
#include "ocsort_common.hpp"
#include "subset.hpp"

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
    return YTA_OK;
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
    YTA_HIP(host_wait(e->stream));
    typename E::Buf n;
    int rc = e->alloc(cap, maxd, n);
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
                                   e->b.a.out + (long long)s * e->b.a.CAP * 8,
                                   sizeof(double) * 8 * n, hipMemcpyDeviceToHost, e->stream));
    }
    YTA_HIP(host_wait(e->stream));
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
