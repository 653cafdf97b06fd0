// Tensor path of the camera-motion engines (yta_sof_apply_tensors in cmc.hip, yta_ecc_apply_tensors
// in ecc.hip): the frames are S device tensors read where they are, addressed through a pointer
// table (frame s = its first pixel's address, its h x w and its row pitch in bytes), and the call
// is stream-ordered against the caller's stream with no host wait.  The protocol (slots, hand-off)
// is tensor_path.hpp's; here is what the two engines add to it: a slot's payload, the one-block
// kernel that brings it into HBM, the checks of the frame table and the typed read of a detection
// row.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.hpp"
#include "tensor_path.hpp"

namespace yta {
namespace cmc {

// One element of a detection row of YTA_F64 / YTA_F32 / YTA_F16, promoted exactly to float64.  A
// scalar load per element: rows may start at any element alignment.
__device__ __forceinline__ double det_el(const void *rows, int dtype, long long i) {
    return dtype == YTA_F64   ? static_cast<const double *>(rows)[i]
           : dtype == YTA_F32 ? (double)static_cast<const float *>(rows)[i]
                              : (double)static_cast<const _Float16 *>(rows)[i];
}

enum { CTS_FRAMES, CTS_HOST_WAITS, CTS_N };
constexpr int CMC_ING_T = 256;

struct CmcTensors {
    FrameRing ring;
    long long stat[CTS_N] = {};   // frames enqueued; calls that blocked on the device
    // the call's arrays in HBM (k_cmc_ingest), read by the engine's kernels; one set serves every
    // frame in flight, since the engine's stream runs them in order
    const uint8_t **ptr = nullptr;   // [S]
    long long *pitch = nullptr;      // [S]
    int *hw = nullptr;               // [S][2]
    int *off = nullptr;              // [S + 1] detection offsets
};

// A slot's block, which the engine's first launch reads: a call's host arrays, S frame addresses,
// S pitches, S x (h, w), S detection counts (SparseOptFlow only).
inline size_t cmc_slot_bytes(size_t S) { return S * (8 + 8 + 8 + 4); }
struct CmcSlotView {
    const uint8_t **ptr;
    long long *pitch;
    int *hw, *counts;
};
inline CmcSlotView cmc_slot_view(void *base, size_t S) {
    char *b = static_cast<char *>(base);
    return {reinterpret_cast<const uint8_t **>(b), reinterpret_cast<long long *>(b + 8 * S),
            reinterpret_cast<int *>(b + 16 * S), reinterpret_cast<int *>(b + 24 * S)};
}

// The slot's arrays into HBM, and the S + 1 detection offsets as the prefix sums of the counts
// (COUNTS false: ECC has none).  One block for any S: each thread takes a run of streams.
template <bool COUNTS>
__global__ __launch_bounds__(CMC_ING_T) void k_cmc_ingest(CmcSlotView in, int S,
                                                          const uint8_t **ptr, long long *pitch,
                                                          int *hw, int *off) {
    __shared__ int part[CMC_ING_T];
    const int t = threadIdx.x;
    const int per = (S + CMC_ING_T - 1) / CMC_ING_T, s0 = min(S, t * per), s1 = min(S, s0 + per);
    int sum = 0;
    for (int s = s0; s < s1; ++s) {
        ptr[s] = in.ptr[s];
        pitch[s] = in.pitch[s];
        hw[2 * s] = in.hw[2 * s];
        hw[2 * s + 1] = in.hw[2 * s + 1];
        if (COUNTS) sum += max(in.counts[s], 0);
    }
    if (!COUNTS) return;
    int r = block_run_scan<CMC_ING_T>(sum, part);
    if (t == 0) off[0] = 0;
    for (int s = s0; s < s1; ++s) {
        r += max(in.counts[s], 0);
        off[s + 1] = r;
    }
}

inline void cmc_tensors_free(CmcTensors &t) {
    t.ring.release();
    for (void *d : {(void *)t.ptr, (void *)t.pitch, (void *)t.hw, (void *)t.off})
        if (d) (void)hipFree(d);
    t.ptr = nullptr;
    t.pitch = nullptr;
    t.hw = nullptr;
    t.off = nullptr;
}

// What both engines refuse before anything is enqueued (a capturing caller stream last).
inline int cmc_check_frames(int S, hipStream_t cs, const void *const *frames, const int *frame_hw,
                            const long long *frame_pitch) {
    YTA_CHECK(frames && frame_hw && frame_pitch, YTA_ERR_INVALID, "null argument");
    for (int s = 0; s < S; ++s) {
        const int h = frame_hw[2 * s], w = frame_hw[2 * s + 1];
        YTA_CHECK(frames[s], YTA_ERR_INVALID, "stream %d: null frame", s);
        YTA_CHECK(h >= 1 && w >= 1, YTA_ERR_INVALID, "stream %d: bad frame %d x %d", s, h, w);
        YTA_CHECK(w <= 0x7fffffff / 3 && frame_pitch[s] >= 3LL * w && frame_pitch[s] <= 0x7fffffffLL,
                  YTA_ERR_INVALID, "stream %d: pitch %lld outside 3 * w = %lld .. 2^31 - 1", s,
                  frame_pitch[s], 3LL * w);
    }
    return frame_refuse_capture(cs);
}

// Take a slot, copy the call's host arrays into it (reusable by the caller at once), order the
// engine's stream after everything queued on the caller's so far, and bring the arrays into HBM.
inline int cmc_hand_in(CmcTensors &t, int S, hipStream_t cs, hipStream_t es,
                       const void *const *frames, const int *frame_hw,
                       const long long *frame_pitch, const int *det_counts, FrameSlot **slot) {
    if (!t.ptr) {
        t.ring.slot_bytes = cmc_slot_bytes((size_t)S);
        t.ring.host_waits = &t.stat[CTS_HOST_WAITS];
        YTA_HIP(hipMalloc((void **)&t.ptr, sizeof(void *) * S));
        YTA_HIP(hipMalloc((void **)&t.pitch, sizeof(long long) * S));
        YTA_HIP(hipMalloc((void **)&t.hw, sizeof(int) * 2 * S));
        YTA_HIP(hipMalloc((void **)&t.off, sizeof(int) * (S + 1)));
    }
    FrameSlot *p = nullptr;
    int rc = t.ring.acquire(&p);
    if (rc) return rc;
    const CmcSlotView hv = cmc_slot_view(p->h, (size_t)S);
    memcpy(hv.ptr, frames, sizeof(void *) * S);
    memcpy(hv.pitch, frame_pitch, sizeof(long long) * S);
    memcpy(hv.hw, frame_hw, sizeof(int) * 2 * S);
    if (det_counts) memcpy(hv.counts, det_counts, sizeof(int) * S);
    ++t.stat[CTS_FRAMES];
    rc = frame_hand_in(p, cs, es);
    if (rc) return rc;
    const CmcSlotView mv = cmc_slot_view(p->m, (size_t)S);
    if (det_counts)
        hipLaunchKernelGGL(k_cmc_ingest<true>, dim3(1), dim3(CMC_ING_T), 0, es, mv, S, t.ptr,
                           t.pitch, t.hw, t.off);
    else
        hipLaunchKernelGGL(k_cmc_ingest<false>, dim3(1), dim3(CMC_ING_T), 0, es, mv, S, t.ptr,
                           t.pitch, t.hw, t.off);
    YTA_HIP(hipGetLastError());
    *slot = p;
    return YTA_OK;
}

inline int cmc_tensor_stats(const CmcTensors &t, long long *out, int n) {
    YTA_CHECK(out || n <= 0, YTA_ERR_INVALID, "null argument");
    for (int k = 0; k < n && k < CTS_N; ++k) out[k] = t.stat[k];
    return YTA_OK;
}

}  // namespace cmc
}  // namespace yta
