// StrongSORT (boxmot/trackers/strongsort/, motion/kalman_filters/strongsort_kf.py,
// utils/matching.py:224-378) on the device: S independent streams per launch sequence, state
// resident in HBM.
//
// Per frame (strong_sort.py:42-99, sort/tracker.py:62-157):
//   k_ss_pre     [S]             camera_update (track.py:129-138) + predict + age / tsu counters
//                                for every track, detection tlwh / xyah, the confirmed-row list
//   k_ss_norm    [dets, S]       f / |f| of every detection row (one wave per row, pinned order)
//   k_ss_gal     [tiles, rows, S] the nearest-neighbour cosine distance over the galleries
//                                (matching.py:290-308, :360-378) on v_mfma_f32_32x32x2_f32: a wave
//                                takes one confirmed track x 32 detections, walks the track's
//                                gallery in tiles of 32 rows (rows past its length masked, so the
//                                budget is padded per tile and no row is materialised per pair),
//                                min over the rows in the epilogue; the epilogue also computes the
//                                gating distance (linear_assignment.py:144-200) from the track's
//                                state and writes lambda * cost + (1 - lambda) * gd in float64,
//                                clamped at max_dist as min_cost_matching does
//   k_ss_match   [S]             stage 1: SciPy replay (lsa_replay.hpp) + the unmatched
//                                lists in min_cost_matching's order; stage 2: IoU cost
//                                (iou_matching.py:10-87) of the unconfirmed tracks and stage 1's
//                                unmatched tracks with time_since_update == 1 against stage 1's
//                                unmatched detections in the order stage 1 returned them, clamp,
//                                replay, births in the order stage 2 returned them
//   k_ss_apply   [S]             NSA update (strongsort_kf.py:124-189), state machine
//                                (track.py:176-186), order-preserving compaction, births
//                                (tracker.py:159-169), output rows
//   k_ss_feat    [tracks, S]     EMA feature (track.py:168-174), features of the births, gallery
//                                ring append (tracker.py:96-106, matching.py:343-358); one wave
//                                per track
// All six take an [S] mask (SsArgs::active; null: every stream): a masked stream's blocks return
// before their first barrier and leave its state untouched (update_streams, update_device_masked,
// update_tensors' `active`).  A tensor frame (yta_strongsort_update_tensors, protocol:
// tensor_path.hpp) wraps them in three: k_ss_ingest in front (counts, offsets, ID counters and the
// widened detection rows; the feature rows stay where the caller has them, k_ss_norm reads them
// through SsArgs::foff / fstride), k_tp_out_offsets and k_tp_pack_rows behind.
//
// Float32 order (the reference's np.dot / np.linalg.norm fix none; tests/strongsort_oracle.py
// restates this one, device against restatement is bit-exact):
//   norm   lane l of a wave sums x[k]^2 over k = l, l + 64, ... in increasing k, then the
//          butterfly p += p[l ^ 32], ^16, ^8, ^4, ^2, ^1; sqrtf and the division are IEEE
//   dot    the MFMA's k-ordered fmaf chain from +0; a lane loads 8 consecutive k of its row
//          (k0 + 8 (lane >> 5) ...), so within a block of 16 the chain visits
//          k = 0, 8, 1, 9, ..., 7, 15
//   cost   1 - dot, min over the track's rows; gallery rows are stored as g / |g|, which is what
//          _cosine_distance makes of them on every call
//   EMA    s = (float)alpha * last + (float)(1 - alpha) * f, s / |s|
//
// Tracks live in slots (Kalman record, counters, feature, gallery ring); the track list is an
// ordered array of slots, so deleting a track moves no gallery.  Stage 2's rows after the
// unconfirmed tracks are in ascending list position (the reference iterates a Python set there).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "kf_xyah.hpp"
#include "lsa_replay.hpp"
#include "subset.hpp"
#include "tensor_path.hpp"

using namespace yta;

namespace {

constexpr double SS_GATE = 9.4877;     // chi2inv95[4], strongsort_kf.py:13
constexpr double SS_INFTY = 1e5;       // linear_assignment.py:10
constexpr int SS_T = 256;
enum { H_NTRK, H_NFREE, H_NEXT, H_ERR, H_NCONF, H_NUND, H_NROWS2, H_NBIRTH, H_N };
enum { T_ID, T_HITS, T_AGE, T_TSU, T_STATE, T_N };   // state: 0 free, 1 tentative, 2 confirmed
constexpr int SS_ERR_CAPACITY = 1, SS_ERR_SOLVER = 2;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct SsArgs {
    int S, CAP, MAXD, D, B;
    double max_dist, max_iou, lambda;
    int max_age, n_init;
    float ema_a, ema_b;
    const double *dets;     // S x MAXD x 6
    const int *ndet;        // S
    const float *feats;     // S x MAXD x D; with foff: packed rows, fstride floats apart
    const int *foff;        // S + 1 row offsets of the packed feats (the tensor path) or null
    long long fstride;
    const int *active;      // S (0: the stream is left exactly as it is) or null: every stream
    const double *warps;    // S x 6 (a NaN first value: no camera update) or null
    double *kf;             // S x CAP x 24, by slot
    int *ti;                // S x CAP x T_N
    double *td;             // S x CAP x 3: conf, cls, det_ind
    float *feat;            // S x CAP x D: features[-1]
    float *gal;             // S x CAP x B x D, rows g / |g|
    int *gcnt;              // S x CAP: rows appended (the ring position is gcnt % B)
    int *order, *order2;    // S x CAP: the track list
    int *freel;             // S x CAP: free slots (stack)
    int *hdr;               // S x H_N
    float *fn;              // S x MAXD x D
    double *dbox;           // S x MAXD x 8: tlwh, xyah
    int *crow;              // S x CAP: list positions of the confirmed tracks
    double *cost;           // S x CAP x MAXD
    int *tmatch;            // S x CAP: detection of list position k or -1
    int *flag;              // S x CAP
    int *und, *cmark;       // S x MAXD
    int *rows2, *rx;        // S x CAP
    int *births;            // S x MAXD: detections that start tracks, in order
    int *sact;              // S x CAP, by slot: what k_ss_feat does (see k_ss_apply)
    double *out;            // S x CAP x 8
    int *nout;              // S
    int *ntrk_out;          // S
};

__device__ __forceinline__ void kf_load(const double *p, KfState &s) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s.m[k] = p[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) s.c[k] = p[8 + k];
}
__device__ __forceinline__ void kf_store(double *p, const KfState &s) {
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = s.m[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) p[8 + k] = s.c[k];
}

// Pinned-order sum of squares over a wave (see the header); every lane returns the sum.
__device__ __forceinline__ float wave_sumsq(const float *x, int D) {
    float p = 0.f;
    for (int k = lane_id(); k < D; k += WAVE) p = p + x[k] * x[k];
#pragma unroll
    for (int off = 32; off; off >>= 1) p = p + __shfl_xor(p, off);
    return p;
}
// dst = src / |src| by one wave (dst may be src)
__device__ __forceinline__ void wave_normalize(const float *src, float *dst, int D) {
    const float n = sqrtf(wave_sumsq(src, D));
    for (int k = lane_id(); k < D; k += WAVE) dst[k] = src[k] / n;
}

// ------------------------------------------------------------------------------------ k_ss_pre
__global__ __launch_bounds__(SS_T) void k_ss_pre(SsArgs a) {
    __shared__ int wsum[16];
    const int s = blockIdx.x, t = threadIdx.x;
    if (a.active && !a.active[s]) return;                  // block-uniform, before any barrier
    const long long tb = (long long)s * a.CAP, db = (long long)s * a.MAXD;
    int *hdr = a.hdr + s * H_N;
    const int n = hdr[H_NTRK], m = a.ndet[s];
    const double *H = a.warps ? a.warps + 6 * s : nullptr;
    const bool warp = H && H[0] == H[0];
    for (int k = t; k < n; k += SS_T) {
        const int slot = a.order[tb + k];
        KfState st;
        kf_load(a.kf + (tb + slot) * KF_REC, st);
        if (warp) kf_camera_update(st.m, H);
        kf_predict<KF_XYAH>(st);
        kf_store(a.kf + (tb + slot) * KF_REC, st);
        int *ti = a.ti + (tb + slot) * T_N;
        ti[T_AGE] += 1;
        ti[T_TSU] += 1;
        a.tmatch[tb + k] = -1;
    }
    for (int j = t; j < m; j += SS_T) {
        const double *d = a.dets + (db + j) * 6;
        double *o = a.dbox + (db + j) * 8;
        const double w = d[2] - d[0], h = d[3] - d[1];   // ops.py xyxy2tlwh
        o[0] = d[0];
        o[1] = d[1];
        o[2] = w;
        o[3] = h;
        o[4] = d[0] + w / 2;                             // detection.py:34-41 to_xyah
        o[5] = d[1] + h / 2;
        o[6] = w / h;
        o[7] = h;
    }
    const int nc = block_compact(
        n, wsum, [&](int k) { return a.ti[(tb + a.order[tb + k]) * T_N + T_STATE] == 2; },
        [&](int k, int pos) { a.crow[tb + pos] = k; });
    if (t == 0) hdr[H_NCONF] = nc;
}

// ----------------------------------------------------------------------------------- k_ss_norm
__global__ __launch_bounds__(SS_T) void k_ss_norm(SsArgs a) {
    const int s = blockIdx.y;
    const int j = blockIdx.x * (SS_T / WAVE) + threadIdx.x / WAVE;
    if ((a.active && !a.active[s]) || j >= a.ndet[s]) return;
    const long long off = ((long long)s * a.MAXD + j) * a.D;
    const float *src = a.foff ? a.feats + ((long long)a.foff[s] + j) * a.fstride : a.feats + off;
    wave_normalize(src, a.fn + off, a.D);
}

// ------------------------------------------------------------------------------------ k_ss_gal
// One wave: min over `len` rows g (row stride D) of 1 - <g, f_j> for the 32 columns j0 + (lane &
// 31) of fn (rows < m).  v_mfma_f32_32x32x2_f32: lane l holds A[l & 31][k = l >> 5] and
// B[k = l >> 5][l & 31]; D register q of lane l is row (q & 3) + 8 (q >> 2) + 4 (l >> 5), column
// l & 31.  VEC: D % 16 == 0, rows read as two float4.
template <bool VEC>
__device__ __forceinline__ float gal_wave_min(const float *g, int len, int D, const float *fn,
                                              int j0, int m) {
    const int lane = lane_id(), r = lane & 31, h = lane >> 5;
    const int j = j0 + r;
    const float *brow = fn + (long long)(j < m ? j : m - 1) * D;
    float cmin = INFINITY;
    for (int r0 = 0; r0 < len; r0 += 32) {
        const int row = r0 + r;
        const float *arow = g + (long long)(row < len ? row : len - 1) * D;
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        for (int k0 = 0; k0 < D; k0 += 16) {
            float av[8], bv[8];
            const int kb = k0 + 8 * h;
            if (VEC) {
                const float4 a0 = *(const float4 *)(arow + kb), a1 = *(const float4 *)(arow + kb + 4);
                const float4 b0 = *(const float4 *)(brow + kb), b1 = *(const float4 *)(brow + kb + 4);
                av[0] = a0.x, av[1] = a0.y, av[2] = a0.z, av[3] = a0.w;
                av[4] = a1.x, av[5] = a1.y, av[6] = a1.z, av[7] = a1.w;
                bv[0] = b0.x, bv[1] = b0.y, bv[2] = b0.z, bv[3] = b0.w;
                bv[4] = b1.x, bv[5] = b1.y, bv[6] = b1.z, bv[7] = b1.w;
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    av[u] = kb + u < D ? arow[kb + u] : 0.f;
                    bv[u] = kb + u < D ? brow[kb + u] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int rr = r0 + (q & 3) + 8 * (q >> 2) + 4 * h;
            if (rr < len) cmin = fminf(cmin, 1.0f - acc[q]);
        }
    }
    return fminf(cmin, __shfl_xor(cmin, 32));
}

template <bool VEC>
__global__ __launch_bounds__(SS_T) void k_ss_gal(SsArgs a) {
    const int s = blockIdx.z, r = blockIdx.y;
    if (a.active && !a.active[s]) return;
    const int *hdr = a.hdr + s * H_N;
    const int m = a.ndet[s];
    if (r >= hdr[H_NCONF]) return;
    const int j0 = (blockIdx.x * (SS_T / WAVE) + threadIdx.x / WAVE) * 32;
    if (j0 >= m) return;                                   // wave-uniform; no barrier below
    const long long tb = (long long)s * a.CAP, db = (long long)s * a.MAXD;
    const int slot = a.order[tb + a.crow[tb + r]];
    const int cnt = a.gcnt[tb + slot], len = cnt < a.B ? cnt : a.B;
    const float c = gal_wave_min<VEC>(a.gal + (tb + slot) * a.B * a.D, len, a.D, a.fn + db * a.D,
                                      j0, m);
    const int lane = lane_id(), j = j0 + (lane & 31);
    if (lane >= 32 || j >= m) return;
    const double *kf = a.kf + (tb + slot) * KF_REC;
    const double pp[4] = {kf[8], kf[12], kf[16], kf[20]};
    const double gd = kf_gating_xyah(kf, pp, a.dbox + (db + j) * 8 + 4);
    double v = (double)c;
    if (gd > SS_GATE) v = SS_INFTY;
    // column-major when rows > columns: the solver then walks the transposed problem's rows
    // along the unit stride
    const int nconf = hdr[H_NCONF];
    double *cost = a.cost + tb * a.MAXD;
    double cv = a.lambda * v + (1 - a.lambda) * gd;
    if (cv > a.max_dist) cv = a.max_dist + 1e-5;           // linear_assignment.py:60
    cost[nconf > m ? (long long)j * a.CAP + r : (long long)r * a.MAXD + j] = cv;
}

// ---------------------------------------------------------------------------------- k_ss_match
// min_cost_matching (linear_assignment.py:59-78) on cost (nr x nc, element (i, j) at
// i * rs + j * cs), which its producer has already clamped (:60, an element-wise step done where
// the matrix is written, chip-wide for stage 1): replay, then the unmatched columns in the
// reference's order (not assigned in column order, then the columns of assigned-but-clamped pairs
// in row order) and the matches.
template <typename OnMatch>
__device__ inline int ss_min_cost_matching(const double *cost, int nr, int nc, long long rs,
                                           long long cs, double max_distance, const LsaWs &w,
                                           LsaShared &sh, int *wsum, int *rx, int *cmark,
                                           int *un_cols, int *err, OnMatch on_match) {
    const int t = threadIdx.x, nt = blockDim.x;
    if (nr == 0 || nc == 0) {                              // :56-57 nothing to match
        for (int j = t; j < nc; j += nt) un_cols[j] = j;
        block_sync();
        return nc;
    }
    for (int j = t; j < nc; j += nt) cmark[j] = 0;
    block_sync();
    if (!lsa_replay_block(cost, nr, nc, rs, cs, w, sh, rx)) {
        if (t == 0) atomicOr(err, SS_ERR_SOLVER);
        for (int i = t; i < nr; i += nt) rx[i] = -1;
        block_sync();
    }
    for (int i = t; i < nr; i += nt)
        if (rx[i] >= 0) cmark[rx[i]] = 1;
    block_sync();
    auto clamped = [&](int i) { return rx[i] >= 0 && cost[i * rs + rx[i] * cs] > max_distance; };
    const int n1 = block_compact(
        nc, wsum, [&](int j) { return !cmark[j]; }, [&](int j, int pos) { un_cols[pos] = j; });
    const int n2 = block_compact(nr, wsum, clamped,
                                 [&](int i, int pos) { un_cols[n1 + pos] = rx[i]; });
    for (int i = t; i < nr; i += nt)
        if (rx[i] >= 0 && !clamped(i)) on_match(i, rx[i]);
    block_sync();
    return n1 + n2;
}

__global__ __launch_bounds__(LSA_T) void k_ss_match(SsArgs a, int ws_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ LsaShared sh;
    __shared__ int wsum[16];
    const int s = blockIdx.x, t = threadIdx.x;
    if (a.active && !a.active[s]) return;                  // block-uniform, before any barrier
    const long long tb = (long long)s * a.CAP, db = (long long)s * a.MAXD;
    int *hdr = a.hdr + s * H_N;
    const int n = hdr[H_NTRK], m = a.ndet[s], nconf = hdr[H_NCONF];
    const LsaWs w = lsa_ws_carve(smem, ws_n);
    double *cost = a.cost + tb * a.MAXD;
    int *und = a.und + db, *tmatch = a.tmatch + tb, *rows2 = a.rows2 + tb;
    const int *crow = a.crow + tb, *order = a.order + tb;
    // stage 1 (tracker.py:128-136); k_ss_gal wrote the matrix column-major when rows > columns
    const bool colmajor = nconf > m;
    const int nund = ss_min_cost_matching(cost, nconf, m, colmajor ? 1 : a.MAXD,
                                          colmajor ? a.CAP : 1, a.max_dist, w, sh, wsum, a.rx + tb,
                                          a.cmark + db, und, hdr + H_ERR,
                                          [&](int i, int j) { tmatch[crow[i]] = j; });
    // stage 2 rows (tracker.py:139-144)
    const int nr_a = block_compact(
        n, wsum, [&](int k) { return a.ti[(tb + order[k]) * T_N + T_STATE] == 1; },
        [&](int k, int pos) { rows2[pos] = k; });
    const int nr_b = block_compact(
        nconf, wsum,
        [&](int i) {
            const int k = crow[i];
            return tmatch[k] < 0 && a.ti[(tb + order[k]) * T_N + T_TSU] == 1;
        },
        [&](int i, int pos) { rows2[nr_a + pos] = crow[i]; });
    block_sync();
    const int nr2 = nr_a + nr_b;
    // iou_cost (iou_matching.py:49-87)
    for (long long e = t; e < (long long)nr2 * nund; e += LSA_T) {
        const int i = (int)(e / nund), c = (int)(e % nund);
        const int slot = order[rows2[i]];
        double v;
        if (a.ti[(tb + slot) * T_N + T_TSU] > 1) {
            v = SS_INFTY;
        } else {
            const double *mm = a.kf + (tb + slot) * KF_REC;
            const double bw = mm[2] * mm[3], bh = mm[3];
            const double bx = mm[0] - bw / 2, by = mm[1] - bh / 2;
            const double *d = a.dbox + (db + und[c]) * 8;
            const double brx = bx + bw, bry = by + bh, crx = d[0] + d[2], cry = d[1] + d[3];
            const double iw = np_max(0.0, np_min(brx, crx) - np_max(bx, d[0]));
            const double ih = np_max(0.0, np_min(bry, cry) - np_max(by, d[1]));
            const double ai = iw * ih;
            v = 1.0 - ai / (bw * bh + d[2] * d[3] - ai);
        }
        if (v > a.max_iou) v = a.max_iou + 1e-5;           // linear_assignment.py:60
        cost[(long long)i * a.MAXD + c] = v;
    }
    block_sync();
    int *births = a.births + db;
    const int nb = ss_min_cost_matching(cost, nr2, nund, a.MAXD, 1, a.max_iou, w, sh, wsum,
                                        a.rx + tb, a.cmark + db, births, hdr + H_ERR,
                                        [&](int i, int j) { tmatch[rows2[i]] = und[j]; });
    for (int k = t; k < nb; k += LSA_T) births[k] = und[births[k]];
    if (t == 0) hdr[H_NBIRTH] = nb;
}

// ---------------------------------------------------------------------------------- k_ss_apply
// Per stream: Kalman updates and the state machine, the new track list (deleted tracks leave,
// births are appended), output rows.  What each slot's feature needs is left in sact for
// k_ss_feat: -1 nothing, j >= 0 the EMA with detection j, -(j + 2) born from detection j.
__global__ __launch_bounds__(SS_T) void k_ss_apply(SsArgs a) {
    __shared__ int wsum[16];
    const int s = blockIdx.x, t = threadIdx.x;
    if (a.active && !a.active[s]) {   // block-uniform, before any barrier: no rows, the old count
        if (t == 0) {
            a.nout[s] = 0;
            a.ntrk_out[s] = a.hdr[s * H_N + H_NTRK];
        }
        return;
    }
    const long long tb = (long long)s * a.CAP, db = (long long)s * a.MAXD;
    int *hdr = a.hdr + s * H_N;
    const int n = hdr[H_NTRK], nb = hdr[H_NBIRTH], nf0 = hdr[H_NFREE], next0 = hdr[H_NEXT];
    int *order = a.order + tb, *order2 = a.order2 + tb, *flag = a.flag + tb;
    const int *tmatch = a.tmatch + tb;
    // matched: Track.update (track.py:152-179); unmatched: mark_missed (:181-186)
    for (int k = t; k < n; k += SS_T) {
        const int slot = order[k], j = tmatch[k];
        int *ti = a.ti + (tb + slot) * T_N;
        a.sact[tb + slot] = j;
        if (j >= 0) {
            const double *d = a.dets + (db + j) * 6;
            KfState st;
            kf_load(a.kf + (tb + slot) * KF_REC, st);
            kf_update_nsa(st, a.dbox + (db + j) * 8 + 4, d[4]);
            kf_store(a.kf + (tb + slot) * KF_REC, st);
            double *td = a.td + (tb + slot) * 3;
            td[0] = d[4];
            td[1] = d[5];
            td[2] = (double)j;
            ti[T_HITS] += 1;
            ti[T_TSU] = 0;
            if (ti[T_STATE] == 1 && ti[T_HITS] >= a.n_init) ti[T_STATE] = 2;
            flag[k] = 0;
        } else {
            flag[k] = ti[T_STATE] == 1 || ti[T_TSU] > a.max_age;
        }
    }
    block_sync();
    // deleted tracks leave the list (order preserved), their slots return to the free stack
    const int kept = block_compact(
        n, wsum, [&](int k) { return !flag[k]; }, [&](int k, int pos) { order2[pos] = order[k]; });
    const int freed = block_compact(
        n, wsum, [&](int k) { return flag[k] != 0; },
        [&](int k, int pos) {
            const int slot = order[k];
            a.ti[(tb + slot) * T_N + T_STATE] = 0;
            a.freel[tb + nf0 + pos] = slot;
        });
    block_sync();
    // births in the order stage 2 returned them (tracker.py:92-93, :159-169; Track.__init__
    // track.py:70-98)
    const int nf = nf0 + freed, born = nb < nf ? nb : nf;
    for (int b = t; b < born; b += SS_T) {
        const int j = a.births[db + b], slot = a.freel[tb + nf - 1 - b];
        order2[kept + b] = slot;
        const double *d = a.dets + (db + j) * 6;
        KfState st;
        kf_initiate<KF_XYAH>(a.dbox + (db + j) * 8 + 4, st);
        kf_store(a.kf + (tb + slot) * KF_REC, st);
        int *ti = a.ti + (tb + slot) * T_N;
        ti[T_ID] = next0 + b;
        ti[T_HITS] = 1;
        ti[T_AGE] = 1;
        ti[T_TSU] = 0;
        ti[T_STATE] = 1;
        double *td = a.td + (tb + slot) * 3;
        td[0] = d[4];
        td[1] = d[5];
        td[2] = (double)j;
        a.gcnt[tb + slot] = 0;
        a.sact[tb + slot] = -(j + 2);
    }
    const int nn = kept + born;
    if (t == 0) {
        if (born < nb) atomicOr(hdr + H_ERR, SS_ERR_CAPACITY);
        hdr[H_NFREE] = nf - born;
        hdr[H_NEXT] = next0 + born;
        hdr[H_NTRK] = nn;
        a.ntrk_out[s] = nn;
    }
    block_sync();
    for (int k = t; k < nn; k += SS_T) order[k] = order2[k];
    block_sync();
    // output rows (strong_sort.py:82-99)
    double *out = a.out + tb * 8;
    const int no = block_compact(
        nn, wsum,
        [&](int k) {
            const int *ti = a.ti + (tb + order[k]) * T_N;
            return ti[T_STATE] == 2 && ti[T_TSU] < 1;
        },
        [&](int k, int pos) {
            const int slot = order[k];
            const double *mm = a.kf + (tb + slot) * KF_REC;
            const double *td = a.td + (tb + slot) * 3;
            const double w = mm[2] * mm[3];
            const double x1 = mm[0] - w / 2, y1 = mm[1] - mm[3] / 2;
            double *o = out + pos * 8;
            o[0] = x1;
            o[1] = y1;
            o[2] = x1 + w;
            o[3] = y1 + mm[3];
            o[4] = (double)a.ti[(tb + slot) * T_N + T_ID];
            o[5] = td[0];
            o[6] = td[1];
            o[7] = td[2];
        });
    if (t == 0) a.nout[s] = no;
}

// ----------------------------------------------------------------------------------- k_ss_feat
// One wave per track of the new list: the EMA feature of a matched track (track.py:168-174), the
// normalised feature of a born one (:90-92), then the gallery append of every confirmed track
// (tracker.py:96-106; the last nn_budget rows are kept, matching.py:354-357).
__global__ __launch_bounds__(SS_T) void k_ss_feat(SsArgs a) {
    const int s = blockIdx.y, lane = lane_id();
    const int k = blockIdx.x * (SS_T / WAVE) + threadIdx.x / WAVE;
    if ((a.active && !a.active[s]) || k >= a.hdr[s * H_N + H_NTRK]) return;
    const long long tb = (long long)s * a.CAP, db = (long long)s * a.MAXD;
    const int slot = a.order[tb + k], act = a.sact[tb + slot];
    float *f = a.feat + (tb + slot) * a.D;
    if (act <= -2) {
        const float *g = a.fn + (db + (-act - 2)) * a.D;
        for (int e = lane; e < a.D; e += WAVE) f[e] = g[e];
    } else if (act >= 0) {
        const float *g = a.fn + (db + act) * a.D;
        for (int e = lane; e < a.D; e += WAVE) {
            const float x = a.ema_a * f[e], y = a.ema_b * g[e];
            f[e] = x + y;
        }
        wave_normalize(f, f, a.D);
    }
    if (a.ti[(tb + slot) * T_N + T_STATE] != 2) return;
    const int cnt = a.gcnt[tb + slot];
    wave_normalize(f, a.gal + ((tb + slot) * a.B + cnt % a.B) * a.D, a.D);
    if (lane == 0) a.gcnt[tb + slot] = cnt + 1 >= 2 * a.B ? cnt + 1 - a.B : cnt + 1;
}

// streams s0 .. s0 + gridDim.x - 1 back to a freshly constructed tracker
__global__ void k_ss_reset(SsArgs a, int s0) {
    const int s = s0 + blockIdx.x;
    const long long tb = (long long)s * a.CAP;
    for (int k = threadIdx.x; k < a.CAP; k += blockDim.x) {
        a.freel[tb + k] = a.CAP - 1 - k;                    // slot 0 is handed out first
        a.ti[(tb + k) * T_N + T_STATE] = 0;
        a.gcnt[tb + k] = 0;
    }
    if (threadIdx.x == 0) {
        int *hdr = a.hdr + s * H_N;
        for (int k = 0; k < H_N; ++k) hdr[k] = 0;
        hdr[H_NFREE] = a.CAP;
        hdr[H_NEXT] = 1;                                    // tracker.py:59
        a.nout[s] = 0;
        a.ntrk_out[s] = 0;
    }
}

// ------------------------------------------------------------------------------- KAT kernels
__global__ __launch_bounds__(LSA_T) void k_lsa_kat(double *cost, int nr, int nc, int *rx, int *err,
                                                   int ws_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ LsaShared sh;
    const LsaWs w = lsa_ws_carve(smem, ws_n);
    if (!lsa_replay_block(cost, nr, nc, nc, 1, w, sh, rx) && threadIdx.x == 0) *err = 1;
}

__global__ __launch_bounds__(SS_T) void k_norm_rows(const float *src, float *dst, long long n, int D) {
    const long long j = (long long)blockIdx.x * (SS_T / WAVE) + threadIdx.x / WAVE;
    if (j >= n) return;
    wave_normalize(src + j * D, dst + j * D, D);
}

template <bool VEC>
__global__ __launch_bounds__(SS_T) void k_gal_kat(const float *gn, const int *lens, int B, int D,
                                                  const float *fn, int m, float *out) {
    const int tk = blockIdx.y;
    const int j0 = (blockIdx.x * (SS_T / WAVE) + threadIdx.x / WAVE) * 32;
    if (j0 >= m) return;
    const float c = gal_wave_min<VEC>(gn + (long long)tk * B * D, lens[tk], D, fn, j0, m);
    const int lane = lane_id(), j = j0 + (lane & 31);
    if (lane < 32 && j < m) out[(long long)tk * m + j] = c;
}

__global__ void k_kf_nsa_kat(int n, double *mean, double *cov, const double *z, const double *conf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    KfState s;
    for (int k = 0; k < 8; ++k) s.m[k] = mean[8 * i + k];
    kf_cov_pack(cov + 64 * i, s);
    kf_update_nsa(s, z + 4 * i, conf[i]);
    for (int k = 0; k < 8; ++k) mean[8 * i + k] = s.m[k];
    kf_cov_full(s, cov + 64 * i);
}

__global__ void k_kf_gating_kat(int n, const double *mean, const double *cov, int m,
                                const double *zs, double *out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)n * m) return;
    const int i = (int)(e / m), j = (int)(e % m);
    const double *P = cov + 64 * (long long)i;
    const double pp[4] = {P[0], P[9], P[18], P[27]};
    out[e] = kf_gating_xyah(mean + 8 * i, pp, zs + 4 * j);
}

struct DevMem {
    std::vector<void *> p;
    ~DevMem() {
        for (void *q : p) (void)hipFree(q);
    }
    template <typename T>
    hipError_t get(T **out, size_t n) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, sizeof(T) * (n ? n : 1));
        if (e == hipSuccess) p.push_back(q);
        *out = (T *)q;
        return e;
    }
};

int lsa_lds_setup(const void *fn, size_t bytes) {
    if (bytes > 64 * 1024)
        YTA_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return YTA_OK;
}

// One launch for everything a tensor frame brings in, on StrongSORT's layout: fixed slabs
// S x MAXD x 6 (the engine never grows) and plain int arrays for the counts.  The only kernel of a
// frame that reads the call's slot (mapped host memory): `counts` (S) and `offs` (S + 1, their
// prefix sums, taken on the host where the counts are checked against max_dets anyway) and `nid`
// (S, null when the caller passed no ID counters).
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

// The accessors of tensor_path.hpp's kernels behind the frame: a stream's output count
// (k_tp_out_offsets), and its track count after the frame stored into the slot (k_tp_pack_rows),
// where n_tracks() reads it after the frame's event.
struct SsNOut {
    const int *nout;
    __device__ int operator()(int s) const { return nout[s]; }
};
struct SsLive {
    const int *ntrk;
    int *live;
    __device__ void operator()(int s) const { live[s] = ntrk[s]; }
};

// A tensor frame's slot block: S ID counters in (8-B aligned), then S counts and S + 1 offsets
// in, S track counts back.
struct SsSlotView {
    long long *nid;
    int *counts, *offs, *live;
};
size_t ss_slot_bytes(size_t S) { return sizeof(long long) * S + sizeof(int) * (3 * S + 1); }
SsSlotView ss_slot_view(void *base, size_t S) {
    long long *nid = static_cast<long long *>(base);
    int *counts = reinterpret_cast<int *>(nid + S);
    return {nid, counts, counts + S, counts + 2 * S + 1};
}
enum { STS_FRAMES, STS_HOST_WAITS, STS_RESERVES, STS_INGEST_SKIPPED, STS_N };

}  // namespace

struct yta_strongsort {
    int device = 0;
    SsArgs a{};
    DevMem mem;
    hipStream_t stream = nullptr;
    // staging of the host-buffer form; the tensor path widens into d_dets and counts into d_ndet
    double *d_dets = nullptr, *d_warps = nullptr, *d_out = nullptr;
    float *d_feats = nullptr;
    int *d_ndet = nullptr, *d_nout = nullptr, *d_ntrk = nullptr;
    int *d_off = nullptr;   // S + 1 detection offsets of a tensor frame (k_ss_ingest)
    size_t lds = 0;
    int ws_n = 0;
    StreamMask mask;        // stream-subset updates (subset.hpp)
    FrameRing ring;                   // the tensor path's slots (ss_slot_view)
    FrameSlot *newest = nullptr;      // the last tensor frame, while its counts are the newest
    std::vector<int> ntrk;            // tracks per stream after the last update the host saw
    long long stat[STS_N] = {};
    ~yta_strongsort() {
        ring.release();
        mask.release();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// One frame on the engine's stream under the mask staged for it (subset.hpp; none: every stream).
// d_foff / fstride: the feature rows are packed, fstride floats apart, stream s from row d_foff[s]
// (null: the slab S x MAXD x D).
int ss_launch(yta_strongsort *e, const double *d_dets, const int *d_ndet, const float *d_feats,
              const double *d_warps, double *d_out, int *d_nout, int *d_ntrk,
              const int *d_foff = nullptr, long long fstride = 0) {
    SsArgs a = e->a;
    int rc = e->mask.stage(a.S, e->stream, &a.active);
    if (rc) return rc;
    a.dets = d_dets;
    a.ndet = d_ndet;
    a.feats = d_feats;
    a.foff = d_foff;
    a.fstride = fstride;
    a.warps = d_warps;
    a.out = d_out;
    a.nout = d_nout;
    a.ntrk_out = d_ntrk;
    const int wpb = SS_T / WAVE;
    hipLaunchKernelGGL(k_ss_pre, dim3(a.S), dim3(SS_T), 0, e->stream, a);
    hipLaunchKernelGGL(k_ss_norm, dim3((a.MAXD + wpb - 1) / wpb, a.S), dim3(SS_T), 0, e->stream, a);
    const dim3 gg((a.MAXD + 32 * wpb - 1) / (32 * wpb), a.CAP, a.S);
    if (a.D % 16 == 0) hipLaunchKernelGGL(k_ss_gal<true>, gg, dim3(SS_T), 0, e->stream, a);
    else hipLaunchKernelGGL(k_ss_gal<false>, gg, dim3(SS_T), 0, e->stream, a);
    hipLaunchKernelGGL(k_ss_match, dim3(a.S), dim3(LSA_T), e->lds, e->stream, a, e->ws_n);
    hipLaunchKernelGGL(k_ss_apply, dim3(a.S), dim3(SS_T), 0, e->stream, a);
    hipLaunchKernelGGL(k_ss_feat, dim3((a.CAP + wpb - 1) / wpb, a.S), dim3(SS_T), 0, e->stream, a);
    YTA_HIP(hipGetLastError());
    return YTA_OK;
}

int ss_check_err(yta_strongsort *e) {
    std::vector<int> hdr((size_t)e->a.S * H_N);
    YTA_HIP(hipMemcpyAsync(hdr.data(), e->a.hdr, sizeof(int) * hdr.size(), hipMemcpyDeviceToHost,
                           e->stream));
    YTA_HIP(host_wait(e->stream));
    for (int s = 0; s < e->a.S; ++s) {
        const int err = hdr[(size_t)s * H_N + H_ERR];
        YTA_CHECK(!(err & SS_ERR_CAPACITY), YTA_ERR_CAPACITY,
                  "strongsort: stream %d needs more than track_capacity = %d tracks (the engine "
                  "must be reset)", s, e->a.CAP);
        YTA_CHECK(!err, YTA_ERR_INVALID, "strongsort: stream %d: non-finite cost matrix", s);
    }
    return YTA_OK;
}

// After a host wait on the engine's stream: the newest tensor frame's track counts (stored into
// its slot by k_tp_pack_rows) become the host's.
void ss_take_live(yta_strongsort *e) {
    if (!e->newest) return;
    memcpy(e->ntrk.data(), ss_slot_view(e->newest->h, e->a.S).live, sizeof(int) * e->a.S);
    e->newest = nullptr;
}

// The host-buffer update on all S streams (det_offsets: S + 1), under e->mask when one is set.
// Runs on the engine's stream, so after every tensor frame in flight.
int ss_update_host(yta_strongsort *e, const double *dets, const int *det_offsets,
                   const float *feats, const double *warps, double *out, int out_capacity,
                   int *out_offsets) {
    const SsArgs &a = e->a;
    std::vector<int> nd(a.S);
    for (int s = 0; s < a.S; ++s) {
        nd[s] = det_offsets[s + 1] - det_offsets[s];
        YTA_CHECK(nd[s] >= 0, YTA_ERR_INVALID, "det_offsets must not decrease");
        YTA_CHECK(nd[s] <= a.MAXD, YTA_ERR_CAPACITY, "stream %d: %d detections > max_dets = %d", s,
                  nd[s], a.MAXD);
        YTA_CHECK(nd[s] == 0 || (dets && feats), YTA_ERR_INVALID, "null detections / features");
    }
    for (int s = 0; s < a.S; ++s) {
        if (!nd[s]) continue;
        YTA_HIP(hipMemcpyAsync(e->d_dets + (size_t)s * a.MAXD * 6, dets + (size_t)det_offsets[s] * 6,
                               sizeof(double) * 6 * nd[s], hipMemcpyHostToDevice, e->stream));
        YTA_HIP(hipMemcpyAsync(e->d_feats + (size_t)s * a.MAXD * a.D,
                               feats + (size_t)det_offsets[s] * a.D, sizeof(float) * a.D * nd[s],
                               hipMemcpyHostToDevice, e->stream));
    }
    YTA_HIP(hipMemcpyAsync(e->d_ndet, nd.data(), sizeof(int) * a.S, hipMemcpyHostToDevice, e->stream));
    if (warps)
        YTA_HIP(hipMemcpyAsync(e->d_warps, warps, sizeof(double) * 6 * a.S, hipMemcpyHostToDevice,
                               e->stream));
    YTA_HIP(host_wait(e->stream));   // nd / the caller's buffers are read by now
    ss_take_live(e);
    int rc = ss_launch(e, e->d_dets, e->d_ndet, e->d_feats, warps ? e->d_warps : nullptr, e->d_out,
                       e->d_nout, e->d_ntrk);
    if (rc) return rc;
    std::vector<int> no(a.S), nt(a.S);
    YTA_HIP(hipMemcpyAsync(no.data(), e->d_nout, sizeof(int) * a.S, hipMemcpyDeviceToHost, e->stream));
    YTA_HIP(hipMemcpyAsync(nt.data(), e->d_ntrk, sizeof(int) * a.S, hipMemcpyDeviceToHost, e->stream));
    rc = ss_check_err(e);
    if (rc) return rc;
    out_offsets[0] = 0;
    for (int s = 0; s < a.S; ++s) out_offsets[s + 1] = out_offsets[s] + no[s];
    YTA_CHECK(out_offsets[a.S] <= out_capacity, YTA_ERR_CAPACITY,
              "out_capacity %d < %d output rows", out_capacity, out_offsets[a.S]);
    YTA_CHECK(out_offsets[a.S] == 0 || out, YTA_ERR_INVALID, "null out");
    for (int s = 0; s < a.S; ++s)
        if (no[s])
            YTA_HIP(hipMemcpyAsync(out + (size_t)out_offsets[s] * 8, e->d_out + (size_t)s * a.CAP * 8,
                                   sizeof(double) * 8 * no[s], hipMemcpyDeviceToHost, e->stream));
    YTA_HIP(host_wait(e->stream));
    e->ntrk = nt;
    return YTA_OK;
}

}  // namespace

extern "C" {

int yta_strongsort_create(int device, int n_streams, int track_capacity, int max_dets,
                          int feat_dim, int nn_budget, const yta_strongsort_params *p,
                          yta_strongsort **engine) {
    YTA_CHECK(engine && p, YTA_ERR_INVALID, "null argument");
    *engine = nullptr;
    YTA_CHECK(n_streams >= 1 && track_capacity >= 1 && max_dets >= 1 && feat_dim >= 1 &&
                  nn_budget >= 1, YTA_ERR_INVALID, "sizes must be positive");
    YTA_CHECK(track_capacity <= LSA_MAX_N && max_dets <= LSA_MAX_N, YTA_ERR_INVALID,
              "track_capacity and max_dets are limited to %d (the solver's work arrays live in "
              "LDS)", LSA_MAX_N);
    YTA_CHECK(p->n_init >= 1 && p->max_age >= 0, YTA_ERR_INVALID, "bad n_init / max_age");
    int rc = select_device(device);
    if (rc) return rc;
    const size_t S = n_streams, C = track_capacity, M = max_dets, D = feat_dim, B = nn_budget;
    // the gallery dominates: S x capacity x nn_budget x D x 4 B
    const double gal_bytes = (double)S * C * B * D * 4;
    const double rest = (double)S * (C * M * 8 + C * D * 4 + M * D * 8 + M * 6 * 8 +
                                     (C + M) * 400.0) + (1 << 20);
    size_t free_b = 0, total_b = 0;
    YTA_HIP(hipMemGetInfo(&free_b, &total_b));
    YTA_CHECK(gal_bytes + rest <= (double)free_b, YTA_ERR_NOMEM,
              "strongsort: the galleries need %.0f MB (%d streams x %d tracks x %d rows x %d x 4 "
              "B) and the rest %.0f MB; the device has %.0f MB free", gal_bytes / 1e6, n_streams,
              track_capacity, nn_budget, feat_dim, rest / 1e6, (double)free_b / 1e6);
    auto *e = new yta_strongsort;
    e->device = device;
    SsArgs &a = e->a;
    a.S = n_streams, a.CAP = track_capacity, a.MAXD = max_dets, a.D = feat_dim, a.B = nn_budget;
    a.max_dist = p->max_dist, a.max_iou = p->max_iou_dist, a.lambda = p->mc_lambda;
    a.max_age = p->max_age, a.n_init = p->n_init;
    a.ema_a = (float)p->ema_alpha;
    a.ema_b = (float)(1 - p->ema_alpha);
    e->ws_n = (int)(C > M ? C : M);
    e->lds = lsa_ws_bytes(e->ws_n);
    DevMem &m = e->mem;
#define SS_GET(ptr, n)                       \
    do {                                     \
        hipError_t _he = m.get(&(ptr), (n)); \
        if (_he != hipSuccess) {             \
            delete e;                        \
            YTA_HIP(_he);                    \
        }                                    \
    } while (0)
    SS_GET(a.kf, S * C * KF_REC);
    SS_GET(a.ti, S * C * T_N);
    SS_GET(a.td, S * C * 3);
    SS_GET(a.feat, S * C * D);
    SS_GET(a.gal, S * C * B * D);
    SS_GET(a.gcnt, S * C);
    SS_GET(a.order, S * C);
    SS_GET(a.order2, S * C);
    SS_GET(a.freel, S * C);
    SS_GET(a.hdr, S * H_N);
    SS_GET(a.fn, S * M * D);
    SS_GET(a.dbox, S * M * 8);
    SS_GET(a.crow, S * C);
    SS_GET(a.cost, S * C * M);
    SS_GET(a.tmatch, S * C);
    SS_GET(a.flag, S * C);
    SS_GET(a.und, S * M);
    SS_GET(a.cmark, S * M);
    SS_GET(a.rows2, S * C);
    SS_GET(a.rx, S * C);
    SS_GET(a.births, S * M);
    SS_GET(a.sact, S * C);
    SS_GET(e->d_dets, S * M * 6);
    SS_GET(e->d_warps, S * 6);
    SS_GET(e->d_out, S * C * 8);
    SS_GET(e->d_feats, S * M * D);
    SS_GET(e->d_ndet, S);
    SS_GET(e->d_nout, S);
    SS_GET(e->d_ntrk, S);
    SS_GET(e->d_off, S + 1);
#undef SS_GET
    e->ntrk.assign(S, 0);
    e->ring.slot_bytes = ss_slot_bytes(S);
    e->ring.host_waits = &e->stat[STS_HOST_WAITS];
    a.nout = e->d_nout;
    a.ntrk_out = e->d_ntrk;
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he == hipSuccess && e->lds > 64 * 1024)
        he = hipFuncSetAttribute((const void *)k_ss_match,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds);
    if (he != hipSuccess) {
        delete e;
        YTA_HIP(he);
    }
    rc = yta_strongsort_reset(e);
    if (rc) {
        delete e;
        return rc;
    }
    *engine = e;
    return YTA_OK;
}

int yta_strongsort_destroy(yta_strongsort *e) {
    if (!e) return YTA_OK;
    (void)select_device(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    delete e;
    return YTA_OK;
}

int yta_strongsort_reset(yta_strongsort *e) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    int rc = select_device(e->device);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ss_reset, dim3(e->a.S), dim3(256), 0, e->stream, e->a, 0);
    YTA_HIP(hipGetLastError());
    YTA_HIP(host_wait(e->stream));   // tensor frames in flight have run and are wiped
    e->newest = nullptr;
    e->ntrk.assign(e->a.S, 0);
    return YTA_OK;
}

int yta_strongsort_reset_stream(yta_strongsort *e, int stream) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    YTA_CHECK(stream >= 0 && stream < e->a.S, YTA_ERR_INVALID, "stream %d outside 0..%d", stream,
              e->a.S - 1);
    int rc = select_device(e->device);
    if (rc) return rc;
    hipLaunchKernelGGL(k_ss_reset, dim3(1), dim3(256), 0, e->stream, e->a, stream);
    YTA_HIP(hipGetLastError());
    YTA_HIP(host_wait(e->stream));
    ss_take_live(e);   // every tensor frame has run: the other streams' counts are in its slot
    e->ntrk[stream] = 0;
    return YTA_OK;
}

int yta_strongsort_capacity(yta_strongsort *e, int *track_capacity, int *max_dets, int *feat_dim,
                            int *nn_budget) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    if (track_capacity) *track_capacity = e->a.CAP;
    if (max_dets) *max_dets = e->a.MAXD;
    if (feat_dim) *feat_dim = e->a.D;
    if (nn_budget) *nn_budget = e->a.B;
    return YTA_OK;
}

int yta_strongsort_update(yta_strongsort *e, const double *dets, const int *det_offsets,
                          const float *feats, const double *warps, double *out, int out_capacity,
                          int *out_offsets, int *n_tracks) {
    YTA_CHECK(e && det_offsets && out_offsets, YTA_ERR_INVALID, "null argument");
    int rc = select_device(e->device);
    if (rc) return rc;
    rc = ss_update_host(e, dets, det_offsets, feats, warps, out, out_capacity, out_offsets);
    if (rc) return rc;
    if (n_tracks) memcpy(n_tracks, e->ntrk.data(), sizeof(int) * e->a.S);
    return YTA_OK;
}

int yta_strongsort_update_streams(yta_strongsort *e, int n_streams, const int *stream_ids,
                                  const double *dets, const int *det_offsets, const float *feats,
                                  const double *warps, double *out, int out_capacity,
                                  int *out_offsets, int *n_tracks) {
    YTA_CHECK(e && out_offsets, YTA_ERR_INVALID, "null argument");
    int rc = select_device(e->device);
    if (rc) return rc;
    const int S = e->a.S;
    std::vector<int> mask, off, full_oo(S + 1, 0);
    rc = subset_expand(S, n_streams, stream_ids, det_offsets, mask, off);
    if (rc) return rc;
    std::vector<double> w;   // a stream not listed gets no camera update either way
    if (warps) w = subset_spread<double>(S, n_streams, stream_ids, warps, 6, NAN);
    e->mask.req_host = mask.data();
    rc = ss_update_host(e, dets, off.data(), feats, warps ? w.data() : nullptr, out, out_capacity,
                        full_oo.data());
    e->mask.req_host = nullptr;
    if (rc) return rc;
    subset_compact(n_streams, stream_ids, full_oo, out_offsets);
    if (n_tracks)
        for (int k = 0; k < n_streams; ++k) n_tracks[k] = e->ntrk[stream_ids[k]];
    return YTA_OK;
}

int yta_strongsort_update_device(yta_strongsort *e, const double *d_dets, const int *d_det_counts,
                                 const float *d_feats, const double *d_warps, double *d_out,
                                 int *d_out_counts, int *d_n_tracks) {
    YTA_CHECK(e && d_dets && d_det_counts && d_feats && d_out && d_out_counts, YTA_ERR_INVALID,
              "null argument");
    int rc = select_device(e->device);
    if (rc) return rc;
    return ss_launch(e, d_dets, d_det_counts, d_feats, d_warps, d_out, d_out_counts,
                     d_n_tracks ? d_n_tracks : e->d_ntrk);
}

int yta_strongsort_update_device_masked(yta_strongsort *e, const int *d_active,
                                        const double *d_dets, const int *d_det_counts,
                                        const float *d_feats, const double *d_warps,
                                        double *d_out, int *d_out_counts, int *d_n_tracks) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    e->mask.req_dev = d_active;
    const int rc = yta_strongsort_update_device(e, d_dets, d_det_counts, d_feats, d_warps, d_out,
                                                d_out_counts, d_n_tracks);
    e->mask.req_dev = nullptr;
    return rc;
}

int yta_strongsort_update_tensors(yta_strongsort *e, void *caller_stream, const void *d_dets,
                                  int dtype, long long row_stride, const int *det_counts,
                                  const float *d_feats, long long feat_stride,
                                  const double *d_warps, const int *d_active,
                                  const long long *next_id, double *d_rows,
                                  long long rows_capacity, int *d_row_offsets, int *d_row_stream) {
    long long total = 0;
    int rc = tensor_check_args(e, e ? e->a.S : 0, e ? e->a.D : 0, d_dets, dtype, row_stride,
                               det_counts, d_feats, feat_stride, d_rows, rows_capacity,
                               d_row_offsets, &total);
    if (rc) return rc;
    const SsArgs &a = e->a;
    const int S = a.S;
    for (int s = 0; s < S; ++s)
        YTA_CHECK(det_counts[s] <= a.MAXD, YTA_ERR_CAPACITY,
                  "stream %d: %d detections > max_dets = %d", s, det_counts[s], a.MAXD);
    YTA_CHECK(!d_warps || (uintptr_t)d_warps % sizeof(double) == 0, YTA_ERR_INVALID,
              "d_warps misaligned");
    rc = select_device(e->device);
    if (rc) return rc;
    const hipStream_t cs = (hipStream_t)caller_stream;
    rc = frame_refuse_capture(cs);
    if (rc) return rc;
    FrameSlot *p = nullptr;
    rc = e->ring.acquire(&p, e->newest);   // not the newest: n_tracks() reads its counts
    if (rc) return rc;
    const SsSlotView hv = ss_slot_view(p->h, S), mv = ss_slot_view(p->m, S);
    memcpy(hv.counts, det_counts, sizeof(int) * S);
    hv.offs[0] = 0;
    for (int s = 0; s < S; ++s) hv.offs[s + 1] = hv.offs[s] + det_counts[s];
    if (next_id) memcpy(hv.nid, next_id, sizeof(long long) * S);
    e->newest = p;
    ++e->stat[STS_FRAMES];
    rc = frame_hand_in(p, cs, e->stream);
    if (rc) return rc;
    {
        const int cps = (3 * a.MAXD + SS_ING_T - 1) / SS_ING_T;
        const unsigned grid = 1u + (total ? (unsigned)S * cps : 0u);
        const long long *nid = next_id ? mv.nid : nullptr;
#define SS_INGEST(T)                                                                             \
    hipLaunchKernelGGL(k_ss_ingest<T>, dim3(grid), dim3(SS_ING_T), 0, e->stream,                 \
                       (const T *)d_dets, row_stride, mv.counts, mv.offs, nid, d_active, S,      \
                       a.MAXD, cps, e->d_ndet, e->d_off, a.hdr, (int)H_N, (int)H_NEXT, e->d_dets)
        if (dtype == YTA_F64) SS_INGEST(double);
        else if (dtype == YTA_F32) SS_INGEST(float);
        else SS_INGEST(_Float16);
#undef SS_INGEST
        YTA_HIP(hipGetLastError());
    }
    e->mask.req_dev = d_active;
    rc = ss_launch(e, e->d_dets, e->d_ndet, d_feats, d_warps, e->d_out, e->d_nout, e->d_ntrk,
                   e->d_off, feat_stride);
    e->mask.req_dev = nullptr;
    if (rc) return rc;
    hipLaunchKernelGGL(k_tp_out_offsets<SsNOut>, dim3(1), dim3(TP_OFFS_T), 0, e->stream,
                       SsNOut{e->d_nout}, S, a.CAP, d_row_offsets, (int *)nullptr);
    hipLaunchKernelGGL(k_tp_pack_rows<SsLive>, dim3(S), dim3(256), 0, e->stream, e->d_out,
                       (long long)a.CAP, S, d_row_offsets, d_rows, rows_capacity, d_row_stream,
                       SsLive{e->d_ntrk, mv.live});
    YTA_HIP(hipGetLastError());
    return frame_hand_back(p, cs, e->stream);
}

int yta_strongsort_tensor_stats(yta_strongsort *e, long long *out, int n) {
    YTA_CHECK(e && (out || n <= 0), YTA_ERR_INVALID, "null argument");
    for (int k = 0; k < n && k < STS_N; ++k) out[k] = e->stat[k];
    return YTA_OK;
}

int yta_strongsort_next_ids(yta_strongsort *e, long long *next_id) {
    YTA_CHECK(e && next_id, YTA_ERR_INVALID, "null argument");
    int rc = select_device(e->device);
    if (rc) return rc;
    std::vector<int> hdr((size_t)e->a.S * H_N);
    YTA_HIP(hipMemcpyAsync(hdr.data(), e->a.hdr, sizeof(int) * hdr.size(), hipMemcpyDeviceToHost,
                           e->stream));
    YTA_HIP(host_wait(e->stream));
    ss_take_live(e);
    for (int s = 0; s < e->a.S; ++s) next_id[s] = hdr[(size_t)s * H_N + H_NEXT];
    return YTA_OK;
}

int yta_strongsort_n_tracks(yta_strongsort *e, int *n_tracks) {
    YTA_CHECK(e && n_tracks, YTA_ERR_INVALID, "null argument");
    if (e->newest) {   // page-locked counts of the newest tensor frame: wait for its event only
        int rc = select_device(e->device);
        if (rc) return rc;
        ++e->stat[STS_HOST_WAITS];
        YTA_HIP(hipEventSynchronize(e->newest->done));
        ss_take_live(e);
    }
    memcpy(n_tracks, e->ntrk.data(), sizeof(int) * e->a.S);
    return YTA_OK;
}

int yta_strongsort_sync(yta_strongsort *e) {
    YTA_CHECK(e, YTA_ERR_INVALID, "null engine");
    int rc = select_device(e->device);
    if (rc) return rc;
    rc = ss_check_err(e);
    ss_take_live(e);   // waited either way
    return rc;
}

int yta_strongsort_get_state(yta_strongsort *e, int stream, int *n_tracks, long long *ints,
                             double *mean, double *cov, float *feat, int *gallery_len,
                             float *gallery) {
    YTA_CHECK(e && n_tracks, YTA_ERR_INVALID, "null argument");
    const SsArgs &a = e->a;
    YTA_CHECK(stream >= 0 && stream < a.S, YTA_ERR_INVALID, "stream out of range");
    int rc = select_device(e->device);
    if (rc) return rc;
    YTA_HIP(host_wait(e->stream));
    const size_t tb = (size_t)stream * a.CAP;
    int hdr[H_N];
    YTA_HIP(hipMemcpy(hdr, a.hdr + stream * H_N, sizeof(hdr), hipMemcpyDeviceToHost));
    const int n = hdr[H_NTRK];
    *n_tracks = n;
    if (!n || !(ints || mean || cov || feat || gallery_len || gallery)) return YTA_OK;
    std::vector<int> order(n), ti((size_t)a.CAP * T_N), gc(a.CAP);
    std::vector<double> kf((size_t)a.CAP * KF_REC);
    YTA_HIP(hipMemcpy(order.data(), a.order + tb, sizeof(int) * n, hipMemcpyDeviceToHost));
    YTA_HIP(hipMemcpy(ti.data(), a.ti + tb * T_N, sizeof(int) * ti.size(), hipMemcpyDeviceToHost));
    YTA_HIP(hipMemcpy(gc.data(), a.gcnt + tb, sizeof(int) * a.CAP, hipMemcpyDeviceToHost));
    YTA_HIP(hipMemcpy(kf.data(), a.kf + tb * KF_REC, sizeof(double) * kf.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; ++k) {
        const int slot = order[k];
        if (ints)
            for (int q = 0; q < T_N; ++q) ints[(size_t)k * T_N + q] = ti[(size_t)slot * T_N + q];
        KfState st;
        for (int q = 0; q < 8; ++q) st.m[q] = kf[(size_t)slot * KF_REC + q];
        for (int q = 0; q < 16; ++q) st.c[q] = kf[(size_t)slot * KF_REC + 8 + q];
        if (mean)
            for (int q = 0; q < 8; ++q) mean[(size_t)k * 8 + q] = st.m[q];
        if (cov) kf_cov_full(st, cov + (size_t)k * 64);
        if (feat)
            YTA_HIP(hipMemcpy(feat + (size_t)k * a.D, a.feat + (tb + slot) * a.D, sizeof(float) * a.D,
                              hipMemcpyDeviceToHost));
        const int len = gc[slot] < a.B ? gc[slot] : a.B;
        if (gallery_len) gallery_len[k] = ti[(size_t)slot * T_N + T_STATE] == 2 ? len : 0;
        if (gallery)     // rows in ring order (the minimum over them does not depend on it)
            YTA_HIP(hipMemcpy(gallery + (size_t)k * a.B * a.D, a.gal + (tb + slot) * a.B * a.D,
                              sizeof(float) * a.B * a.D, hipMemcpyDeviceToHost));
    }
    return YTA_OK;
}

int yta_strongsort_hip_stream(yta_strongsort *e, void **stream) {
    YTA_CHECK(e && stream, YTA_ERR_INVALID, "null argument");
    *stream = (void *)e->stream;
    return YTA_OK;
}

int yta_lsa_replay(int device, int nr, int nc, const double *cost, int *rows, int *cols) {
    YTA_CHECK(nr >= 0 && nc >= 0, YTA_ERR_INVALID, "negative size");
    if (nr == 0 || nc == 0) return YTA_OK;
    YTA_CHECK(cost && rows && cols, YTA_ERR_INVALID, "null buffer");
    YTA_CHECK(nr <= LSA_MAX_N && nc <= LSA_MAX_N, YTA_ERR_INVALID, "at most %d rows / columns",
              LSA_MAX_N);
    int rc = select_device(device);
    if (rc) return rc;
    DevMem m;
    double *dc;
    int *drx, *derr;
    YTA_HIP(m.get(&dc, (size_t)nr * nc));
    YTA_HIP(m.get(&drx, nr));
    YTA_HIP(m.get(&derr, 1));
    YTA_HIP(hipMemcpy(dc, cost, sizeof(double) * nr * nc, hipMemcpyHostToDevice));
    YTA_HIP(hipMemset(derr, 0, sizeof(int)));
    const int n = nr > nc ? nr : nc;
    const size_t lds = lsa_ws_bytes(n);
    rc = lsa_lds_setup((const void *)k_lsa_kat, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lsa_kat, dim3(1), dim3(LSA_T), lds, 0, dc, nr, nc, drx, derr, n);
    YTA_HIP(hipGetLastError());
    std::vector<int> rx(nr);
    int err = 0;
    YTA_HIP(hipMemcpy(rx.data(), drx, sizeof(int) * nr, hipMemcpyDeviceToHost));
    YTA_HIP(hipMemcpy(&err, derr, sizeof(int), hipMemcpyDeviceToHost));
    YTA_CHECK(!err, YTA_ERR_INVALID, "cost matrix is infeasible (non-finite entries)");
    int k = 0;
    for (int i = 0; i < nr; ++i)
        if (rx[i] >= 0) {
            rows[k] = i;
            cols[k++] = rx[i];
        }
    return YTA_OK;
}

int yta_nn_cosine_min(int device, int n_tracks, int budget, int feat_dim, const float *gallery,
                      const int *lens, int n_dets, const float *feats, float *out) {
    YTA_CHECK(n_tracks >= 0 && n_dets >= 0 && budget >= 1 && feat_dim >= 1, YTA_ERR_INVALID,
              "bad size");
    if (n_tracks == 0 || n_dets == 0) return YTA_OK;
    YTA_CHECK(gallery && lens && feats && out, YTA_ERR_INVALID, "null buffer");
    for (int t = 0; t < n_tracks; ++t)
        YTA_CHECK(lens[t] >= 1 && lens[t] <= budget, YTA_ERR_INVALID, "lens[%d] out of range", t);
    int rc = select_device(device);
    if (rc) return rc;
    DevMem m;
    const size_t ng = (size_t)n_tracks * budget, D = feat_dim;
    float *dg, *df, *dout;
    int *dl;
    YTA_HIP(m.get(&dg, ng * D));
    YTA_HIP(m.get(&df, (size_t)n_dets * D));
    YTA_HIP(m.get(&dout, (size_t)n_tracks * n_dets));
    YTA_HIP(m.get(&dl, n_tracks));
    YTA_HIP(hipMemcpy(dg, gallery, sizeof(float) * ng * D, hipMemcpyHostToDevice));
    YTA_HIP(hipMemcpy(df, feats, sizeof(float) * n_dets * D, hipMemcpyHostToDevice));
    YTA_HIP(hipMemcpy(dl, lens, sizeof(int) * n_tracks, hipMemcpyHostToDevice));
    const int wpb = SS_T / WAVE;
    // rows past lens[t] are never read by the product; normalising them is harmless (x / 0)
    hipLaunchKernelGGL(k_norm_rows, dim3((unsigned)((ng + wpb - 1) / wpb)), dim3(SS_T), 0, 0, dg, dg,
                       (long long)ng, feat_dim);
    hipLaunchKernelGGL(k_norm_rows, dim3((n_dets + wpb - 1) / wpb), dim3(SS_T), 0, 0, df, df,
                       (long long)n_dets, feat_dim);
    const dim3 gg((n_dets + 32 * wpb - 1) / (32 * wpb), n_tracks);
    if (feat_dim % 16 == 0)
        hipLaunchKernelGGL(k_gal_kat<true>, gg, dim3(SS_T), 0, 0, dg, dl, budget, feat_dim, df,
                           n_dets, dout);
    else
        hipLaunchKernelGGL(k_gal_kat<false>, gg, dim3(SS_T), 0, 0, dg, dl, budget, feat_dim, df,
                           n_dets, dout);
    YTA_HIP(hipGetLastError());
    YTA_HIP(hipMemcpy(out, dout, sizeof(float) * n_tracks * n_dets, hipMemcpyDeviceToHost));
    return YTA_OK;
}

int yta_kf_nsa_update(int device, int n, double *mean, double *cov, const double *z,
                      const double *conf) {
    YTA_CHECK(n >= 0, YTA_ERR_INVALID, "negative size");
    if (n == 0) return YTA_OK;
    YTA_CHECK(mean && cov && z && conf, YTA_ERR_INVALID, "null buffer");
    int rc = select_device(device);
    if (rc) return rc;
    DevMem m;
    double *dm, *dc, *dz, *dq;
    YTA_HIP(m.get(&dm, (size_t)n * 8));
    YTA_HIP(m.get(&dc, (size_t)n * 64));
    YTA_HIP(m.get(&dz, (size_t)n * 4));
    YTA_HIP(m.get(&dq, n));
    YTA_HIP(hipMemcpy(dm, mean, sizeof(double) * n * 8, hipMemcpyHostToDevice));
    YTA_HIP(hipMemcpy(dc, cov, sizeof(double) * n * 64, hipMemcpyHostToDevice));
    YTA_HIP(hipMemcpy(dz, z, sizeof(double) * n * 4, hipMemcpyHostToDevice));
    YTA_HIP(hipMemcpy(dq, conf, sizeof(double) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_kf_nsa_kat, dim3((n + 63) / 64), dim3(64), 0, 0, n, dm, dc, dz, dq);
    YTA_HIP(hipGetLastError());
    YTA_HIP(hipMemcpy(mean, dm, sizeof(double) * n * 8, hipMemcpyDeviceToHost));
    YTA_HIP(hipMemcpy(cov, dc, sizeof(double) * n * 64, hipMemcpyDeviceToHost));
    return YTA_OK;
}

int yta_kf_xyah_gating(int device, int n, const double *mean, const double *cov, int m,
                       const double *zs, double *out) {
    YTA_CHECK(n >= 0 && m >= 0, YTA_ERR_INVALID, "negative size");
    if (n == 0 || m == 0) return YTA_OK;
    YTA_CHECK(mean && cov && zs && out, YTA_ERR_INVALID, "null buffer");
    int rc = select_device(device);
    if (rc) return rc;
    DevMem mm;
    double *dm, *dc, *dz, *dout;
    YTA_HIP(mm.get(&dm, (size_t)n * 8));
    YTA_HIP(mm.get(&dc, (size_t)n * 64));
    YTA_HIP(mm.get(&dz, (size_t)m * 4));
    YTA_HIP(mm.get(&dout, (size_t)n * m));
    YTA_HIP(hipMemcpy(dm, mean, sizeof(double) * n * 8, hipMemcpyHostToDevice));
    YTA_HIP(hipMemcpy(dc, cov, sizeof(double) * n * 64, hipMemcpyHostToDevice));
    YTA_HIP(hipMemcpy(dz, zs, sizeof(double) * m * 4, hipMemcpyHostToDevice));
    const long long tot = (long long)n * m;
    hipLaunchKernelGGL(k_kf_gating_kat, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, n, dm,
                       dc, m, dz, dout);
    YTA_HIP(hipGetLastError());
    YTA_HIP(hipMemcpy(out, dout, sizeof(double) * tot, hipMemcpyDeviceToHost));
    return YTA_OK;
}

}  // extern "C"
