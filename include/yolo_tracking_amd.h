/*
 * yolo_tracking_amd — C ABI of the MI355X tracker.update() hot path.
 *
 * Every entry point returns an int status (YTA_OK = 0, negative = error; the message is available
 * from yta_last_error(), thread-local).  No torch / HIP types cross this boundary: plain pointers,
 * sizes and opaque handles only.  Host buffers are caller-owned; device buffers are owned by the
 * library (except in the *_device entry points, which take caller-owned device pointers).
 *
 * What each entry point replaces in the reference (BoxMOT 10.0.51, /root/reference):
 *   yta_bytetrack_*          boxmot/trackers/bytetrack/byte_tracker.py:114-281  BYTETracker.__init__/update
 *                            (created by boxmot/tracker_zoo.py:56-64 create_tracker('bytetrack', ...))
 *   yta_botsort_*            boxmot/trackers/botsort/bot_sort.py:185-420  BoTSORT.__init__/update
 *                            (created by boxmot/tracker_zoo.py:66-81 create_tracker('botsort', ...));
 *                            the ReID forward pass (reid_multibackend.py:303-311) and the CMC
 *                            estimator (sof.py) stay outside: their outputs are inputs here
 *   yta_ocsort_*             boxmot/trackers/ocsort/ocsort.py:188-379  OCSort.__init__/update
 *                            (created by boxmot/tracker_zoo.py:42-55 create_tracker('ocsort', ...))
 *   yta_deepocsort_*         boxmot/trackers/deepocsort/deep_ocsort.py:308-520  DeepOCSort.__init__/
 *                            update (created by boxmot/tracker_zoo.py:83-99); ReID and CMC outside
 *   yta_kf8_run              deep_ocsort.py:103-293 KalmanBoxTracker (new KF) + deepocsort_kf.py
 *   yta_hybridsort_*         boxmot/trackers/hybridsort/hybridsort.py:329-570  HybridSORT.__init__/
 *                            update without its PerClassDecorator (the host replays it call by
 *                            call, boxmot/utils/__init__.py:22-61; created by
 *                            boxmot/tracker_zoo.py:100-114); ReID outside
 *   yta_kf9_run              hybridsort.py:106-320 KalmanBoxTracker + hybridsort_kf.py:339-528
 *   yta_lap_padded           boxmot/utils/association.py:20-28 linear_assignment -> lap.lapjv(cost,
 *                            extend_cost=True)
 *   yta_lap_rect             the same call's optimum where ties cannot change the tracker result
 *                            (association.py:20-28 at ocsort.py:266-291, :315-342)
 *   yta_kf7_run              boxmot/motion/kalman_filters/ocsort_kf.py:339-526 predict / update incl.
 *                            freeze / unfreeze (observation-centric re-update)
 *   yta_box_affinity         boxmot/utils/iou.py:6-188  iou/giou/diou/ciou/centroid_batch
 *   yta_iou_distance         boxmot/utils/matching.py:94-119 iou_distance (+ fuse_score :213-221)
 *   yta_kf_xyah_initiate     boxmot/motion/kalman_filters/bytetrack_kf.py:55-86
 *   yta_kf_xyah_predict      boxmot/motion/kalman_filters/bytetrack_kf.py:155-192 (multi_predict)
 *   yta_kf_xyah_update       boxmot/motion/kalman_filters/bytetrack_kf.py:194-226 (+ project :126-153)
 *   yta_lap_limited          boxmot/utils/matching.py:56-71 linear_assignment -> lap.lapjv(cost,
 *                            extend_cost=True, cost_limit=thresh)
 *   yta_embedding_distance   boxmot/utils/matching.py:145-167 embedding_distance (max(0, cdist cosine))
 *   yta_aw_max_metric        boxmot/utils/association.py:79-108 compute_aw_max_metric
 *   yta_gsi_*                boxmot/postprocessing/gsi.py:12-72 linear_interpolation / gaussian_smooth
 *   yta_reid_preprocess*     boxmot/appearance/reid_multibackend.py:189-224
 *                            ReIDDetectMultiBackend.preprocess (crop, cv2.resize INTER_LINEAR,
 *                            BGR -> RGB, ImageNet standardisation, NCHW batch)
 *   yta_reid_normalize*      boxmot/appearance/reid_multibackend.py:303-311 get_features'
 *                            `features / np.linalg.norm(features)`
 *   yta_strongsort_*         boxmot/trackers/strongsort/strong_sort.py:13-99 StrongSORT
 *                            (sort/tracker.py, sort/track.py, sort/linear_assignment.py,
 *                            sort/iou_matching.py, motion/kalman_filters/strongsort_kf.py,
 *                            utils/matching.py:224-378); ReID and ECC outside
 *   yta_lsa_replay           scipy.optimize.linear_sum_assignment as called by
 *                            strongsort/sort/linear_assignment.py:61
 *   yta_nn_cosine_min        boxmot/utils/matching.py:247-308 _nn_cosine_distance
 *   yta_kf_nsa_update        boxmot/motion/kalman_filters/strongsort_kf.py:124-189
 *   yta_kf_xyah_gating       boxmot/motion/kalman_filters/strongsort_kf.py:191-233
 */
#ifndef YOLO_TRACKING_AMD_H
#define YOLO_TRACKING_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YTA_OK 0
#define YTA_ERR_INVALID (-1)   /* bad argument (shape, null pointer, unknown kind)        */
#define YTA_ERR_HIP (-2)       /* HIP runtime failure (no device, launch or copy failure)  */
#define YTA_ERR_CAPACITY (-3)  /* track / detection / output capacity exceeded            */
#define YTA_ERR_NOMEM (-4)     /* host or device allocation failed                        */

/* ---- library ---------------------------------------------------------------------------- */
int yta_version(void);                       /* returns the ABI version (positive) */
const char *yta_last_error(void);            /* message of the last failing call on this thread */
int yta_device_count(int *count);

/* ---- association primitives (parity / KAT entry points; synchronous, host buffers) ---------
 * Boxes are [x1, y1, x2, y2] float64 rows. */
#define YTA_AFF_IOU 0
#define YTA_AFF_GIOU 1
#define YTA_AFF_DIOU 2
#define YTA_AFF_CIOU 3
#define YTA_AFF_CENTROID 4
/* out[i*nb + j] = affinity(a_i, b_j), exactly iou.py's *_batch(a, b) (centroid uses img_w/img_h) */
int yta_box_affinity(int device, int kind, const double *a, int na, const double *b, int nb,
                     double img_w, double img_h, double *out);
/* out = 1 - iou_batch(a, b); if scores != NULL, then fuse_score: 1 - (1 - out) * scores[j] */
int yta_iou_distance(int device, const double *a, int na, const double *b, int nb,
                     const double *scores, double *out);

/* Grid-pruned pair search (the candidate machinery behind the tracker's association and
 * duplicate removal): every (i, j) with 1 - IoU(a_i, b_j) < thresh, thresh <= 1; pairs[2k] = i,
 * pairs[2k+1] = j in no particular order; *n_pairs = total found (only `cap` are written). */
int yta_grid_pairs(int device, const double *a, int na, const double *b, int nb, double thresh,
                   int *pairs, int cap, int *n_pairs);

/* ---- ByteTrack Kalman filter, xyah state (parity / KAT entry points) -----------------------
 * mean: n x 8, cov: n x 8 x 8 (row-major, full matrices), meas / z: n x 4 [xc, yc, a, h]. */
int yta_kf_xyah_initiate(int device, int n, const double *meas, double *mean, double *cov);
/* Camera-motion correction KAT (SURVEY.md §8(b) affine_apply), in place on n states (mean 8,
 * covariance 8 x 8 row-major, block-diagonal over {x, y, x', y'} / {w, h, w', h'} as every state
 * of these trackers is), warps n row-major 2x3, with the engines' own device functions:
 *   kind 0  BoT-SORT STrack.multi_gmc (bot_sort.py:95-111): kf_gmc (kf_xyah.hpp)
 *   kind 1  DeepOCSORT apply_affine_correction, new-KF branch (deepocsort_kf.py:387-405;
 *           deep_ocsort.py:250-267 calls it per tracker): kf8_affine (kf_deep.hpp) */
int yta_affine_apply(int device, int kind, int n, const double *warps, double *mean, double *cov);
/* in place; the caller applies the reference's `mean[7] = 0` for non-tracked tracks beforehand */
int yta_kf_xyah_predict(int device, int n, double *mean, double *cov);
int yta_kf_xyah_update(int device, int n, double *mean, double *cov, const double *z);

/* Device self-test of the block-wide scan / reduction primitives the kernels are built on (DPP
 * cross-lane operations) at several block sizes.  0 when every result matches a serial answer. */
int yta_selftest(int device);

/* Host evaluation (no device needed) of the block placement k_apply uses (xcd_stream_blocks,
 * csrc/common.hpp): for a launch of gx blocks per stream over n_streams streams, stream[lin] /
 * block[lin] = the logical (stream, block) that hardware block lin = blockIdx.x + gx * blockIdx.y
 * works on; both arrays hold gx * n_streams ints. */
int yta_apply_block_map(int gx, int n_streams, int *stream, int *block);

/* Host evaluation (no device needed) of the conservative pre-tests ByteTrack's k_s1_edges puts in
 * front of its float64 IoU (csrc/grid.hpp: box_pack16, box16_meet), with origin and scale derived
 * as the kernel derives them from the stream's high detections.
 * pool: nr boxes x1,y1,x2,y2; high / score: nc boxes and scores; thresh: match_thresh.
 * out[i * nc + j]: bit 0 = the packed boxes of pool row i and detection j meet; bit 1 = the pair
 * also passes the second stage (a bound on IoU x score against 1 - thresh), which was measured
 * and not kept: the kernel has none, every pair that meets passes, bit 1 = bit 0
 * and score / thresh are not read.  3 for a detection that is not binned (unusable or larger than
 * 4 x the mean size: the kernel tests those pairs in float64 only). */
int yta_s1_pretest(int nr, const double *pool, int nc, const double *high, const double *score,
                   double thresh, unsigned char *out);

/* ---- linear assignment with lapx cost_limit semantics -------------------------------------
 * Minimises sum(matched cost) + cost_limit/2 * (#unmatched rows + #unmatched cols); x[r] = col or
 * -1, y[c] = row or -1 (lap.lapjv(cost, extend_cost=True, cost_limit=cost_limit)). */
int yta_lap_limited(int device, int nr, int nc, const double *cost, double cost_limit, int *x,
                    int *y);

/* Padded dense assignment (association.py:20-28: lap.lapjv(cost, extend_cost=True), OCSORT
 * family): zero-padded to max(nr, nc) square, every row / column of the smaller side matched;
 * x[r] = col or -1, y[c] = row or -1.  The same operation and tie-breaking sequence as the
 * restated lapjv (oracle/lapjv.c). */
int yta_lap_padded(int device, int nr, int nc, const double *cost, int *x, int *y);

/* The optimum of the same padded problem by the rectangular solver the OCSORT-family engines use
 * where the result does not depend on lapjv's tie-breaking (lap_rect.hpp): warm
 * start from row minima, shortest augmenting paths with bound pruning.  Every row / column of the
 * smaller side is matched; equal to yta_lap_padded whenever the optimum is unique.  At most 8192
 * entries on the larger side. */
int yta_lap_rect(int device, int nr, int nc, const double *cost, int *x, int *y);
/* The OCSORT-family first-round solve (ocsort_common.hpp first_round_lap, association.py:20-28)
 * exactly as the engines launch it (chip-wide row pre-pass + one LAP_T-thread block), no fast
 * path: na x nb cost (rows = detections).  rx (na): tracker of each detection or -1; *done: 1 =
 * solved, 0 = the engine would replay lapjv (more detections than trackers and the optimum not
 * certified unique); *n_tight: tight non-matching edges the certificate examined (-1 unless
 * na > nb). */
int yta_lap_first_round(int device, int na, int nb, const double *cost, int *rx, int *done,
                        int *n_tight);

/* ---- ByteTrack engine: S independent streams, state resident in HBM -----------------------
 * One engine = S trackers with identical parameters (BYTETracker(track_thresh, match_thresh,
 * track_buffer, frame_rate)).  Stream s keeps its own tracks and its own ID counter. */
typedef struct yta_bytetrack yta_bytetrack;
typedef struct {
    double track_thresh;   /* bytetrack.yaml:1   (ctor default 0.45) */
    double match_thresh;   /* bytetrack.yaml:3   (ctor default 0.8)  */
    int track_buffer;      /* bytetrack.yaml:2   (ctor default 25)   */
    int frame_rate;        /* bytetrack.yaml:4   (ctor default 30)   */
} yta_bytetrack_params;

/* track_capacity: live (tracked + lost) tracks per stream; max_dets: detections per stream per
 * frame.  The host-buffer update grows both on demand; the device-buffer update treats them as
 * hard limits (YTA_ERR_CAPACITY from yta_bytetrack_sync). */
int yta_bytetrack_create(int device, int n_streams, int track_capacity, int max_dets,
                         const yta_bytetrack_params *params, yta_bytetrack **engine);
int yta_bytetrack_destroy(yta_bytetrack *engine);
int yta_bytetrack_reset(yta_bytetrack *engine);

/* Grow the per-stream track capacity / max detections (never shrinks), keeping every stream's
 * state.  yta_bytetrack_update() calls this itself when a frame would not fit. */
int yta_bytetrack_reserve(yta_bytetrack *engine, int track_capacity, int max_dets);
int yta_bytetrack_capacity(yta_bytetrack *engine, int *track_capacity, int *max_dets);

/* Host-buffer update of all S streams (one frame each).  dets: packed rows of
 * [x1, y1, x2, y2, conf, cls] float64 for stream 0, then stream 1, ...; det_offsets: S+1
 * prefix offsets (rows).  next_id: S counters (in: the last issued ID per stream, i.e. the
 * reference's BaseTrack._count; out: updated), may be NULL to use the engine's own counters.
 * out: caller buffer of out_capacity rows x 8 float64 [x1,y1,x2,y2,id,conf,cls,det_ind];
 * out_offsets: S+1 prefix offsets written by the call.  Synchronous.
 * out_capacity >= det_offsets[S] always suffices (every output row is a track matched to or born
 * from one of the frame's detections) and is required: a smaller buffer fails with
 * YTA_ERR_CAPACITY before anything is staged or launched, so the same call can be retried.  An
 * error reported after the launch (device error flags, HIP failure) means the frame HAS been
 * applied on the device; next_id is still written back then.  The same rules hold for every
 * tracker's host-buffer update below. */
int yta_bytetrack_update(yta_bytetrack *engine, const double *dets, const int *det_offsets,
                         long long *next_id, double *out, int out_capacity, int *out_offsets);

/* Device-resident update for throughput runs: d_dets / d_det_offsets are device pointers laid out
 * as above; results stay on the device: d_out holds S * track_capacity rows x 8, stream s at row
 * s * track_capacity, d_out_counts[s] rows.  Asynchronous on the engine's HIP stream. */
int yta_bytetrack_update_device(yta_bytetrack *engine, const double *d_dets,
                                const int *d_det_offsets, double *d_out, int *d_out_counts);
int yta_bytetrack_sync(yta_bytetrack *engine);      /* waits; reports device-side errors */
/* The S per-stream ID counters on the device (waits): the last ID each stream issued, i.e. the
 * reference's BaseTrack._count after that stream's frames (basetrack.py:37-40), for the
 * device-buffer path where no host copy follows the frames. */
int yta_bytetrack_next_ids(yta_bytetrack *engine, long long *next_id);

/* Pipelined host-buffer update (ByteTrack engines): submit enqueues one frame of every stream and
 * returns at once; collect waits for the OLDEST submitted frame and reports it.  Up to three
 * frames are in flight, so frame f's detections travel host -> device while frame f-1's kernels
 * run and frame f-2's rows travel back: both PCIe directions and the kernels overlap (the synchronous
 * yta_bytetrack_update does them one after the other).  Results are identical to
 * yta_bytetrack_update frame by frame.
 *   submit: dets / det_offsets as yta_bytetrack_update; next_id: S counters written to the device
 *     before the frame, or NULL to continue the engine's own (with frames in flight pass NULL:
 *     the host copies are a frame behind); out: out_capacity >= det_offsets[S] rows x 8, filled
 *     by the matching collect (rows beyond out_offsets[S] unspecified).  Page-locked dets / out
 *     are DMA'd directly and must stay untouched until the frame is collected; pageable dets are
 *     staged during the call (reusable at once).  A fourth submit before a collect fails with
 *     YTA_ERR_INVALID; so do the synchronous update / reset / reserve while frames are in flight.
 *   collect: next_id (S, may be NULL) receives the counters after that frame; out_offsets S + 1
 *     row offsets into that frame's out; device error flags are reported here. */
int yta_bytetrack_submit(yta_bytetrack *engine, const double *dets, const int *det_offsets,
                         const long long *next_id, double *out, int out_capacity);
int yta_bytetrack_collect(yta_bytetrack *engine, long long *next_id, int *out_offsets);
/* Accounting of the pipelined path since the last reset (n doubles, up to 21): frames collected;
 * detection bytes DMA'd straight from the caller's page-locked buffer / staged through the
 * engine's pinned buffers; output-row bytes DMA'd straight into the caller's buffer / staged;
 * host milliseconds spent staging detections, inside submit, waiting in collect, copying staged
 * rows out; GPU milliseconds (per frame, from its events, summed) of the copy-in, the kernels +
 * row snapshot, the copy-out, and the frame's whole span (copy-in start to copy-out end); host
 * milliseconds inside the direct copy-in call, the kernel launches and the copy-out call, the
 * small offset copy in, the small counter / offset copies out (0: the kernels store them), and
 * the page-locked checks; the submits that waited for the newest frame's kernels to bound the
 * track capacity, and the submits that drained the pipeline to check or grow it.
 * reset != 0 zeroes the accounting after the read. */
int yta_bytetrack_pipe_stats(yta_bytetrack *engine, double *stats, int n, int reset);
/* float32 detections (ultralytics hands BoxMOT float32 boxes; the reference promotes them to
 * float64 exactly, byte_tracker.py:143): packed rows of 6 float32 cross PCIe at half the bytes and
 * are widened on the device, so every result equals the float64 call on the promoted rows.  Same
 * contracts as yta_bytetrack_submit / yta_bytetrack_update otherwise. */
int yta_bytetrack_submit_f32(yta_bytetrack *engine, const float *dets, const int *det_offsets,
                             const long long *next_id, double *out, int out_capacity);
int yta_bytetrack_update_f32(yta_bytetrack *engine, const float *dets, const int *det_offsets,
                             long long *next_id, double *out, int out_capacity,
                             int *out_offsets);

/* Host-buffer update of a SUBSET of the streams (update(ctx, n_streams,
 * stream_ids, ...)).  In the reference every camera stream is its own tracker
 * (examples/track.py:43-57) and a stream without a new frame is simply not called
 * (examples/val.py:184-226 runs sequences of different lengths side by side).  stream_ids:
 * n_streams ascending ids in 0..S-1; dets / det_offsets (n_streams + 1) / next_id (n_streams) /
 * out / out_offsets (n_streams + 1) as yta_bytetrack_update, over those streams in id order.
 * Every other stream is left exactly as it was: tracks, Kalman state, frame counter, ID counter. */
int yta_bytetrack_update_streams(yta_bytetrack *engine, int n_streams, const int *stream_ids,
                                 const double *dets, const int *det_offsets, long long *next_id,
                                 double *out, int out_capacity, int *out_offsets);
/* Device form of the subset update: d_active = S ints on the device, nonzero = update that stream
 * this call (NULL = every stream); skipped streams report 0 rows in d_out_counts. */
int yta_bytetrack_update_device_masked(yta_bytetrack *engine, const int *d_active,
                                       const double *d_dets, const int *d_det_offsets,
                                       double *d_out, int *d_out_counts);
/* Reset ONE stream to a freshly created tracker (no tracks, frame and ID counters 0), as
 * constructing a new BYTETracker for that camera would (byte_tracker.py:115-130); the other
 * streams are untouched.  Also for BoT-SORT engines. */
int yta_bytetrack_reset_stream(yta_bytetrack *engine, int stream);

/* Parity introspection: copy stream s's live tracks, tracked list first then lost list, in list
 * order.  Per track: list (0 tracked / 1 lost), id, state (0 New 1 Tracked 2 Lost 3 Removed),
 * activated, frame_id, start_frame, tracklet_len (ints: 7 x int64 per track), mean (8 f64), cov
 * (64 f64).  *n_tracks receives the count; buffers must hold track_capacity entries. */
int yta_bytetrack_get_state(yta_bytetrack *engine, int stream, int *n_tracks, long long *ints,
                            double *mean, double *cov);
/* Measurement: when enabled, HIP events are recorded around each phase of a frame on the
 * engine's stream; collect returns per-phase milliseconds summed over the covered frames, 6 values
 * in launch order: k_s1_prep, k_s1_edges, k_s1_lap (BoT-SORT and match_thresh > 1: the fused
 * k_stage1 in the first, the next two 0), stage23, apply, finish. */
int yta_bytetrack_profile(yta_bytetrack *engine, int enable);
int yta_bytetrack_profile_collect(yta_bytetrack *engine, double *ms, int *frames);
/* Last frame's counts summed over streams (synchronises): dets, high, second, pool, activated,
 * unconfirmed, leftovers, rest, births, tracked', lost', tracked, lost, output rows, stage-1
 * candidate edges, stage-2+3 candidate edges, then the cumulative number of stream-frames whose
 * stage-1 / stage-2+3 association did not fit in LDS and ran over global memory, then (ByteTrack)
 * the lost-list Kalman records the last frame left untouched (lazy prediction), then (ByteTrack)
 * the stage-1 candidate edges left to the solver after the single-edge components, then the
 * cumulative number of stream-frames whose duplicate-removal grid (k_finish) did not fit in LDS
 * (21 int64). */
int yta_bytetrack_stats(yta_bytetrack *engine, long long *stats);
/* Introspection of the engine's launch modes (writes min(n, YTA_BT_MODES) int64): the few-stream
 * mode chosen at create (YTA_SPLIT23), the mode the kernel arguments carry (stage 2 / 3 in two
 * blocks per stream), the fallback arenas pooled, cached HIP graphs enabled (YTA_GRAPHS), BoT-SORT
 * split stage 1 (YTA_BS_SPLIT), graph captures and graph replays so far, track capacity, max
 * detections.  The third is the number of pooled global fallback arenas (a stream-frame whose
 * association does not fit in LDS is redone over one of them by the launch's redo kernel, which
 * runs that many blocks): two per stream in the split mode up to a bound of 32 (YTA_WS_POOL).  The first two agree for the engine's whole life, reserve() included. */
#define YTA_BT_MODES 9
int yta_bytetrack_modes(yta_bytetrack *engine, long long *out, int n);
/* Tuning / testing: bytes of LDS the association kernels may use per stream (default 150 KiB,
 * at most 150 KiB); a stream-frame that does not fit runs over global memory.  0 forces the
 * global-memory path for every stream. */
int yta_bytetrack_set_lds(yta_bytetrack *engine, int bytes);
/* Throughput helper: the engine's HIP stream (hipStream_t as void*) */
int yta_bytetrack_hip_stream(yta_bytetrack *engine, void **stream);

/* Tensor path: one frame of all S streams from device rows to device rows, stream-ordered, for a
 * detector that runs on the same device.  Results equal yta_bytetrack_update's, bit for bit, on
 * the same values.
 *   Stream order.  caller_stream is a hipStream_t (NULL: the legacy default stream).  The call
 *     returns without waiting for the device.  What it enqueues runs on the engine's own stream,
 *     after everything queued on caller_stream at the time of the call; on return caller_stream
 *     has been made to wait for the frame's last launch, so later work on it sees the outputs and
 *     may free or overwrite the inputs.  Work on any OTHER stream needs its own ordering.
 *     A caller_stream that is being captured into a graph is refused (YTA_ERR_INVALID).
 *   In.  d_dets: rows [x1, y1, x2, y2, conf, cls] of dtype (YTA_F64 / YTA_F32 / YTA_F16),
 *     row_stride elements apart (>= 6: a column slice of a wider tensor is fine, any alignment of
 *     whole elements), stream 0's det_counts[0] rows first, then stream 1's, ...  float32 and
 *     float16 values are promoted exactly, as the reference promotes float32
 *     (byte_tracker.py:143).  A 16-byte aligned float64 tensor with row_stride 6 is read in
 *     place; anything else is widened into the engine's staging by one launch, which also turns
 *     det_counts into the device offsets.  det_counts: S ints in HOST memory.  next_id: S counters
 *     in HOST memory written to the device before the frame, or NULL to continue the engine's
 *     own; both are copied during the call and reusable at once.  d_active: S ints on the device,
 *     nonzero = update that stream (see yta_bytetrack_update_device_masked), or NULL.
 *   Out.  d_rows (16-byte aligned, rows_capacity >= sum(det_counts) rows x 8 float64) receives the
 *     packed [x1,y1,x2,y2,id,conf,cls,det_ind] rows, stream after stream; d_row_offsets (S + 1
 *     ints) delimit the streams; d_row_stream (rows_capacity ints, may be NULL) holds each row's
 *     stream id and -1 from d_row_offsets[S] on.  Rows past d_row_offsets[S] are unspecified.
 *     Nothing is copied to the host.
 *   Capacity.  Both capacities grow as needed before anything is enqueued, so the frame never
 *     raises the device's capacity flags.  max_dets follows det_counts.  Track capacity is bounded
 *     on the host: the live tracks after the newest tensor frame known to have run (its kernels
 *     store them into page-locked memory) plus every detection enqueued since.  If
 *     track_capacity >= live tracks + every detection enqueued since the caller last synchronised
 *     the engine, no call waits for the device (host_waits below stays 0); otherwise the call
 *     waits for the engine's stream, reads the exact counters and grows the engine if they
 *     require it.  Frames fed through yta_bytetrack_update_device in between are not counted.
 *   Mixing.  The synchronous entry points wait for the tensor frames in flight and see their
 *     state; device error flags are reported by the next call that synchronises
 *     (yta_bytetrack_sync).  With pipelined frames in flight the call fails with YTA_ERR_INVALID.
 */
#define YTA_F64 0
#define YTA_F32 1
#define YTA_F16 2
int yta_bytetrack_update_tensors(yta_bytetrack *engine, void *caller_stream, const void *d_dets,
                                 int dtype, long long row_stride, const int *det_counts,
                                 const int *d_active, const long long *next_id, double *d_rows,
                                 long long rows_capacity, int *d_row_offsets, int *d_row_stream);
/* Accounting of the tensor path (writes min(n, 4) int64, also for BoT-SORT engines): frames
 * enqueued; host_waits, the calls that blocked on the device; reserves, the times the engine
 * grew; ingest_skipped, the frames whose float64 rows were read in place. */
int yta_bytetrack_tensor_stats(yta_bytetrack *engine, long long *out, int n);

/* ---- BoT-SORT engine: S independent streams ----------------------------------------------
 * The same engine object as ByteTrack (yta_bytetrack_destroy / reset / reserve / capacity / sync /
 * get_state / profile / stats / set_lds / hip_stream all apply; get_state's mean is xywh) with
 * BoT-SORT's association (IoU + gated cosine appearance cost), xywh Kalman filter, feature EMA
 * and class vote.  IDs start from 0 per stream at creation (BaseTrack.clear_count, :205). */
typedef struct yta_bytetrack yta_botsort;
typedef struct {
    double track_high_thresh;     /* botsort.yaml / ctor default 0.5  */
    double track_low_thresh;      /* 0.1  */
    double new_track_thresh;      /* 0.6  */
    double match_thresh;          /* 0.8  */
    double proximity_thresh;      /* 0.5  */
    double appearance_thresh;     /* 0.25 */
    int track_buffer;             /* 30   */
    int frame_rate;               /* 30   */
    int fuse_first_associate;     /* 0    */
    int with_reid;                /* 1: feat_dim-wide float32 ReID features per high detection */
} yta_botsort_params;

int yta_botsort_create(int device, int n_streams, int track_capacity, int max_dets, int feat_dim,
                       const yta_botsort_params *params, yta_botsort **engine);
/* Host-buffer update (synchronous).  dets / det_offsets / next_id / out / out_offsets as
 * yta_bytetrack_update.  feats: for each stream in order, the rows get_features returned for its
 * detections with conf > track_high_thresh, in detection order (float32, feat_dim wide; NULL
 * when with_reid is 0).  warps: S camera-motion 2x3 affines (row-major) or NULL for identity;
 * applied as STrack.multi_gmc (bot_sort.py:95-111) to the predicted pool and the unconfirmed
 * tracks (:290-295). */
int yta_botsort_update(yta_botsort *engine, const double *dets, const int *det_offsets,
                       const float *feats, const double *warps, long long *next_id, double *out,
                       int out_capacity, int *out_offsets);
/* Device-resident update (asynchronous): d_feats holds feat_dim floats per detection row of
 * d_dets (only the high rows are read); d_warps S row-major 2x3 camera warps (multi_gmc,
 * bot_sort.py:95-111, 290-295) or NULL for the identity. */
int yta_botsort_update_device(yta_botsort *engine, const double *d_dets, const int *d_det_offsets,
                              const float *d_feats, const double *d_warps, double *d_out,
                              int *d_out_counts);
/* Tensor path (see yta_bytetrack_update_tensors for the stream order, the inputs, the outputs and
 * the capacity rules).  d_feats: one feat_dim-wide float32 row per DETECTION row, feat_stride
 * floats apart (>= feat_dim; NULL when with_reid is 0); only the rows of detections with
 * conf > track_high_thresh are read, so the others may hold anything.  d_warps: S row-major 2x3
 * warps on the device or NULL for the identity, as yta_botsort_update_device.  The host never sees
 * the warps, so it cannot refuse non-finite entries as yta_botsort_update does: finite warps are
 * the caller's responsibility. */
int yta_botsort_update_tensors(yta_botsort *engine, void *caller_stream, const void *d_dets,
                               int dtype, long long row_stride, const int *det_counts,
                               const float *d_feats, long long feat_stride, const double *d_warps,
                               const int *d_active, const long long *next_id, double *d_rows,
                               long long rows_capacity, int *d_row_offsets, int *d_row_stream);
/* Subset update (see yta_bytetrack_update_streams): feats cover the listed streams' high
 * detections in id order, warps n_streams 2x3 affines (or NULL). */
int yta_botsort_update_streams(yta_botsort *engine, int n_streams, const int *stream_ids,
                               const double *dets, const int *det_offsets, const float *feats,
                               const double *warps, long long *next_id, double *out,
                               int out_capacity, int *out_offsets);
/* Parity introspection, in yta_bytetrack_get_state's track order: smoothed features
 * (feat_dim floats per track, may be NULL), class histograms (8 x (class, summed score) float64
 * per track, may be NULL) and their entry counts (may be NULL). */
int yta_botsort_get_features(yta_botsort *engine, int stream, int *n_tracks, float *feats,
                             double *cls_hist, int *n_cls);

/* ---- OCSORT engine: S independent streams ------------------------------------------------
 * OCSort(per_class, det_thresh, max_age, min_hits, asso_threshold, delta_t, asso_func, inertia,
 * use_byte) per stream; the KalmanBoxTracker.count ID counter per stream (next_id in / out as
 * for ByteTrack; the Python front-end shares one counter per process like the reference). */
typedef struct yta_ocsort yta_ocsort;
#define YTA_ASSO_IOU 0
#define YTA_ASSO_GIOU 1
#define YTA_ASSO_DIOU 2
#define YTA_ASSO_CIOU 3
#define YTA_ASSO_CENTROID 4
typedef struct {
    double det_thresh;       /* ocsort.yaml: 0      (ctor default 0.2)  */
    int max_age;             /* 30                                      */
    int min_hits;            /* 1                   (ctor default 3)    */
    double asso_threshold;   /* iou_thresh 0.3                          */
    int delta_t;             /* 3  (1..8)                               */
    int asso_func;           /* YTA_ASSO_*: giou    (ctor default iou)  */
    double inertia;          /* 0.2                                     */
    int use_byte;            /* 0                                       */
} yta_ocsort_params;

int yta_ocsort_create(int device, int n_streams, int track_capacity, int max_dets,
                      const yta_ocsort_params *params, yta_ocsort **engine);
int yta_ocsort_destroy(yta_ocsort *engine);
int yta_ocsort_reset(yta_ocsort *engine);
int yta_ocsort_capacity(yta_ocsort *engine, int *track_capacity, int *max_dets);
/* Host-buffer update (synchronous): dets / det_offsets / next_id / out / out_offsets as
 * yta_bytetrack_update; img_wh: S x (width, height) of the frames (img.shape[1], img.shape[0];
 * read by the centroid cost only, may be NULL otherwise).  Output rows per stream in the
 * reference's order (reversed tracker list), id = tracker id + 1. */
int yta_ocsort_update(yta_ocsort *engine, const double *dets, const int *det_offsets,
                      const int *img_wh, long long *next_id, double *out, int out_capacity,
                      int *out_offsets);
/* Device-resident update (asynchronous): d_out holds S * track_capacity rows x 8. */
int yta_ocsort_update_device(yta_ocsort *engine, const double *d_dets, const int *d_det_offsets,
                             const int *d_img_wh, double *d_out, int *d_out_counts);
int yta_ocsort_sync(yta_ocsort *engine);
/* Tensor path of the OC-SORT family: yta_bytetrack_update_tensors' contract (stream order, d_dets
 * / dtype / row_stride / det_counts / next_id / d_active in, d_rows / d_row_offsets /
 * d_row_stream out, mixing with the synchronous entry points) on this engine; results equal
 * yta_ocsort_update's bit for bit on the same values.  img_wh: S x (width, height) in HOST memory,
 * copied during the call (needed by the centroid cost only, NULL otherwise; centroid without it
 * is YTA_ERR_INVALID).  Capacity: max_dets follows det_counts; a stream's trackers after the
 * frame are at most those alive after the newest tensor frame known to have run plus every
 * detection enqueued since, and only a bound that does not fit waits for the engine's stream,
 * reads the exact counters and grows the engine as yta_ocsort_update would, so the device never
 * raises its capacity flags here.  Every argument is checked before anything is enqueued. */
int yta_ocsort_update_tensors(yta_ocsort *engine, void *caller_stream, const void *d_dets,
                              int dtype, long long row_stride, const int *det_counts,
                              const int *img_wh, const int *d_active, const long long *next_id,
                              double *d_rows, long long rows_capacity, int *d_row_offsets,
                              int *d_row_stream);
/* Accounting of the tensor path (writes min(n, 4) int64): frames enqueued; host_waits, the calls
 * that blocked on the device; reserves, the times the engine grew; ingest_skipped, the frames
 * whose float64 rows were read in place. */
int yta_ocsort_tensor_stats(yta_ocsort *engine, long long *out, int n);
/* The S per-stream ID counters as the device holds them (waits for the engine's stream). */
int yta_ocsort_next_ids(yta_ocsort *engine, long long *next_id);
/* Stream subsets (see yta_bytetrack_update_streams): the listed streams (ascending ids) updated,
 * every other stream left exactly as it was; per-stream arguments (dets, img_wh n x 2, next_id,
 * out_offsets n + 1) cover the listed streams in id order.  The device form takes an [S] mask on
 * the device (nonzero = update; skipped streams report 0 rows).  reset_stream: one stream back to
 * a freshly constructed tracker (ocsort.py:188-216), the others untouched.  The same three calls
 * exist for DeepOCSORT (feats of the listed streams' kept detections, warps n x 6) and
 * HybridSORT (feats of the listed streams' rows). */
int yta_ocsort_update_streams(yta_ocsort *engine, int n_streams, const int *stream_ids,
                              const double *dets, const int *det_offsets, const int *img_wh,
                              long long *next_id, double *out, int out_capacity,
                              int *out_offsets);
int yta_ocsort_update_device_masked(yta_ocsort *engine, const int *d_active, const double *d_dets,
                                    const int *d_det_offsets, const int *d_img_wh, double *d_out,
                                    int *d_out_counts);
int yta_ocsort_reset_stream(yta_ocsort *engine, int stream);
/* Parity introspection, tracker-list order: ints 7 x int64 per tracker (id, age, hits,
 * hit_streak, time_since_update, kf.observed, kf.attr_saved is not None), x (7 f64), P (49 f64). */
int yta_ocsort_get_state(yta_ocsort *engine, int stream, int *n_tracks, long long *ints,
                         double *x, double *P);
/* Last frame's counts summed over streams: dets, first-round dets, BYTE dets, live trackers,
 * output rows, births, LAP calls, fast-path frames (8 int64). */
int yta_ocsort_stats(yta_ocsort *engine, long long *stats);
/* Solver counters since create / reset, summed over streams (4 int64): first-round solves of the
 * transposed problem (more detections than trackers, association.py:20-28 with dummy columns),
 * those of them whose optimum was not certified unique (exact ties: lapjv replayed instead),
 * lapjv replays in any round (the single-wavefront restatement of lapx's tie-breaking), and -IoU
 * rounds (BYTE / OCR) solved on the rows and columns that have a positive entry. */
#define YTA_LAP_STATS 4
/* n: the length of stats; min(n, YTA_LAP_STATS) values are written (round 6: the n argument is
 * new - round 5 wrote 4 values with no length, round 4 three). */
int yta_ocsort_lap_stats(yta_ocsort *engine, long long *stats, int n);
int yta_ocsort_hip_stream(yta_ocsort *engine, void **stream);
/* Test-only snapshot of the stage-1 matrices, which the later rounds of a frame overwrite.  Off
 * by default (one host branch per update).  When on, yta_ocsort_update / _update_device /
 * _update_streams copy the matrices device to device on the engine's stream, after the last cost
 * kernel and before the first solver kernel; results and launch order are otherwise unchanged.
 * yta_ocsort_update_tensors refuses (YTA_ERR_INVALID) while the switch is on.  Enabling or
 * disabling waits for the engine's stream; disabling frees the copies. */
int yta_ocsort_debug_costs_enable(yta_ocsort *engine, int on);
/* The last update's snapshot of one stream (waits for the engine's stream).  dims[0] = n_high (the
 * matrix rows: first-round detections), dims[1] = n_trk (the columns: trackers after prediction
 * and NaN culling).  rows: n_high input-row indices of the matrix rows; ids: n_trk track ids of
 * the columns; boxes: n_trk x 4 predicted boxes (x1, y1, x2, y2) of the columns, the association
 * function's tracker inputs; asso, cost: n_high x n_trk row-major, the association function's
 * values and -(asso + angle).  Every array may be NULL (then not written): call once for dims, then with
 * arrays of those sizes. */
int yta_ocsort_debug_costs(yta_ocsort *engine, int stream, int *dims, int *rows, long long *ids,
                           double *boxes, double *asso, double *cost);
/* OCSORT Kalman KAT: n tracks initialised from z0 (n x 4, [u, v, s, r]) run `steps` steps of
 * predict + update(z[step] (n x 4 per step); a NaN first value = update(None)), freeze /
 * unfreeze included; final x (n x 7) and full P (n x 49). */
int yta_kf7_run(int device, int n, int steps, const double *z0, const double *z, double *x_out,
                double *P_out);

/* ---- DeepOCSORT engine: S independent streams --------------------------------------------
 * DeepOCSort(det_thresh, max_age, min_hits, iou_threshold, delta_t, asso_func, inertia,
 * w_association_emb, alpha_fixed_emb, aw_param, embedding_off, cmc_off, aw_off) per stream
 * (boxmot/trackers/deepocsort/deep_ocsort.py:308-520; per_class is stored but unused by the
 * reference's update).  The ReID forward pass (:387 get_features) and the CMC estimator (:391
 * cmc.apply) stay outside: their outputs are inputs here.  KalmanBoxTracker.count starts at 1
 * and ids are reported as stored (no +1). */
typedef struct yta_deepocsort yta_deepocsort;
typedef struct {
    double det_thresh;          /* deepocsort.yaml: 0   (ctor default 0.3); must be < 1 */
    int max_age;                /* 30                                                  */
    int min_hits;               /* 1                    (ctor default 3)               */
    double iou_threshold;       /* iou_thresh 0.3                                      */
    int delta_t;                /* 3  (0..8)                                           */
    int asso_func;              /* YTA_ASSO_*: giou     (ctor default iou)             */
    double inertia;             /* 0.2                                                 */
    double w_association_emb;   /* 0.5 (create_tracker does not pass the yaml's 0.75)  */
    double alpha_fixed_emb;     /* 0.95                                                */
    double aw_param;            /* 0.5                                                 */
    int embedding_off;          /* 0                                                   */
    int cmc_off;                /* 0                                                   */
    int aw_off;                 /* 0                                                   */
} yta_deepocsort_params;

int yta_deepocsort_create(int device, int n_streams, int track_capacity, int max_dets,
                          int feat_dim, const yta_deepocsort_params *params,
                          yta_deepocsort **engine);
int yta_deepocsort_destroy(yta_deepocsort *engine);
int yta_deepocsort_reset(yta_deepocsort *engine);
int yta_deepocsort_capacity(yta_deepocsort *engine, int *track_capacity, int *max_dets);
/* Host-buffer update (synchronous).  dets / det_offsets / next_id / out / out_offsets as
 * yta_ocsort_update; feats: feat_dim float32 per detection with conf > det_thresh, in input order
 * (what get_features returns for dets[conf > det_thresh]); warps: S x 6 float64 row-major 2x3
 * affines from the CMC estimator (NULL = identity for every stream); img_wh as yta_ocsort_update. */
int yta_deepocsort_update(yta_deepocsort *engine, const double *dets, const int *det_offsets,
                          const float *feats, const double *warps, const int *img_wh,
                          long long *next_id, double *out, int out_capacity, int *out_offsets);
/* Device-resident update (asynchronous).  d_feats holds feat_dim float32 for EVERY input row
 * (rows at or below det_thresh are ignored); d_warps S x 6 or NULL; d_out S * track_capacity
 * rows x 8. */
int yta_deepocsort_update_device(yta_deepocsort *engine, const double *d_dets,
                                 const int *d_det_offsets, const float *d_feats,
                                 const double *d_warps, const int *d_img_wh, double *d_out,
                                 int *d_out_counts);
int yta_deepocsort_sync(yta_deepocsort *engine);
/* Tensor path (see yta_ocsort_update_tensors).  d_feats: one feat_dim-wide float32 row per
 * DETECTION row, feat_stride floats apart (>= feat_dim; read in place when equal, else gathered
 * by one strided device copy; NULL with embedding_off); rows of detections at or below det_thresh
 * are never read, as in yta_deepocsort_update_device.  d_warps: S x 6 float64 on the device or
 * NULL for the identity; finite warps are the caller's responsibility. */
int yta_deepocsort_update_tensors(yta_deepocsort *engine, void *caller_stream, const void *d_dets,
                                  int dtype, long long row_stride, const int *det_counts,
                                  const float *d_feats, long long feat_stride,
                                  const double *d_warps, const int *img_wh, const int *d_active,
                                  const long long *next_id, double *d_rows,
                                  long long rows_capacity, int *d_row_offsets, int *d_row_stream);
/* As yta_ocsort_tensor_stats / yta_ocsort_next_ids. */
int yta_deepocsort_tensor_stats(yta_deepocsort *engine, long long *out, int n);
int yta_deepocsort_next_ids(yta_deepocsort *engine, long long *next_id);
/* Stream subsets and per-stream reset: as yta_ocsort_update_streams / _update_device_masked /
 * _reset_stream (deep_ocsort.py:308-347 for a fresh tracker). */
int yta_deepocsort_update_streams(yta_deepocsort *engine, int n_streams, const int *stream_ids,
                                  const double *dets, const int *det_offsets, const float *feats,
                                  const double *warps, const int *img_wh, long long *next_id,
                                  double *out, int out_capacity, int *out_offsets);
int yta_deepocsort_update_device_masked(yta_deepocsort *engine, const int *d_active,
                                        const double *d_dets, const int *d_det_offsets,
                                        const float *d_feats, const double *d_warps,
                                        const int *d_img_wh, double *d_out, int *d_out_counts);
int yta_deepocsort_reset_stream(yta_deepocsort *engine, int stream);
/* Parity introspection, tracker-list order: ints 7 x int64 per tracker (id, age, hits,
 * hit_streak, time_since_update, kf.observed, frozen), x (8 f64), P (64 f64), emb (feat_dim f64
 * per tracker; may be NULL). */
int yta_deepocsort_get_state(yta_deepocsort *engine, int stream, int *n_tracks, long long *ints,
                             double *x, double *P, double *emb);
/* Last frame's counts summed over streams: dets, kept dets, 0, live trackers, output rows,
 * births, LAP calls, fast-path frames (8 int64). */
int yta_deepocsort_stats(yta_deepocsort *engine, long long *stats);
/* Solver counters since create / reset, summed over streams (4 int64): first-round solves of the
 * transposed problem (more detections than trackers, association.py:20-28 with dummy columns),
 * those of them whose optimum was not certified unique (exact ties: lapjv replayed instead),
 * lapjv replays in any round (the single-wavefront restatement of lapx's tie-breaking), and -IoU
 * rounds (BYTE / OCR) solved on the rows and columns that have a positive entry. */
int yta_deepocsort_lap_stats(yta_deepocsort *engine, long long *stats, int n);
int yta_deepocsort_hip_stream(yta_deepocsort *engine, void **stream);
/* As yta_ocsort_debug_costs_enable / yta_ocsort_debug_costs.  dims: n_high, n_trk, n_pos (1: the
 * frame ran the dense embedding tiles and row scans), col_ovf (1: a column listed more pairs than
 * fit, so the column weights came from the dense scan).  asso, emb, cost: n_high x n_trk; rw:
 * n_high and cw: n_trk adaptive weights (defined with embeddings on and aw_off = 0).  emb holds the
 * dot products as stored: defined only where asso is not <= 0 (elsewhere the listed-pair path
 * writes nothing, and every reader takes 0 there, association.py:165).  cost is the final
 * -(asso + angle + embedding term). */
int yta_deepocsort_debug_costs_enable(yta_deepocsort *engine, int on);
int yta_deepocsort_debug_costs(yta_deepocsort *engine, int stream, int *dims, int *rows,
                               long long *ids, double *boxes, double *asso, double *emb,
                               double *rw, double *cw, double *cost);
/* DeepOCSORT Kalman KAT (deep_ocsort.py:103-136, 198-293 new-KF branch): n tracks initialised
 * from boxes b0 (n x 4, x1 y1 x2 y2) run `steps` steps of [affine (warps: steps x n x 6, NULL =
 * none)], predict + update(b[step] (n x 4); a NaN first value = update(None)) with the reference's
 * clamps, Q(w, h), R(w, h), freeze / unfreeze replay; final x (n x 8) and full P (n x 64). */
int yta_kf8_run(int device, int n, int steps, const double *b0, const double *b,
                const double *warps, double *x_out, double *P_out);

/* ---- HybridSORT engine: S independent streams --------------------------------------------
 * HybridSORT(det_thresh, max_age, min_hits, iou_threshold, delta_t, asso_func, inertia) per stream
 * (boxmot/trackers/hybridsort/hybridsort.py:329-570) with its hard-wired association settings
 * (:346-360: TCM weight 0, ReID weight 1.3, long-term ReID weight 0 with the 0.4 correction, no
 * BYTE round, no ECC).  One update call = one undecorated HybridSORT.update: the per-class
 * decorator's calls (one per class, each over all trackers) are issued by the caller.  The ReID
 * forward pass (:394 get_features) stays outside: its rows are inputs here.  KalmanBoxTracker.count
 * starts at 0 and ids are reported + 1; det_ind reports the detection's score (dets0[:, 6]). */
typedef struct yta_hybridsort yta_hybridsort;
typedef struct {
    double det_thresh;          /* hybridsort.yaml: 0                                      */
    int max_age;                /* 30                                                      */
    int min_hits;               /* 1                                                       */
    double iou_threshold;       /* iou_thresh 0.3                                          */
    int delta_t;                /* 3  (0..8)                                               */
    int asso_func;              /* YTA_ASSO_IOU..YTA_ASSO_CIOU: giou (centroid: the reference
                                   calls the asso function without the image size, :516)   */
    double inertia;             /* 0.2                                                     */
} yta_hybridsort_params;

int yta_hybridsort_create(int device, int n_streams, int track_capacity, int max_dets,
                          int feat_dim, const yta_hybridsort_params *params,
                          yta_hybridsort **engine);
int yta_hybridsort_destroy(yta_hybridsort *engine);
int yta_hybridsort_reset(yta_hybridsort *engine);
int yta_hybridsort_capacity(yta_hybridsort *engine, int *track_capacity, int *max_dets);
/* Host-buffer update (synchronous).  dets / det_offsets / next_id / out / out_offsets as
 * yta_ocsort_update; feats: feat_dim float32 for EVERY input row, in input order (what
 * get_features returns for the call's boxes). */
int yta_hybridsort_update(yta_hybridsort *engine, const double *dets, const int *det_offsets,
                          const float *feats, long long *next_id, double *out, int out_capacity,
                          int *out_offsets);
/* Device-resident update (asynchronous): d_feats feat_dim float32 per input row; d_out
 * S * track_capacity rows x 8; d_out_counts S ints (may be NULL). */
int yta_hybridsort_update_device(yta_hybridsort *engine, const double *d_dets,
                                 const int *d_det_offsets, const float *d_feats, double *d_out,
                                 int *d_out_counts);
int yta_hybridsort_sync(yta_hybridsort *engine);
/* Tensor path (see yta_ocsort_update_tensors; no image size: asso_func is never centroid).
 * d_feats: one feat_dim-wide float32 row per detection row, feat_stride floats apart (>=
 * feat_dim; read in place when equal, else gathered by one strided device copy). */
int yta_hybridsort_update_tensors(yta_hybridsort *engine, void *caller_stream, const void *d_dets,
                                  int dtype, long long row_stride, const int *det_counts,
                                  const float *d_feats, long long feat_stride,
                                  const int *d_active, const long long *next_id, double *d_rows,
                                  long long rows_capacity, int *d_row_offsets, int *d_row_stream);
/* As yta_ocsort_tensor_stats / yta_ocsort_next_ids. */
int yta_hybridsort_tensor_stats(yta_hybridsort *engine, long long *out, int n);
int yta_hybridsort_next_ids(yta_hybridsort *engine, long long *next_id);
/* Stream subsets and per-stream reset: as yta_ocsort_update_streams / _update_device_masked /
 * _reset_stream (hybridsort.py:329-361 for a fresh tracker). */
int yta_hybridsort_update_streams(yta_hybridsort *engine, int n_streams, const int *stream_ids,
                                  const double *dets, const int *det_offsets, const float *feats,
                                  long long *next_id, double *out, int out_capacity,
                                  int *out_offsets);
int yta_hybridsort_update_device_masked(yta_hybridsort *engine, const int *d_active,
                                        const double *d_dets, const int *d_det_offsets,
                                        const float *d_feats, double *d_out, int *d_out_counts);
int yta_hybridsort_reset_stream(yta_hybridsort *engine, int stream);
/* Parity introspection, tracker-list order: ints 6 x int64 per tracker (id, age, hits,
 * hit_streak, time_since_update, kf.observed), dbl 3 x f64 (conf, cls, det_ind), x (9 f64),
 * P (81 f64), feat (feat_dim float32 smooth_feat per tracker; may be NULL). */
int yta_hybridsort_get_state(yta_hybridsort *engine, int stream, int *n_tracks, long long *ints,
                             double *dbl, double *x, double *P, float *feat);
/* The cls of every live tracker of a stream in list order (PerClassDecorator's active classes,
 * boxmot/utils/__init__.py:38). */
int yta_hybridsort_classes(yta_hybridsort *engine, int stream, double *cls, int cap, int *n);
/* Last frame's counts summed over streams: dets, kept dets, live trackers, output rows, births,
 * LAP calls, long-term corrections, feature jobs (8 int64). */
int yta_hybridsort_stats(yta_hybridsort *engine, long long *stats);
/* Solver counters since create / reset, summed over streams (4 int64): first-round solves of the
 * transposed problem (more detections than trackers, association.py:20-28 with dummy columns),
 * those of them whose optimum was not certified unique (exact ties: lapjv replayed instead),
 * lapjv replays in any round (the single-wavefront restatement of lapx's tie-breaking), and -IoU
 * rounds (BYTE / OCR) solved on the rows and columns that have a positive entry. */
int yta_hybridsort_lap_stats(yta_hybridsort *engine, long long *stats, int n);
int yta_hybridsort_hip_stream(yta_hybridsort *engine, void **stream);
/* As yta_ocsort_debug_costs_enable / yta_ocsort_debug_costs.  emb: n_high x n_trk cosine
 * distances max(0, 1 - u.v / (|u| |v|)); cost: -(asso + angle) + 1.3 emb. */
int yta_hybridsort_debug_costs_enable(yta_hybridsort *engine, int on);
int yta_hybridsort_debug_costs(yta_hybridsort *engine, int stream, int *dims, int *rows,
                               long long *ids, double *boxes, double *emb, double *cost);
/* HybridSORT Kalman KAT (hybridsort.py:112-320): n tracks initialised from rows b0 (n x 5:
 * x1 y1 x2 y2 score) run `steps` steps of predict (velocity clamp) + update(b[step] (n x 5); a
 * NaN first value = update(None)) with the freeze / unfreeze replay; final x (n x 9) and full P
 * (n x 81). */
int yta_kf9_run(int device, int n, int steps, const double *b0, const double *b, double *x_out,
                double *P_out);

/* embedding_distance (matching.py:145-167): out (n x m) = max(0, 1 - t.d / (|t| |d|)) of float32
 * track / detection feature rows (dim wide) in float64, through the BoT-SORT engine's cosine. */
int yta_embedding_distance(int device, const float *track_feats, int n, const float *det_feats,
                           int m, int dim, double *out);
/* compute_aw_max_metric (association.py:79-108): out (nr x nc) = ((w * rw_i) * cw_j) * emb_ij with
 * the row / column weights 1 - max(second / top - bottom, 0) / (1 - bottom) (0 when top == 0, 1
 * when the row / column has fewer than two entries) — the DeepOCSORT engine's AW code. */
int yta_aw_max_metric(int device, const double *emb_cost, int nr, int nc, double w_association_emb,
                      double bottom, double *out);

/* ---- GSI post-processing (boxmot/postprocessing/gsi.py; synchronous, host buffers) ----------
 * linear_interpolation (gsi.py:12-30) of a MOT result table already sorted by (id, frame)
 * (np.lexsort, stable): rows n x ncol float64 (frame, id, ...); for consecutive rows of one id
 * with f_pre + 1 < f < f_pre + interval the missing frames are inserted in front of the row as
 * row_pre + ((row - row_pre) / (f - f_pre)) * i.  virt0 = 1 when the first row's id is -1 (it then
 * pairs with the reference's initial zero row at frame -1, gsi.py:16).  *n_out = rows of the
 * result (YTA_ERR_CAPACITY when > out_cap; out is then untouched). */
int yta_gsi_interpolate(int device, const double *rows, int n, int ncol, int interval, int virt0,
                        double *out, long long out_cap, long long *n_out);
/* gaussian_smooth (gsi.py:33-59): per track k (rows track_off[k] .. track_off[k+1]-1 of t / y),
 * GaussianProcessRegressor(RBF(len_scale[k], 'fixed')).fit(t, y).predict(t) for the 4 columns of
 * y (n x 4: x, y, w, h) -> out (n x 4).  band_width[k] = max(i - j) over the track's pairs with
 * (t_i / l - t_j / l)^2 <= 120 (pairs beyond it have K < e^-60 and are dropped).  A kernel matrix
 * that is not positive definite fails with YTA_ERR_INVALID (sklearn: LinAlgError). */
int yta_gsi_smooth(int device, const double *t, const double *y, const int *track_off,
                   const double *len_scale, const int *band_width, int n_tracks, double *out);

/* ---- ReID crop preprocessing (boxmot/appearance/reid_multibackend.py:189-224) ----------------
 * For each box (x1, y1, x2, y2 float64): box.astype(int) (truncation), x1 = max(0, x1),
 * y1 = max(0, y1), x2 = min(w - 1, x2), y2 = min(h - 1, y2), crop = img[y1:y2, x1:x2] (Python
 * slice semantics: a negative stop counts from the end); cv2.resize(crop, (out_w, out_h),
 * INTER_LINEAR) in OpenCV's fixed-point form (INTER_AREA when both scale factors are exactly 2);
 * BGR -> RGB; (v / 255 - mean) / std in float64 with the ImageNet mean / std of :214-215; stored as
 * float32 (half = 0) or float16 (half = 1, the reference's fp16 .to(torch.half)) into
 * out[n][3][out_h][out_w].  img: h x w x 3 uint8 BGR, row-major.
 * yta_reid_preprocess: synchronous, host buffers; an empty crop fails with YTA_ERR_INVALID naming
 * the box (cv2.resize asserts !ssize.empty()) and nothing is written. */
int yta_reid_preprocess(int device, const uint8_t *img, int h, int w, const double *xyxys, int n,
                        int out_h, int out_w, int half, void *out);
/* Asynchronous device-buffer form over a batch of images (one launch for every box of every
 * camera stream): box b reads image box_img[b] (box_img nullable = image 0) stored at
 * d_imgs + d_img_off[i] with dims d_img_hw[2 i] (h), d_img_hw[2 i + 1] (w).  An empty crop is
 * zero-filled and counted into *d_n_empty (nullable; the caller zeroes it).  stream: a
 * hipStream_t (NULL = the default stream). */
int yta_reid_preprocess_device(const uint8_t *d_imgs, const long long *d_img_off,
                               const int *d_img_hw, const double *d_xyxys, const int *d_box_img,
                               int n, int out_h, int out_w, int half, void *d_out, int *d_n_empty,
                               void *stream);
/* Tensor form: the stateless sibling of yta_reid_preprocess_device for frames that are device
 * tensors, run on `stream`.  d_frames: a device array of the images' first-pixel addresses (any
 * number of separately allocated, pitched or offset views); d_img_hw as above; d_img_pitch: a
 * device array of the bytes between rows of each image (>= 3 w and below 2^31, no alignment
 * requirement; the pixel stride is 3).  d_boxes: rows x1 y1 x2 y2 of dtype (YTA_F64 / YTA_F32 / YTA_F16), row_stride
 * (>= 4) elements apart, aligned to the element size only; values are promoted to float64, which
 * is exact, so the crops equal yta_reid_preprocess's on the promoted boxes.  Box values never reach
 * the host: an empty crop is zero-filled and counted into *d_n_empty, as in the device form. */
int yta_reid_preprocess_tensors(const void *const *d_frames, const int *d_img_hw,
                                const long long *d_img_pitch, const void *d_boxes, int dtype,
                                long long row_stride, const int *d_box_img, int n, int out_h,
                                int out_w, int half, void *d_out, int *d_n_empty, void *stream);
/* get_features (reid_multibackend.py:310): feats[0..count) /= ||feats||_2 over the whole batch,
 * float32 in place (sum of squares accumulated in float64).  Synchronous, host buffer. */
int yta_reid_normalize(int device, float *feats, long long count);
/* Device form: d_work holds >= 256 doubles of scratch. */
int yta_reid_normalize_device(float *d_feats, long long count, double *d_work, void *stream);

/* ---- StrongSORT (boxmot/trackers/strongsort/strong_sort.py:13-99) ---------------------------
 * S streams per engine.  Per frame and stream: camera_update of every track by the 2x3 warp
 * (sort/track.py:129-138), predict (strongsort_kf.py:87-122), the matching cascade of the confirmed
 * tracks on min-over-gallery cosine distance (utils/matching.py:290-308, :360-378) gated by the
 * Mahalanobis distance (sort/linear_assignment.py:144-200), IoU matching of the rest
 * (sort/iou_matching.py:10-87, sort/tracker.py:139-153), both solved by a replay of
 * scipy.optimize.linear_sum_assignment (sort/linear_assignment.py:59-78: its tie-breaking decides
 * the order of the births, hence the ids), the NSA update (strongsort_kf.py:124-189), the EMA
 * feature (sort/track.py:168-174), births / deletions (sort/tracker.py:88-94) and the gallery
 * (sort/tracker.py:96-106, utils/matching.py:343-358).  The ReID features and the ECC warp
 * (strong_sort.py:63, :68) are inputs.  The float32 products and norms, whose order the reference
 * leaves to BLAS, have the fixed order stated in csrc/strongsort.hip. */
typedef struct yta_strongsort yta_strongsort;
typedef struct {
    double max_dist;       /* strongsort.yaml / strong_sort.py:19   0.2   */
    double max_iou_dist;   /* strong_sort.py:20                      0.7   */
    int max_age;           /* strong_sort.py:21                      30    */
    int n_init;            /* strong_sort.py:22                      1     */
    double mc_lambda;      /* strong_sort.py:24                      0.995 */
    double ema_alpha;      /* strong_sort.py:25                      0.9   */
} yta_strongsort_params;
/* nn_budget (strong_sort.py:23, utils/matching.py:356-357): gallery rows kept per track.  The
 * galleries take n_streams x track_capacity x nn_budget x feat_dim x 4 B; a size above the
 * device's free memory returns YTA_ERR_NOMEM with the figures in yta_last_error() and allocates
 * nothing.  track_capacity and max_dets are limited to 3072. */
int yta_strongsort_create(int device, int n_streams, int track_capacity, int max_dets,
                          int feat_dim, int nn_budget, const yta_strongsort_params *params,
                          yta_strongsort **engine);
int yta_strongsort_destroy(yta_strongsort *engine);
/* Empty track lists, id counters back to 1 (sort/tracker.py:58-59). */
int yta_strongsort_reset(yta_strongsort *engine);
int yta_strongsort_capacity(yta_strongsort *engine, int *track_capacity, int *max_dets,
                            int *feat_dim, int *nn_budget);
/* Host-buffer update (synchronous), strong_sort.py:42-99.  dets: rows x1 y1 x2 y2 conf cls of all
 * streams, stream s = rows det_offsets[s] .. det_offsets[s + 1]; feats: feat_dim float32 per row
 * (what get_features returns, strong_sort.py:68); warps: S x 6 float64 row-major 2x3 or NULL, a row
 * whose first value is NaN = no camera update for that stream (strong_sort.py:62: the estimator
 * runs only while the tracker holds a track); out: rows x1 y1 x2 y2 id conf cls det_ind
 * (strong_sort.py:83-96), stream s = rows out_offsets[s] .. out_offsets[s + 1]; n_tracks (S, may be
 * NULL): tracks held after the frame, tentative ones included.  YTA_ERR_CAPACITY when a stream
 * needs more than track_capacity tracks; the engine must then be reset. */
int yta_strongsort_update(yta_strongsort *engine, const double *dets, const int *det_offsets,
                          const float *feats, const double *warps, double *out, int out_capacity,
                          int *out_offsets, int *n_tracks);
/* Device-resident update (asynchronous on the engine's stream).  d_dets: S x max_dets x 6,
 * d_det_counts: S, d_feats: S x max_dets x feat_dim, d_warps: S x 6 or NULL, d_out: S x
 * track_capacity x 8, d_out_counts: S, d_n_tracks: S or NULL.  yta_strongsort_sync waits and
 * reports a capacity error. */
int yta_strongsort_update_device(yta_strongsort *engine, const double *d_dets,
                                 const int *d_det_counts, const float *d_feats,
                                 const double *d_warps, double *d_out, int *d_out_counts,
                                 int *d_n_tracks);
int yta_strongsort_sync(yta_strongsort *engine);
/* Tensor path: device rows in, device rows out, stream-ordered, after yta_bytetrack_update_tensors'
 * contract.  The frame runs on the engine's stream after everything queued on caller_stream (a
 * hipStream_t, NULL = the default stream), and caller_stream is made to wait for the frame's last
 * launch before the call returns; a capturing stream is refused.  Nothing is waited for on the
 * host.  d_dets: packed rows x1 y1 x2 y2 conf cls of dtype (YTA_F64 / YTA_F32 / YTA_F16),
 * row_stride (>= 6) elements apart, aligned to the element size only, stream s = the next
 * det_counts[s] rows; promoted exactly to float64.  d_feats: one feat_dim-wide float32 row per
 * detection row, feat_stride (>= feat_dim) floats apart, read where they are (columns past
 * feat_dim are never read).  d_warps: S x 6 float64 on the device or NULL; a row whose first value
 * is NaN = no camera update for that stream.  d_active: S ints on the device (0 = the stream is
 * left exactly as it was and reports no row) or NULL.  det_counts (S) and next_id (S ID counters
 * written before the frame, to the active streams; NULL = keep the device's) are host memory,
 * copied during the call.  d_rows (16-B aligned): rows_capacity >= sum(det_counts) rows x1 y1 x2
 * y2 id conf cls det_ind, stream s = rows d_row_offsets[s] .. d_row_offsets[s + 1] (S + 1 ints);
 * d_row_stream (rows_capacity ints, may be NULL): each row's stream, -1 from d_row_offsets[S] on.
 * Results are bit-identical to yta_strongsort_update on the promoted values.  Every argument is
 * checked before anything is enqueued.  The engine never grows: a det_counts[s] > max_dets or a
 * rows_capacity below sum(det_counts) returns YTA_ERR_CAPACITY with the engine unchanged; a stream
 * that needs more than track_capacity tracks raises the device flag, which the next
 * yta_strongsort_sync reports, as for yta_strongsort_update_device. */
int yta_strongsort_update_tensors(yta_strongsort *engine, void *caller_stream, const void *d_dets,
                                  int dtype, long long row_stride, const int *det_counts,
                                  const float *d_feats, long long feat_stride,
                                  const double *d_warps, const int *d_active,
                                  const long long *next_id, double *d_rows,
                                  long long rows_capacity, int *d_row_offsets, int *d_row_stream);
/* Accounting of the tensor path since create, up to n of 4 int64: frames enqueued, calls that
 * blocked on the device (yta_strongsort_n_tracks after a tensor frame, or 64 frames in flight),
 * reserves (always 0: the engine does not grow) and ingest_skipped (always 0: float64 rows are
 * not special-cased, every frame is widened into the engine's slab). */
int yta_strongsort_tensor_stats(yta_strongsort *engine, long long *out, int n);
/* The S per-stream ID counters (sort/tracker.py:59 _next_id) as the device holds them; waits for
 * the engine's stream. */
int yta_strongsort_next_ids(yta_strongsort *engine, long long *next_id);
/* Tracks held per stream (S ints, tentative ones included) after the last host-buffer or tensor
 * update.  After a tensor frame it waits for that frame's completion event (one counted host
 * wait) and reads the counts the frame left in page-locked memory; nothing is copied. */
int yta_strongsort_n_tracks(yta_strongsort *engine, int *n_tracks);
/* Stream subset of yta_strongsort_update: the n_streams listed streams (stream_ids ascending) are
 * updated, every other stream is left exactly as it was.  det_offsets (n_streams + 1), warps
 * (n_streams x 6 or NULL), out_offsets (n_streams + 1) and n_tracks (n_streams, may be NULL) cover
 * the listed streams in id order. */
int yta_strongsort_update_streams(yta_strongsort *engine, int n_streams, const int *stream_ids,
                                  const double *dets, const int *det_offsets, const float *feats,
                                  const double *warps, double *out, int out_capacity,
                                  int *out_offsets, int *n_tracks);
/* yta_strongsort_update_device under a device mask: d_active S ints (0 = the stream's state is
 * untouched, its d_out_counts entry is 0 and its d_n_tracks entry the count it had) or NULL. */
int yta_strongsort_update_device_masked(yta_strongsort *engine, const int *d_active,
                                        const double *d_dets, const int *d_det_counts,
                                        const float *d_feats, const double *d_warps,
                                        double *d_out, int *d_out_counts, int *d_n_tracks);
/* One stream back to a freshly constructed tracker (empty list, id counter 1, empty galleries,
 * error flag cleared); the others are untouched.  Synchronous. */
int yta_strongsort_reset_stream(yta_strongsort *engine, int stream);
/* Tracks of one stream in list order (parity introspection); every pointer but n_tracks may be
 * NULL.  ints: n x 5 (id, hits, age, time_since_update, state 1 tentative / 2 confirmed); mean
 * n x 8; cov n x 64; feat n x feat_dim (features[-1]); gallery_len n; gallery n x nn_budget x
 * feat_dim, rows g / |g| in ring order. */
int yta_strongsort_get_state(yta_strongsort *engine, int stream, int *n_tracks, long long *ints,
                             double *mean, double *cov, float *feat, int *gallery_len,
                             float *gallery);
int yta_strongsort_hip_stream(yta_strongsort *engine, void **stream);
/* scipy.optimize.linear_sum_assignment(cost) (sort/linear_assignment.py:61) replayed on the
 * device, ties included: min(nr, nc) pairs sorted by row. */
int yta_lsa_replay(int device, int nr, int nc, const double *cost, int *rows, int *cols);
/* _nn_cosine_distance (utils/matching.py:247-308) per track: gallery n_tracks x budget x feat_dim
 * raw rows, lens[t] (1..budget) valid rows; feats n_dets x feat_dim raw; out n_tracks x n_dets
 * float32 = min over the rows of 1 - <g / |g|, f / |f|> in the engine's float32 order. */
int yta_nn_cosine_min(int device, int n_tracks, int budget, int feat_dim, const float *gallery,
                      const int *lens, int n_dets, const float *feats, float *out);
/* strongsort_kf.py:124-189 update(mean, covariance, measurement, confidence) of n tracks in place
 * (mean n x 8, cov n x 64 full, z n x 4, conf n). */
int yta_kf_nsa_update(int device, int n, double *mean, double *cov, const double *z,
                      const double *conf);
/* strongsort_kf.py:191-233 gating_distance(mean, covariance, measurements) of n tracks against m
 * measurements (zs m x 4) -> out n x m. */
int yta_kf_xyah_gating(int device, int n, const double *mean, const double *cov, int m,
                       const double *zs, double *out);

/* ---- Camera-motion compensation: SparseOptFlow (boxmot/motion/cmc/sof.py:15-162) -------------
 * The estimator BoTSORT (bot_sort.py:228, :293) and DeepOCSort (deep_ocsort.py:351, :391) call once
 * per frame: apply(img, dets) -> 2x3 float64 warp.  Per stream: gray (cvtColor BGR2GRAY), resize
 * by `scale` (INTER_LINEAR), on the first frame goodFeaturesToTrack(maxCorners 3000, quality
 * 0.01, minDistance 1, blockSize 3) under generate_mask (cmc_interface.py:13-24: a 2 % border and
 * every det box x scale); afterwards calcOpticalFlowPyrLK (21x21, 3 levels) of the stored corners
 * from the previous accepted frame, estimateAffinePartial2D(RANSAC 3 px, 2000 iters, 0.99) + LM
 * refinement, translation / scale.  The reference's quirks are kept: the corners are detected once
 * and only filtered (sof.py:155 stores the tracked points under another name), a failed estimate
 * returns the identity and keeps the previous frame.  S streams per engine, every stream's frame
 * in the same launches.  Restatement and parity: oracle/cmc_sof.py (unpinned against cv2 itself). */
typedef struct yta_sof yta_sof;
/* max_h / max_w: the largest input frame (pixels) any stream will pass (device-buffer form; the
 * host-buffer form grows them). */
int yta_sof_create(int device, int n_streams, double scale, int max_h, int max_w,
                   yta_sof **engine);
int yta_sof_destroy(yta_sof *engine);
int yta_sof_reset(yta_sof *engine);
/* Host-buffer apply (synchronous).  frames: stream s's h x w x 3 uint8 BGR frame at
 * frames + frame_off[s] (bytes), frame_hw[2 s] = h, frame_hw[2 s + 1] = w; dets: packed float64
 * rows of det_stride (>= 4) columns, x1 y1 x2 y2 first, stream s at rows det_off[s] ..
 * det_off[s+1]-1 (the rows the tracker passes to cmc.apply); warps: S x 6 float64 out. */
int yta_sof_apply(yta_sof *engine, const uint8_t *frames, const long long *frame_off,
                  const int *frame_hw, const double *dets, int det_stride, const int *det_off,
                  double *warps);
/* Device-buffer apply (asynchronous on the engine stream): the same layout in device memory;
 * d_warps (S x 6 float64) can be handed straight to yta_botsort_update_device /
 * yta_deepocsort_update_device. */
int yta_sof_apply_device(yta_sof *engine, const uint8_t *d_frames, const long long *d_frame_off,
                         const int *d_frame_hw, const double *d_dets, int det_stride,
                         const int *d_det_off, double *d_warps);
/* Tensor apply: the frames and the detection rows are read where they are in device memory, and
 * the call is stream-ordered with no host wait (the protocol of yta_bytetrack_update_tensors: the
 * host arrays go into a ring of mapped page-locked slots, an event hands over from caller_stream
 * to the engine's stream, the frame runs there as plain launches, a second event hands back; a
 * slot is reused after its event has completed; a capturing caller_stream is refused).  To the
 * caller it behaves like one kernel on caller_stream: the inputs may be overwritten right after
 * it, d_warps is visible to later work on that stream.
 *   frames: S device addresses, stream s's first pixel; frame_hw[2 s] = h, frame_hw[2 s + 1] = w;
 *     frame_pitch[s]: bytes between rows (>= 3 w, below 2^31, no alignment requirement; pixel
 *     stride 3).
 *     frames, frame_hw, frame_pitch and det_counts are host arrays, copied during the call.
 *   d_dets: rows of dtype (YTA_F64 / YTA_F32 / YTA_F16), row_stride elements apart (>= 4; >= 5
 *     with conf_thresh), x1 y1 x2 y2 [conf] first, stream s's det_counts[s] rows after stream
 *     s - 1's; promoted to float64 (exact).  conf_thresh (nullable): only rows with
 *     (double)row[4] > *conf_thresh enter the first frame's mask (the rows the trackers pass,
 *     bot_sort.py:266-267, deep_ocsort.py:378-379); a NaN confidence is excluded.
 *   d_warps: S x 6 float64 out, device memory.
 * A frame larger than max_h x max_w grows the engine as yta_sof_apply does (a host wait, counted);
 * the synchronous entry points wait for the engine's stream and so see the frames in flight. */
int yta_sof_apply_tensors(yta_sof *engine, void *caller_stream, const void *const *frames,
                          const int *frame_hw, const long long *frame_pitch, const void *d_dets,
                          int dtype, long long row_stride, const int *det_counts,
                          const double *conf_thresh, double *d_warps);
/* Accounting of the tensor path (writes min(n, 2) int64): frames enqueued; host_waits, the calls
 * that blocked on the device (engine growth, or 64 frames in flight). */
int yta_sof_tensor_stats(yta_sof *engine, long long *out, int n);
int yta_sof_sync(yta_sof *engine);
/* Parity introspection of stream s: the stored corners (prev_keypoints, n x 2 float32, up to
 * cap), whether the stream has its first frame, and the stored previous gray frame (h x w uint8,
 * may be NULL). */
int yta_sof_get_state(yta_sof *engine, int stream, int *initialized, int *n_kp, float *kp,
                      int cap, int *h, int *w, uint8_t *prev_img, int img_cap);
/* Last apply's per-stream outcome (S ints): 0 first frame (corners detected or none found),
 * 1 estimated (warp from RANSAC / 2-point model), 2 identity (no corners left / fewer than two
 * tracked / RANSAC found no model). */
int yta_sof_outcome(yta_sof *engine, int *outcome);
int yta_sof_hip_stream(yta_sof *engine, void **stream);

/* Known-answer entries for the estimator's stages (synchronous, host buffers, one image):
 * gray small image (preprocess) of an h x w x 3 BGR frame -> out (round(h*scale) x round(w*scale));
 * min-eigenvalue map (cornerMinEigenVal, blockSize 3, ksize 3) of a gray image -> float32;
 * goodFeaturesToTrack under a mask -> corners (n x 2 float32, up to 3000). */
int yta_sof_kat_preprocess(int device, const uint8_t *frame, int h, int w, double scale,
                           uint8_t *out, int *out_h, int *out_w);
int yta_sof_kat_min_eigen(int device, const uint8_t *gray, int h, int w, float *eig);
int yta_sof_kat_corners(int device, const uint8_t *gray, const uint8_t *mask, int h, int w,
                        float *corners, int *n);
/* calcOpticalFlowPyrLK of n points between two gray images (same size) -> next (n x 2 float32),
 * status (n uint8); estimateAffinePartial2D(RANSAC) + refinement of n point pairs -> M (2 x 3
 * float64), *ok = 0 when no model (fewer than 2 points). */
int yta_sof_kat_lk(int device, const uint8_t *prev, const uint8_t *next, int h, int w,
                   const float *pts, int n, float *next_pts, uint8_t *status);
int yta_sof_kat_affine(int device, const float *src, const float *dst, int n, double *M, int *ok);

/* ---- Camera-motion compensation: ECC (boxmot/motion/cmc/ecc.py:13-104) -------------------------
 * get_cmc_method('ecc') (motion/cmc/__init__.py:9-11, built by hybridsort.py:366): apply(img, dets)
 * -> 2x3 float32 warp = cv2.findTransformECC(prev, curr, eye(2, 3), warp_mode, (COUNT | EPS,
 * max_iter, eps), None, 1) (ecc.py:73-81) on the gray frames resized by `scale`, translation divided
 * by `scale` (ecc.py:87-89); the identity on the first frame (ecc.py:66-68) and when OpenCV raises
 * (NaN correlation, or a step that would minimise it; ecc.py:82-84: prev_img kept).  warp_mode:
 * MOTION_TRANSLATION 0, MOTION_EUCLIDEAN 1 (the reference's default), MOTION_AFFINE 2
 * (MOTION_HOMOGRAPHY is refused; align=True's preview image: yta_ecc_aligned).  S streams per engine, one 1024-thread block runs a stream's
 * whole Gauss-Newton loop.  Restatement and parity: oracle/cmc_ecc.py (unpinned against cv2). */
typedef struct yta_ecc yta_ecc;
int yta_ecc_create(int device, int n_streams, int warp_mode, double eps, int max_iter,
                   double scale, int max_h, int max_w, yta_ecc **engine);
int yta_ecc_destroy(yta_ecc *engine);
int yta_ecc_reset(yta_ecc *engine);
/* Host-buffer apply (synchronous): frames as yta_sof_apply; warps: S x 6 float32 out. */
int yta_ecc_apply(yta_ecc *engine, const uint8_t *frames, const long long *frame_off,
                  const int *frame_hw, float *warps);
/* Device-buffer apply (asynchronous on the engine stream), then yta_ecc_sync. */
int yta_ecc_apply_device(yta_ecc *engine, const uint8_t *d_frames, const long long *d_frame_off,
                         const int *d_frame_hw, float *d_warps);
/* Tensor apply: as yta_sof_apply_tensors without detections; d_warps: S x 6 float32 out, device
 * memory.  The engine keeps its own copy of every estimate, so yta_ecc_aligned does not read
 * d_warps again (it may be recycled by then).  A larger frame grows the slots (a host wait,
 * counted); one whose warp tables would not fit the LDS stage is refused with YTA_ERR_CAPACITY
 * before anything is enqueued, and the engine is left as it was. */
int yta_ecc_apply_tensors(yta_ecc *engine, void *caller_stream, const void *const *frames,
                          const int *frame_hw, const long long *frame_pitch, float *d_warps);
/* As yta_sof_tensor_stats. */
int yta_ecc_tensor_stats(yta_ecc *engine, long long *out, int n);
int yta_ecc_sync(yta_ecc *engine);
/* Last apply per stream (each array S entries, may be NULL): outcome 0 first frame, 1 estimated,
 * 2 identity (OpenCV would have raised); Gauss-Newton iterations run; the final correlation rho. */
int yta_ecc_outcome(yta_ecc *engine, int *outcome, int *iters, double *rho);
/* Whether stream s has its first frame, and its stored previous gray frame (h x w uint8, may be
 * NULL). */
int yta_ecc_get_state(yta_ecc *engine, int stream, int *initialized, int *h, int *w,
                      uint8_t *prev_img, int img_cap);
/* align=True (ecc.py:91-98, replaces the cv2.warpAffine(prev_img, warp, (w, h), INTER_LINEAR)
 * call there): stream s's previous gray frame - the template its last estimate registered against
 * - warped by the returned matrix, h x w uint8 into out (cap bytes).  *h = *w = 0 and nothing
 * written when the last apply was not an estimate (first frame, or OpenCV would have raised: the
 * reference returns before ecc.py:91).  out = NULL: only *h / *w (size query). */
int yta_ecc_aligned(yta_ecc *engine, int stream, uint8_t *out, long long cap, int *h, int *w);
int yta_ecc_hip_stream(yta_ecc *engine, void **stream);

/* ---- OSNet omni-scale block kernels (boxmot/appearance/backbones/osnet.py LightConv3x3 /
 * ChannelGate / OSBlock; the ReID network's forward, appearance/osnet.py).  Device pointers,
 * asynchronous on `stream` (a hipStream_t; NULL = default), NCHW planes, float32 (half = 0) or
 * float16 (half = 1) storage, float32 arithmetic.
 * yta_osnet_dw3x3: per sample n and channel c (plane of H x W at x + n x_n_stride + c x_c_stride,
 * elements): depthwise 3x3 with zero padding 1 (w: C x 9 float32, BatchNorm folded) + b[c] +
 * ReLU; channels c < n_first go to plane c of y_first (sample stride yf_n_stride) and add their
 * plane sum to plane_sum[n ps_n_stride + c] (float32, may be NULL), the others to plane
 * c - n_first of y_rest.  yta_osnet_gate_sum: out[n][c] = sum_b stack[n][b][c] * gate[n][b][c]
 * for the 4 branches (stack N x 4 x C x P, gate N x 4 x C, out N x C x P). */
int yta_osnet_dw3x3(const void *x, long long x_n_stride, long long x_c_stride, const float *w,
                    const float *b, int N, int C, int H, int W, int half, void *y_first,
                    long long yf_n_stride, int n_first, void *y_rest, long long yr_n_stride,
                    float *plane_sum, long long ps_n_stride, void *stream);
int yta_osnet_gate_sum(const void *stack, const void *gate, int N, int C, int P, int half,
                       void *out, void *stream);
/* yta_osnet_pointwise: every 1x1 convolution of the network (osnet.py Conv1x1 / Conv1x1Linear /
 * LightConv3x3.conv1 / the ChannelGate-free layers, the fc) as an MFMA GEMM over strided tensors
 * (elements; sample n, channel c, pixel p of a tensor at base + n * sn + c * sc + p * sp):
 *   y[n][g cout_g + co][p] = relu?( sum_{k < k1} w[g][k][co] x1[n][g k1 + k][p]
 *                                 + sum_{k < k2} w[g][k1 + k][co] x2[n][k][p]
 *                                 + bias[g cout_g + co] + res[n][g cout_g + co][p] )
 * w: float32 [G][k1 + k2][cout_g] (k-major: BatchNorm folded, transposed); bias, x2 (k2 = 0),
 * res may be NULL.  relu: 0 none, 1 ReLU, 2 ReLU6 (clamp to [0, 6]: mobilenetv2.py ConvBlock),
 * 3 ReLU on both sides of the residual, relu(relu(. + bias) + res) (mlfn.py:87-92). */
typedef struct yta_pw_args {
    const void *x1;
    long long x1n, x1c, x1p;
    const void *x2;
    long long x2n, x2c, x2p;
    const float *w;
    const float *bias;
    const void *res;
    long long rn, rc, rp;
    void *y;
    long long yn, yc, yp;
    int k1, k2, G, cout_g, P, N, relu, pad;
} yta_pw_args;
int yta_osnet_pointwise(const yta_pw_args *args, int half, void *stream);
/* yta_osnet_stem: conv1 (7x7, stride 2, padding 3, 3 -> C0 <= 128; w: float32 C0 x 3 x 7 x 7,
 * BatchNorm folded) + b + ReLU: x N x 3 x H x W -> y N x C0 x ((H-1)/2+1) x ((W-1)/2+1).
 * yta_osnet_pool: kind 0 max 3x3 stride 2 padding 1, 1 average 2x2 stride 2, 2 global mean
 * (y N x C).  yta_osnet_gate: the ChannelGate's fc1 + ReLU, fc2 + sigmoid on the four branches'
 * pooled planes (plane_sum N x 4 x mid float32 sums over P pixels; w1 hid x mid, b1 hid, w2
 * mid x hid, b2 mid in the storage type) -> gate N x 4 x mid. */
int yta_osnet_stem(const void *x, int N, int H, int W, const float *w, const float *b, int C0,
                   int half, void *y, void *stream);
int yta_osnet_pool(const void *x, int N, int C, int H, int W, int kind, int half, void *y,
                   void *stream);
int yta_osnet_gate(const float *plane_sum, int N, int mid, int hid, int P, const void *w1,
                   const void *b1, const void *w2, const void *b2, int half, void *gate,
                   void *stream);
/* ---- OSNet-IBN / OSNet-AIN (osnet.py IN=True, osnet_ain.py): nn.InstanceNorm2d(affine=True) in
 * eval mode, which has no running statistics and cannot be folded into a convolution.
 * yta_osnet_instnorm: per (sample, channel) plane of P contiguous elements (x, res, y: N x C x P)
 *   y = relu?( gamma[c] (x - mean) / sqrt(var + 1e-5) + beta[c] + res )
 * with the plane's own mean and biased variance in float32 (mean first, then the centred sums; no
 * E[x^2] - mean^2), summed in a fixed order without atomics: the same input gives the same bits.
 * res may be NULL (AIN's identity sits outside the norm, IBN's inside: it passes the summed tensor
 * and no res); y must not alias x.  A plane of up to yta_osnet_instnorm_resident() elements is
 * read from memory once; larger planes are read three times.
 * yta_osnet_instnorm_maxpool: the stem of both variants, max_pool2d(relu(instance norm(x)), 3, 2,
 * 1): x N x C x H x W -> y N x C x ((H-1)/2+1) x ((W-1)/2+1), the normalised plane never written.
 * work: N x C x H x W elements of scratch, read only when H W exceeds the resident bound (NULL
 * otherwise): such planes go through yta_osnet_instnorm and yta_osnet_pool.
 * yta_osnet_stem_linear: yta_osnet_stem without the ReLU (the clamp belongs after the norm). */
int yta_osnet_instnorm_resident(void);
int yta_osnet_instnorm(const void *x, const void *res, const float *gamma, const float *beta,
                       int N, int C, int P, int relu, int half, void *y, void *stream);
int yta_osnet_instnorm_maxpool(const void *x, const float *gamma, const float *beta, int N, int C,
                               int H, int W, int half, void *work, void *y, void *stream);
int yta_osnet_stem_linear(const void *x, int N, int H, int W, const float *w, const float *b,
                          int C0, int half, void *y, void *stream);

/* ---- MobileNetV2 (boxmot/appearance/backbones/mobilenetv2.py; appearance/mobilenetv2.py).  The
 * same conventions as the OSNet kernels: device pointers, asynchronous on `stream`, NCHW planes,
 * float32 (half = 0) or float16 (half = 1) storage, float32 arithmetic, BatchNorms folded into
 * float32 weights and biases, no floating-point atomics (the same input gives the same bits).
 * The projection (Bottleneck.conv3, :52-55 and :60, + the residual of :61-62), conv9 (:102,
 * :177) and an unfused expand are yta_osnet_pointwise (relu = 0 / 2 / 2); the global mean (:182)
 * is yta_osnet_pool kind 2.
 * yta_mbv2_stem: conv1 = ConvBlock(3, C0, 3, s=2, p=1) (:94, :39-40): w float32 C0 x 3 x 3 x 3,
 * C0 in 1..64, + b, clamp to [0, 6]: x N x 3 x H x W -> y N x C0 x ((H-1)/2+1) x ((W-1)/2+1).
 * yta_mbv2_dw3x3: Bottleneck.dwconv2 = ConvBlock(C, C, 3, stride, 1, g=C) (:49-51): depthwise 3x3,
 * zero padding 1, stride 1 or 2 (w C x 9) + b[c], clamp to [0, 6]: x N x C x H x W ->
 * y N x C x ((H-1)/stride+1) x ((W-1)/stride+1).
 * yta_mbv2_expand_dw: Bottleneck.conv1 and .dwconv2 (:58-59) in one launch,
 *   y = relu6(dw3x3_stride(relu6(W1 x + b1)) + b2),  x N x Cin x H x W -> y N x Cmid x Ho x Wo,
 * w1 float32 [Cin][Cmid] (k-major, as yta_osnet_pointwise takes it), wdw Cmid x 9.  The Cmid-channel
 * expanded activation exists only in LDS and registers, and the depthwise filter zero-pads THAT
 * activation: a tap outside the image contributes 0, not relu6(b1).  The value between the two
 * layers stays float32 even with float16 storage, so with half = 1 this is one rounding closer to
 * the reference's float32 result than yta_osnet_pointwise followed by yta_mbv2_dw3x3, which stores
 * the expanded tensor as float16 in between.  Cin, Cmid, H and W are arbitrary. */
int yta_mbv2_stem(const void *x, int N, int H, int W, const float *w, const float *b, int C0,
                  int half, void *y, void *stream);
int yta_mbv2_dw3x3(const void *x, const float *w, const float *b, int N, int C, int H, int W,
                   int stride, int half, void *y, void *stream);
int yta_mbv2_expand_dw(const void *x, const float *w1, const float *b1, const float *wdw,
                       const float *b2, int N, int Cin, int Cmid, int H, int W, int stride,
                       int half, void *y, void *stream);

/* ---- MLFN (boxmot/appearance/backbones/mlfn.py; appearance/mlfn.py).  The conventions of the
 * OSNet and MobileNetV2 kernels: device pointers, asynchronous on `stream`, NCHW planes, float32
 * (half = 0) or float16 (half = 1) storage, float32 arithmetic, BatchNorms folded into float32
 * weights and biases, no atomics (the same input gives the same bits).  The stem (:182-184, the
 * bias of conv1 folded into the BatchNorm's) is yta_osnet_stem, the max pool (:185) and the plane
 * means (:42, :193) yta_osnet_pool kinds 0 and 2; fm_conv1 (:66-68), fm_conv3 with both ReLUs
 * and the residual (:85-92, relu = 3; where the block has a downsample, fm_conv3 runs with
 * relu = 1 and is the res of the downsample's 1x1, relu = 1), fc_x and fc_s (:194-195) are
 * yta_osnet_pointwise.
 * yta_mlfn_gconv3x3: MLFNBlock.fm_conv2, fm_bn2, ReLU and the factor selection (:71-82) in one
 * launch: a grouped 3x3 convolution, zero padding 1, stride 1 or 2, G groups of n = C / G
 * channels (w float32 C x n x 9, b float32 C), then
 *   y[b][c] = relu(conv(x)[b][c] + b[c]) * scale[b * scale_stride + c / n],
 * x N x C x H x W -> y N x C x ((H-1)/stride+1) x ((W-1)/stride+1).  Channel c takes the scale of
 * group c / n: the reference's repeat / view / permute (:78-81) gives s[g] to channels g n ..
 * g n + n - 1, not to c % G.  scale float32, N rows of G with a row stride in elements (a slot of
 * the N x 16 G selection buffer); NULL: a plain grouped convolution + bias + ReLU.  C, G (dividing
 * C), H and W are arbitrary; N and G at most 65535.
 * yta_mlfn_fsm: MLFNBlock.fsm (:41-52) after its average pool: pooled N x cin plane means in the
 * storage type (yta_osnet_pool kind 2 of the block input), three 1x1 layers with bias (w1
 * [cin][f0], w2 [f0][f1], w3 [f1][G]: float32, k-major as yta_osnet_pointwise takes them), ReLU,
 * ReLU, sigmoid.  The result, rounded to the storage type, goes to sel[n * sel_stride + g]
 * (float32: the scale of yta_mlfn_gconv3x3 and, with float32 storage, the input of fc_s) and, when
 * sel_t is not NULL, to sel_t[n * sel_t_stride + g] in the storage type (fc_s's input with
 * float16 storage).  cin + f0 + f1 <= 3072.
 * yta_mlfn_subsample: y = x[:, :, ::stride, ::stride], the pixels the stride-2 1x1 downsample
 * (:57, :90) reads: x N x C x H x W -> y N x C x ((H-1)/stride+1) x ((W-1)/stride+1).
 * yta_mlfn_mean2: y = (a + b) * 0.5 over count elements (:197). */
int yta_mlfn_gconv3x3(const void *x, const float *w, const float *b, const float *scale,
                      long long scale_stride, int N, int C, int G, int H, int W, int stride,
                      int half, void *y, void *stream);
int yta_mlfn_fsm(const void *pooled, int N, int cin, int f0, int f1, int G, const float *w1,
                 const float *b1, const float *w2, const float *b2, const float *w3,
                 const float *b3, int half, float *sel, long long sel_stride, void *sel_t,
                 long long sel_t_stride, void *stream);
int yta_mlfn_subsample(const void *x, int N, int C, int H, int W, int stride, int half, void *y,
                       void *stream);
int yta_mlfn_mean2(const void *a, const void *b, long long count, int half, void *y,
                   void *stream);

/* ---- LMBN-n (boxmot/appearance/backbones/lmbn/lmbn_n.py, lmbn/bnneck.py; appearance/lmbn.py).
 * The conventions of the MLFN section: device pointers, asynchronous on `stream`, float32
 * (half = 0) or float16 (half = 1) storage, float32 arithmetic, BatchNorms folded into float32
 * weights and biases, no atomics (the same input gives the same bits).  The trunk, the three
 * branches and the bottleneck behind the global branch are OSNet x1.0 layers (yta_osnet_*).
 * yta_lmbn_pool: the pooling stage (lmbn_n.py:98-105) in one read of x N x C x H x W: per
 * (n, c) plane its maximum, its mean, and the means of AdaptiveAvgPool2d((2, 1))'s two bins,
 * rows [0, ceil(H / 2)) and [floor(H / 2), H) (an odd H puts the middle row into both; H = 1 makes
 * both row 0), each to its own N x C output in the storage type.  An output that is NULL is
 * neither computed into nor touched; at least one must be given.  The maximum starts from the
 * plane's first element (planes may be negative throughout) and is exact in both storage types.
 * yta_lmbn_neck: the seven heads (:107-120) and torch.stack(dim=2).flatten(1, 2) (:127-131) in
 * one launch.  heads: YTA_LMBN_HEADS descriptors in host memory (copied before the call returns).
 * Head j reads N rows of K_j values in the storage type, row n at x + n * x_stride elements
 * (x_stride >= K; two heads may read two halves of one buffer), and writes
 *   y[n * 7 C + c * 7 + j] = act(sum_k w[k * C + c] x[n][k] + bias[c]),   c < C,
 * w float32 K x C (k-major, as yta_osnet_pointwise takes it; heads may share one), bias float32 C
 * or NULL; act: relu != 0 clamps at 0 first, then, where scale or shift is given (float32 C, a
 * missing one is 1 or 0), v * scale[c] + shift[c]: a BatchNorm that follows the ReLU
 * (reduction_ch_*.bn behind `shared`) and cannot fold into w.  N, C and every K are arbitrary
 * (> 0); N at most 65535 * 32. */
#define YTA_LMBN_HEADS 7
typedef struct yta_lmbn_head {
    const void *x;
    long long x_stride;
    const float *w;
    const float *bias;
    const float *scale;
    const float *shift;
    int K, relu;
} yta_lmbn_head;
int yta_lmbn_pool(const void *x, int N, int C, int H, int W, int half, void *mx, void *mean,
                  void *upper, void *lower, void *stream);
int yta_lmbn_neck(const yta_lmbn_head *heads, int N, int C, int half, void *y, void *stream);

/* ---- CLIP-ReID ViT (boxmot/appearance/backbones/clip/clip/model.py VisionTransformer,
 * make_model.py:96-122; appearance/clip.py).  Device pointers, asynchronous on `stream`, float32
 * (half = 0) or float16 (half = 1) storage, float32 arithmetic, no atomics (the same input gives
 * the same bits).  Activations are row-major (rows, channels) matrices, a token a row; a row
 * stride is in elements and at least the row's length, so a call can read or write every L-th
 * row (token 0 of each sample) or a column slot of a wider buffer.  The necks (make_model.py
 * :111-112) arrive folded into ln_post's affine and into proj.
 * yta_clip_linear: y[m][j] = act(sum_k x[m][k] w[j][k] + bias[j]) (+ res[m][j]) for M rows, an
 * LDS-tiled MFMA GEMM (mfma_f32_32x32x16_f16 / mfma_f32_32x32x2f32, both operand tiles staged in
 * two LDS buffers).  w in the storage type, Nout rows of K (a Linear's weight as stored; both
 * operands are then K-contiguous and staged alike), bias float32 or NULL, res in the storage type
 * or NULL (it may be y), act 0: none, 1: QuickGELU v * sigmoid(1.702 v) (model.py:164-166), ahead
 * of the residual.  M, K and Nout are arbitrary (> 0).
 * yta_clip_layernorm: y[m] = (x[m] - mean) / sqrt(var + eps) * gamma + beta over C channels of
 * each of M rows (model.py:155-161); gamma, beta float32; the mean first, then the biased
 * variance around it, float32.  y may be x.
 * yta_clip_patches: x N x 3 x H x W (H, W multiples of 16) -> y (N H/16 W/16) x 768, row
 * (n, gy, gx), column (c, dy, dx) as conv1.weight.reshape(width, 768) orders them: the patch
 * embedding (:239-241) is yta_clip_linear on these rows.
 * yta_clip_tokens: y N x (G + 1) x width = ln_pre(cat(class_embedding, patch rows of sample n) +
 * positional_embedding) (:242-248); patches N G rows in the storage type; class_embedding
 * (width), positional_embedding ((G + 1) x width), gamma, beta float32.
 * yta_clip_attention: nn.MultiheadAttention's core (:183-185) on qkv N x L x 3 width (q | k | v,
 * head h columns 64 h .. 64 h + 63 of each third): for the first Lq <= L queries of each sample
 * and head softmax(q k^T / 8) v -> y N x Lq x width, heads concatenated.  head_dim must be 64 and
 * divide width; L at most 256 (K and V of a head sit in LDS); anything else is YTA_ERR_INVALID.
 * A query's result has the same bits whatever Lq is. */
int yta_clip_linear(const void *x, long long x_stride, const void *w, long long w_stride,
                    const float *bias, const void *res, long long res_stride, int M, int K,
                    int Nout, int act, int half, void *y, long long y_stride, void *stream);
int yta_clip_layernorm(const void *x, long long x_stride, long long M, int C, const float *gamma,
                       const float *beta, float eps, int half, void *y, long long y_stride,
                       void *stream);
int yta_clip_patches(const void *x, int N, int H, int W, int half, void *y, void *stream);
int yta_clip_tokens(const void *patches, long long patch_stride, const float *class_embedding,
                    const float *positional_embedding, int N, int G, int width,
                    const float *gamma, const float *beta, float eps, int half, void *y,
                    void *stream);
int yta_clip_attention(const void *qkv, int N, int L, int width, int head_dim, int Lq, int half,
                       void *y, void *stream);

#ifdef __cplusplus
}
#endif
#endif
