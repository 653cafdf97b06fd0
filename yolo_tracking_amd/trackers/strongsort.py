"""StrongSORT on the MI355X: the reference's `StrongSORT` surface over the HIP engine.

Reference: boxmot/trackers/strongsort/strong_sort.py:13-99 (StrongSORT), sort/tracker.py:13-169
(Tracker), sort/track.py:23-198 (Track), sort/linear_assignment.py:13-200,
sort/iou_matching.py:10-87, boxmot/motion/kalman_filters/strongsort_kf.py:21-233 and
boxmot/utils/matching.py:224-378 (NearestNeighborDistanceMetric).  Tracker state (xyah Kalman
filters, counters, the EMA feature and the gallery of up to nn_budget rows per track) lives in HBM
inside the C-ABI engine (yolo_tracking_amd/csrc/strongsort.hip); both assignment problems of a
frame are solved on the device by a replay of scipy.optimize.linear_sum_assignment, whose choice
among equal (clamped) costs decides the order of the births and so the ids.

The ReID forward pass (:68 get_features) and the ECC estimate (:63) are inputs of the engine:
`StrongSORT` builds them as the reference does (build_reid / get_cmc_method('ecc')) unless an
object with get_features is passed as the weights, or `cmc=` is given.
"""
import ctypes
import inspect

import numpy as np

from .. import _lib
from ._streams import StreamSubset
from ._tensors import TensorFrame, TensorPath, is_cuda_tensor, takes_device_frames
from ..appearance import build_reid
from ..motion.cmc import get_cmc_method


class StrongSortEngine(StreamSubset, TensorPath):
    """S independent StrongSORT streams sharing one device engine; one update() = one
    StrongSORT.update (strong_sort.py:42-99) per stream after its features and warp are known."""
    _abi = "strongsort"

    def __init__(self, n_streams=1, feat_dim=512, max_dist=0.2, max_iou_dist=0.7, max_age=30,
                 n_init=1, nn_budget=100, mc_lambda=0.995, ema_alpha=0.9, device=0,
                 track_capacity=512, max_dets=256):
        if nn_budget is None:
            # matching.py:356: an unbounded gallery grows with the track's age; the device
            # gallery is a ring of nn_budget rows
            raise ValueError("nn_budget=None (an unbounded gallery) is not supported: give the "
                             "number of rows kept per track")
        self.lib = _lib.load_library()
        self.n_streams = int(n_streams)
        self.device = _lib.parse_device(device)
        self.feat_dim = int(feat_dim)
        self.nn_budget = int(nn_budget)
        prm = _lib.SsParams(float(max_dist), float(max_iou_dist), int(max_age), int(n_init),
                            float(mc_lambda), float(ema_alpha))
        h = ctypes.c_void_p()
        _lib.check(self.lib.yta_strongsort_create(
            self.device, self.n_streams, int(track_capacity), int(max_dets), self.feat_dim,
            self.nn_budget, ctypes.byref(prm), ctypes.byref(h)))
        self._h = h
        self._out = np.empty((0, 8), dtype=np.float64)
        self._out_off = np.zeros(self.n_streams + 1, dtype=np.int32)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.yta_strongsort_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _lib.check(self.lib.yta_strongsort_reset(self._h))

    def reset_stream(self, stream):
        """Reset one stream to a freshly constructed tracker (ids restart at 1, empty galleries);
        the others are untouched."""
        _lib.check(self.lib.yta_strongsort_reset_stream(self._h, int(stream)))

    def capacity(self):
        c, d = ctypes.c_int(), ctypes.c_int()
        _lib.check(self.lib.yta_strongsort_capacity(self._h, ctypes.byref(c), ctypes.byref(d),
                                                    None, None))
        return c.value, d.value

    def n_tracks(self):
        """Tracks each stream holds (tentative ones included): the reference runs its camera
        motion estimator only on frames where this is >= 1 (strong_sort.py:62).  The counts are
        those after the last update() / update_streams() / update_tensors().  After a tensor frame
        this waits for that frame's completion event and reads the counts it left in page-locked
        memory: one host wait (counted in tensor_stats()["host_waits"]), no copy."""
        n = np.zeros(self.n_streams, dtype=np.int32)
        _lib.check(self.lib.yta_strongsort_n_tracks(self._h, _lib.ptr(n)))
        return n

    def _pack_host(self, dets_per_stream, feats_per_stream, warps):
        """The host-buffer call's packed detections, offsets, feature rows and S x 6 warps (NaN
        rows for the streams without one) for n listed streams."""
        S = len(dets_per_stream)
        dets = [np.asarray(d, dtype=np.float64).reshape(-1, 6) for d in dets_per_stream]
        off = np.zeros(S + 1, dtype=np.int32)
        np.cumsum([len(d) for d in dets], out=off[1:])
        packed = np.ascontiguousarray(np.concatenate(dets)) if off[-1] else np.zeros((0, 6))
        rows = []
        for s, d in enumerate(dets):
            if not len(d):
                continue
            f = None if feats_per_stream is None else feats_per_stream[s]
            if f is None:
                raise ValueError(f"stream {s}: {len(d)} detections but no features")
            f = np.asarray(f, dtype=np.float32).reshape(-1, self.feat_dim)
            if len(f) != len(d):
                raise ValueError(f"stream {s}: {len(f)} feature rows for {len(d)} detections")
            rows.append(f)
        feats = np.ascontiguousarray(np.concatenate(rows)) if rows else None
        w = None
        if warps is not None:
            assert len(warps) == S
            w = np.full((S, 6), np.nan)
            for s, m in enumerate(warps):
                if m is not None:
                    w[s] = np.asarray(m, dtype=np.float64).reshape(6)
        cap, _ = self.capacity()
        need = max(min(int(off[-1]), cap * S), 1)   # an output row is matched to a detection
        if len(self._out) < need:
            self._out = np.empty((2 * need, 8), dtype=np.float64)
        return packed, off, feats, w

    def update(self, dets_per_stream, feats_per_stream, warps=None):
        """dets_per_stream: S float64 (M_s, 6) rows x1 y1 x2 y2 conf cls; feats_per_stream: S
        float32 (M_s, D), the get_features rows of every detection; warps: None or S entries, each
        a 2x3 warp or None (no camera update for that stream).  Returns S (K_s, 8) arrays
        [x1, y1, x2, y2, id, conf, cls, det_ind]."""
        S = self.n_streams
        assert len(dets_per_stream) == S
        packed, off, feats, w = self._pack_host(dets_per_stream, feats_per_stream, warps)
        _lib.check(self.lib.yta_strongsort_update(
            self._h, _lib.ptr(packed), _lib.ptr(off), _lib.ptr(feats), _lib.ptr(w),
            _lib.ptr(self._out), len(self._out), _lib.ptr(self._out_off), None))
        o = self._out_off
        return [self._out[o[s]:o[s + 1]].copy() for s in range(S)]

    def update_streams(self, streams, dets_per_stream, feats_per_stream, warps=None):
        """update() for the listed stream ids only: every per-stream argument and the result
        follow `streams` (any order); the other streams of the engine are left exactly as they
        were (no predict, no ageing, no gallery write, ID counter unchanged)."""
        ids, order = self._subset(streams, len(dets_per_stream))
        packed, off, feats, w = self._pack_host(
            self._reorder(dets_per_stream, order), self._reorder(feats_per_stream, order),
            self._reorder(warps, order))
        n = len(ids)
        o = np.zeros(n + 1, dtype=np.int32)
        _lib.check(self.lib.yta_strongsort_update_streams(
            self._h, n, _lib.ptr(ids), _lib.ptr(packed), _lib.ptr(off), _lib.ptr(feats),
            _lib.ptr(w), _lib.ptr(self._out), len(self._out), _lib.ptr(o), None))
        return self._subset_result(o, order)

    def update_tensors(self, dets, feats, warps=None, counts=None, active=None, next_id=None,
                       stream=None):
        """Stream-ordered update from device tensors to device tensors
        (yta_strongsort_update_tensors): nothing crosses the link and nothing is waited for.
        dets: a list of S CUDA tensors (M_s, 6), or one (total, 6) tensor (a column slice of a
        wider tensor is passed with its row stride) with `counts`, the S per-stream row counts
        (host ints); float64, float32 or float16, promoted exactly.  feats: one float32
        feat_dim-wide row per detection row (a list of S (M_s, D) CUDA tensors or one (total, D)
        tensor, a column slice included), read where they are.  warps: a float64 CUDA tensor of
        S x 6 values whose NaN rows mean "no camera update for that stream", or a host sequence
        of S entries, each a 2x3 warp or None (copied on the stream).  active: optional (S,)
        integer / bool CUDA tensor, nonzero = update that stream; the others keep every byte of
        their state and report no row.  next_id: optional host int64 (S,) ID counters written
        before the frame (read next_ids() after a synchronisation).  stream: the torch stream the
        inputs were produced on and the outputs are consumed on (default: the current one).
        Returns (rows (total, 8) float64, offsets (S + 1,) int32, row_stream (total,) int32) on
        the engine's device: stream s's rows are rows[offsets[s]:offsets[s + 1]], row_stream[r] is
        row r's stream and -1 from offsets[S] on.  Results equal update()'s bit for bit.
        The engine does not grow: more than max_dets rows for a stream raises CapacityError with
        nothing enqueued; a stream outgrowing track_capacity is reported by the next sync().
        Raises ValueError, before anything is enqueued, for tensors on another device or of the
        wrong shape or dtype."""
        if warps is not None and not is_cuda_tensor(warps):
            if len(warps) != self.n_streams:
                raise ValueError(f"warps: {len(warps)} entries for {self.n_streams} streams")
            w = np.full((self.n_streams, 6), np.nan)
            for s, m in enumerate(warps):
                if m is not None:
                    w[s] = np.asarray(m, dtype=np.float64).reshape(6)
            warps = w
        f = TensorFrame(self, dets, counts, active, next_id, stream, feats=feats, warps=warps)
        _lib.check(self.lib.yta_strongsort_update_tensors(
            self._h, *f.common_head(), f._p(f.feats), int(f.feat_stride), f._p(f.warps),
            *f.common_tail()))
        return f.result()

    def state(self, stream=0):
        """Tracks of one stream in list order: id, hits, age, time_since_update, state (1
        tentative, 2 confirmed); Kalman mean (8), covariance (8x8); features[-1]; the gallery rows
        (g / |g|, ring order) and their count."""
        cap, _ = self.capacity()
        n = ctypes.c_int()
        _lib.check(self.lib.yta_strongsort_get_state(self._h, int(stream), ctypes.byref(n), None,
                                                     None, None, None, None, None))
        k = n.value
        ints = np.empty((k, 5), dtype=np.int64)
        mean = np.empty((k, 8))
        cov = np.empty((k, 8, 8))
        feat = np.empty((k, self.feat_dim), dtype=np.float32)
        glen = np.empty(k, dtype=np.int32)
        gal = np.empty((k, self.nn_budget, self.feat_dim), dtype=np.float32)
        if k:
            _lib.check(self.lib.yta_strongsort_get_state(
                self._h, int(stream), ctypes.byref(n), _lib.ptr(ints), _lib.ptr(mean),
                _lib.ptr(cov), _lib.ptr(feat), _lib.ptr(glen), _lib.ptr(gal)))
        return dict(id=ints[:, 0], hits=ints[:, 1], age=ints[:, 2], time_since_update=ints[:, 3],
                    state=ints[:, 4], mean=mean, covariance=cov, feat=feat, gallery_len=glen,
                    gallery=gal)


class StrongSORT:
    """Drop-in for boxmot.trackers.strongsort.strong_sort.StrongSORT (strong_sort.py:13-99).

    model_weights / fp16 name the reference's ReID model: a path builds ReIDDetectMultiBackend
    (build_reid); an object with get_features(xyxys, img) -> (n, D) float32 passed in its place
    (or as `reid=`) is used as the feature producer.  Camera motion: ECC on the GPU as in the
    reference (:40 get_cmc_method('ecc')()); `cmc=` replaces it (an object with
    apply(img, dets) -> 2x3).  As in the reference the estimator is called only on frames where
    the tracker holds a track (:62).  update() also takes a CUDA tensor of detections (and a
    CUDA frame and embeddings) and then returns a CUDA tensor: see _update_tensor.
    """

    def __init__(self, model_weights=None, device=0, fp16=False, max_dist=0.2, max_iou_dist=0.7,
                 max_age=30, n_init=1, nn_budget=100, mc_lambda=0.995, ema_alpha=0.9, reid=None,
                 cmc=None, feat_dim=None, track_capacity=512, max_dets=256):
        if nn_budget is None:
            raise ValueError("nn_budget=None (an unbounded gallery) is not supported: give the "
                             "number of rows kept per track")
        if reid is None and hasattr(model_weights, "get_features"):
            reid = model_weights
        self.model = build_reid(reid, model_weights, device, fp16)              # :27-31
        self.cmc = cmc if cmc is not None else get_cmc_method("ecc")(device=device)   # :40
        self._kw = dict(max_dist=max_dist, max_iou_dist=max_iou_dist, max_age=max_age,
                        n_init=n_init, nn_budget=nn_budget, mc_lambda=mc_lambda,
                        ema_alpha=ema_alpha, device=device, track_capacity=track_capacity,
                        max_dets=max_dets)
        self._engine = None
        if feat_dim is not None:
            self._engine = StrongSortEngine(1, feat_dim=int(feat_dim), **self._kw)

    def _update_tensor(self, dets, img, embs):
        """update() for a CUDA tensor of detections (embs, when given, a CUDA tensor with one row
        per detection): the features and the rows stay on the device.  With a CUDA `img` (uint8
        (h, w, 3), rows any pitch >= 3 * w) nothing crosses the link: the crops and the ECC
        estimate read the frame and the boxes where they are
        (ReIDDetectMultiBackend.get_features, ECC.apply) and the warp goes to the engine as a
        device tensor.  A caller-supplied `reid=` or `cmc=` object that is not this package's gets
        `img.cpu().numpy()` (one download per call) and NumPy boxes.
        As in the reference (:62) the estimator runs only on frames entered with >= 1 track, and
        a skipped frame never becomes ECC's prev_img, so the decision cannot be left to the
        device: it reads n_tracks(), which waits for the PREVIOUS frame's completion event (page-
        locked counts, no copy) and never for the frame being enqueued.  That wait is the price of
        reproducing the reference's skipping; learning K for the returned slice (and whether the
        frame overran track_capacity) is the other, at the end of the call."""
        import torch
        img_dev = is_cuda_tensor(img)
        assert img_dev or isinstance(img, np.ndarray), \
            f"Unsupported 'img' input format '{type(img)}', valid format is np.ndarray"
        assert dets.dim() == 2, "Unsupported 'dets' dimensions, valid number of dimensions is two"
        assert dets.shape[1] == 6, "Unsupported 'dets' 2nd dimension lenght, valid lenghts is 6"
        n = dets.shape[0]
        img_host = None if img_dev else img
        box_host = None

        def host_img():   # for a foreign reid / cmc object: one download per call
            nonlocal img_host
            if img_host is None:
                img_host = img.cpu().numpy()
            return img_host

        def host_boxes():
            nonlocal box_host
            if box_host is None:
                box_host = dets[:, 0:4].double().cpu().numpy()
            return box_host

        warp = None
        if self._engine is not None and self._engine.n_tracks()[0] >= 1:        # :62-65
            if img_dev and takes_device_frames(self.cmc):                        # stays in HBM
                w = self.cmc.apply(img, dets[:, 0:4])
                warp = w.double().reshape(1, 6) if is_cuda_tensor(w) \
                    else [np.asarray(w, dtype=np.float64)]
            else:
                warp = [np.asarray(self.cmc.apply(host_img(), host_boxes()), dtype=np.float64)]
        feats = None
        if n:                                                                    # :68
            if embs is not None:
                if not is_cuda_tensor(embs) or embs.dim() != 2 or len(embs) != n:
                    raise ValueError("embs: with tensor dets, a CUDA tensor with one row per "
                                     "detection is needed")
                feats = embs.float()
            elif self.model is None:
                raise RuntimeError("StrongSORT needs a ReID producer: pass model weights, an "
                                   "object with get_features(xyxys, img), or update(dets, img, "
                                   "embs=...)")
            elif img_dev and takes_device_frames(self.model):
                feats = self.model.get_features(dets[:, 0:4], img, as_tensor=True).float()
            elif "as_tensor" in inspect.signature(self.model.get_features).parameters:
                feats = self.model.get_features(host_boxes(), host_img(), as_tensor=True).float()
            else:
                feats = torch.from_numpy(np.ascontiguousarray(self.model.get_features(
                    host_boxes(), host_img()), dtype=np.float32)).to(dets.device)
            feats = feats.reshape(n, -1)
        if self._engine is None:
            if feats is None:   # no track, no detection: nothing to remember
                return dets.new_zeros((0, 8), dtype=torch.float64)
            self._engine = StrongSortEngine(1, feat_dim=feats.shape[1], **self._kw)
        if feats is None:
            feats = torch.zeros((0, self._engine.feat_dim), dtype=torch.float32,
                                device=dets.device)
        rows, off, _ = self._engine.update_tensors([dets], [feats], warps=warp)
        self._engine.sync()   # a track_capacity overrun is raised here, as update() raises it
        return rows[:int(off[1])]

    def update(self, dets, img, embs=None):
        """dets / img: np.ndarray as the reference; a CUDA tensor (N, 6) of detections is taken
        where it is (embs then a CUDA tensor too, img a CUDA uint8 tensor or an ndarray) and the
        (K, 8) result is then a CUDA tensor (empty where the ndarray form returns np.array([]))."""
        if is_cuda_tensor(dets):
            return self._update_tensor(dets, img, embs)
        assert isinstance(
            dets, np.ndarray
        ), f"Unsupported 'dets' input format '{type(dets)}', valid format is np.ndarray"
        assert isinstance(
            img, np.ndarray
        ), f"Unsupported 'img' input format '{type(img)}', valid format is np.ndarray"
        assert (
            len(dets.shape) == 2
        ), "Unsupported 'dets' dimensions, valid number of dimensions is two"
        assert (
            dets.shape[1] == 6
        ), "Unsupported 'dets' 2nd dimension lenght, valid lenghts is 6"
        dets = np.asarray(dets, dtype=np.float64)
        xyxy = dets[:, 0:4]
        warp = None
        if self._engine is not None and self._engine.n_tracks()[0] >= 1:        # :62-65
            warp = np.asarray(self.cmc.apply(img, xyxy), dtype=np.float64)
        feats = None
        if len(dets):                                                            # :68
            if embs is not None:
                feats = np.asarray(embs, dtype=np.float32)
            elif self.model is None:
                raise RuntimeError("StrongSORT needs a ReID producer: pass model weights, an "
                                   "object with get_features(xyxys, img), or update(dets, img, "
                                   "embs=...)")
            else:
                feats = np.asarray(self.model.get_features(xyxy, img), dtype=np.float32)
            feats = feats.reshape(len(dets), -1)
        if self._engine is None:
            if feats is None:
                return np.array([])     # no track, no detection: nothing to remember
            self._engine = StrongSortEngine(1, feat_dim=feats.shape[1], **self._kw)
        out = self._engine.update([dets], [feats], None if warp is None else [warp])[0]
        if len(out) == 0:
            return np.array([])                                                  # :99
        return out

    @property
    def tracks(self):
        """Snapshot of the device tracks (list order)."""
        return self._engine.state(0) if self._engine is not None else None

    def reset(self):
        if self._engine is not None:
            self._engine.reset()
        if hasattr(self.cmc, "reset"):
            self.cmc.reset()


__all__ = ["StrongSORT", "StrongSortEngine"]
