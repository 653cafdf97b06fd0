"""Plumbing of the tensor path (yta_bytetrack_update_tensors / yta_botsort_update_tensors and the
OC-SORT family's yta_ocsort / yta_deepocsort / yta_hybridsort _update_tensors): checks
the caller's device tensors, lays them out as the C ABI wants them and allocates the outputs.
Everything here is host-side bookkeeping or a torch call on the caller's stream; no value is read
back from the device.  Anything wrong raises ValueError before a single launch.
"""
import ctypes

import numpy as np

from .. import _lib


def is_cuda_tensor(x):
    """True for a torch tensor in device memory, without importing torch for anything else."""
    return type(x).__module__.split(".")[0] == "torch" and bool(getattr(x, "is_cuda", False))


def _dtype_codes(torch):
    return {torch.float64: _lib.YTA_F64, torch.float32: _lib.YTA_F32, torch.float16: _lib.YTA_F16}


def _check(torch, t, name, device, cols, dtypes):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if not t.is_cuda or t.device.index != device:
        raise ValueError(f"{name}: tensor on {t.device}, the engine runs on cuda:{device}")
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{name}: expected shape (n, {cols}), got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name}: dtype {t.dtype} is none of "
                         f"{', '.join(str(d) for d in dtypes)}")


def _rows(torch, parts, counts, n_streams, name, device, cols, dtypes):
    """One (total, cols) tensor and the S per-stream row counts from either a list of S tensors
    or one tensor + counts.  Checks only; the concatenation happens in `prepare`."""
    if isinstance(parts, (list, tuple)):
        if counts is not None:
            raise ValueError(f"{name}: counts go with one packed tensor, not with a list")
        if len(parts) != n_streams:
            raise ValueError(f"{name}: {len(parts)} tensors for {n_streams} streams")
        for k, t in enumerate(parts):
            _check(torch, t, f"{name}[{k}]", device, cols, dtypes)
        if len({t.dtype for t in parts}) != 1:
            raise ValueError(f"{name}: the streams' tensors differ in dtype")
        return list(parts), np.array([t.shape[0] for t in parts], dtype=np.int32)
    _check(torch, parts, name, device, cols, dtypes)
    if counts is None:
        if n_streams != 1:
            raise ValueError(f"{name}: one packed tensor for {n_streams} streams needs counts")
        counts = [parts.shape[0]]
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if len(c) != n_streams or (c < 0).any():
        raise ValueError(f"counts: expected {n_streams} non-negative entries, got {c.tolist()}")
    if int(c.sum()) != parts.shape[0]:
        raise ValueError(f"counts sum to {int(c.sum())}, {name} has {parts.shape[0]} rows")
    return parts, np.ascontiguousarray(c, dtype=np.int32)


def _pack(torch, rows, min_stride):
    """The checked rows as one tensor whose columns are adjacent and whose rows are a fixed
    stride >= min_stride apart (a column slice of a wider tensor passes as it is)."""
    t = (rows[0] if len(rows) == 1 else torch.cat(rows)) if isinstance(rows, list) else rows
    if t.shape[0] and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < min_stride)):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), min_stride))


class TensorFrame:
    """One frame's checked inputs and fresh outputs, ready for the C call."""

    def __init__(self, engine, dets, counts, active, next_id, stream, feats=None, warps=None,
                 img_shapes=None):
        import torch
        self.torch = torch
        S, dev = engine.n_streams, engine.device
        codes = _dtype_codes(torch)
        # ---- checks first: nothing is allocated or enqueued for a frame that is refused
        dets, self.counts = _rows(torch, dets, counts, S, "dets", dev, 6, tuple(codes))
        total = int(self.counts.sum())
        self.wh = None   # S x (width, height), host (the OC-SORT family's centroid cost)
        if img_shapes is not None:
            if len(img_shapes) != S:
                raise ValueError(f"img_shapes: {len(img_shapes)} shapes for {S} streams")
            self.wh = np.ascontiguousarray([[int(sh[1]), int(sh[0])] for sh in img_shapes],
                                           dtype=np.int32)
        elif getattr(engine, "asso_func", None) == "centroid":
            raise ValueError("img_shapes: the centroid cost needs the image sizes")
        D = getattr(engine, "feat_dim", 0)
        if D:
            if feats is None:
                raise ValueError("feats: this engine runs with ReID features")
            feats, fc = _rows(torch, feats, None if isinstance(feats, (list, tuple))
                              else self.counts, S, "feats", dev, D, (torch.float32,))
            if not np.array_equal(fc, self.counts):
                raise ValueError("feats: one row per detection row is needed, got "
                                 f"{fc.tolist()} rows for {self.counts.tolist()} detections")
        if active is not None:
            if not isinstance(active, torch.Tensor) or not active.is_cuda or \
                    active.device.index != dev or tuple(active.shape) != (S,) or \
                    active.dtype not in (torch.int32, torch.int64, torch.bool, torch.uint8):
                raise ValueError(f"active: expected an integer or bool ({S},) tensor on cuda:{dev}")
        if warps is not None:
            if isinstance(warps, torch.Tensor):
                if not warps.is_cuda or warps.device.index != dev or warps.numel() != 6 * S or \
                        warps.dtype != torch.float64:
                    raise ValueError(f"warps: expected float64 ({S}, 2, 3) on cuda:{dev}")
            else:
                warps = np.ascontiguousarray(warps, dtype=np.float64)
                if warps.size != 6 * S:
                    raise ValueError(f"warps: expected ({S}, 2, 3), got {warps.shape}")
        self.nid = None
        if next_id is not None:
            self.nid = np.ascontiguousarray(next_id, dtype=np.int64).reshape(-1)
            if len(self.nid) != S:
                raise ValueError(f"next_id: expected {S} counters, got {len(self.nid)}")
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        self.stream = stream
        # ---- layout and outputs, all on the caller's stream
        with torch.cuda.stream(stream):
            self.dets, self.row_stride = _pack(torch, dets, 6)
            self.dtype = codes[self.dets.dtype]
            self.feats, self.feat_stride = (None, 0)
            if D:
                self.feats, self.feat_stride = _pack(torch, feats, D)
            self.active = None
            if active is not None:
                self.active = active.to(torch.int32).contiguous()
            self.warps = None
            if warps is not None:
                if not isinstance(warps, torch.Tensor):
                    warps = torch.from_numpy(warps.reshape(S, 6)).to(self.dets.device)
                self.warps = warps.reshape(S, 6).contiguous()
            d = self.dets.device
            self.rows = torch.empty((total, 8), dtype=torch.float64, device=d)
            self.offsets = torch.empty(S + 1, dtype=torch.int32, device=d)
            self.row_stream = torch.empty(total, dtype=torch.int32, device=d)

    @staticmethod
    def _p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    def common_head(self):
        return (ctypes.c_void_p(self.stream.cuda_stream), self._p(self.dets), self.dtype,
                int(self.row_stride), _lib.ptr(self.counts))

    def common_tail(self):
        return (self._p(self.active), _lib.ptr(self.nid), self._p(self.rows), self.rows.shape[0],
                ctypes.c_void_p(self.offsets.data_ptr()), self._p(self.row_stream))

    def result(self):
        return self.rows, self.offsets, self.row_stream


class TensorPath:
    """update_tensors' companions for the trackers' engines (`_abi` names the C prefix:
    yta_<_abi>_tensor_stats / _next_ids / _sync)."""
    _abi = None

    def _call(self, name, *args):
        _lib.check(getattr(self.lib, f"yta_{self._abi}_{name}")(self._h, *args))

    def tensor_stats(self):
        """Accounting of update_tensors: frames enqueued, calls that blocked on the device,
        engine growths, float64 frames read in place."""
        names = ["frames", "host_waits", "reserves", "ingest_skipped"]
        buf = (ctypes.c_longlong * len(names))()
        self._call("tensor_stats", buf, len(names))
        return {k: int(buf[i]) for i, k in enumerate(names)}

    def next_ids(self):
        """The S per-stream ID counters on the device (waits for the engine's stream)."""
        nid = np.zeros(self.n_streams, dtype=np.int64)
        self._call("next_ids", _lib.ptr(nid))
        return nid

    def sync(self):
        """Wait for the engine's stream; raises if a frame since the last wait set a device
        error flag."""
        self._call("sync")


def frame_table(frames, n_streams, device, name="frames"):
    """The pointer table of S device frames for yta_sof_apply_tensors / yta_ecc_apply_tensors /
    yta_reid_preprocess_tensors: `frames` is a list of S CUDA uint8 (h, w, 3) tensors with strides
    (pitch, 3, 1), pitch >= 3 * w (contiguous frames, pitched decoder surfaces, offset views,
    slices of a batch tensor), or one (S, h, w, 3) tensor.  Returns (frames, addresses (S uint64),
    hw (2 S int32), pitch (S int64)); the frames are returned so the caller keeps them alive.
    Checks only: nothing is copied and no value is read from the device."""
    import torch
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4:
            raise ValueError(f"{name}: one tensor must be (S, h, w, 3), got {tuple(frames.shape)}")
        frames = list(frames.unbind(0))
    if not isinstance(frames, (list, tuple)) or len(frames) != n_streams:
        n = len(frames) if isinstance(frames, (list, tuple)) else type(frames).__name__
        raise ValueError(f"{name}: {n} frames for {n_streams} streams")
    ptr = np.zeros(n_streams, dtype=np.uint64)
    hw = np.zeros(2 * n_streams, dtype=np.int32)
    pitch = np.zeros(n_streams, dtype=np.int64)
    for s, f in enumerate(frames):
        who = f"{name}[{s}]"
        if not isinstance(f, torch.Tensor):
            raise ValueError(f"{who}: expected a torch tensor, got {type(f).__name__}")
        if not f.is_cuda or f.device.index != device:
            raise ValueError(f"{who}: tensor on {f.device}, the engine runs on cuda:{device}")
        if f.dtype != torch.uint8:
            raise ValueError(f"{who}: dtype {f.dtype}, frames are uint8 BGR")
        if f.dim() != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError(f"{who}: expected shape (h, w, 3), got {tuple(f.shape)}")
        h, w = int(f.shape[0]), int(f.shape[1])
        if f.stride(2) != 1 or (w > 1 and f.stride(1) != 3):
            raise ValueError(f"{who}: strides {f.stride()}: the channels must be adjacent and "
                             "the pixels 3 bytes apart (interleaved BGR)")
        p = int(f.stride(0)) if h > 1 else max(int(f.stride(0)), 3 * w)
        if p < 3 * w:
            raise ValueError(f"{who}: row pitch {p} below 3 * w = {3 * w}")
        ptr[s], hw[2 * s], hw[2 * s + 1], pitch[s] = f.data_ptr(), h, w, p
    return list(frames), ptr, hw, pitch


def takes_device_frames(obj):
    """True for this package's own producers (ReIDDetectMultiBackend, SparseOptFlow, ECC,
    IdentityCMC), which take a CUDA frame and CUDA boxes where they are.  Any other `reid=` /
    `cmc=` object is handed a NumPy frame and NumPy rows, as the reference's interface has it."""
    from ..appearance.reid_multibackend import ReIDDetectMultiBackend
    from ..motion.cmc import ECC, IdentityCMC, SparseOptFlow
    return isinstance(obj, (ReIDDetectMultiBackend, SparseOptFlow, ECC, IdentityCMC))
