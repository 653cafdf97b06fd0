"""SparseOptFlow camera-motion compensation on the MI355X.

Reference: boxmot/motion/cmc/sof.py:15-162 (SparseOptFlow: __init__, apply), cmc_interface.py:13-40
(generate_mask, preprocess).  `SparseOptFlow().apply(img, dets)` returns the reference's 2x3
float64 warp; the work runs in csrc/cmc.hip (gray + resize, goodFeaturesToTrack on the first frame,
pyramidal Lucas-Kanade, RANSAC + LM similarity fit) through the C ABI.  `SofEngine` runs S camera
streams per call (every stream's frame in the same launches); its device form writes the S warps
straight into a device buffer that yta_botsort_update_device / yta_deepocsort_update_device read.
`SofEngine.apply_tensors` takes the frames and the detection rows as CUDA tensors where they are
(yta_sof_apply_tensors: stream-ordered, nothing crosses the link, no host wait) and returns the
warps as a CUDA tensor; `SparseOptFlow.apply` goes that way when `img` is a CUDA tensor.
There is no CPU fallback: without the HIP library or a device this raises YTAError.
"""
import ctypes

import numpy as np

from .. import _lib


class SofEngine:
    """S independent SparseOptFlow estimators sharing one device engine."""

    def __init__(self, n_streams=1, scale=0.1, device=0, max_h=1080, max_w=1920):
        self.lib = _lib.load_library()
        self.n_streams = int(n_streams)
        self.scale = float(scale)
        self.device = _lib.parse_device(device)
        h = ctypes.c_void_p()
        _lib.check(self.lib.yta_sof_create(self.device, self.n_streams, self.scale, int(max_h),
                                           int(max_w), ctypes.byref(h)))
        self._h = h
        self._warps = np.zeros((self.n_streams, 6), dtype=np.float64)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.yta_sof_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _lib.check(self.lib.yta_sof_reset(self._h))

    def apply(self, imgs, dets_per_stream):
        """imgs: S (h, w, 3) uint8 BGR frames; dets_per_stream: S (n, >= 4) arrays whose first
        four columns are x1 y1 x2 y2 (the rows the tracker passes to cmc.apply).  Returns
        (S, 2, 3) float64 warps."""
        assert len(imgs) == self.n_streams and len(dets_per_stream) == self.n_streams
        frames, off, hw = [], np.zeros(self.n_streams, np.int64), np.zeros(2 * self.n_streams,
                                                                           np.int32)
        o = 0
        for s, im in enumerate(imgs):
            im = np.ascontiguousarray(im, dtype=np.uint8)
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("SparseOptFlow needs (h, w, 3) BGR uint8 frames")
            frames.append(im.reshape(-1))
            off[s] = o
            hw[2 * s], hw[2 * s + 1] = im.shape[0], im.shape[1]
            o += im.size
        packed = np.concatenate(frames) if len(frames) > 1 else frames[0]
        rows = [np.asarray(d, dtype=np.float64).reshape(len(d), -1)[:, :4] if len(d)
                else np.zeros((0, 4)) for d in dets_per_stream]
        doff = np.zeros(self.n_streams + 1, np.int32)
        np.cumsum([len(r) for r in rows], out=doff[1:])
        dets = np.ascontiguousarray(np.concatenate(rows)) if doff[-1] else np.zeros((1, 4))
        _lib.check(self.lib.yta_sof_apply(self._h, _lib.ptr(packed), _lib.ptr(off), _lib.ptr(hw),
                                          _lib.ptr(dets), 4, _lib.ptr(doff),
                                          _lib.ptr(self._warps)))
        return self._warps.reshape(self.n_streams, 2, 3).copy()

    def apply_tensors(self, frames, dets=None, counts=None, conf_thresh=None, stream=None):
        """The tensor form of apply (yta_sof_apply_tensors).  frames: a list of S CUDA uint8
        (h, w, 3) tensors with strides (pitch, 3, 1), or one (S, h, w, 3) tensor (frame_table in
        trackers/_tensors.py).  dets: a list of S CUDA tensors (n_s, >= 4) of float64 / float32 /
        float16, or one packed tensor with `counts` (TensorFrame's conventions); x1 y1 x2 y2
        [conf] come first, a column slice of a wider tensor is read in place; None: no boxes.
        conf_thresh: only rows with conf (column 4) > conf_thresh enter the mask, chosen on the
        device.  Returns an (S, 2, 3) float64 CUDA tensor, ordered on `stream` (default: the
        current stream): the inputs may be overwritten right after the call."""
        import torch
        from ..trackers import _tensors as T
        S, dev = self.n_streams, self.device
        keep, ptr, hw, pitch = T.frame_table(frames, S, dev)
        need = 4 if conf_thresh is None else 5
        if dets is None:
            dets, counts = torch.zeros((0, need), dtype=torch.float64,
                                       device=keep[0].device), [0] * S
        first = dets[0] if isinstance(dets, (list, tuple)) and len(dets) else dets
        cols = first.shape[1] if isinstance(first, torch.Tensor) and first.dim() == 2 else need
        if cols < need:
            raise ValueError(f"dets: {cols} columns, x1 y1 x2 y2"
                             f"{' conf' if need == 5 else ''} are needed")
        codes = T._dtype_codes(torch)
        rows, cnt = T._rows(torch, dets, counts, S, "dets", dev, cols, tuple(codes))
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        with torch.cuda.stream(stream):
            rows, row_stride = T._pack(torch, rows, need)
            warps = torch.empty((S, 6), dtype=torch.float64, device=keep[0].device)
        th = None if conf_thresh is None else ctypes.byref(ctypes.c_double(float(conf_thresh)))
        _lib.check(self.lib.yta_sof_apply_tensors(
            self._h, ctypes.c_void_p(stream.cuda_stream), _lib.ptr(ptr), _lib.ptr(hw),
            _lib.ptr(pitch), ctypes.c_void_p(rows.data_ptr()) if rows.numel() else None,
            codes[rows.dtype], int(row_stride), _lib.ptr(cnt), th,
            ctypes.c_void_p(warps.data_ptr())))
        return warps.view(S, 2, 3)

    def tensor_stats(self):
        """Accounting of apply_tensors: frames enqueued, calls that blocked on the device."""
        buf = (ctypes.c_longlong * 2)()
        _lib.check(self.lib.yta_sof_tensor_stats(self._h, buf, 2))
        return {"frames": int(buf[0]), "host_waits": int(buf[1])}

    def outcome(self):
        """Per stream: 0 first frame, 1 estimated, 2 identity (see yta_sof_outcome)."""
        out = np.zeros(self.n_streams, np.int32)
        _lib.check(self.lib.yta_sof_outcome(self._h, _lib.ptr(out)))
        return out

    def state(self, stream=0, with_image=False):
        init, n, hh, ww = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        kp = np.zeros((3000, 2), np.float32)
        _lib.check(self.lib.yta_sof_get_state(self._h, int(stream), ctypes.byref(init),
                                              ctypes.byref(n), _lib.ptr(kp), len(kp),
                                              ctypes.byref(hh), ctypes.byref(ww), None, 0))
        st = {"initialized": bool(init.value), "keypoints": kp[:n.value].copy()}
        if with_image and init.value:
            img = np.zeros((hh.value, ww.value), np.uint8)
            _lib.check(self.lib.yta_sof_get_state(self._h, int(stream), ctypes.byref(init),
                                                  ctypes.byref(n), None, 0, ctypes.byref(hh),
                                                  ctypes.byref(ww), _lib.ptr(img), img.size))
            st["prev_img"] = img
        return st


class SparseOptFlow:
    """Drop-in for boxmot.motion.cmc.sof.SparseOptFlow (sof.py:15-61): same constructor
    arguments (warp_mode / eps / max_iter / align / grayscale / draw_optical_flow are accepted
    and, as in the reference, unused by apply), `apply(img, dets) -> 2x3 float64`.  A CUDA `img`
    (uint8 (h, w, 3), rows any pitch >= 3 * w) is read where it is and the warp comes back as a
    CUDA (2, 3) tensor (dets then NumPy or CUDA); NumPy in gives NumPy out."""

    def __init__(self, warp_mode=None, eps=1e-5, max_iter=100, scale=0.1, align=False,
                 grayscale=True, draw_optical_flow=False, device=0):
        if not grayscale:
            raise NotImplementedError("SparseOptFlow(grayscale=False): cvtColor is skipped and "
                                      "goodFeaturesToTrack would receive a 3-channel frame")
        self.scale = scale
        self.align = align
        self.grayscale = grayscale
        self.draw_optical_flow = draw_optical_flow
        self._device = device
        self._engine = None

    def apply(self, img, dets):
        from ..trackers._tensors import is_cuda_tensor
        if is_cuda_tensor(img):
            import torch
            if self._engine is None:
                self._engine = SofEngine(1, self.scale, self._device, img.shape[0], img.shape[1])
            if dets is not None and not is_cuda_tensor(dets):
                d = np.asarray(dets, dtype=np.float64)
                dets = torch.from_numpy(d.reshape(len(d), -1)).to(img.device) if d.size else None
            elif dets is not None and dets.shape[0] == 0:
                dets = None
            return self._engine.apply_tensors([img], None if dets is None else [dets])[0]
        img = np.asarray(img)
        if self._engine is None:
            self._engine = SofEngine(1, self.scale, self._device, img.shape[0], img.shape[1])
        d = np.zeros((0, 4)) if dets is None else np.asarray(dets, dtype=np.float64)
        return self._engine.apply([img], [d])[0]
