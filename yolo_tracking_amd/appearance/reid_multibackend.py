"""Device-side ReID preprocessing, mirroring boxmot/appearance/reid_multibackend.py.

The reference crops, resizes (cv2 INTER_LINEAR), colour-converts and standardises every detection
on the CPU in a Python loop (`preprocess`, :189-224), stacks the crops, copies them to the device,
runs the ReID network (`forward`, :226-299) and divides the features by one global norm
(`get_features`, :303-311).  Here the image goes to HBM once and `yta_reid_preprocess_device`
writes every crop of every camera stream in one launch, straight into the NCHW tensor the network
reads; `yta_reid_normalize_device` does the global normalisation before the single copy back.
An image that is already a CUDA tensor (uint8 (h, w, 3), rows any pitch >= 3 * w) is read where it
is (`yta_reid_preprocess_tensors`), with NumPy or CUDA boxes; CUDA boxes (float64 / float32 /
float16 rows, a column slice of a wider tensor included) never reach the host, so an empty crop is
then a zero crop instead of an error.

The network: OSNet (appearance/osnet.py, an eval-mode inference graph with folded BatchNorms,
channels-last, batched branches) built from `weights` as the reference builds it from the weight
file name (reid_multibackend.py:57-80): osnet_x0_25 .. osnet_x1_0, and the instance-norm members
of the family, osnet_ibn_x1_0 and osnet_ain_x1_0 (and their narrower widths), whose norms run in
csrc/osnet.hip as well, or MobileNetV2 (appearance/mobilenetv2.py: mobilenetv2_x1_0 and
mobilenetv2_x1_4, csrc/mbv2.hip), or MLFN (appearance/mlfn.py: mlfn, csrc/mlfn.hip), or LMBN-n
(appearance/lmbn.py: lmbn_n, OSNet x1.0 layers in three branches and a seven-head neck,
csrc/lmbn.hip; 3584 features), or the CLIP-ReID ViT-B/16 (appearance/clip.py: clip,
csrc/clip.hip; 1280 features); the reference's .pt state dicts load unchanged
(torch.load(weights_only=True)); an LMBN-n checkpoint's tensors are what runs, where the
reference never reads them (appearance/lmbn.py).  ResNet-50 / ResNet-101 and HA-CNN are not
rebuilt.  A weight file that is not on disk would be
downloaded by the reference (gdown, :61-64) or end the program (:67-72); there is no network here,
so a missing file raises FileNotFoundError.  Freshly initialised weights (benchmarks, plumbing
tests) are an explicit opt-in: `random_init=True`.  `model=` (any torch module on the device
taking (N, 3, 256, 128)) replaces the network; the ONNX / OpenVINO / TensorRT / TFLite export
backends (:82-178) are not rebuilt.  There is no CPU fallback (a missing library raises YTAError).
"""
import warnings
from pathlib import Path
import ctypes

import numpy as np

try:   # before libyta.so loads: the library then binds to torch's HIP runtime (one per process)
    import torch  # noqa: F401
except ImportError:   # pragma: no cover
    torch = None

from .. import _lib
from . import _backbone, clip, lmbn, mlfn, mobilenetv2, osnet

# The rebuilt backbone families as (module, class), in the order a weight file's name is tried
# against them (each module's model_name): the OSNet family first (the trackers' default weights),
# LMBN-n and CLIP-ReID last (by the file's name alone).  tools/bench_osnet.py picks its class here
# as well.
FAMILIES = ((osnet, osnet.OSNetReID), (mobilenetv2, mobilenetv2.MobileNetV2ReID),
            (mlfn, mlfn.MLFNReID), (lmbn, lmbn.LMBNReID), (clip, clip.ClipReID))

OUT_W, OUT_H = 128, 256   # cv2.resize(crop, (128, 256)) at :200-204


def crop_rects(xyxys, h, w):
    """(n, 4) int rows (y0, y1, x0, x1) of `img[y1:y2, x1:x2]` as :193-199 computes them
    (truncation, clamps, Python slice semantics).  Rows with y1 <= y0 or x1 <= x0 are empty."""
    b = np.asarray(xyxys, dtype=np.float64).reshape(-1, 4).astype("int")
    x1 = np.maximum(0, b[:, 0])
    y1 = np.maximum(0, b[:, 1])
    x2 = np.minimum(w - 1, b[:, 2])
    y2 = np.minimum(h - 1, b[:, 3])

    def stop(s, n):
        s = np.where(s < 0, s + n, s)
        return np.clip(s, 0, n)

    return np.stack([np.minimum(y1, h), stop(y2, h), np.minimum(x1, w), stop(x2, w)], axis=1)


def _check_crops(xyxys, h, w):
    r = crop_rects(xyxys, h, w)
    bad = np.nonzero((r[:, 1] <= r[:, 0]) | (r[:, 3] <= r[:, 2]))[0]
    if len(bad):   # cv2.resize asserts !ssize.empty() (cv2.error in the reference)
        i = int(bad[0])
        raise ValueError(f"box {i} {np.asarray(xyxys)[i].tolist()}: empty crop in a {h}x{w} image")


def preprocess_host(xyxys, img, fp16=False, device=0, out_w=OUT_W, out_h=OUT_H):
    """`preprocess` through the synchronous host-buffer ABI -> (N, 3, out_h, out_w) NumPy array
    (float32, or float16 with fp16)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3, "img must be H x W x 3 uint8 (BGR)"
    boxes = np.ascontiguousarray(xyxys, dtype=np.float64).reshape(-1, 4)
    out = np.empty((len(boxes), 3, out_h, out_w), dtype=np.float16 if fp16 else np.float32)
    _lib.check(_lib.load_library().yta_reid_preprocess(
        device, _lib.ptr(img), img.shape[0], img.shape[1], _lib.ptr(boxes), len(boxes), out_h,
        out_w, int(bool(fp16)), _lib.ptr(out)))
    return out


def normalize_host(features, device=0):
    """get_features' `features / np.linalg.norm(features)` through yta_reid_normalize."""
    f = np.array(features, dtype=np.float32, order="C")
    _lib.check(_lib.load_library().yta_reid_normalize(device, _lib.ptr(f), f.size))
    return f


class ReIDDetectMultiBackend:
    """reid_multibackend.py:59 ReIDDetectMultiBackend(weights, device, fp16) with a
    caller-supplied network (`model`, a torch module on `device`)."""

    def __init__(self, weights="osnet_x0_25_msmt17.pt", device=0, fp16=False, model=None,
                 random_init=False):
        import torch
        self.torch = torch
        self.weights = weights
        idx = _lib.parse_device(device)
        self.device = torch.device("cuda", idx)
        self.fp16 = bool(fp16)
        self.nhwc = False
        self.lib = _lib.load_library()
        self.random_init = bool(random_init)
        if model is None and weights is not None:
            model = self._build_backbone(weights)
        self.model = model

    def _build_backbone(self, weights):
        """reid_multibackend.py:57-80 as a dispatch on the weight file name: the first family of
        FAMILIES whose VARIANTS hold a name that occurs in it."""
        for family, cls in FAMILIES:
            name = family.model_name(weights)
            if name is not None:
                break
        else:
            raise NotImplementedError(
                f"ReID weights {str(weights)!r}: only the OSNet family (osnet_x0_25 .. osnet_x1_0, "
                "osnet_ibn_x1_0, osnet_ain_x1_0 and their other widths), MobileNetV2 "
                "(mobilenetv2_x1_0, mobilenetv2_x1_4), MLFN (mlfn), LMBN-n (lmbn_n) and the "
                "CLIP-ReID ViT-B/16 (clip) are rebuilt on the MI355X path; pass "
                "model=<torch module> for other networks")
        w = Path(weights)
        if w.is_file():
            sd = _backbone.load_checkpoint(w)
        elif self.random_init:
            warnings.warn(f"ReID weights {str(w)!r} not on disk: {name} runs with fresh random "
                          "weights (random_init=True)", RuntimeWarning, stacklevel=3)
            sd = None
        else:
            raise FileNotFoundError(
                f"ReID weights {str(w)!r} not found and there is no network to download them "
                f"(reid_multibackend.py:61-72); pass an existing {name} checkpoint, model=<torch "
                "module>, or random_init=True for untrained weights")
        return cls(name, sd, device=self.device, half=self.fp16)

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _preprocess_tensors(self, items):
        """preprocess_batch when an image or a box array is a CUDA tensor: the frames through a
        pointer table, the boxes where they are.  Sizes come from the tensors' shapes; the small
        tables go up from page-locked memory on the current stream, so nothing waits."""
        from ..trackers._tensors import _dtype_codes, _pack, frame_table, is_cuda_tensor
        torch, d = self.torch, self.device
        codes = _dtype_codes(torch)
        imgs, boxes, owner = [], [], []
        for i, (xyxys, img) in enumerate(items):
            if not is_cuda_tensor(img):
                img = torch.from_numpy(np.ascontiguousarray(img, dtype=np.uint8)).to(d)
            imgs.append(img)
            if is_cuda_tensor(xyxys):
                if xyxys.dim() != 2 or xyxys.shape[1] < 4 or xyxys.dtype not in codes or \
                        xyxys.device != img.device:
                    raise ValueError(f"boxes of image {i}: expected a float64 / float32 / float16 "
                                     f"(n, >= 4) tensor on {img.device}, got {xyxys.dtype} "
                                     f"{tuple(xyxys.shape)} on {xyxys.device}")
                b = xyxys[:, :4]
            else:
                b = np.asarray(xyxys, dtype=np.float64).reshape(-1, 4)
                _check_crops(b, int(img.shape[0]), int(img.shape[1]))
                b = torch.from_numpy(np.ascontiguousarray(b)).to(d)
            boxes.append(b)
            owner.append(np.full(b.shape[0], i, dtype=np.int32))
        imgs, ptr, hw, pitch = frame_table(imgs, len(imgs), d.index, "img")
        n = int(sum(b.shape[0] for b in boxes))
        out = torch.empty((n, 3, OUT_H, OUT_W), dtype=torch.half if self.fp16 else torch.float,
                          device=d)
        if n == 0:
            return out
        if len({b.dtype for b in boxes}) != 1:   # promotion to float64 is exact
            boxes = [b.double() for b in boxes]
        rows, row_stride = _pack(torch, boxes, 4)
        # one table: addresses, pitches, (h, w) pairs, then the owner of every box
        k = len(imgs)
        meta = np.zeros(3 * k + (n + 1) // 2, dtype=np.int64)
        meta[:k] = ptr.view(np.int64)
        meta[k:2 * k] = pitch
        meta[2 * k:3 * k] = hw.view(np.int64)
        meta[3 * k:].view(np.int32)[:n] = np.concatenate(owner)
        d_meta = torch.from_numpy(meta).pin_memory().to(d, non_blocking=True)
        p0 = d_meta.data_ptr()
        _lib.check(self.lib.yta_reid_preprocess_tensors(
            ctypes.c_void_p(p0), ctypes.c_void_p(p0 + 16 * k), ctypes.c_void_p(p0 + 8 * k),
            ctypes.c_void_p(rows.data_ptr()), codes[rows.dtype], int(row_stride),
            ctypes.c_void_p(p0 + 24 * k), n, OUT_H, OUT_W, int(self.fp16),
            ctypes.c_void_p(out.data_ptr()), None, self._stream()))
        return out

    def preprocess_batch(self, items):
        """One launch for the boxes of several images: items = [(xyxys, img), ...] -> (sum n, 3,
        256, 128) device tensor, crops in item order.  An image may be a CUDA uint8 (h, w, 3)
        tensor and the boxes a CUDA tensor (see _preprocess_tensors); with NumPy boxes an empty
        crop raises as in the reference, with CUDA boxes it is a zero crop."""
        from ..trackers._tensors import is_cuda_tensor
        if any(is_cuda_tensor(img) or is_cuda_tensor(b) for b, img in items):
            return self._preprocess_tensors(items)
        torch = self.torch
        boxes, owner, offs, hws, bufs = [], [], [], [], []
        off = 0
        for i, (xyxys, img) in enumerate(items):
            img = np.ascontiguousarray(img, dtype=np.uint8)
            h, w = img.shape[:2]
            b = np.asarray(xyxys, dtype=np.float64).reshape(-1, 4)
            _check_crops(b, h, w)
            boxes.append(b)
            owner.append(np.full(len(b), i, dtype=np.int32))
            offs.append(off)
            hws += [h, w]
            bufs.append(img.reshape(-1))
            off += img.size
        boxes = np.concatenate(boxes) if boxes else np.empty((0, 4))
        n = len(boxes)
        dt = torch.half if self.fp16 else torch.float
        out = torch.empty((n, 3, OUT_H, OUT_W), dtype=dt, device=self.device)
        if n == 0:
            return out
        d = self.device
        d_img = torch.from_numpy(np.concatenate(bufs)).to(d, non_blocking=False)
        d_off = torch.tensor(offs, dtype=torch.int64, device=d)
        d_hw = torch.tensor(hws, dtype=torch.int32, device=d)
        d_box = torch.from_numpy(np.ascontiguousarray(boxes)).to(d)
        d_own = torch.from_numpy(np.concatenate(owner)).to(d)
        _lib.check(self.lib.yta_reid_preprocess_device(
            ctypes.c_void_p(d_img.data_ptr()), ctypes.c_void_p(d_off.data_ptr()),
            ctypes.c_void_p(d_hw.data_ptr()), ctypes.c_void_p(d_box.data_ptr()),
            ctypes.c_void_p(d_own.data_ptr()), n, OUT_H, OUT_W, int(self.fp16),
            ctypes.c_void_p(out.data_ptr()), None, self._stream()))
        return out

    def preprocess(self, xyxys, img):
        """reid_multibackend.py:189-224 -> (N, 3, 256, 128) tensor on the device."""
        return self.preprocess_batch([(xyxys, img)])

    def forward(self, im_batch):
        """:226-299 for the `pt` backend: the network on the batch -> NumPy."""
        if self.model is None:
            raise RuntimeError("ReIDDetectMultiBackend(weights=None): no network (pass weights "
                               "naming an OSNet variant or model=<torch module>)")
        if self.fp16 and im_batch.dtype != self.torch.float16:
            im_batch = im_batch.half()
        if self.nhwc:
            im_batch = im_batch.permute(0, 2, 3, 1)
        features = self.model(im_batch)
        if isinstance(features, (list, tuple)):
            return (self.to_numpy(features[0]) if len(features) == 1
                    else [self.to_numpy(x) for x in features])
        return self.to_numpy(features)

    def to_numpy(self, x):
        return x.cpu().numpy() if isinstance(x, self.torch.Tensor) else x

    def warmup(self, imgsz=[(256, 128, 3)]):
        im = np.random.randint(0, 255, *imgsz, dtype=np.uint8)
        im = self.preprocess(xyxys=np.array([[0, 0, 128, 256]]), img=im)
        if self.model is not None:
            self.forward(im)

    def normalize_(self, features):
        """In-place global normalisation of a float32 device tensor (get_features :310)."""
        assert features.dtype == self.torch.float32 and features.is_contiguous()
        # partial sums: a fresh block from the caching allocator on the current stream, so calls
        # on different streams (one per camera) never share a workspace
        work = self.torch.empty(256, dtype=self.torch.float64, device=self.device)
        _lib.check(self.lib.yta_reid_normalize_device(
            ctypes.c_void_p(features.data_ptr()), features.numel(),
            ctypes.c_void_p(work.data_ptr()), self._stream()))
        return features

    def get_features(self, xyxys, img, as_tensor=False):
        """:303-311: features of the crops, divided by their global norm (NumPy (N, D)).
        as_tensor: hand the same normalised features back as a device tensor instead (the
        trackers' tensor path, where the embeddings never leave HBM).  img and xyxys may be CUDA
        tensors (preprocess_batch)."""
        torch = self.torch
        on_device = type(xyxys).__module__.split(".")[0] == "torch" and xyxys.is_cuda
        if (xyxys.shape[0] if on_device else np.asarray(xyxys).size) == 0:
            return torch.empty((0, 0), device=self.device) if as_tensor else np.array([])
        with torch.no_grad():
            crops = self.preprocess(xyxys, img)
            if self.model is None:
                self.forward(crops)   # raises
            f = self.model(crops.half() if self.fp16 else crops)
            if isinstance(f, (list, tuple)):
                f = f[0]
            dt = f.dtype
            f = self.normalize_(f.float().contiguous())
            return f.to(dt) if as_tensor else f.to(dt).cpu().numpy()
