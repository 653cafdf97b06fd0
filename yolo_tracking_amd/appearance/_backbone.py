"""The driver layer the ReID backbones share (osnet.py, mobilenetv2.py, mlfn.py, lmbn.py, clip.py).

Each backbone is an eval-mode inference graph built from a checkpoint in the reference's key layout:
BatchNorms are folded on the host in float64 (bn_affine, fold_bn), parameters are cast once to the
storage type for PyTorch's operators and to float32 for the kernels (1x1 weights k-major: kmajor),
and crops run through the graph in chunks (ReIDBackbone).  Kernels holds what every HIP forward
needs: the device, the storage type, the current stream, a checked call of a C entry point, and
the entry points more than one family uses (yta_osnet_pointwise, yta_osnet_pool, yta_osnet_stem).
Entry points of one family stay in that family's module, as functions or methods taking a Kernels.
"""
import re

import numpy as np

BN_EPS = 1e-5
CHUNK = 1024   # crops per forward pass: bounds the activations (the block's tensors stay in cache)


def load_checkpoint(path):
    """torch.load(path, weights_only=True) of a reference weight file: a state_dict, or a dict
    holding one under 'state_dict'; 'module.' prefixes dropped (reid_model_factory
    load_pretrained_weights)."""
    import torch
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ck, dict) and "state_dict" in ck:
        ck = ck["state_dict"]
    return {re.sub(r"^module\.", "", k): v for k, v in ck.items()}


def to_f64(sd, drop=()):
    """The state dict (tensors or arrays) as float64 tensors, without the keys that start with one
    of the prefixes in `drop`."""
    import torch
    return {k: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(torch.float64)
            for k, v in sd.items() if not k.startswith(tuple(drop))}


def bn_affine(sd, bn):
    """(scale, shift) of the eval-mode BatchNorm `bn`: y = scale x + shift, in sd's float64."""
    scale = sd[bn + ".weight"] / (sd[bn + ".running_var"] + BN_EPS).sqrt()
    return scale, sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale


def fold_bn(sd, conv, bn):
    """(weight, bias) of the convolution or linear layer `conv` (a weight of any rank, output
    channels first; its bias where it has one) followed by the eval-mode BatchNorm `bn`."""
    w = sd[conv + ".weight"]
    scale, bias = bn_affine(sd, bn)
    if conv + ".bias" in sd:
        bias = bias + sd[conv + ".bias"] * scale
    return w * scale.reshape((-1,) + (1,) * (w.dim() - 1)), bias


def f32(x, device):
    """A kernel's float32 operand on the device."""
    import torch
    return x.to(device, torch.float32).contiguous()


def kmajor(w, device, groups=1):
    """A 1x1 weight (groups * cout_g, K[, 1, 1]) as the float32 [groups][K][cout_g] that
    yta_osnet_pointwise (and yta_mbv2_expand_dw, one group) reads: lanes along the output
    channels."""
    return f32(w, device).reshape(groups, -1, w.shape[1]).transpose(1, 2).contiguous()


class Kernels:
    """The HIP entry points on tensors of one device and storage type."""

    def __init__(self, torch, device, dtype):
        import ctypes
        from .. import _lib
        self.torch, self.device, self.dtype = torch, device, dtype
        self.ct, self._lib = ctypes, _lib
        self.half = int(dtype == torch.float16)
        self.es = 2 if self.half else 4    # bytes per stored element
        self.P = ctypes.c_void_p

    def lib(self):
        return self._lib.load_library()

    def stream(self):
        return self.P(self.torch.cuda.current_stream(self.device).cuda_stream)

    def empty(self, *shape, dtype=None):
        return self.torch.empty(shape, dtype=dtype or self.dtype, device=self.device)

    def call(self, name, *args):
        """The C entry point `name` on the device's current stream, which goes last in every
        signature and is appended here; raises YTAError unless it returns YTA_OK.  Pointers go as
        addresses (data_ptr(), plus a byte offset where needed) or None."""
        self._lib.check(getattr(self.lib(), name)(*args, self.stream()))

    def pw(self, x1, w, bias=None, *, k1, G=1, cout_g, P, N, relu, x2=None, k2=0, res=None,
           out=None, x1s=None, x2s=None, ys=None):
        """1x1 convolution / linear layer through yta_osnet_pointwise: x1 (N, G k1, P) [and x2
        (N, k2, P), concatenated along k] -> (N, G cout_g, P), + bias, + res, then the epilogue
        `relu` names.  x1s / x2s / ys: (sample, channel, pixel) element strides, default
        NCHW-contiguous; a linear layer on rows (n, k) is x1s=(0, 1, k), ys=(0, 1, cout), P=n,
        N=1 with its own `out`."""
        if out is None:
            out = self.empty(N, G * cout_g, P)
        a = self._lib.PwArgs()
        a.x1 = x1.data_ptr()
        a.x1n, a.x1c, a.x1p = x1s or (G * k1 * P, P, 1)
        if x2 is not None:
            a.x2 = x2.data_ptr()
            a.x2n, a.x2c, a.x2p = x2s or (k2 * P, P, 1)
        a.w = w.data_ptr()
        a.bias = bias.data_ptr() if bias is not None else None
        if res is not None:
            a.res = res.data_ptr()
            a.rn, a.rc, a.rp = (G * cout_g * P, P, 1)
        a.y = out.data_ptr()
        a.yn, a.yc, a.yp = ys or (G * cout_g * P, P, 1)
        a.k1, a.k2, a.G, a.cout_g, a.P, a.N, a.relu = k1, k2, G, cout_g, P, N, int(relu)
        self.call("yta_osnet_pointwise", self.ct.byref(a), self.half)
        return out

    def pool(self, x, kind):
        """yta_osnet_pool on x (n, c, h, w): kind 0 the 3x3 stride-2 max pool (padding 1), 1 the
        2x2 average pool, 2 the plane means (n, c)."""
        n, c, h, w = x.shape
        y = (self.empty(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1) if kind == 0 else
             self.empty(n, c, h // 2, w // 2) if kind == 1 else self.empty(n, c))
        self.call("yta_osnet_pool", x.data_ptr(), n, c, h, w, kind, self.half, y.data_ptr())
        return y

    def stem(self, x, w, b, relu=True):
        """The 7x7 stride-2 stem convolution (padding 3) + bias [+ ReLU]: x (n, 3, h, w) ->
        (n, c0, ceil(h / 2), ceil(w / 2)); w (c0, 3, 7, 7) and b float32."""
        n, _, h, wd = x.shape
        c0 = w.shape[0]
        y = self.empty(n, c0, (h - 1) // 2 + 1, (wd - 1) // 2 + 1)
        self.call("yta_osnet_stem" if relu else "yta_osnet_stem_linear", x.data_ptr(), n, h, wd,
                  w.data_ptr(), b.data_ptr(), c0, self.half, y.data_ptr())
        return y


class ReIDBackbone:
    """What the *ReID classes (and the single-block graphs of MLFN and CLIP) share: the
    device / hip / storage type / chunk setup, the chunked call and the dispatch between the HIP
    forward and the same graph on PyTorch's operators."""

    def _setup(self, device, half, hip, chunk=None, double=False):
        """double: float64, the yardstick evaluation of the hip=False graph (CLIP-ReID's tests)."""
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.hip = bool(hip) and self.device.type == "cuda"
        if double and (half or self.hip):
            raise ValueError("double=True is the float64 evaluation of the hip=False graph")
        self.dtype = torch.float64 if double else torch.float16 if half else torch.float32
        if chunk is not None:
            self.chunk = int(chunk)
        self.K = Kernels(torch, self.device, self.dtype) if self.hip else None

    def __call__(self, crops):
        torch = self.torch
        with torch.no_grad():
            n = crops.shape[0]
            if n <= self.chunk:
                return self._forward(crops)
            return torch.cat([self._forward(crops[i:i + self.chunk])
                              for i in range(0, n, self.chunk)])

    def _forward(self, crops):
        return self._forward_hip(crops) if self.hip else self._forward_torch(crops)
