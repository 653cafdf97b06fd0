"""MobileNetV2 feature extractor for the MI355X ReID producer.

Reference: boxmot/appearance/backbones/mobilenetv2.py (MobileNetV2, Bottleneck, ConvBlock;
mobilenetv2_x1_0 / mobilenetv2_x1_4; Sandler et al., CVPR 2018), built by reid_multibackend.py
from the weight file name and run in eval mode, where the network returns the globally averaged
conv9 feature map (fc_dims=None: no fc; 1280-d at width 1.0, 1792-d at 1.4).  As in
appearance/osnet.py this is an inference graph, not a module tree: every BatchNorm is folded into
the convolution before it (float64 on the host), and parameters come from a checkpoint in the
reference's key layout (conv1.conv.weight, conv3.0.dwconv2.bn.running_var, conv3.0.conv3.1.weight,
conv9.bn.bias, ...), so the reference's .pt files load unchanged; classifier.* keys are ignored.
Parity with the reference module is pinned by tests/golden/mobilenetv2_x0_25.npz.

On a GPU every layer runs in HIP (csrc/mbv2.hip, and k_pw / k_pool of csrc/osnet.hip): the stem,
per Bottleneck one yta_mbv2_expand_dw launch (1x1 expand + ReLU6 + depthwise 3x3 + ReLU6, the
6x-expanded activation never written to memory) and the linear projection with the residual in
its epilogue, conv9 + ReLU6, the global mean.  `fused=False` runs expand and depthwise as two
launches (yta_osnet_pointwise relu = 2, yta_mbv2_dw3x3) for the A/B measurement and the tests.
`hip=False` runs the same folded graph on PyTorch's operators: what a CPU device gets, and the
measurement baseline.
"""
import math

import numpy as np

from ._backbone import CHUNK, ReIDBackbone, f32, fold_bn, kmajor, to_f64

VARIANTS = {"mobilenetv2_x1_0": 1.0, "mobilenetv2_x1_4": 1.4}
# MobileNetV2.__init__'s _make_layer calls: (expansion t, channels c at width 1, blocks n, stride s)
STAGES = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1),
          (6, 160, 3, 2), (6, 320, 1, 1))


def model_name(weights):
    """The MobileNetV2 variant a weight file name names (reid_model_factory.get_model_name)."""
    s = str(weights)
    for name in VARIANTS:
        if name in s:
            return name
    return None


def feature_dim(width_mult):
    return int(1280 * width_mult) if width_mult > 1 else 1280


def layout(width_mult):
    """(C0, [(key, cin, cmid, cout, stride, residual)], feature_dim): int(c * width_mult), that
    is truncation, as the reference computes its channel counts."""
    cin = c0 = int(32 * width_mult)
    blocks = []
    for stage, (t, c, n, s) in enumerate(STAGES):
        cout = int(c * width_mult)
        for i in range(n):
            stride = s if i == 0 else 1
            blocks.append((f"conv{stage + 2}.{i}", cin, cin * t, cout, stride,
                           stride == 1 and cin == cout))
            cin = cout
    return c0, blocks, feature_dim(width_mult)


def random_state_dict(name="mobilenetv2_x1_0", seed=0, width_mult=None):
    """A state_dict in the reference's key layout with freshly initialised weights (kaiming normal
    fan-out for convolutions, identity BatchNorms): what the reference's constructor gives
    without pretrained weights, minus the classifier."""
    rng = np.random.default_rng(seed)
    sd = {}

    def conv(key, cout, cin_g, k):
        std = math.sqrt(2.0 / (cout * k * k))
        sd[key + ".weight"] = rng.normal(0, std, (cout, cin_g, k, k)).astype(np.float32)

    def bn(key, c):
        sd[key + ".weight"] = np.ones(c, np.float32)
        sd[key + ".bias"] = np.zeros(c, np.float32)
        sd[key + ".running_mean"] = np.zeros(c, np.float32)
        sd[key + ".running_var"] = np.ones(c, np.float32)

    c0, blocks, fdim = layout(VARIANTS[name] if width_mult is None else width_mult)
    conv("conv1.conv", c0, 3, 3)
    bn("conv1.bn", c0)
    for key, cin, cmid, cout, _, _ in blocks:
        conv(key + ".conv1.conv", cmid, cin, 1)
        bn(key + ".conv1.bn", cmid)
        conv(key + ".dwconv2.conv", cmid, 1, 3)
        bn(key + ".dwconv2.bn", cmid)
        conv(key + ".conv3.0", cout, cmid, 1)
        bn(key + ".conv3.1", cout)
    conv("conv9.conv", fdim, blocks[-1][3], 1)
    bn("conv9.bn", fdim)
    return sd


class MobileNetV2ReID(ReIDBackbone):
    """Eval-mode MobileNetV2 feature extractor: crops (N, 3, H, W) -> (N, feature_dim) in the
    crops' dtype (float32 or float16), on the crops' device.  width_mult overrides the width the
    name stands for (the golden network is x0.25).  count_clamped (hip=False only): after a
    forward, .clamped is the number of ConvBlocks in which a value reached 6."""

    def __init__(self, name="mobilenetv2_x1_0", state_dict=None, device="cuda:0", half=False,
                 chunk=CHUNK, hip=True, fused=True, width_mult=None, channels_last=False,
                 count_clamped=False):
        if name not in VARIANTS:
            raise KeyError(f"unknown MobileNetV2 variant {name!r}")
        self._setup(device, half, hip, chunk)
        torch = self.torch
        self.name = name
        self.width_mult = VARIANTS[name] if width_mult is None else width_mult
        self.c0, self.layout, self.feature_dim = layout(self.width_mult)
        self.fused = bool(fused)
        if self.hip and channels_last:
            raise ValueError("the HIP kernels take NCHW planes (channels_last=False)")
        self.fmt = torch.channels_last if channels_last else torch.contiguous_format
        self.count_clamped = bool(count_clamped)
        self.clamped = None
        sd = random_state_dict(name, width_mult=width_mult) if state_dict is None else state_dict
        self._build(to_f64(sd, drop=("classifier.",)))

    # ---- parameter folding (float64 on the host, then cast once)
    def _t(self, x):
        x = x.to(self.device, self.dtype)
        return x.contiguous(memory_format=self.fmt) if x.dim() == 4 and x.shape[1] > 1 \
            else x.contiguous()

    def _build(self, sd):
        d = self.device
        ws, bs = fold_bn(sd, "conv1.conv", "conv1.bn")
        w9, b9 = fold_bn(sd, "conv9.conv", "conv9.bn")
        if ws.shape[0] != self.c0 or w9.shape[0] != self.feature_dim:
            raise ValueError(f"{self.name} (width {self.width_mult}): the state_dict has "
                             f"{ws.shape[0]} stem channels and {w9.shape[0]} features, expected "
                             f"{self.c0} and {self.feature_dim}")
        self.T = {"stem": (self._t(ws), self._t(bs)), "conv9": (self._t(w9), self._t(b9))}
        self.H = {"stem": (f32(ws, d), f32(bs, d)), "conv9": (kmajor(w9, d), f32(b9, d))}
        self.blocks = []
        for key, cin, cmid, cout, stride, res in self.layout:
            w1, b1 = fold_bn(sd, key + ".conv1.conv", key + ".conv1.bn")
            wd, bd = fold_bn(sd, key + ".dwconv2.conv", key + ".dwconv2.bn")
            w3, b3 = fold_bn(sd, key + ".conv3.0", key + ".conv3.1")
            assert w1.shape[:2] == (cmid, cin) and w3.shape[:2] == (cout, cmid), key
            tp = tuple(self._t(v) for v in (w1, b1, wd, bd, w3, b3))
            hp = (kmajor(w1, d), f32(b1, d), f32(wd.reshape(cmid, 9), d), f32(bd, d),
                  kmajor(w3, d), f32(b3, d))
            self.blocks.append((cin, cmid, cout, stride, res, tp, hp))

    # ---- the HIP forward
    def _forward_hip(self, crops):
        K = self.K
        x = crops.to(self.device, self.dtype).contiguous()
        n, _, h, w = x.shape
        ws, bs = self.H["stem"]
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = K.empty(n, self.c0, h, w)
        K.call("yta_mbv2_stem", x.data_ptr(), n, x.shape[2], x.shape[3], ws.data_ptr(),
               bs.data_ptr(), self.c0, K.half, y.data_ptr())
        x = y
        for cin, cmid, cout, s, res, _, (w1, b1, wd, bd, w3, b3) in self.blocks:
            pw1, pb1, pwd, pbd = w1.data_ptr(), b1.data_ptr(), wd.data_ptr(), bd.data_ptr()
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            m = K.empty(n, cmid, ho, wo)
            if self.fused:
                K.call("yta_mbv2_expand_dw", x.data_ptr(), pw1, pb1, pwd, pbd, n, cin, cmid, h, w,
                       s, K.half, m.data_ptr())
            else:
                e = K.pw(x, w1, b1, k1=cin, cout_g=cmid, P=h * w, N=n, relu=2)
                K.call("yta_mbv2_dw3x3", e.data_ptr(), pwd, pbd, n, cmid, h, w, s, K.half,
                       m.data_ptr())
            x = K.pw(m, w3, b3, k1=cmid, cout_g=cout, P=ho * wo, N=n, relu=0,
                     res=x if res else None).view(n, cout, ho, wo)
            h, w = ho, wo
        w9, b9 = self.H["conv9"]
        y = K.pw(x, w9, b9, k1=x.shape[1], cout_g=self.feature_dim, P=h * w, N=n, relu=2)
        return K.pool(y.view(n, self.feature_dim, h, w), 2)

    # ---- the same graph on PyTorch's operators
    def _relu6(self, x):
        x = x.clamp(0, 6)
        if self.count_clamped:
            self.clamped += int((x == 6).any())
        return x

    def _forward_torch(self, crops):
        F = self.torch.nn.functional
        self.clamped = 0 if self.count_clamped else None
        x = crops.to(self.device, self.dtype).contiguous(memory_format=self.fmt)
        w, b = self.T["stem"]
        x = self._relu6(F.conv2d(x, w, b, stride=2, padding=1))
        for _, cmid, _, s, res, (w1, b1, wd, bd, w3, b3), _ in self.blocks:
            m = self._relu6(F.conv2d(x, w1, b1))
            m = self._relu6(F.conv2d(m, wd, bd, stride=s, padding=1, groups=cmid))
            m = F.conv2d(m, w3, b3)
            x = x + m if res else m
        w, b = self.T["conv9"]
        x = self._relu6(F.conv2d(x, w, b))
        return x.float().mean(dim=(2, 3)).to(self.dtype)
