"""MLFN feature extractor for the MI355X ReID producer.

Reference: boxmot/appearance/backbones/mlfn.py (MLFN, MLFNBlock; mlfn; Chang et al., CVPR 2018),
built by reid_multibackend.py from the weight file name and run in eval mode, where the network
returns v = (fc_x(global mean) + fc_s(the 16 blocks' factor selections)) / 2, embed_dim = 1024
values.  As in appearance/osnet.py and appearance/mobilenetv2.py this is an inference graph, not a
module tree: every BatchNorm is folded into the convolution before it (float64 on the host; the
biases of conv1 and of the selection modules' 1x1s fold into the BatchNorm's bias), and parameters
come from a checkpoint in the reference's key layout (conv1.weight, conv1.bias, bn1.*,
feature.3.fm_conv2.weight, feature.3.fsm.1.bias, feature.3.fsm.8.running_var,
feature.3.downsample.0.weight, fc_x.0.weight, fc_s.1.*, ...), so the reference's .pt files load
unchanged; classifier.* keys are ignored.  Parity with the reference module is pinned by
tests/golden/mlfn_small.npz.

On a GPU every layer runs in HIP (csrc/mlfn.hip, and k_stem / k_pool / k_pw of csrc/osnet.hip).
Per MLFNBlock: the input's plane means (yta_osnet_pool kind 2), yta_mlfn_fsm into the block's
slot of the N x 16 G selection buffer, fm_conv1 + ReLU (yta_osnet_pointwise), yta_mlfn_gconv3x3
(grouped 3x3 + ReLU + the selection as a per-(sample, group) scale), then fm_conv3 with both ReLUs
and the identity residual in its epilogue (relu = 3) or, where the block has a downsample,
fm_conv3 + ReLU followed by the downsample's 1x1 with fm_conv3's result as its residual (behind
yta_mlfn_subsample where the stride is 2).  fc_x and fc_s run as GEMMs with the samples on the
pixel axis; yta_mlfn_mean2 averages them.  `hip=False` runs the same folded graph on PyTorch's
operators: what a CPU device gets, and the measurement baseline.
"""
import math

import numpy as np

from ._backbone import CHUNK, ReIDBackbone, f32, fold_bn, kmajor, to_f64

# name -> (groups, channels, embed_dim): mlfn.py MLFN.__init__'s defaults
VARIANTS = {"mlfn": (32, (64, 256, 512, 1024, 2048), 1024)}
BLOCKS = 16


def model_name(weights):
    """The MLFN variant a weight file name names (reid_model_factory.get_model_name)."""
    s = str(weights)
    for name in VARIANTS:
        if name in s:
            return name
    return None


def layout(groups=32, channels=(64, 256, 512, 1024, 2048), embed_dim=1024):
    """The 16 blocks' (cin, cout, stride, fsm_channels) as MLFN.__init__ lists them
    (mlfn.py:125-148).  A block has a downsample where cin != cout or stride == 2 (:55)."""
    c = tuple(channels)
    if len(c) != 5:
        raise ValueError("channels: five counts (the stem and the four stages)")
    blocks = [(c[0], c[1], 1, (128, 64)), (c[1], c[1], 1, (128, 64)), (c[1], c[1], 1, (128, 64)),
              (c[1], c[2], 2, (256, 128))] + [(c[2], c[2], 1, (256, 128))] * 3 + \
             [(c[2], c[3], 2, (512, 128))] + [(c[3], c[3], 1, (512, 128))] * 5 + \
             [(c[3], c[4], 2, (512, 128))] + [(c[4], c[4], 1, (512, 128))] * 2
    assert len(blocks) == BLOCKS
    return blocks


def block_keys(key, cin, cout, stride, fsm_channels, groups):
    """(kind, name, shape arguments) of one MLFNBlock's parameters in module order: ('conv', name,
    cout, cin per group, kernel, bias) and ('bn', name, channels)."""
    mid = cout // 2
    f0, f1 = fsm_channels
    out = [("conv", key + "fm_conv1", mid, cin, 1, False), ("bn", key + "fm_bn1", mid),
           ("conv", key + "fm_conv2", mid, mid // groups, 3, False), ("bn", key + "fm_bn2", mid),
           ("conv", key + "fm_conv3", cout, mid, 1, False), ("bn", key + "fm_bn3", cout),
           ("conv", key + "fsm.1", f0, cin, 1, True), ("bn", key + "fsm.2", f0),
           ("conv", key + "fsm.4", f1, f0, 1, True), ("bn", key + "fsm.5", f1),
           ("conv", key + "fsm.7", groups, f1, 1, True), ("bn", key + "fsm.8", groups)]
    if cin != cout or stride > 1:
        out += [("conv", key + "downsample.0", cout, cin, 1, False),
                ("bn", key + "downsample.1", cout)]
    return out


def _draw(rng, sd, entries, randomise_bn):
    """Fill sd for `entries` (block_keys rows), drawing from rng in the rows' order: a
    convolution's weight N(0, 2 / (cout k k)) (kaiming normal, fan-out), then, only with
    randomise_bn, its bias N(0, 0.1^2) (zeros otherwise, nothing drawn); a BatchNorm, only with
    randomise_bn, running_mean N(0, 0.1^2), running_var U[0.75, 1.25], weight U[0.75, 1.25],
    bias N(0, 0.1^2) in this order (identity otherwise, nothing drawn); the weight of a block's
    last selection BatchNorm (fsm.8) is then multiplied by 0.3."""
    for e in entries:
        if e[0] == "conv":
            _, key, cout, cin_g, k, bias = e
            std = math.sqrt(2.0 / (cout * k * k))
            sd[key + ".weight"] = rng.normal(0, std, (cout, cin_g, k, k)).astype(np.float32)
            if bias:
                sd[key + ".bias"] = (rng.normal(0, 0.1, cout) if randomise_bn
                                     else np.zeros(cout)).astype(np.float32)
        else:
            _, key, c = e
            if randomise_bn:
                sd[key + ".running_mean"] = rng.normal(0, 0.1, c).astype(np.float32)
                sd[key + ".running_var"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
                gamma = rng.uniform(0.75, 1.25, c)
                sd[key + ".weight"] = (gamma * (0.3 if key.endswith("fsm.8") else 1.0)) \
                    .astype(np.float32)
                sd[key + ".bias"] = rng.normal(0, 0.1, c).astype(np.float32)
            else:
                sd[key + ".weight"] = np.ones(c, np.float32)
                sd[key + ".bias"] = np.zeros(c, np.float32)
                sd[key + ".running_mean"] = np.zeros(c, np.float32)
                sd[key + ".running_var"] = np.ones(c, np.float32)


def random_block_state_dict(seed, cin, cout, stride, fsm_channels, groups, randomise_bn=False):
    """One MLFNBlock's state_dict (keys without a prefix), drawn as random_state_dict draws a
    block's."""
    sd = {}
    _draw(np.random.default_rng(seed), sd, block_keys("", cin, cout, stride, fsm_channels, groups),
          randomise_bn)
    return sd


def random_state_dict(seed=0, groups=32, channels=(64, 256, 512, 1024, 2048), embed_dim=1024,
                      randomise_bn=False):
    """A state_dict in the reference's key layout, without classifier.*, all float32.

    Drawn from np.random.default_rng(seed) in module order: conv1, bn1, then per block
    feature.{i}: fm_conv1, fm_bn1, fm_conv2, fm_bn2, fm_conv3, fm_bn3, fsm.1, fsm.2, fsm.4,
    fsm.5, fsm.7, fsm.8 and, where the block has one, downsample.0, downsample.1; then fc_x.0,
    fc_x.1, fc_s.0, fc_s.1.  Per parameter as _draw documents: convolution weights are kaiming
    normal (fan-out) as the reference's constructor initialises them; without randomise_bn the
    biases are zero and the BatchNorms the identity (what mlfn(pretrained=False) gives), with it
    biases are N(0, 0.1^2) and every BatchNorm has running_mean N(0, 0.1^2), running_var
    U[0.75, 1.25], weight U[0.75, 1.25], bias N(0, 0.1^2), the weight of each block's fsm.8
    times 0.3 so that the selection values do not saturate."""
    rng = np.random.default_rng(seed)
    sd = {}
    c = tuple(channels)
    entries = [("conv", "conv1", c[0], 3, 7, True), ("bn", "bn1", c[0])]
    for i, (cin, cout, stride, fsm) in enumerate(layout(groups, c, embed_dim)):
        entries += block_keys(f"feature.{i}.", cin, cout, stride, fsm, groups)
    entries += [("conv", "fc_x.0", embed_dim, c[4], 1, False), ("bn", "fc_x.1", embed_dim),
                ("conv", "fc_s.0", embed_dim, groups * BLOCKS, 1, False),
                ("bn", "fc_s.1", embed_dim)]
    _draw(rng, sd, entries, randomise_bn)
    return sd


def _subsample(K, x, s):
    n, c, h, w = x.shape
    y = K.empty(n, c, (h - 1) // s + 1, (w - 1) // s + 1)
    K.call("yta_mlfn_subsample", x.data_ptr(), n, c, h, w, s, K.half, y.data_ptr())
    return y


def _gconv(K, x, w, b, groups, stride, scale_ptr, scale_stride):
    n, c, h, wd = x.shape
    y = K.empty(n, c, (h - 1) // stride + 1, (wd - 1) // stride + 1)
    K.call("yta_mlfn_gconv3x3", x.data_ptr(), w.data_ptr(), b.data_ptr(), scale_ptr, scale_stride,
           n, c, groups, h, wd, stride, K.half, y.data_ptr())
    return y


def _linear(K, x, w, b, k, cout, n):
    """relu(x w^T + b) on rows x (n, k) as one GEMM, the samples on the pixel axis."""
    return K.pw(x, w, b, k1=k, cout_g=cout, P=n, N=1, relu=1, x1s=(0, 1, k), ys=(0, 1, cout),
                out=K.empty(n, cout))


class MLFNBlockGraph(ReIDBackbone):
    """One eval-mode MLFNBlock (mlfn.py:18-92) with folded BatchNorms from a state_dict whose keys
    start with `prefix`: x (N, cin, H, W) -> (y (N, cout, Ho, Wo), s (N, groups)).  MLFNReID is 16
    of these between the stem and the two projections; the block fixtures run one alone."""

    def __init__(self, state_dict, cin, cout, stride, fsm_channels, groups=32, prefix="",
                 device="cuda:0", half=False, hip=True, _folded=None):
        self._setup(device, half, hip)
        self.cin, self.cout, self.mid, self.stride = cin, cout, cout // 2, stride
        self.f0, self.f1 = fsm_channels
        self.groups = groups
        self.down = cin != cout or stride > 1
        if self.mid % groups:
            raise ValueError(f"groups {groups} does not divide the {self.mid} mid channels")
        sd = to_f64(state_dict, drop=("classifier.",)) if _folded is None else _folded
        p = prefix
        names = [("fm_conv1", "fm_bn1"), ("fm_conv2", "fm_bn2"), ("fm_conv3", "fm_bn3"),
                 ("fsm.1", "fsm.2"), ("fsm.4", "fsm.5"), ("fsm.7", "fsm.8")]
        if self.down:
            names.append(("downsample.0", "downsample.1"))
        folded = [fold_bn(sd, p + c, p + b) for c, b in names]
        shapes = [(self.mid, cin, 1, 1), (self.mid, self.mid // groups, 3, 3),
                  (cout, self.mid, 1, 1), (self.f0, cin, 1, 1), (self.f1, self.f0, 1, 1),
                  (groups, self.f1, 1, 1), (cout, cin, 1, 1)]
        for (c, _), (w, _), shape in zip(names, folded, shapes):
            if tuple(w.shape) != shape:
                raise ValueError(f"{p + c}.weight is {tuple(w.shape)}, expected {shape}")
        # the torch graph's parameters (storage type) and the kernels' (float32; 1x1s k-major)
        d = self.device
        self.T = [(w.to(d, self.dtype).contiguous(), b.to(d, self.dtype).contiguous())
                  for w, b in folded]
        self.H = None
        if self.hip:
            self.H = [(f32(w.reshape(self.mid, -1), d) if i == 1 else kmajor(w, d), f32(b, d))
                      for i, (w, b) in enumerate(folded)]

    def forward_torch(self, x):
        F = self.torch.nn.functional
        T = self.T
        s = x.float().mean(dim=(2, 3), keepdim=True).to(self.dtype)
        s = F.relu(F.conv2d(s, *T[3]))
        s = F.relu(F.conv2d(s, *T[4]))
        s = self.torch.sigmoid(F.conv2d(s, *T[5]))
        m = F.relu(F.conv2d(x, *T[0]))
        m = F.relu(F.conv2d(m, *T[1], stride=self.stride, padding=1, groups=self.groups))
        # channel c takes s[c // n] (mlfn.py:78-81)
        m = m * s.repeat_interleave(self.mid // self.groups, dim=1)
        m = F.relu(F.conv2d(m, *T[2]))
        r = F.conv2d(x, *T[6], stride=self.stride) if self.down else x
        return F.relu(r + m), s.flatten(1)

    def forward_hip(self, x, sel, sel_t, slot):
        """x contiguous (N, cin, H, W); the selection goes to columns slot G .. slot G + G - 1 of
        sel (float32, N x slots G) and, when given, of sel_t (the storage type)."""
        K, H, G = self.K, self.H, self.groups
        n, _, h, w = x.shape
        row = sel.shape[1]
        sel_ptr = sel.data_ptr() + 4 * slot * G
        selt_ptr = None if sel_t is None else sel_t.data_ptr() + sel_t.element_size() * slot * G
        pooled = K.pool(x, 2)
        K.call("yta_mlfn_fsm", pooled.data_ptr(), n, self.cin, self.f0, self.f1, G,
               *[t.data_ptr() for t in (*H[3], *H[4], *H[5])], K.half, sel_ptr, row, selt_ptr, row)
        m = K.pw(x, *H[0], k1=self.cin, cout_g=self.mid, P=h * w, N=n, relu=1) \
            .view(n, self.mid, h, w)
        m = _gconv(K, m, *H[1], G, self.stride, sel_ptr, row)
        ho, wo = m.shape[2:]
        if self.down:
            m = K.pw(m, *H[2], k1=self.mid, cout_g=self.cout, P=ho * wo, N=n, relu=1)
            xs = _subsample(K, x, self.stride) if self.stride > 1 else x
            y = K.pw(xs, *H[6], k1=self.cin, cout_g=self.cout, P=ho * wo, N=n, relu=1, res=m)
        else:
            y = K.pw(m, *H[2], k1=self.mid, cout_g=self.cout, P=ho * wo, N=n, relu=3, res=x)
        return y.view(n, self.cout, ho, wo)

    def __call__(self, x):
        torch = self.torch
        with torch.no_grad():
            x = x.to(self.device, self.dtype).contiguous()
            if not self.hip:
                return self.forward_torch(x)
            sel = torch.empty((x.shape[0], self.groups), dtype=torch.float32, device=self.device)
            y = self.forward_hip(x, sel, None, 0)
            return y, sel.to(self.dtype)


class MLFNReID(ReIDBackbone):
    """Eval-mode MLFN feature extractor: crops (N, 3, H, W) -> (N, embed_dim) in the crops' dtype
    (float32 or float16), on the crops' device.  groups / channels / embed_dim override the sizes
    the name stands for (the golden network is groups 4, channels 16 .. 256, 64 features)."""

    def __init__(self, name="mlfn", state_dict=None, device="cuda:0", half=False, chunk=CHUNK,
                 hip=True, groups=None, channels=None, embed_dim=None):
        if name not in VARIANTS:
            raise KeyError(f"unknown MLFN variant {name!r}")
        g0, c0, e0 = VARIANTS[name]
        self.name = name
        self.groups = g0 if groups is None else int(groups)
        self.channels = tuple(c0 if channels is None else channels)
        self.feature_dim = self.embed_dim = e0 if embed_dim is None else int(embed_dim)
        self.layout = layout(self.groups, self.channels, self.embed_dim)
        if self.channels[0] % 16:
            raise ValueError(f"channels[0] = {self.channels[0]}: the stem kernel takes a multiple "
                             "of 16 output channels")
        self._setup(device, half, hip, chunk)
        sd = random_state_dict(0, self.groups, self.channels, self.embed_dim) \
            if state_dict is None else state_dict
        self._build(to_f64(sd, drop=("classifier.",)))

    def _build(self, sd):
        c, d = self.channels, self.device
        ws, bs = fold_bn(sd, "conv1", "bn1")
        wx, bx = fold_bn(sd, "fc_x.0", "fc_x.1")
        wsel, bsel = fold_bn(sd, "fc_s.0", "fc_s.1")
        want = ((c[0], 3, 7, 7), (self.embed_dim, c[4], 1, 1),
                (self.embed_dim, self.groups * BLOCKS, 1, 1))
        got = tuple(tuple(w.shape) for w in (ws, wx, wsel))
        if got != want:
            raise ValueError(f"{self.name}: the state_dict's conv1 / fc_x.0 / fc_s.0 weights are "
                             f"{got}, expected {want}")
        self.T = [(w.to(d, self.dtype).contiguous(), b.to(d, self.dtype).contiguous())
                  for w, b in ((ws, bs), (wx, bx), (wsel, bsel))]
        if self.hip:
            self.H = [(f32(ws, d), f32(bs, d)), (kmajor(wx, d), f32(bx, d)),
                      (kmajor(wsel, d), f32(bsel, d))]
        self.blocks = [MLFNBlockGraph(None, cin, cout, stride, fsm, self.groups,
                                      prefix=f"feature.{i}.", device=d,
                                      half=self.dtype == self.torch.float16, hip=self.hip,
                                      _folded=sd)
                       for i, (cin, cout, stride, fsm) in enumerate(self.layout)]

    def _forward_hip(self, crops):
        torch, K = self.torch, self.K
        x = crops.to(self.device, self.dtype).contiguous()
        n, G = x.shape[0], self.groups
        x = K.pool(K.stem(x, *self.H[0]), 0)
        sel = K.empty(n, BLOCKS * G, dtype=torch.float32)
        sel_t = K.empty(n, BLOCKS * G) if K.half else None
        for i, blk in enumerate(self.blocks):
            x = blk.forward_hip(x, sel, sel_t, i)
        pooled = K.pool(x, 2)
        fx = _linear(K, pooled, *self.H[1], self.channels[4], self.embed_dim, n)
        fs = _linear(K, sel_t if K.half else sel, *self.H[2], BLOCKS * G, self.embed_dim, n)
        v = K.empty(n, self.embed_dim)
        K.call("yta_mlfn_mean2", fx.data_ptr(), fs.data_ptr(), v.numel(), K.half, v.data_ptr())
        return v

    def _forward_torch(self, crops):
        torch = self.torch
        F = torch.nn.functional
        x = crops.to(self.device, self.dtype).contiguous()
        x = F.relu(F.conv2d(x, *self.T[0], stride=2, padding=3))
        x = F.max_pool2d(x, 3, 2, 1)
        sel = []
        for blk in self.blocks:
            x, s = blk.forward_torch(x)
            sel.append(s)
        x = x.float().mean(dim=(2, 3), keepdim=True).to(self.dtype)
        fx = F.relu(F.conv2d(x, *self.T[1]))
        fs = F.relu(F.conv2d(torch.cat(sel, 1)[:, :, None, None], *self.T[2]))
        return ((fx + fs) * 0.5).flatten(1)
