"""LMBN-n feature extractor for the MI355X ReID producer.

Reference: boxmot/appearance/backbones/lmbn/lmbn_n.py (LMBN_n; Herzog et al., "Lightweight
Multi-Branch Network for Person Re-Identification", ICIP 2021), lmbn/bnneck.py (BNNeck, BNNeck3),
lmbn/attention.py (BatchFeatureErase_Top, BatchDropTop) and the OSBlock / Conv1x1 / ConvLayer of
backbones/osnet.py, built by reid_multibackend.py from the weight file name (lmbn_n_duke.pt,
lmbn_n_market.pt, lmbn_n_cuhk03_d.pt) and run in eval mode.  The channel counts are osnet_x1_0's
(64, 256, 384, 512), fixed by the reference's constructor.

What runs (eval mode), with the reference's key prefixes:
  backone           the OSNet stem (backone.0: 7x7 stride-2 conv, BN, ReLU), max pool 3/2/1,
                    backone.2 = OSBlock(64, 256), OSBlock(256, 256), Conv1x1(256, 256) + 2x2
                    average pool, backone.3 = OSBlock(256, 384);
  three branches    global_branch, partial_branch, channel_branch: the same layers with separate
                    weights, each on backone's output: <b>.0.1 = OSBlock(384, 384), <b>.0.2.0 =
                    Conv1x1(384, 384) + 2x2 average pool (<b>.0 is osnet.conv3[1:], and slicing
                    an nn.Sequential keeps the modules' names 1 and 2), <b>.1.0 =
                    OSBlock(384, 512), <b>.1.1 = OSBlock(512, 512), <b>.2 = Conv1x1(512, 512)
                    -> glo, par, cha (N, 512, 16, 8 at 256 x 128 crops);
  feat              batch_drop_block.drop_batch_bottleneck = OSBlock(512, 512) on glo.  In eval
                    mode BatchDropTop is the identity and batch_drop_block returns (feat, feat):
                    both the "global" and the "drop" head read feat, glo is not used again;
  pooling           v0 = mean(feat), v1 = max(feat), v2 = max(par), v3 / v4 = the means of par's
                    upper / lower bin (AdaptiveAvgPool2d((2, 1)): rows [0, ceil(H / 2)) and
                    [floor(H / 2), H), which share the middle row of an odd H), v5 / v6 =
                    mean(cha)[:, :256] / [:, 256:];
  heads             f0 .. f4 = BNNeck3's after_neck: a bias-free 1x1 (512 -> 512) and a BatchNorm1d,
                    folded into one linear layer, no ReLU.  In the order of the output's stack
                    they are reduction_0 (v0), reduction_4 (v1: the drop head), reduction_1 (v2),
                    reduction_2 (v3), reduction_3 (v4): HEAD_REDUCTION.  f5, f6 =
                    reduction_ch_0.bn / reduction_ch_1.bn (BNNeck: a BatchNorm only) of
                    shared(v5) / shared(v6), shared
                    = 1x1 (256 -> 512) + BN + ReLU with the same weights for both halves; the
                    second BatchNorm follows the ReLU and cannot fold into the weight:
                    f = s * relu(W' v + b') + t;
  output            stack([f0 .. f6], dim=2).flatten(1, 2): (N, 3584), feature c * 7 + j.
*.classifier.* keys are ignored.  As in appearance/osnet.py this is an inference graph: every
BatchNorm that directly follows a convolution is folded into it on the host in float64.

The OS blocks, the transitions and the stem are OSNetReID's folding and forward code, applied to
LMBN's key prefixes (LMBNReID subclasses it); the three branches run one after another on the
current stream.  On a GPU the pooling stage is yta_lmbn_pool (feat read once for two statistics,
par once for three) and the seven heads with the interleaving stack are one yta_lmbn_neck launch
(csrc/lmbn.hip).  fused_neck=False keeps the neck as the existing entry points express it: seven
yta_osnet_pointwise launches storing 7 elements apart, plus the channel heads' affine as two
elementwise operations on the strided views; it is the A/B baseline and an independent check.
`hip=False` runs the same folded graph on PyTorch's operators: what a CPU device gets, and the
measurement baseline.

Deliberate deviation from the reference.  In boxmot 10.0.51 load_pretrained_weights handles a
path containing "lmbn" with model.load_state_dict(model_dict), which loads the model's own fresh
dict and never reads the checkpoint, and LMBN_n's constructor downloads ImageNet OSNet weights.
Here the checkpoint's tensors are what runs: keys as listed above ('module.' prefixes dropped by
load_checkpoint); a leading 'model.' on every key is dropped as well, since LightMBN's trainer
keeps the network in an attribute of that name.  No published LMBN file was at hand when this was
written, so the 'model.' handling rests on reading LightMBN's code, not on a loaded file.  A
checkpoint that lacks a non-classifier key raises a ValueError naming the first missing key.
Parity with the reference module is pinned by tests/golden/lmbn_n.npz.
"""
from pathlib import Path

import numpy as np

from ._backbone import CHUNK, bn_affine, f32, fold_bn, to_f64
from .mlfn import _draw
from .osnet import WIDTHS, OSNetReID, _Reduce

VARIANTS = {"lmbn_n": WIDTHS["osnet_x1_0"]}
BRANCHES = ("global_branch", "partial_branch", "channel_branch")
HEADS = 7
FEATURE_DIM = 512 * HEADS
# head j of the output (j < 5) is reduction_{HEAD_REDUCTION[j]}: lmbn_n.py:107-111 and :127-129
HEAD_REDUCTION = (0, 4, 1, 2, 3)
DROP = "batch_drop_block.drop_batch_bottleneck"


def model_name(weights):
    """'lmbn_n' where it occurs in the weight file's name (reid_model_factory.get_model_name tests
    model.name, not the path)."""
    s = Path(str(weights)).name
    for name in VARIANTS:
        if name in s:
            return name
    return None


def _os_block_keys(key, cin, cout):
    """One OSBlock's parameters in module order as mlfn._draw's rows: conv1, conv2a .. conv2d
    (LightConv3x3: a 1x1, a depthwise 3x3, a BatchNorm), gate.fc1 / fc2 (with biases), conv3 and,
    where cin != cout, downsample."""
    mid = cout // 4
    out = [("conv", key + ".conv1.conv", mid, cin, 1, False), ("bn", key + ".conv1.bn", mid)]
    lights = [key + ".conv2a"] + [f"{key}.{br}.{d}" for br, depth in
                                  (("conv2b", 2), ("conv2c", 3), ("conv2d", 4))
                                  for d in range(depth)]
    for k in lights:
        out += [("conv", k + ".conv1", mid, mid, 1, False),
                ("conv", k + ".conv2", mid, 1, 3, False), ("bn", k + ".bn", mid)]
    out += [("conv", key + ".gate.fc1", mid // 16, mid, 1, True),
            ("conv", key + ".gate.fc2", mid, mid // 16, 1, True),
            ("conv", key + ".conv3.conv", cout, mid, 1, False), ("bn", key + ".conv3.bn", cout)]
    if cin != cout:
        out += [("conv", key + ".downsample.conv", cout, cin, 1, False),
                ("bn", key + ".downsample.bn", cout)]
    return out


def _conv_bn(key, cout, cin, k=1):
    return [("conv", key + ".conv", cout, cin, k, False), ("bn", key + ".bn", cout)]


def layout(name="lmbn_n"):
    """The network's parameters without classifiers, in the reference's module order, as
    mlfn._draw's rows: backone, the three branches, reduction_0 .. reduction_4, shared,
    reduction_ch_0, reduction_ch_1, batch_drop_block."""
    c = VARIANTS[name]
    rows = _conv_bn("backone.0", c[0], 3, 7)
    rows += _os_block_keys("backone.2.0", c[0], c[1]) + _os_block_keys("backone.2.1", c[1], c[1])
    rows += _conv_bn("backone.2.2.0", c[1], c[1]) + _os_block_keys("backone.3", c[1], c[2])
    for b in BRANCHES:
        rows += _os_block_keys(b + ".0.1", c[2], c[2]) + _conv_bn(b + ".0.2.0", c[2], c[2])
        rows += _os_block_keys(b + ".1.0", c[2], c[3]) + _os_block_keys(b + ".1.1", c[3], c[3])
        rows += _conv_bn(b + ".2", c[3], c[3])
    for i in range(5):
        rows += [("conv", f"reduction_{i}.reduction", c[3], c[3], 1, False),
                 ("bn", f"reduction_{i}.bn", c[3])]
    rows += [("conv", "shared.0", c[3], c[3] // 2, 1, False), ("bn", "shared.1", c[3]),
             ("bn", "reduction_ch_0.bn", c[3]), ("bn", "reduction_ch_1.bn", c[3])]
    rows += _os_block_keys(DROP, c[3], c[3])
    return rows


def state_keys(name="lmbn_n"):
    """The float keys a checkpoint must hold (classifiers excluded), in layout()'s order."""
    keys = []
    for row in layout(name):
        if row[0] == "conv":
            keys.append(row[1] + ".weight")
            if row[5]:
                keys.append(row[1] + ".bias")
        else:
            keys += [row[1] + s for s in (".weight", ".bias", ".running_mean", ".running_var")]
    return keys


def random_state_dict(seed=0, randomise_bn=False, name="lmbn_n"):
    """A state_dict in the reference's key layout, without *.classifier.*, all float32.

    Drawn from np.random.default_rng(seed) in layout()'s order (the reference's module order:
    backone.0, backone.2.0, backone.2.1, backone.2.2.0, backone.3; per branch <b>.0.1, <b>.0.2.0,
    <b>.1.0, <b>.1.1, <b>.2; reduction_0 .. reduction_4; shared.0, shared.1; reduction_ch_0.bn,
    reduction_ch_1.bn; batch_drop_block.drop_batch_bottleneck; within an OSBlock conv1, conv2a,
    conv2b.0 .. conv2d.3 (conv1, conv2, bn each), gate.fc1, gate.fc2, conv3, downsample), each
    parameter as mlfn._draw documents: convolution weights kaiming normal (fan-out); without
    randomise_bn the gates' biases are zero and every BatchNorm is the identity, with it the
    biases are N(0, 0.1^2) and every BatchNorm has running_mean N(0, 0.1^2), running_var
    U[0.75, 1.25], weight U[0.75, 1.25], bias N(0, 0.1^2), drawn in this order, and every
    depthwise 3x3 weight (c, 1, 3, 3) is then multiplied by sqrt(c) / 2, which makes it
    N(0, 1 / 18).  The constructor's fan-out counts all c output channels for a filter that sums
    nine taps, so a LightConv3x3 shrinks its input about sqrt(c / 2)-fold; training's batch
    statistics undo that, running statistics near 1 do not, and after 30 such layers the maps
    would be the biases alone, flat across the plane and the same for every crop."""
    sd = {}
    _draw(np.random.default_rng(seed), sd, layout(name), randomise_bn)
    if randomise_bn:
        for k, w in sd.items():
            if k.endswith(".conv2.weight") and w.shape[1:] == (1, 3, 3):
                sd[k] = w * np.float32(0.5 * np.sqrt(w.shape[0]))
    return sd


class LMBNReID(OSNetReID):
    """Eval-mode LMBN-n feature extractor: crops (N, 3, H, W) -> (N, 3584) in the crops' dtype
    (float32 or float16), on the crops' device.  H and W are arbitrary multiples of 16 (the
    branches' last planes are H / 16 x W / 16)."""

    def __init__(self, name="lmbn_n", state_dict=None, device="cuda:0", half=False, chunk=CHUNK,
                 hip=True, fused_neck=True, channels_last=None):
        if name not in VARIANTS:
            raise KeyError(f"unknown LMBN variant {name!r}")
        self._setup(device, half, hip, chunk)
        torch = self.torch
        self.name = name
        self.widths, self.kind = VARIANTS[name], "plain"
        self.feature_dim = FEATURE_DIM
        self.fused_neck = bool(fused_neck)
        if channels_last is None:
            channels_last = not self.hip
        if self.hip and channels_last:
            raise ValueError("the HIP block kernels take NCHW planes (channels_last=False)")
        self.fmt = torch.channels_last if channels_last else torch.contiguous_format
        sd = random_state_dict(0, name=name) if state_dict is None else state_dict
        if sd and all(k.startswith("model.") for k in sd):
            sd = {k[len("model."):]: v for k, v in sd.items()}
        for k in state_keys(name):
            if k not in sd:
                raise ValueError(f"{name}: the checkpoint has no {k!r} (the key layout of "
                                 "lmbn_n.py's LMBN_n is expected; see appearance/lmbn.py)")
        self._build(to_f64({k: v for k, v in sd.items() if ".classifier." not in k}))

    # ---- parameter folding
    def _seq(self, sd, *keys):
        """OSNetReID's folded form of a run of modules: an OSBlock per key, a transition (1x1 +
        BN + ReLU, then the 2x2 average pool) where the key names a Conv1x1 (<key>.conv.weight)."""
        out = []
        for key in keys:
            if key + ".conv.weight" in sd:
                t, k = self._pair(*fold_bn(sd, key + ".conv", key + ".bn"))
                out.append(_Reduce(*t, *k))
            else:
                out.append(self._block(sd, key))
        return out

    def _build(self, sd):
        d = self.device
        w, b = fold_bn(sd, "backone.0.conv", "backone.0.bn")
        self.stem = (self._t(w), self._t(b), f32(w, d), f32(b, d))
        self.trunk = self._seq(sd, "backone.2.0", "backone.2.1", "backone.2.2.0", "backone.3")
        # per branch: its blocks and its closing Conv1x1 (no pool) both ways
        self.branches = [(self._seq(sd, b + ".0.1", b + ".0.2.0", b + ".1.0", b + ".1.1"),
                          self._pair(*fold_bn(sd, b + ".2.conv", b + ".2.bn"))) for b in BRANCHES]
        self.drop = self._block(sd, DROP)
        # heads: (weight (C, K), bias, relu, scale, shift) in float64, then both ways
        C = self.widths[3]
        heads = []
        for i in HEAD_REDUCTION:
            w, b = fold_bn(sd, f"reduction_{i}.reduction", f"reduction_{i}.bn")
            heads.append((w.reshape(C, C), b, 0, None, None))
        w, b = fold_bn(sd, "shared.0", "shared.1")
        for i in range(2):
            heads.append((w.reshape(C, C // 2), b, 1, *bn_affine(sd, f"reduction_ch_{i}.bn")))
        self.headsT = [(self._t(w), self._t(b), relu, None if s is None else self._t(s),
                        None if t is None else self._t(t)) for w, b, relu, s, t in heads]
        if self.hip:
            wsh = f32(w.reshape(C, C // 2).t(), d)       # the two channel heads share it
            self.headsH = [(f32(w.t(), d) if j < 5 else wsh, f32(b, d), relu,
                            None if s is None else f32(s, d), None if t is None else f32(t, d))
                           for j, (w, b, relu, s, t) in enumerate(heads)]

    # ---- the folded graph on PyTorch's operators
    def _maps_torch(self, crops):
        """(feat, par, cha): the three maps the pooling stage reads."""
        F = self.torch.nn.functional
        x = crops.to(self.device, self.dtype).contiguous(memory_format=self.fmt)
        x = F.relu(F.conv2d(x, self.stem[0], self.stem[1], stride=2, padding=3))
        x = self._blocks_torch(F.max_pool2d(x, 3, stride=2, padding=1), self.trunk)
        maps = [F.relu(F.conv2d(self._blocks_torch(x, blocks), *last[0]))
                for blocks, last in self.branches]
        return self._os_block(maps[0], self.drop), maps[1], maps[2]

    def _pool_torch(self, feat, par, cha):
        """The seven pooled vectors v0 .. v6 (means in float32, as OSNetReID's global mean)."""
        F = self.torch.nn.functional
        dt, half = self.dtype, self.widths[3] // 2
        bins = F.adaptive_avg_pool2d(par.float(), (2, 1)).to(dt)
        mc = cha.float().mean(dim=(2, 3)).to(dt)
        return [feat.float().mean(dim=(2, 3)).to(dt), feat.amax(dim=(2, 3)), par.amax(dim=(2, 3)),
                bins[:, :, 0, 0], bins[:, :, 1, 0], mc[:, :half], mc[:, half:]]

    def _neck_torch(self, pooled):
        torch = self.torch
        F = torch.nn.functional
        outs = []
        for v, (w, b, relu, s, t) in zip(pooled, self.headsT):
            f = F.linear(v, w, b)
            if relu:
                f = F.relu(f) * s + t
            outs.append(f)
        return torch.stack(outs, dim=2).flatten(1, 2)

    def _forward_torch(self, crops):
        return self._neck_torch(self._pool_torch(*self._maps_torch(crops)))

    # ---- the HIP forward
    def _maps_hip(self, crops):
        K = self.K
        x = crops.to(self.device, self.dtype).contiguous()
        n = x.shape[0]
        x = self._blocks_hip(K.pool(K.stem(x, self.stem[2], self.stem[3]), 0), self.trunk)
        maps = []
        for blocks, last in self.branches:
            y = self._blocks_hip(x, blocks)
            c, h, w = y.shape[1:]
            wk, bk = last[1]
            maps.append(K.pw(y, wk, bk, k1=c, cout_g=wk.shape[2], P=h * w, N=n, relu=True)
                        .view(n, wk.shape[2], h, w))
        return self._os_block_hip(maps[0], self.drop), maps[1], maps[2]

    def _pool_hip(self, feat, par, cha):
        """v0 .. v4 as rows of one (5, N, C) buffer and mean(cha) (N, C): three launches, each map
        read once."""
        K = self.K
        n, c, h, w = feat.shape
        v, mc = K.empty(5, n, c), K.empty(n, c)
        p = [v[j].data_ptr() for j in range(5)]
        K.call("yta_lmbn_pool", feat.data_ptr(), n, c, h, w, K.half, p[1], p[0], None, None)
        K.call("yta_lmbn_pool", par.data_ptr(), n, c, h, w, K.half, p[2], None, p[3], p[4])
        K.call("yta_lmbn_pool", cha.data_ptr(), n, c, h, w, K.half, None, mc.data_ptr(), None, None)
        return v, mc

    def _neck_inputs(self, v, mc):
        """Per head (its pooled rows as a view, row stride, K)."""
        c = v.shape[2]
        return [(v[j], c, c) for j in range(5)] + \
               [(mc[:, i * (c // 2):(i + 1) * (c // 2)], c, c // 2) for i in range(2)]

    def _neck_hip(self, v, mc):
        K, lib = self.K, self.K._lib
        n, c = mc.shape
        y = K.empty(n, HEADS * c)
        ins = self._neck_inputs(v, mc)
        if self.fused_neck:
            heads = (lib.LmbnHead * lib.LMBN_HEADS)()
            for h, (x, stride, k), (w, b, relu, s, t) in zip(heads, ins, self.headsH):
                h.x, h.x_stride, h.K, h.relu = x.data_ptr(), stride, k, relu
                h.w, h.bias = w.data_ptr(), b.data_ptr()
                h.scale = s.data_ptr() if s is not None else None
                h.shift = t.data_ptr() if t is not None else None
            K.call("yta_lmbn_neck", heads, n, c, K.half, y.data_ptr())
            return y
        # the unfused form: a GEMM per head, the samples on the pixel axis, stores 7 apart
        for j, ((x, stride, k), (w, b, relu, s, t)) in enumerate(zip(ins, self.headsH)):
            col = y.view(n, c, HEADS)[:, :, j]
            K.pw(x, w, b, k1=k, cout_g=c, P=n, N=1, relu=relu, x1s=(0, 1, stride),
                 ys=(0, HEADS, HEADS * c), out=col)
            if s is not None:
                col.mul_(s.to(self.dtype)).add_(t.to(self.dtype))
        return y

    def _forward_hip(self, crops):
        return self._neck_hip(*self._pool_hip(*self._maps_hip(crops)))

    def heads(self, feat, par, cha):
        """The pooling stage and the neck alone, on three (N, 512, H, W) maps of any sign (the
        head fixture of tests/golden/lmbn_n.npz) -> (N, 3584)."""
        with self.torch.no_grad():
            maps = [m.to(self.device, self.dtype).contiguous() for m in (feat, par, cha)]
            if self.hip:
                return self._neck_hip(*self._pool_hip(*maps))
            return self._neck_torch(self._pool_torch(*maps))
