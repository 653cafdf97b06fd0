"""OSNet feature extractor for the MI355X ReID producer ("OSNet forward").

Reference: boxmot/appearance/backbones/osnet.py (OSNet, OSBlock, LightConv3x3, ChannelGate,
osnet_x1_0 / x0_75 / x0_5 / x0_25; Zhou et al., ICCV 2019), built by
reid_multibackend.py:74-80 and run in eval mode (:238-241), where the network returns the 512-d
fc feature.  This is an inference graph, not a module tree: every BatchNorm is folded into the
convolution / linear layer before it (eval mode: y = gamma (x - mean) / sqrt(var + eps) + beta),
activations stay channels-last (NHWC, MIOpen's fast path on gfx950), and the four branches of
every omni-scale block run batched: their first LightConv 1x1s as one convolution over the
concatenated output channels, the deeper 1x1s as one grouped convolution per depth (groups =
branches still running), every depthwise 3x3 as one grouped convolution, and the shared channel
gate over all four branches at once.  Parameters are taken from a checkpoint in the reference's
key layout (torchreid's names: conv1.conv.weight, conv2.0.conv2b.1.bn.running_var, ...), so the
reference's .pt weight files load unchanged; parity with the reference network is pinned by
tests/golden/osnet_x0_25.npz (the reference module with random weights, eval mode).

OSNet-IBN (osnet.py with IN=True: osnet_ibn_x1_0) and OSNet-AIN (backbones/osnet_ain.py:
osnet_ain_x1_0 .. x0_25) are the same graph plus nn.InstanceNorm2d(affine=True), which in eval
mode still normalises every (crop, channel) plane by that plane's own statistics and so cannot be
folded: after the stem convolution (conv -> IN -> ReLU -> max pool) and at the end of a block,
either around the residual sum (IBN, stage conv2 only: relu(IN(conv3(x2) + identity))) or inside
it (AIN's OSBlockINin: relu(IN(conv3(x2)) + identity), conv3 without BatchNorm).  AIN names its
branches conv2.{t}.layers.{d} and its transitions pool2.0 / pool3.0; parity is pinned by
tests/golden/osnet_ain_x0_25.npz and osnet_ibn_x0_25.npz.
"""
import math
from collections import namedtuple

import numpy as np

from ._backbone import (BN_EPS, CHUNK, ReIDBackbone, f32, fold_bn, kmajor,  # noqa: F401
                        load_checkpoint, to_f64)

WIDTHS = {"osnet_x1_0": (64, 256, 384, 512), "osnet_x0_75": (48, 192, 288, 384),
          "osnet_x0_5": (32, 128, 192, 256), "osnet_x0_25": (16, 64, 96, 128)}
# name -> (widths, kind): plain (osnet.py), ibn (osnet.py IN=True: instance norm after the stem
# convolution and at the end of the two conv2 blocks), ain (osnet_ain.py: the same stem, blocks
# per stage as AIN_BLOCKS, 'in' = OSBlockINin).  The reference registers osnet_ibn_x1_0 only; the
# narrower IBN widths are the same class with other channel counts.
VARIANTS = {name: (w, "plain") for name, w in WIDTHS.items()}
VARIANTS.update({name.replace("osnet_", "osnet_ibn_"): (w, "ibn") for name, w in WIDTHS.items()})
VARIANTS.update({name.replace("osnet_", "osnet_ain_"): (w, "ain") for name, w in WIDTHS.items()})
AIN_BLOCKS = (("in", "in"), ("os", "in"), ("in", "os"))
FEATURE_DIM = 512
IN_EPS = 1e-5   # nn.InstanceNorm2d's default


def model_name(weights):
    """The OSNet variant a weight file name names (reid_model_factory.get_model_name)."""
    s = str(weights)
    for name in sorted(VARIANTS, key=len, reverse=True):
        if name in s:
            return name
    return None


def _block_norms(kind, stage):
    """The instance norm of the two blocks of stage 0..2 (conv2..conv4): None, 'ibn' or 'in'."""
    if kind == "ibn":
        return ("ibn", "ibn") if stage == 0 else (None, None)
    if kind == "ain":
        return tuple("in" if b == "in" else None for b in AIN_BLOCKS[stage])
    return (None, None)


def random_state_dict(name="osnet_x0_25", seed=0):
    """A state_dict in the reference's key layout with freshly initialised weights (kaiming
    normal fan-out for convolutions, N(0, 0.01) for the fc, identity BatchNorms and instance
    norms, the latter without running statistics): what the reference's constructor gives without
    pretrained weights, in the key layout of the variant's class (osnet.py / osnet_ain.py)."""
    rng = np.random.default_rng(seed)
    sd = {}

    def conv(key, cout, cin, k, bias=False):
        std = math.sqrt(2.0 / (cout * k * k))
        sd[key + ".weight"] = rng.normal(0, std, (cout, cin, k, k)).astype(np.float32)
        if bias:
            sd[key + ".bias"] = np.zeros(cout, np.float32)

    def bn(key, c):
        sd[key + ".weight"] = np.ones(c, np.float32)
        sd[key + ".bias"] = np.zeros(c, np.float32)
        sd[key + ".running_mean"] = np.zeros(c, np.float32)
        sd[key + ".running_var"] = np.ones(c, np.float32)

    def inorm(key, c):
        sd[key + ".weight"] = np.ones(c, np.float32)
        sd[key + ".bias"] = np.zeros(c, np.float32)

    def light(key, c):
        conv(key + ".conv1", c, c, 1)
        std = math.sqrt(2.0 / (c * 9))
        sd[key + ".conv2.weight"] = rng.normal(0, std, (c, 1, 3, 3)).astype(np.float32)
        bn(key + ".bn", c)

    def block(key, cin, cout, norm=None):
        """norm: None, 'ibn' (OSBlock(IN=True)) or 'in' (OSBlockINin: conv3 without BatchNorm)."""
        mid = cout // 4
        conv(key + ".conv1.conv", mid, cin, 1)
        bn(key + ".conv1.bn", mid)
        if kind == "ain":
            for t in range(4):
                for d in range(t + 1):
                    light(f"{key}.conv2.{t}.layers.{d}", mid)
        else:
            light(key + ".conv2a", mid)
            for br, depth in (("conv2b", 2), ("conv2c", 3), ("conv2d", 4)):
                for d in range(depth):
                    light(f"{key}.{br}.{d}", mid)
        conv(key + ".gate.fc1", mid // 16, mid, 1, bias=True)
        conv(key + ".gate.fc2", mid, mid // 16, 1, bias=True)
        conv(key + ".conv3.conv", cout, mid, 1)
        if norm != "in":
            bn(key + ".conv3.bn", cout)
        if cin != cout:
            conv(key + ".downsample.conv", cout, cin, 1)
            bn(key + ".downsample.bn", cout)
        if norm:
            inorm(key + ".IN", cout)

    c, kind = VARIANTS[name]
    conv("conv1.conv", c[0], 3, 7)
    if kind == "plain":
        bn("conv1.bn", c[0])
    else:
        inorm("conv1.bn", c[0])
    for stage, (cin, cout, reduce) in enumerate(((c[0], c[1], True), (c[1], c[2], True),
                                                 (c[2], c[3], False))):
        key = f"conv{stage + 2}"
        norms = _block_norms(kind, stage)
        block(key + ".0", cin, cout, norms[0])
        block(key + ".1", cout, cout, norms[1])
        if reduce:
            red = f"pool{stage + 2}.0" if kind == "ain" else key + ".2.0"
            conv(red + ".conv", cout, cout, 1)
            bn(red + ".bn", cout)
    conv("conv5.conv", c[3], c[3], 1)
    bn("conv5.bn", c[3])
    sd["fc.0.weight"] = rng.normal(0, 0.01, (FEATURE_DIM, c[3])).astype(np.float32)
    sd["fc.0.bias"] = np.zeros(FEATURE_DIM, np.float32)
    bn("fc.1", FEATURE_DIM)
    return sd


# A transition between stages (1x1 conv + BatchNorm + ReLU + 2x2 average pool): (w, b) in the
# storage type for PyTorch's operators, (wk, bk) the kernels' float32 operands, wk k-major.
_Reduce = namedtuple("_Reduce", "w b wk bk")
# One omni-scale block.  conv1 / conv3 / ds: (weight, bias) for PyTorch's operators (ds None
# without a downsample, conv3's bias None in an OSBlockINin); gate: fc1 weight, bias, fc2 weight,
# bias (both forwards), hid its hidden width; layers: one _Layer per depth; norm: None, 'ibn' or
# 'in', inorm that instance norm's pair as _norm gives it (None without one); conv1k / conv3k /
# dsk: the kernels' float32 (weight, bias), weights k-major (conv3k spans [x2; x] where the
# downsample shares its GEMM; dsk only where the downsample is a GEMM of its own, else None).
_OSBlock = namedtuple("_OSBlock", "mid cin cout hid norm inorm conv1 layers gate conv3 ds "
                                  "conv1k conv3k dsk")
# Depth d of a block's branches: `nlive` branches still running, their 1x1 weights stacked (pw;
# pwk for the grouped GEMM) and their depthwise 3x3s with the BatchNorm folded (dw, db; dwk, dbk).
_Layer = namedtuple("_Layer", "nlive pw dw db pwk dwk dbk")


class OSNetReID(ReIDBackbone):
    """Eval-mode OSNet feature extractor: crops (N, 3, H, W) -> (N, 512) in the crops' dtype
    (float32 or float16), on the crops' device.

    On a GPU every layer runs in csrc/osnet.hip (NCHW): the stem (7x7 conv), the pools, every
    1x1 convolution and the fc as MFMA GEMMs with bias / residual / ReLU epilogues, the depthwise
    3x3s, the channel gates, the gated branch sums and (osnet_ibn_* / osnet_ain_*) the instance
    norms; PyTorch only allocates the activations.
    `hip=False` runs the same folded graph on PyTorch's kernels (MIOpen), for comparison, and is
    what a CPU device gets."""

    def __init__(self, name="osnet_x0_25", state_dict=None, device="cuda:0", half=False,
                 chunk=CHUNK, channels_last=None, hip=True):
        if name not in VARIANTS:
            raise KeyError(f"unknown OSNet variant {name!r}")
        self._setup(device, half, hip, chunk)
        torch = self.torch
        self.name = name
        self.widths, self.kind = VARIANTS[name]
        if channels_last is None:
            channels_last = not self.hip
        if self.hip and channels_last:
            raise ValueError("the HIP block kernels take NCHW planes (channels_last=False)")
        self.fmt = torch.channels_last if channels_last else torch.contiguous_format
        self._build(to_f64(random_state_dict(name) if state_dict is None else state_dict))

    # ---- parameter folding (float64 on the host, then cast once)
    def _t(self, x):
        return x.to(self.device, self.dtype).contiguous(memory_format=self.fmt) \
            if x.dim() == 4 else x.to(self.device, self.dtype).contiguous()

    def _pair(self, w, b):
        """A folded 1x1 layer both ways: (w, b) for PyTorch's operators, (w k-major, b) float32."""
        return (self._t(w), self._t(b)), (kmajor(w, self.device), f32(b, self.device))

    def _build(self, sd):
        P, d = {}, self.device
        if self.kind == "plain":
            w, b = fold_bn(sd, "conv1.conv", "conv1.bn")
            P["stem"] = (self._t(w), self._t(b))
        else:   # conv -> instance norm -> ReLU: conv1.bn is the norm's affine pair, nothing folds
            w, b = sd["conv1.conv.weight"], self.torch.zeros_like(sd["conv1.bn.bias"])
            P["stem"] = (self._t(w), None)
            P["stem_norm"] = self._norm(sd, "conv1.bn")
        H = {"stem": (f32(w, d), f32(b, d))}      # the HIP kernels' float32 operands
        self.blocks = []
        for stage in (2, 3, 4):
            for i, norm in enumerate(_block_norms(self.kind, stage - 2)):
                self.blocks.append(self._block(sd, f"conv{stage}.{i}", norm))
            red = f"pool{stage}.0" if self.kind == "ain" else f"conv{stage}.2.0"
            if red + ".conv.weight" in sd:
                t, k = self._pair(*fold_bn(sd, red + ".conv", red + ".bn"))
                self.blocks.append(_Reduce(*t, *k))
        P["conv5"], H["conv5"] = self._pair(*fold_bn(sd, "conv5.conv", "conv5.bn"))
        P["fc"], H["fc"] = self._pair(*fold_bn(sd, "fc.0", "fc.1"))   # fc.0.bias folds as well
        self.P = P
        self.H = H

    def _norm(self, sd, key):
        """An instance norm's affine pair: (gamma, beta) for PyTorch's operator in the storage
        type, then as the float32 operands of yta_osnet_instnorm."""
        g, b = sd[key + ".weight"], sd[key + ".bias"]
        return (self._t(g), self._t(b), f32(g, self.device), f32(b, self.device))

    def _block(self, sd, key, norm=None):
        """norm: None (OSBlock), 'ibn' (OSBlock(IN=True): the norm around conv3 + identity) or
        'in' (OSBlockINin: the norm on conv3 alone, which has no BatchNorm, inside the residual)."""
        torch, dev = self.torch, self.device
        w1, b1 = fold_bn(sd, key + ".conv1.conv", key + ".conv1.bn")
        mid = w1.shape[0]
        if self.kind == "ain":
            branches = [[f"{key}.conv2.{t}.layers.{d}" for d in range(t + 1)] for t in range(4)]
        else:
            branches = [[key + ".conv2a"]] + [[f"{key}.{br}.{d}" for d in range(depth)]
                                              for br, depth in (("conv2b", 2), ("conv2c", 3),
                                                                ("conv2d", 4))]
        layers = []   # depth d: the branches still running, 1x1 weights stacked, dw folded
        for d in range(4):
            live = [br[d] for br in branches if len(br) > d]
            pw = torch.cat([sd[k + ".conv1.weight"] for k in live], 0)
            dws, dbs = zip(*[fold_bn(sd, k + ".conv2", k + ".bn") for k in live])
            dw, db = torch.cat(dws, 0), torch.cat(dbs, 0)
            layers.append(_Layer(len(live), self._t(pw), self._t(dw), self._t(db),
                                 kmajor(pw, dev, 1 if d == 0 else len(live)),
                                 f32(dw.reshape(-1), dev), f32(db, dev)))
        g = (self._t(sd[key + ".gate.fc1.weight"].reshape(-1, mid)),
             self._t(sd[key + ".gate.fc1.bias"]),
             self._t(sd[key + ".gate.fc2.weight"].reshape(mid, -1)),
             self._t(sd[key + ".gate.fc2.bias"]))
        if norm == "in":
            w3, b3 = sd[key + ".conv3.conv.weight"], None
        else:
            w3, b3 = fold_bn(sd, key + ".conv3.conv", key + ".conv3.bn")
        ds = None
        cout, cin = w3.shape[0], w1.shape[1]
        w3k, b3k = w3.reshape(cout, mid), b3
        dsk = None
        if key + ".downsample.conv.weight" in sd:
            wd, bd = fold_bn(sd, key + ".downsample.conv", key + ".downsample.bn")
            ds = (self._t(wd), self._t(bd))
            if norm == "in":   # the norm stands between conv3 and the sum: a GEMM of its own
                dsk = (kmajor(wd, dev), f32(bd, dev))
            else:
                # conv3(x2) + downsample(x): one GEMM over the concatenated inputs [x2; x]
                w3k, b3k = torch.cat([w3k, wd.reshape(cout, cin)], 1), b3 + bd
        return _OSBlock(mid, cin, cout, g[0].shape[0], norm,
                        self._norm(sd, key + ".IN") if norm else None,
                        (self._t(w1), self._t(b1)), layers, g,
                        (self._t(w3), self._t(b3) if b3 is not None else None), ds,
                        (kmajor(w1, dev), f32(b1, dev)),
                        (kmajor(w3k, dev), f32(b3k, dev) if b3k is not None else None), dsk)

    # ---- the folded graph on PyTorch's operators
    def _os_block(self, x, blk):
        F = self.torch.nn.functional
        torch = self.torch
        mid = blk.mid
        g1w, g1b, g2w, g2b = blk.gate
        x1 = F.relu(F.conv2d(x, *blk.conv1))
        outs = []                       # branch outputs, finished at depths 1, 2, 3, 4
        y = None
        for d, lay in enumerate(blk.layers):
            inp = x1 if d == 0 else y[:, mid:]          # branches that go one layer deeper
            if d == 0:
                y = F.conv2d(inp, lay.pw)               # all four branches' first 1x1 at once
            else:
                y = F.conv2d(inp, lay.pw, groups=lay.nlive)   # one 1x1 per running branch
            y = F.relu(F.conv2d(y, lay.dw, lay.db, padding=1, groups=lay.dw.shape[0]))
            outs.append(y[:, :mid])                     # the branch ending at this depth
        br = torch.stack(outs, 1)                       # (N, 4, mid, H, W)
        pooled = br.float().mean(dim=(3, 4)).to(br.dtype)          # (N, 4, mid)
        gate = torch.sigmoid(F.linear(F.relu(F.linear(pooled, g1w, g1b)), g2w, g2b))
        x2 = (br * gate[..., None, None]).sum(1)
        x2 = x2.contiguous(memory_format=self.fmt)
        x3 = F.conv2d(x2, *blk.conv3)
        idt = F.conv2d(x, *blk.ds) if blk.ds is not None else x
        if blk.norm == "in":
            x3 = F.instance_norm(x3, weight=blk.inorm[0], bias=blk.inorm[1], eps=IN_EPS)
        out = x3 + idt
        if blk.norm == "ibn":
            out = F.instance_norm(out, weight=blk.inorm[0], bias=blk.inorm[1], eps=IN_EPS)
        return F.relu(out)

    def _blocks_torch(self, x, blocks):
        """A run of omni-scale blocks and transitions (what _build leaves in self.blocks)."""
        F = self.torch.nn.functional
        for blk in blocks:
            if isinstance(blk, _Reduce):
                x = F.avg_pool2d(F.relu(F.conv2d(x, blk.w, blk.b)), 2, stride=2)
            else:
                x = self._os_block(x, blk)
        return x

    def _forward_torch(self, crops):
        F = self.torch.nn.functional
        x = crops.to(self.device, self.dtype).contiguous(memory_format=self.fmt)
        w, b = self.P["stem"]
        x = F.conv2d(x, w, b, stride=2, padding=3)
        if self.kind != "plain":
            g, bt = self.P["stem_norm"][:2]
            x = F.instance_norm(x, weight=g, bias=bt, eps=IN_EPS)
        x = F.max_pool2d(F.relu(x), 3, stride=2, padding=1)
        x = self._blocks_torch(x, self.blocks)
        w, b = self.P["conv5"]
        x = F.relu(F.conv2d(x, w, b))
        v = x.float().mean(dim=(2, 3)).to(self.dtype)
        w, b = self.P["fc"]
        return F.relu(F.linear(v, w, b))

    # ---- the HIP forward (csrc/osnet.hip): every layer a kernel of ours
    def _os_block_hip(self, x, blk):
        """One OSBlock: conv1 (GEMM + bias + ReLU); per depth the branches' 1x1s (one GEMM, grouped
        by branch after depth 0) and the depthwise 3x3 + bias + ReLU, which routes the branch
        ending at that depth into the (N, 4, mid, H, W) stack with its plane sums; the channel gate
        on those sums; the gated branch sum; conv3 and the downsample 1x1 as one GEMM over [x2; x]
        (or + x) with ReLU.  With an instance norm the GEMM leaves the ReLU to yta_osnet_instnorm:
        IBN normalises that sum; an OSBlockINin normalises conv3 alone and adds the identity (x,
        or the downsample as a GEMM of its own) as the norm's residual."""
        K, torch = self.K, self.torch
        mid, cin, cout, norm = blk.mid, blk.cin, blk.cout, blk.norm
        n, _, h, w = x.shape
        hw = h * w
        z = K.pw(x, *blk.conv1k, k1=cin, cout_g=mid, P=hw, N=n, relu=True)
        stack = K.empty(n, 4, mid, h, w)
        psum = K.empty(n, 4, mid, dtype=torch.float32)
        for d, lay in enumerate(blk.layers):
            nlive = lay.nlive
            y = (K.pw(z, lay.pwk, k1=mid, cout_g=4 * mid, P=hw, N=n, relu=False) if d == 0 else
                 K.pw(z, lay.pwk, k1=mid, G=nlive, cout_g=mid, P=hw, N=n, relu=False))
            rest = K.empty(n, (nlive - 1) * mid, h, w) if nlive > 1 else None
            K.call("yta_osnet_dw3x3", y.data_ptr(), nlive * mid * hw, hw, lay.dwk.data_ptr(),
                   lay.dbk.data_ptr(), n, nlive * mid, h, w, K.half,
                   stack.data_ptr() + d * mid * hw * K.es, 4 * mid * hw, mid,
                   rest.data_ptr() if rest is not None else None, (nlive - 1) * mid * hw,
                   psum.data_ptr() + d * mid * 4, 4 * mid)
            z = rest
        gate = K.empty(n, 4, mid)
        K.call("yta_osnet_gate", psum.data_ptr(), n, mid, blk.hid, hw,
               *[t.data_ptr() for t in blk.gate], K.half, gate.data_ptr())
        x2 = K.empty(n, mid, h, w)
        K.call("yta_osnet_gate_sum", stack.data_ptr(), gate.data_ptr(), n, mid, hw, K.half,
               x2.data_ptr())
        w3, b3 = blk.conv3k
        if norm == "in":
            y3 = K.pw(x2, w3, None, k1=mid, cout_g=cout, P=hw, N=n, relu=False)
            idt = (K.pw(x, *blk.dsk, k1=cin, cout_g=cout, P=hw, N=n, relu=False)
                   if blk.ds is not None else x)
            out = self._instnorm(y3, blk.inorm, n, cout, hw, res=idt)
        else:
            if blk.ds is not None:
                out = K.pw(x2, w3, b3, k1=mid, cout_g=cout, P=hw, N=n, relu=not norm, x2=x, k2=cin)
            else:
                out = K.pw(x2, w3, b3, k1=mid, cout_g=cout, P=hw, N=n, relu=not norm, res=x)
            if norm:
                out = self._instnorm(out, blk.inorm, n, cout, hw)
        return out.view(n, cout, h, w)

    def _instnorm(self, x, pair, n, c, p, res=None):
        """relu(instance norm(x) + res) through yta_osnet_instnorm (x, res: n x c x p)."""
        out = self.K.empty(n, c, p)
        self.K.call("yta_osnet_instnorm", x.data_ptr(), res.data_ptr() if res is not None else None,
                    pair[2].data_ptr(), pair[3].data_ptr(), n, c, p, 1, self.K.half,
                    out.data_ptr())
        return out

    def _blocks_hip(self, x, blocks):
        """_blocks_torch in HIP: a transition is its 1x1 GEMM + ReLU and the 2x2 average pool."""
        K = self.K
        n = x.shape[0]
        for blk in blocks:
            if isinstance(blk, _Reduce):
                c, h, w = x.shape[1:]
                cr = blk.wk.shape[2]
                y = K.pw(x, blk.wk, blk.bk, k1=c, cout_g=cr, P=h * w, N=n, relu=True)
                x = K.pool(y.view(n, cr, h, w), 1)
            else:
                x = self._os_block_hip(x, blk)
        return x

    def _forward_hip(self, crops):
        K = self.K
        x = crops.to(self.device, self.dtype).contiguous()
        n = x.shape[0]
        stem = K.stem(x, *self.H["stem"], relu=self.kind == "plain")
        if self.kind == "plain":
            x = K.pool(stem, 0)
        else:   # instance norm + ReLU + max pool in one pass over the stem's planes
            c0, sh, sw = stem.shape[1:]
            pair = self.P["stem_norm"]
            work = (self.torch.empty_like(stem)
                    if sh * sw > K.lib().yta_osnet_instnorm_resident() else None)
            x = K.empty(n, c0, (sh - 1) // 2 + 1, (sw - 1) // 2 + 1)
            K.call("yta_osnet_instnorm_maxpool", stem.data_ptr(), pair[2].data_ptr(),
                   pair[3].data_ptr(), n, c0, sh, sw, K.half,
                   work.data_ptr() if work is not None else None, x.data_ptr())
        x = self._blocks_hip(x, self.blocks)
        w5, b5 = self.H["conv5"]
        c, h, w = x.shape[1:]
        y = K.pw(x, w5, b5, k1=c, cout_g=w5.shape[2], P=h * w, N=n, relu=True)
        v = K.pool(y.view(n, w5.shape[2], h, w), 2)                 # (n, C) means
        wf, bf = self.H["fc"]
        feat = K.empty(n, wf.shape[2])
        # the fc as a GEMM over the crops: one "sample", the crops on the pixel axis
        K.pw(v, wf, bf, k1=c, cout_g=wf.shape[2], P=n, N=1, relu=True, x1s=(0, 1, c),
             ys=(0, 1, wf.shape[2]), out=feat)
        return feat
