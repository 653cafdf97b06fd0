"""Make tests/golden/osnet_ain_x0_25.npz and osnet_ibn_x0_25.npz (container-only): the
reference's OSNet-AIN x0.25 (boxmot/appearance/backbones/osnet_ain.py osnet_ain_x0_25) and its
OSNet with IN=True at the x0.25 widths (backbones/osnet.py; the reference registers this class as
osnet_ibn_x1_0 only, the widths are a constructor argument), loaded from their files (they import
only torch), built with random weights (seeded), randomised BatchNorm statistics and affine pairs
as make_osnet_golden.py does, and instance-norm pairs that exercise the affine step: gamma in
+-[0.75, 1.25] with every fifth entry negative, small beta.  Eval mode; instance norms keep no
running statistics, so they normalise by each plane's own.  Stored: the float32 state_dict
(reference key names, without classifier.*), the input seed and the features of two inputs that
the tests regenerate from the seed, drawn in this order from np.random.default_rng(INPUT_SEED):
4 crops of 256 x 128 ("features"), then 2 crops of 64 x 32 ("features_small": stage 4 runs on
4 x 2 = 8-element planes).  Pretrained weights cannot be fetched here, so parity is pinned on these
random-weight vectors."""
import importlib.util
import os

import numpy as np
import torch

REF = "/root/reference/boxmot/appearance/backbones/"
INPUT_SEED = 20261020
SHAPES = (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32)))


def _load(fname):
    spec = importlib.util.spec_from_file_location("ref_" + fname[:-3], REF + fname)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():   # non-trivial BN statistics so folding is exercised
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.5 + 0.75)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) * 0.5 + 0.75)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            if isinstance(m, torch.nn.InstanceNorm2d):
                w = torch.rand(m.weight.shape, generator=g) * 0.5 + 0.75
                w[::5] *= -1
                m.weight.copy_(w)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            if isinstance(m, torch.nn.Conv2d) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)


def _save(net, name):
    net.eval()
    rng = np.random.default_rng(INPUT_SEED)
    out = {"sd__" + k: v.detach().numpy() for k, v in net.state_dict().items()
           if v.dtype.is_floating_point and not k.startswith("classifier.")}
    for key, shape in SHAPES:
        x = rng.standard_normal(shape).astype(np.float32)
        with torch.no_grad():
            y = net(torch.from_numpy(x)).numpy().astype(np.float32)
            y64 = net.double()(torch.from_numpy(x).double()).numpy()
            net.float()
        out[key] = y
        print(name, key, y.shape, "scale %.3f" % np.abs(y).max(), "non-zero %.2f" % (y != 0).mean(),
              "float32 vs float64 %.2e" % (np.abs(y - y64).max() / np.abs(y64).max()))
    out["input_seed"] = np.array(INPUT_SEED)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".npz")
    np.savez_compressed(path, **out)
    print(name, "params", sum(v.size for k, v in out.items() if k.startswith("sd__")),
          "bytes", os.path.getsize(path))


def main():
    ain = _load("osnet_ain.py")
    torch.manual_seed(11)
    net = ain.osnet_ain_x0_25(num_classes=751, pretrained=False)
    _randomise(net, 12)
    _save(net, "osnet_ain_x0_25")
    ibn = _load("osnet.py")
    torch.manual_seed(13)
    net = ibn.OSNet(751, blocks=[ibn.OSBlock] * 3, layers=[2, 2, 2], channels=[16, 64, 96, 128],
                    IN=True)
    _randomise(net, 14)
    _save(net, "osnet_ibn_x0_25")


if __name__ == "__main__":
    main()
