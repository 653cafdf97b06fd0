"""Make tests/golden/mobilenetv2_x0_25.npz (container-only): the reference's MobileNetV2
(boxmot/appearance/backbones/mobilenetv2.py, loaded from its file: it imports only torch) at
width_mult=0.25 (channels 8, 4, 6, 8, 16, 24, 40, 80; 1280 features), random weights under
torch.manual_seed(21), eval mode.

BatchNorm recipe (generator seed 22): running_mean N(0, 0.1^2), running_var U[0.75, 1.25], gamma
U[1.5, 2.5], beta N(0, 0.3^2).  NOT the recipe of make_osnet_golden.py (gamma in [0.75, 1.25]):
with that one no activation of this network reaches 6, and a build that clamps with ReLU instead
of ReLU6 would pass.  The script counts the ConvBlocks whose output reaches 6 and asserts that the
upper clamp is active in at least half of them for every input, and that the feature maximum stays
below 6 (unsaturated features).  It also prints how far the features move with ReLU in place of
ReLU6.

Stored: the float32 state_dict (sd__ keys, reference names, without classifier.*), the input
seed, the features of three inputs the tests regenerate from the seed, drawn in this order from
np.random.default_rng(INPUT_SEED) as standard_normal float32: "features" (4, 3, 256, 128),
"features_small" (2, 3, 64, 32) (last planes 2 x 1), "features_odd" (2, 3, 70, 38) (planes 35 x 19,
18 x 10, 9 x 5, 5 x 3, 3 x 2: stride 2 on odd sizes); and the (key, shape) lists of the reference's
mobilenetv2_x1_0 and mobilenetv2_x1_4 state_dicts without classifier.* (shapes_x1_0__keys /
shapes_x1_0__dims, shapes_x1_4__keys / shapes_x1_4__dims: the names and the shapes, zero-padded to
four dimensions; one array each, since 530 separate entries would push the file past 1 MiB.  Names
and shapes only, so the real widths are pinned without their weights)."""
import importlib.util
import os

import numpy as np
import torch

REF = "/root/reference/boxmot/appearance/backbones/"
INPUT_SEED = 20261021
SHAPES = (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32)),
          ("features_odd", (2, 3, 70, 38)))


def _load(fname):
    spec = importlib.util.spec_from_file_location("ref_" + fname[:-3], REF + fname)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _randomise(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.5 + 0.75)
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 1.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)


def main():
    ref = _load("mobilenetv2.py")
    torch.manual_seed(21)
    net = ref.MobileNetV2(751, width_mult=0.25, loss="softmax")
    _randomise(net, 22)
    net.eval()
    blocks = [m for m in net.modules() if isinstance(m, ref.ConvBlock)]
    stats = []
    hooks = [b.register_forward_hook(lambda _m, _i, o: stats.append((o == 6).float().mean().item()))
             for b in blocks]
    out = {"sd__" + k: v.detach().numpy() for k, v in net.state_dict().items()
           if v.dtype.is_floating_point and not k.startswith("classifier.")}
    rng = np.random.default_rng(INPUT_SEED)
    relu6 = ref.F.relu6
    for key, shape in SHAPES:
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
        with torch.no_grad():
            del stats[:]
            y = net(x).numpy().astype(np.float32)
            active, worst = sum(s > 0 for s in stats), max(stats)
            y64 = net.double()(x.double()).numpy()
            net.float()
            ref.F.relu6 = ref.F.relu          # what a ReLU-only build would compute
            y_relu = net(x).numpy()
            ref.F.relu6 = relu6
        scale = np.abs(y).max()
        print(key, y.shape, "feature max %.2f" % scale,
              "clamp active in %d of %d ConvBlocks, at most %.0f %% of a layer" %
              (active, len(blocks), 100 * worst),
              "float32 vs float64 %.2e" % (np.abs(y - y64).max() / np.abs(y64).max()),
              "ReLU instead of ReLU6 moves the features by %.1f x scale" %
              (np.abs(y_relu - y).max() / scale))
        assert active >= len(blocks) / 2, "the upper clamp must be active in half the ConvBlocks"
        assert scale < 6, "saturated features"
        out[key] = y
    for h in hooks:
        h.remove()
    out["input_seed"] = np.array(INPUT_SEED)
    for tag, fn in (("x1_0", ref.mobilenetv2_x1_0), ("x1_4", ref.mobilenetv2_x1_4)):
        full = {k: v for k, v in fn(751, "softmax", pretrained=False).state_dict().items()
                if v.dtype.is_floating_point and not k.startswith("classifier.")}
        out[f"shapes_{tag}__keys"] = np.array(list(full))
        out[f"shapes_{tag}__dims"] = np.array([tuple(v.shape) + (0,) * (4 - v.dim())
                                               for v in full.values()], dtype=np.int32)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mobilenetv2_x0_25.npz")
    np.savez_compressed(path, **out)
    print("params", sum(v.size for k, v in out.items() if k.startswith("sd__")),
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
