"""CPU: the MobileNetV2 graph (appearance/mobilenetv2.py: folded BatchNorms, ReLU6, residuals,
truncated channel counts) against the reference's module in eval mode
(tests/golden/mobilenetv2_x0_25.npz: random weights, BatchNorms with gamma in [1.5, 2.5] so that
the upper clamp of ReLU6 is active in most ConvBlocks), float32 on PyTorch's CPU operators, at
256 x 128 crops, at 64 x 32 (last planes 2 x 1) and at 70 x 38 (stride 2 on odd planes).  Bar: 1e-5
of the feature scale, the OSNet-IN CPU test's; the reference's own float32 result is within 5.3e-7
of its float64 one."""
import os

import numpy as np
import pytest
import torch

from yolo_tracking_amd.appearance import mobilenetv2 as mb
from yolo_tracking_amd.appearance import osnet

SHAPES = (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32)),
          ("features_odd", (2, 3, 70, 38)))


def load_golden():
    """(npz, state_dict, {features key: (input, features)}): inputs in the generator's draw
    order."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "mobilenetv2_x0_25.npz"))
    sd = {k[4:]: g[k] for k in g.files if k.startswith("sd__")}
    rng = np.random.default_rng(int(g["input_seed"]))
    cases = {key: (rng.standard_normal(shape).astype(np.float32), g[key]) for key, shape in SHAPES}
    return g, sd, cases


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.mark.parametrize("key", [k for k, _ in SHAPES])
def test_graph_matches_reference_module(golden, key):
    _, sd, cases = golden
    x, ref = cases[key]
    net = mb.MobileNetV2ReID("mobilenetv2_x1_0", sd, device="cpu", width_mult=0.25,
                             count_clamped=True)
    assert not net.hip and net.feature_dim == 1280 and net.name == "mobilenetv2_x1_0"
    y = net(torch.from_numpy(x)).numpy()
    assert y.shape == ref.shape == (x.shape[0], 1280)
    err, scale = np.abs(y - ref).max(), np.abs(ref).max()
    print(key, "max error", err, "scale", scale, "ConvBlocks at 6:", net.clamped, "of 36")
    assert err <= 1e-5 * scale
    assert net.clamped >= 18 and scale < 6     # the fixture exercises the upper clamp


@pytest.mark.parametrize("name", ["mobilenetv2_x1_0", "mobilenetv2_x1_4"])
def test_random_state_dict_has_the_reference_keys_and_shapes(golden, name):
    g, _, _ = golden
    prefix = "shapes_" + name[-4:] + "__"
    recorded = {str(k): tuple(int(v) for v in d if v) for k, d in zip(g[prefix + "keys"],
                                                                      g[prefix + "dims"])}
    assert len(recorded) > 250 and not any(k.startswith("classifier.") for k in recorded)
    rnd = mb.random_state_dict(name, seed=1)
    assert {k: v.shape for k, v in rnd.items()} == recorded
    assert all(v.dtype == np.float32 for v in rnd.values())


def test_widths_truncate():
    c0, blocks, fdim = mb.layout(1.4)
    assert [c0] + sorted({b[3] for b in blocks}) == [44, 22, 33, 44, 89, 134, 224, 448]
    assert fdim == 1792 and mb.layout(1.0)[2] == 1280 and mb.layout(0.25)[2] == 1280
    assert len(blocks) == 17
    assert [(b[1], b[2], b[4]) for b in blocks[:3]] == [(44, 44, 1), (22, 132, 2), (33, 198, 1)]
    assert [b[5] for b in blocks[:3]] == [False, False, True]
    assert mb.VARIANTS == {"mobilenetv2_x1_0": 1.0, "mobilenetv2_x1_4": 1.4}


@pytest.mark.parametrize("name,dim", [("mobilenetv2_x1_0", 1280), ("mobilenetv2_x1_4", 1792)])
def test_full_widths_run(name, dim):
    sd = mb.random_state_dict(name)
    sd["classifier.weight"] = np.zeros((751, dim), np.float32)    # a checkpoint's extra keys
    sd["classifier.bias"] = np.zeros(751, np.float32)
    net = mb.MobileNetV2ReID(name, sd, device="cpu")
    y = net(torch.ones(1, 3, 64, 32))
    assert y.shape == (1, dim) and net.feature_dim == dim and torch.isfinite(y).all()
    with pytest.raises(KeyError):
        mb.MobileNetV2ReID("mobilenetv2_x2_0", device="cpu")


def test_model_names():
    assert mb.model_name("weights/mobilenetv2_x1_4_dukemtmcreid.pt") == "mobilenetv2_x1_4"
    assert mb.model_name("mobilenetv2_x1_0_msmt17.pt") == "mobilenetv2_x1_0"
    assert mb.model_name("resnet50_msmt17.pt") is None
    assert mb.model_name("osnet_x0_25_msmt17.pt") is None
    assert osnet.model_name("osnet_ain_x1_0_msmt17.pt") == "osnet_ain_x1_0"
    assert osnet.model_name("mobilenetv2_x1_0_msmt17.pt") is None
    assert osnet.model_name("resnet50_msmt17.pt") is None


def test_backend_dispatch_errors(tmp_path):
    """The name dispatch runs before any device work: a missing MobileNetV2 file is a
    FileNotFoundError, any other network still NotImplementedError (its text names the rebuilt
    networks)."""
    from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
    with pytest.raises(FileNotFoundError, match="mobilenetv2_x1_0"):
        ReIDDetectMultiBackend(tmp_path / "mobilenetv2_x1_0_msmt17.pt", device=0)
    with pytest.raises(NotImplementedError, match="osnet_ain_x1_0") as e:
        ReIDDetectMultiBackend(tmp_path / "resnet50_msmt17.pt", device=0)
    assert "mobilenetv2_x1_0" in str(e.value) and "mobilenetv2_x1_4" in str(e.value)
    with pytest.raises(FileNotFoundError):
        ReIDDetectMultiBackend(tmp_path / "osnet_x0_25_msmt17.pt", device=0)
