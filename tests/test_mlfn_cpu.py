"""CPU: the MLFN graph (appearance/mlfn.py: folded BatchNorms and convolution biases, grouped 3x3,
factor selection as a per-(sample, group) scale, both ReLUs around the residual, the two
projections) against the reference's module in eval mode (tests/golden/mlfn_small.npz: groups 4,
channels 16 .. 256, 64 features, weights regenerated from the stored seed), float32 on PyTorch's
CPU operators, at 256 x 128 crops, at 64 x 32 (last planes 2 x 1) and at 70 x 38 (stride 2 on odd
planes), and single blocks against the reference's MLFNBlock.  Bar per input: max(1e-5, 4 x the
reference's own float32-versus-float64 deviation stored with it) of the feature scale; 1e-5 is
the project's CPU bar, and the folded graph cannot be asked to beat the reference's own float32
noise."""
import re

import numpy as np
import pytest
import torch

import mlfn_golden
from yolo_tracking_amd.appearance import mlfn as M
from yolo_tracking_amd.appearance import mobilenetv2, osnet

KEYS = [k for k, _ in mlfn_golden.SHAPES]


@pytest.mark.parametrize("key", KEYS)
def test_graph_matches_reference_module(key):
    _, sd, cases, _ = mlfn_golden.load()
    x, ref, dev = cases[key]
    net = M.MLFNReID("mlfn", sd, device="cpu", **mlfn_golden.NET)
    assert not net.hip and net.feature_dim == 64 and net.name == "mlfn"
    y = net(torch.from_numpy(x)).numpy()
    assert y.dtype == np.float32 and y.shape == ref.shape == (x.shape[0], 64)
    err, scale = np.abs(y - ref).max(), np.abs(ref).max()
    bar = max(1e-5, 4 * dev)
    print(key, "error / scale", err / scale, "bar", bar, "reference float32 vs float64", dev)
    assert err <= bar * scale


@pytest.mark.parametrize("i", range(mlfn_golden.N_BLOCKS))
def test_block_matches_reference_block(i):
    cfg, bsd, x, y_ref, s_ref = mlfn_golden.load()[3][i]
    blk = mlfn_golden.block_graph(cfg, bsd, device="cpu")
    assert blk.down == (cfg[0] != cfg[1] or cfg[2] == 2)
    y, s = blk(torch.from_numpy(x))
    y, s = y.numpy(), s.numpy()
    assert y.shape == y_ref.shape and s.shape == s_ref.shape == (x.shape[0], cfg[5])
    ey, es = np.abs(y - y_ref).max() / np.abs(y_ref).max(), np.abs(s - s_ref).max() / s_ref.max()
    print("block", cfg, "error / scale: y", ey, "s", es)
    assert ey <= 1e-5 and es <= 1e-5
    assert (y_ref == 0).any() and s_ref.max() - s_ref.min() > 0.1


def test_fixture_is_small_and_has_no_network_weights():
    g = mlfn_golden.load()[0]
    assert not any(k.startswith("sd__") for k in g.files)
    assert all(float(g[k + "__f64dev"]) <= 1e-5 for k in KEYS)   # the GPU test's 1e-4 presumes it


def test_random_state_dict_has_the_reference_keys_and_shapes():
    g = mlfn_golden.load()[0]
    recorded = {str(k): tuple(int(v) for v in d if v)
                for k, d in zip(g["shapes__keys"], g["shapes__dims"])}
    assert len(recorded) > 500 and not any(k.startswith("classifier.") for k in recorded)
    for k in ("conv1.bias", "feature.3.fm_conv2.weight", "feature.3.fsm.1.bias",
              "feature.3.fsm.8.running_var", "feature.3.downsample.0.weight", "fc_x.0.weight",
              "fc_s.1.running_mean"):
        assert k in recorded, k
    assert "feature.1.downsample.0.weight" not in recorded
    for rb in (False, True):
        rnd = M.random_state_dict(1, randomise_bn=rb)
        assert {k: v.shape for k, v in rnd.items()} == recorded
        assert all(v.dtype == np.float32 for v in rnd.values())
    a, b = M.random_state_dict(2), M.random_state_dict(2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["fc_x.0.weight"], M.random_state_dict(3)["fc_x.0.weight"])
    assert (a["bn1.weight"] == 1).all() and (a["conv1.bias"] == 0).all()
    r = M.random_state_dict(2, randomise_bn=True)
    assert r["feature.0.fsm.8.weight"].max() < 0.4 < r["feature.0.fsm.5.weight"].min()


def test_layout_full_size():
    blocks = M.layout()
    assert len(blocks) == 16 and M.VARIANTS == {"mlfn": (32, (64, 256, 512, 1024, 2048), 1024)}
    assert [i for i, b in enumerate(blocks) if b[2] == 2] == [3, 7, 13]
    assert blocks[0] == (64, 256, 1, (128, 64)) and blocks[3] == (256, 512, 2, (256, 128))
    assert blocks[7] == (512, 1024, 2, (512, 128)) and blocks[15] == (2048, 2048, 1, (512, 128))
    sd = M.random_state_dict(0)
    for i, (cin, cout, stride, _) in enumerate(blocks):
        assert (f"feature.{i}.downsample.0.weight" in sd) == (cin != cout or stride == 2), i
    assert [i for i in range(16) if f"feature.{i}.downsample.0.weight" in sd] == [0, 3, 7, 13]


def test_full_size_runs():
    sd = M.random_state_dict(0)
    sd["classifier.weight"] = np.zeros((751, 1024), np.float32)    # a checkpoint's extra keys
    sd["classifier.bias"] = np.zeros(751, np.float32)
    net = M.MLFNReID("mlfn", sd, device="cpu")
    y = net(torch.ones(1, 3, 64, 32))
    assert y.shape == (1, 1024) and net.feature_dim == 1024 and torch.isfinite(y).all()
    with pytest.raises(KeyError):
        M.MLFNReID("mlfn_x2", device="cpu")
    with pytest.raises(ValueError, match="multiple of 16"):
        M.MLFNReID("mlfn", device="cpu", groups=2, channels=(8, 16, 32, 64, 128), embed_dim=8)


def test_model_names():
    assert M.model_name("mlfn_msmt17.pt") == "mlfn"
    assert M.model_name("weights/mlfn_dukemtmcreid.pt") == "mlfn"
    for other in ("osnet_x0_25_msmt17.pt", "osnet_ain_x1_0_msmt17.pt",
                  "mobilenetv2_x1_4_dukemtmcreid.pt", "resnet50_msmt17.pt"):
        assert M.model_name(other) is None, other
    for name in ("mlfn_msmt17.pt", "mlfn_market1501.pt", "mlfn_dukemtmcreid.pt"):
        assert osnet.model_name(name) is None and mobilenetv2.model_name(name) is None


def test_backend_dispatch_errors(tmp_path):
    """The name dispatch runs before any device work: a missing MLFN file is a
    FileNotFoundError, ResNet still NotImplementedError with every rebuilt network named."""
    from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
    with pytest.raises(FileNotFoundError, match="mlfn"):
        ReIDDetectMultiBackend(tmp_path / "mlfn_market1501.pt", device=0)
    with pytest.raises(NotImplementedError, match="osnet_ain_x1_0") as e:
        ReIDDetectMultiBackend(tmp_path / "resnet50_msmt17.pt", device=0)
    text = str(e.value)
    assert all(n in text for n in ("mobilenetv2_x1_0", "mobilenetv2_x1_4", "mlfn"))


def test_library_exports_the_mlfn_entries():
    from yolo_tracking_amd import _lib
    names = ("yta_mlfn_gconv3x3", "yta_mlfn_fsm", "yta_mlfn_subsample", "yta_mlfn_mean2")
    lib = _lib.load_library()
    header = open(_lib.__file__.replace("yolo_tracking_amd/_lib.py",
                                        "include/yolo_tracking_amd.h")).read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None
        assert re.search(r"\bint %s\(" % n, header), n
