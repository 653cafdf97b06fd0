"""CPU: the LMBN-n graph (appearance/lmbn.py: OSNet x1.0 trunk, three branches, the bottleneck
behind the global branch, seven pooled vectors, seven heads interleaved into 3584 features)
against the reference's module in eval mode (tests/golden/lmbn_n.npz, weights regenerated from the
stored seed), float32 on PyTorch's CPU operators, at 256 x 128 crops, at 64 x 32 (last planes
4 x 2), at 80 x 48 (5 x 3: the two bins overlap) and at 16 x 32 (1 x 2: both bins are row 0), and
the pooling stage and the neck alone on signed maps.  Bar per input: max(1e-5, 4 x the
reference's own float32-versus-float64 deviation stored with it) of the feature scale, the
project's CPU rule; the head fixture at 1e-5."""
import re

import numpy as np
import pytest
import torch

import lmbn_golden
from yolo_tracking_amd.appearance import clip, mlfn, mobilenetv2, osnet
from yolo_tracking_amd.appearance import lmbn as L

KEYS = [k for k, _ in lmbn_golden.SHAPES]
NAMES = ("lmbn_n_duke.pt", "weights/lmbn_n_market.pt", "lmbn_n_cuhk03_d.pt")
_net = {}


def _cpu_net():
    if not _net:
        _net["v"] = L.LMBNReID("lmbn_n", lmbn_golden.load()[1], device="cpu")
    return _net["v"]


def test_checksum_of_the_regenerated_weights():
    g, sd, _, _ = lmbn_golden.load()     # load() asserts the checksum
    assert not any(k.startswith("sd__") and g[k].size > 512 for k in g.files)
    assert sum(k.startswith("sd__") for k in g.files) == 8      # the neck running means only
    assert len(sd) == 1065 and sum(v.size for v in sd.values()) == 6521496
    assert all(float(g[k + "__f64dev"]) <= 1e-5 for k in KEYS)  # the GPU test's 1e-4 presumes it


@pytest.mark.parametrize("key", KEYS)
def test_graph_matches_reference_module(key):
    x, ref, dev = lmbn_golden.load()[2][key]
    net = _cpu_net()
    assert not net.hip and net.feature_dim == 3584 and net.name == "lmbn_n"
    y = net(torch.from_numpy(x)).numpy()
    assert y.dtype == np.float32 and y.shape == ref.shape == (x.shape[0], 3584)
    err, scale = np.abs(y - ref).max(), np.abs(ref).max()
    bar = max(1e-5, 4 * dev)
    print(key, "error / scale", err / scale, "bar", bar, "reference float32 vs float64", dev)
    assert err <= bar * scale


def test_head_fixture():
    """Signed maps of 5 x 3 (overlapping bins, planes that are negative throughout) through the
    pooling stage and the neck alone."""
    head = lmbn_golden.load()[3]
    net = _cpu_net()
    maps = [torch.from_numpy(head[k]) for k in ("feat", "par", "cha")]
    assert (maps[0].amax(dim=(2, 3)) < 0).any() and (maps[1].amax(dim=(2, 3)) < 0).any()
    pooled = net._pool_torch(*maps)
    want = head["pooled"]
    got = torch.stack(pooled[:5] + [torch.cat(pooled[5:], 1)]).numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    y = net.heads(*maps).numpy()
    ref = head["features"]
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print("head fixture error / scale", err)
    assert y.shape == ref.shape == (2, 3584) and err <= 1e-5


def test_random_state_dict_has_the_reference_keys_and_shapes():
    g = lmbn_golden.load()[0]
    recorded = {str(k): tuple(int(v) for v in d if v)
                for k, d in zip(g["shapes__keys"], g["shapes__dims"])}
    assert len(recorded) == 1065 and not any(".classifier." in k for k in recorded)
    for k in ("backone.0.conv.weight", "backone.2.2.0.bn.running_var", "backone.3.conv1.conv.weight",
              "global_branch.0.1.conv2d.3.bn.weight", "partial_branch.0.2.0.conv.weight",
              "channel_branch.1.0.downsample.conv.weight", "channel_branch.2.bn.bias",
              "reduction_4.reduction.weight", "shared.0.weight", "shared.1.running_mean",
              "reduction_ch_1.bn.running_var",
              "batch_drop_block.drop_batch_bottleneck.gate.fc2.bias"):
        assert k in recorded, k
    assert "global_branch.1.1.downsample.conv.weight" not in recorded
    for rb in (False, True):
        rnd = L.random_state_dict(1, randomise_bn=rb)
        assert {k: v.shape for k, v in rnd.items()} == recorded
        assert sorted(rnd) == sorted(L.state_keys())
        assert all(v.dtype == np.float32 for v in rnd.values())
    a, b = L.random_state_dict(2), L.random_state_dict(2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["shared.0.weight"], L.random_state_dict(3)["shared.0.weight"])
    for k in a:     # the identity-BN form: what the constructor gives without pretrained weights
        if k.endswith((".running_mean", ".bias")):
            assert (a[k] == 0).all(), k
        if k.endswith(".running_var") or (k.endswith(".weight") and a[k].ndim == 1):
            assert (a[k] == 1).all(), k
    r = L.random_state_dict(2, randomise_bn=True)
    assert r["shared.1.running_var"].min() >= 0.75 and np.abs(r["shared.1.bias"]).max() > 0


def test_model_names():
    assert L.VARIANTS.keys() == {"lmbn_n"}
    for name in NAMES:
        assert L.model_name(name) == "lmbn_n", name
        for family in (osnet, mobilenetv2, mlfn, clip):
            assert family.model_name(name) is None, (family.__name__, name)
    assert L.model_name("lmbn_n/osnet_x0_25_msmt17.pt") is None
    assert L.model_name("lmbn_n/clip_market1501.pt") is None
    for other in ("osnet_x1_0_msmt17.pt", "mlfn_msmt17.pt", "resnet50_msmt17.pt",
                  "hacnn_market1501.pt"):
        assert L.model_name(other) is None, other


def test_backend_dispatch_errors(tmp_path):
    """The name dispatch runs before any device work."""
    from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
    with pytest.raises(FileNotFoundError, match="lmbn_n"):
        ReIDDetectMultiBackend(tmp_path / "lmbn_n_duke.pt", device=0)
    for name in ("resnet50_msmt17.pt", "hacnn_market1501.pt"):
        with pytest.raises(NotImplementedError, match="lmbn_n") as e:
            ReIDDetectMultiBackend(tmp_path / name, device=0)
        text = str(e.value)
        assert all(n in text for n in ("osnet_x0_25", "osnet_x1_0", "osnet_ibn_x1_0",
                                       "osnet_ain_x1_0", "mobilenetv2_x1_0", "mobilenetv2_x1_4",
                                       "mlfn", "clip"))


def test_checkpoint_forms_load(tmp_path):
    """'module.' prefixes, 'model.' prefixes, a 'state_dict' wrapper and classifier keys: each
    loads to the same network as the bare state_dict."""
    from yolo_tracking_amd.appearance._backbone import load_checkpoint
    sd = {k: torch.from_numpy(v) for k, v in L.random_state_dict(4, randomise_bn=True).items()}
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((1, 3, 32, 16))
                         .astype(np.float32))
    want = L.LMBNReID("lmbn_n", sd, device="cpu")(x)
    extra = {f"reduction_{i}.classifier.weight": torch.zeros(751, 512) for i in range(5)}
    extra.update({f"reduction_ch_{i}.classifier.weight": torch.zeros(751, 512) for i in range(2)})
    full = dict(sd, **extra)
    forms = {"module": {"module." + k: v for k, v in full.items()},
             "model": {"model." + k: v for k, v in full.items()},
             "module.model": {"module.model." + k: v for k, v in full.items()},
             "state_dict": {"state_dict": full, "epoch": 3},
             "classifiers": full}
    for name, ck in forms.items():
        path = tmp_path / f"lmbn_n_{name.replace('.', '_')}.pt"
        torch.save(ck, path)
        y = L.LMBNReID("lmbn_n", load_checkpoint(path), device="cpu")(x)
        assert torch.equal(y, want), name


def test_missing_key_is_named():
    sd = L.random_state_dict(4)
    del sd["shared.0.weight"]
    with pytest.raises(ValueError, match=r"shared\.0\.weight"):
        L.LMBNReID("lmbn_n", sd, device="cpu")
    with pytest.raises(KeyError):
        L.LMBNReID("lmbn_x", device="cpu")


def test_library_exports_the_lmbn_entries():
    from yolo_tracking_amd import _lib
    names = ("yta_lmbn_pool", "yta_lmbn_neck")
    lib = _lib.load_library()
    header = open(_lib.__file__.replace("yolo_tracking_amd/_lib.py",
                                        "include/yolo_tracking_amd.h")).read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None
        assert re.search(r"\bint %s\(" % n, header), n
    import ctypes
    assert ctypes.sizeof(_lib.LmbnHead) == 56 and _lib.LMBN_HEADS == 7
    assert "#define YTA_LMBN_HEADS 7" in header
