"""CPU: the OSNet-IBN and OSNet-AIN graphs (appearance/osnet.py: instance norms, the AIN key
layout, OSBlockINin's norm inside the residual) against the reference's modules in eval mode
(tests/golden/osnet_ain_x0_25.npz, osnet_ibn_x0_25.npz: random weights, BatchNorm statistics and
instance-norm pairs with negative gammas), float32 on PyTorch's CPU operators, at 256 x 128 crops
and at 64 x 32 (8-element planes in stage 4).  Bar: 1e-5 of the feature scale, the plain network's
(test_reid_cpu.py); the reference's own float32 result is within 1.3e-7 of its float64 one."""
import os

import numpy as np
import pytest
import torch

from yolo_tracking_amd.appearance.osnet import (VARIANTS, WIDTHS, OSNetReID, model_name,
                                                random_state_dict)

NAMES = ("osnet_ain_x0_25", "osnet_ibn_x0_25")


def load_golden(name):
    """(state_dict, {features key: (input, features)}): inputs in the generator's draw order."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", name + ".npz"))
    sd = {k[4:]: g[k] for k in g.files if k.startswith("sd__")}
    rng = np.random.default_rng(int(g["input_seed"]))
    cases = {}
    for key, shape in (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32))):
        cases[key] = (rng.standard_normal(shape).astype(np.float32), g[key])
    return sd, cases


@pytest.fixture(scope="module", params=NAMES)
def golden(request):
    return (request.param,) + load_golden(request.param)


@pytest.mark.parametrize("key", ["features", "features_small"])
def test_graph_matches_reference_module(golden, key):
    name, sd, cases = golden
    x, ref = cases[key]
    y = OSNetReID(name, sd, device="cpu")(torch.from_numpy(x)).numpy()
    assert y.shape == ref.shape
    err = np.abs(y - ref).max()
    print(name, key, "max error", err, "scale", np.abs(ref).max())
    assert err <= 1e-5 * np.abs(ref).max()


def test_random_state_dict_has_the_reference_keys(golden):
    name, sd, _ = golden
    rnd = random_state_dict(name)
    assert set(rnd) == set(sd)
    for k, v in sd.items():
        assert rnd[k].shape == v.shape and rnd[k].dtype == np.float32, k
    norms = [k[:-7] for k in rnd if k.endswith(".weight") and (k.endswith(".IN.weight")
                                                                 or k == "conv1.bn.weight")]
    assert len(norms) == (5 if "ain" in name else 3)
    for k in norms:   # identity instance norms, no running statistics
        assert (rnd[k + ".weight"] == 1).all() and (rnd[k + ".bias"] == 0).all()
        assert k + ".running_mean" not in rnd and k + ".running_var" not in rnd


@pytest.mark.parametrize("name", ["osnet_ain_x1_0", "osnet_ibn_x1_0"])
def test_x1_0_variants_run(name):
    y = OSNetReID(name, random_state_dict(name), device="cpu")(torch.zeros(2, 3, 256, 128))
    assert y.shape == (2, 512) and torch.isfinite(y).all()


def test_variant_table_and_names():
    assert len(VARIANTS) == 12
    for name, w in WIDTHS.items():
        assert VARIANTS[name] == (w, "plain")
        assert VARIANTS[name.replace("osnet_", "osnet_ibn_")] == (w, "ibn")
        assert VARIANTS[name.replace("osnet_", "osnet_ain_")] == (w, "ain")
    assert model_name("weights/osnet_ain_x1_0_msmt17.pt") == "osnet_ain_x1_0"
    assert model_name("osnet_ibn_x1_0_msmt17.pt") == "osnet_ibn_x1_0"
    # what resolved before still resolves to the same value
    assert model_name("weights/osnet_x0_25_msmt17.pt") == "osnet_x0_25"
    assert model_name("osnet_x1_0_market1501.pt") == "osnet_x1_0"
    assert model_name("resnet50_msmt17.pt") is None
    for name in ("osnet_x0_5", "osnet_x1_0"):
        y = OSNetReID(name, random_state_dict(name), device="cpu")(torch.zeros(2, 3, 256, 128))
        assert y.shape == (2, 512) and torch.isfinite(y).all()
    with pytest.raises(KeyError):
        OSNetReID("osnet_ain_x2_0", device="cpu")
