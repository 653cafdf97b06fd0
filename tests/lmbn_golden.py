"""tests/golden/lmbn_n.npz for the LMBN tests (made by tests/golden/make_lmbn_golden.py): the
network's weights are regenerated from the stored seed and checked against the stored checksum,
then the eight stored neck running means (sd__<key>) go over the generated ones."""
import os

import numpy as np

from yolo_tracking_amd.appearance import lmbn as L

SHAPES = (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32)),
          ("features_odd", (2, 3, 80, 48)), ("features_row", (1, 3, 16, 32)))
HEAD_SHAPE = (2, 512, 5, 3)
_cache = {}


def checksum(sd):
    s = sum(float(np.sum(sd[k], dtype=np.float64)) for k in sorted(sd))
    q = sum(float(np.sum(np.square(sd[k], dtype=np.float64))) for k in sorted(sd))
    return np.array([s, q], np.float64)


def load():
    """(npz, network state_dict, {key: (input, features, float32-vs-float64 deviation)},
    head fixture {feat, par, cha, pooled, features}), computed once and shared: treat as
    read-only."""
    if _cache:
        return _cache["v"]
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lmbn_n.npz"))
    sd = L.random_state_dict(int(g["net_seed"]), randomise_bn=True)
    got, want = checksum(sd), g["net_checksum"]
    assert np.allclose(got, want, rtol=1e-9, atol=0), (
        f"random_state_dict drifted: the generated weights sum to {got}, the fixture recorded "
        f"{want}; the weight generator (or NumPy's stream) changed, not the network")
    for k in g.files:
        if k.startswith("sd__"):
            assert sd[k[4:]].shape == g[k].shape, k
            sd[k[4:]] = g[k]
    rng = np.random.default_rng(int(g["input_seed"]))
    cases = {key: (rng.standard_normal(shape).astype(np.float32), g[key],
                   float(g[key + "__f64dev"])) for key, shape in SHAPES}
    head = {k: g["head__" + k] for k in ("feat", "par", "cha", "pooled", "features")}
    _cache["v"] = (g, sd, cases, head)
    return _cache["v"]
