"""tests/golden/mlfn_small.npz for the MLFN tests (made by tests/golden/make_mlfn_golden.py): the
network's weights are regenerated from the stored seed and checked against the stored checksum."""
import os

import numpy as np

from yolo_tracking_amd.appearance import mlfn as M

NET = dict(groups=4, channels=(16, 32, 64, 128, 256), embed_dim=64)
SHAPES = (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32)),
          ("features_odd", (2, 3, 70, 38)))
N_BLOCKS = 3
_cache = {}


def checksum(sd):
    s = sum(float(np.sum(sd[k], dtype=np.float64)) for k in sorted(sd))
    q = sum(float(np.sum(np.square(sd[k], dtype=np.float64))) for k in sorted(sd))
    return np.array([s, q], np.float64)


def load():
    """(npz, network state_dict, {key: (input, features, float32-vs-float64 deviation)},
    [(cfg, block state_dict, x, y, s)]), computed once and shared: treat as read-only."""
    if _cache:
        return _cache["v"]
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "mlfn_small.npz"))
    sd = M.random_state_dict(int(g["net_seed"]), randomise_bn=True, **NET)
    got, want = checksum(sd), g["net_checksum"]
    assert np.allclose(got, want, rtol=1e-9, atol=0), (
        f"random_state_dict drifted: the generated weights sum to {got}, the fixture recorded "
        f"{want}; the weight generator (or NumPy's stream) changed, not the network")
    rng = np.random.default_rng(int(g["input_seed"]))
    cases = {key: (rng.standard_normal(shape).astype(np.float32), g[key],
                   float(g[key + "__f64dev"])) for key, shape in SHAPES}
    blocks = []
    for i in range(N_BLOCKS):
        pre = f"blk{i}__sd__"
        cfg = [int(v) for v in g[f"blk{i}__cfg"]]
        blocks.append((cfg, {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)},
                       g[f"blk{i}__x"], g[f"blk{i}__y"], g[f"blk{i}__s"]))
    _cache["v"] = (g, sd, cases, blocks)
    return _cache["v"]


def block_graph(cfg, bsd, **kw):
    cin, cout, stride, f0, f1, groups = cfg
    return M.MLFNBlockGraph(bsd, cin, cout, stride, (f0, f1), groups, **kw)
