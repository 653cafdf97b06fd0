"""tests/golden/clip_small.npz for the CLIP-ReID tests (made by tests/golden/make_clip_golden.py):
the networks' weights and inputs are regenerated from the stored seeds, the weights checked
against the stored checksum."""
import os

import numpy as np

from yolo_tracking_amd.appearance import clip as C

# key -> (width, (grid rows, grid columns), output_dim, crops)
NETS = {"a": (128, (16, 8), 32, 4), "b": (64, (3, 5), 16, 3)}
_cache = {}


def checksum(sd):
    s = sum(float(np.sum(sd[k], dtype=np.float64)) for k in sorted(sd))
    q = sum(float(np.sum(np.square(sd[k], dtype=np.float64))) for k in sorted(sd))
    return np.array([s, q], np.float64)


def load():
    """(npz, {key: (state_dict, input, features, float32-vs-float64 deviation)}, (block
    state_dict, x, y)), computed once and shared: treat as read-only."""
    if _cache:
        return _cache["v"]
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "clip_small.npz"))
    cases = {}
    for key, (width, (gh, gw), od, crops) in NETS.items():
        sd = C.random_state_dict(int(g[key + "__seed"]), width, gh * gw, od)
        got, want = checksum(sd), g[key + "__checksum"]
        assert np.allclose(got, want, rtol=1e-9, atol=0), (
            f"random_state_dict drifted: net {key}'s generated weights sum to {got}, the fixture "
            f"recorded {want}; the weight generator (or NumPy's stream) changed, not the network")
        x = np.random.default_rng(int(g[key + "__input_seed"])) \
            .standard_normal((crops, 3, 16 * gh, 16 * gw)).astype(np.float32)
        cases[key] = (sd, x, g[key], float(g[key + "__f64dev"]))
    pre = "blk__sd__"
    block = ({k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}, g["blk__x"], g["blk__y"])
    _cache["v"] = (g, cases, block)
    return _cache["v"]
