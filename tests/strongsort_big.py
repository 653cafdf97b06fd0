"""Inputs that take StrongSORT's kernels past one block, one tile and one trip of their loops
(plain NumPy, no device): solver matrices whose ties decide the answer, gallery products that cross
every tile edge, and one synthetic stream with several hundred objects.

The expected values are computed by the callers from tests/strongsort_oracle.py, from SciPy or in
float64; nothing here touches the device.  The one expensive piece, the restatement's run over
the big stream, is computed once per process (big_run) and shared by the test modules.
"""
import functools

import numpy as np

import strongsort_oracle as so

TOP = 0.2 + 1e-5                    # min_cost_matching's clamp value at max_dist = 0.2


# ------------------------------------------------------------------------------ solver matrices
def _sparse(nr, nc, seed, k, quant, hopeless, cols):
    rng = np.random.default_rng(seed)
    c = np.full((nr, nc), TOP)
    cols = np.asarray(cols)
    for i in range(nr):
        if hopeless(i):
            continue
        at = cols[rng.choice(len(cols), k, replace=False)]
        v = rng.random(k) * 0.2
        if quant:
            v = np.floor(v / (0.2 / quant)) * (0.2 / quant)
        c[i, at] = v
    return c


def sparse_clamped(nr, nc, seed, k, quant=0):
    """A clamped cost matrix in which the choice among equal costs decides most of the answer:
    every entry is the clamp value except k per row (columns drawn without replacement, values
    rng.random() * 0.2, with `quant` floored to multiples of 0.2 / quant, which makes exact ties
    among the finite costs too); every third row keeps no finite entry at all (a hopeless row)."""
    return _sparse(nr, nc, seed, k, quant, lambda i: i % 3 == 0, np.arange(nc))


def last_columns(nr, nc, seed, k=3, width=88):
    """sparse_clamped whose unclamped entries sit only in the last `width` columns: far more rows
    compete for them than there are, the rest is decided among clamped entries."""
    return _sparse(nr, nc, seed, k, 0, lambda i: i % 3 == 0, np.arange(nc - width, nc))


def first_rows_hopeless(nr, nc, seed, k=3, n=200):
    """sparse_clamped whose hopeless rows are the first n rows instead of every third."""
    return _sparse(nr, nc, seed, k, 0, lambda i: i < n, np.arange(nc))


def clamped_pairs(c, rows, cols, top=TOP):
    """Columns of the assigned-but-clamped pairs in row order, and their share of the pairs."""
    at = c[rows, cols] >= top
    return np.asarray(cols)[at], at.mean()


def is_decisive(c, rows, cols):
    """At least 10 % of the assigned pairs are clamped, and their columns in row order are
    neither ascending nor descending: the tie-breaking rule, not the optimum, placed them."""
    q, share = clamped_pairs(c, rows, cols)
    d = np.diff(q)
    return bool(share >= 0.1 and len(q) > 2 and (d > 0).any() and (d < 0).any())


# ------------------------------------------------------------------------------ gallery product
GALLERY_SHAPES = [(4, 65, 512, 161), (3, 33, 24, 129), (3, 32, 16, 128), (2, 100, 100, 300),
                  (2, 64, 17, 33), (2, 31, 16, 127)]          # (T, B, D, M)


def gallery_case(T, B, D, M):
    """-> (gallery (T, B, D), lens (T,), feats (M, D), poisoned [(t, j)]).  Track lengths B, B - 1,
    B // 2, 1.  Every seventh detection is a near match of one gallery row, taken from all over
    the gallery, so the minima come from different gallery tiles and detection tiles, the partial
    last ones included.  The rows past a track's length are exact copies of a detection's feature
    (cost 0 if they were read); `poisoned` lists those (track, detection) pairs."""
    rng = np.random.default_rng(1000 * B + D + M)
    gal = rng.standard_normal((T, B, D)).astype(np.float32)
    feats = (rng.standard_normal((M, D)) * rng.uniform(0.5, 3, (M, 1))).astype(np.float32)
    lens = np.array([B, B - 1, max(1, B // 2), 1][:T], np.int32)
    for j in range(0, M, 7):
        feats[j] = gal[(j // 7) % T, (5 * j) % B] * np.float32(1.3) + np.float32(0.02) * feats[j]
    plain = [j for j in range(M) if j % 7]                 # never a planted detection
    poisoned = []
    for t in range(T):
        for r in range(lens[t], B):
            j = plain[(11 * r + 3 * t) % len(plain)]
            gal[t, r] = feats[j]
            poisoned.append((t, j))
    return gal, lens, feats, poisoned


def nn_cosine_min_f64(gal, lens, feats):
    """min over a track's rows of 1 - <g / |g|, f / |f|>, everything in float64."""
    f = feats.astype(np.float64)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    out = np.empty((len(gal), len(f)))
    for t in range(len(gal)):
        g = gal[t, :lens[t]].astype(np.float64)
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        out[t] = (1.0 - g @ f.T).min(axis=0)
    return out


# ---------------------------------------------------------------------------------- big stream
def big_stream(seed, n_obj, n_frames, D, thin_at=(), late=0.0):
    """tests/golden/make_goldens_strongsort.py's make_stream at a size that leaves one block:
    a 9000 x 6000 canvas (a few hundred boxes do not all overlap), a fraction `late` of the
    objects starts after frame 0, a `thin_at` frame loses 60 % of its detections, every other
    frame 3 % at random.  The 6 % appearance failures and the random feature scale are kept.
    Per frame: dets (M, 6), raw feats (M, D) float32, warp (2, 3)."""
    rng = np.random.default_rng(seed)
    Wd, Ht = 9000.0, 6000.0
    c = np.stack([rng.uniform(100, Wd - 100, n_obj), rng.uniform(100, Ht - 100, n_obj)], 1)
    wh = np.stack([rng.uniform(40, 120, n_obj), rng.uniform(80, 240, n_obj)], 1)
    vel = rng.uniform(-3, 3, (n_obj, 2))
    base = rng.standard_normal((n_obj, D))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    cls = rng.integers(0, 3, n_obj).astype(np.float64)
    start = np.where(rng.random(n_obj) < late, rng.integers(1, max(2, n_frames - 1), n_obj), 0)
    frames = []
    for f in range(n_frames):
        c = c + vel
        ang = rng.uniform(-1.5e-3, 1.5e-3)
        warp = np.array([[np.cos(ang), -np.sin(ang), rng.uniform(-1.5, 1.5)],
                         [np.sin(ang), np.cos(ang), rng.uniform(-1.5, 1.5)]])
        miss = 0.6 if f in thin_at else 0.03
        rows, feats = [], []
        for o in rng.permutation(n_obj):
            if f < start[o] or rng.random() < miss:
                continue
            cc = c[o] + rng.uniform(-1, 1, 2)
            w, h = wh[o] * rng.uniform(0.98, 1.02, 2)
            rows.append([cc[0] - w / 2, cc[1] - h / 2, cc[0] + w / 2, cc[1] + h / 2,
                         rng.uniform(0.3, 0.99), cls[o]])
            if rng.random() < 0.06:                # an appearance failure: stage 2 takes the track
                e = rng.standard_normal(D)
            else:
                e = base[o] + 0.05 * rng.standard_normal(D)
            feats.append(e * rng.uniform(0.5, 4.0))
        frames.append((np.asarray(rows, dtype=np.float64).reshape(-1, 6),
                       np.asarray(feats, dtype=np.float32).reshape(-1, D), warp))
    return frames


BIG_P = dict(max_age=2, n_init=1, nn_budget=3, mc_lambda=0.995, ema_alpha=0.9, max_dist=0.2,
             max_iou_dist=0.7)
BIG_D = 16
BIG_CAP = 1024                       # track_capacity = max_dets of the engines that run it


class BigRun:
    """The restatement over the big stream: p, frames, per-frame rows and track counts (ntrk), the
    tracker after the last frame (oracle), and per frame the sizes the device kernels see
    (stats)."""


@functools.lru_cache(maxsize=None)
def big_run():
    """big_stream(5, 720, 7, 16, thin_at=(4,), late=0.2) through StrongSortOracle, once per
    process.  Asserts, from the oracle's trace and track lists, that the stream crosses the
    thresholds the tests are there for; a change that shifts it below one fails here instead of
    quietly testing less."""
    frames = big_stream(5, 720, 7, BIG_D, thin_at=(4,), late=0.2)
    orc = so.StrongSortOracle(**BIG_P)
    orc.trace = []
    rows, ntrk, stats = [], [], []
    for d, ft, w in frames:
        before = {t.id for t in orc.tracks}
        first_new = orc.next_id
        rows.append(orc.update(d, ft, w))
        raw1, raw2 = orc.trace[-1]
        after = {t.id for t in orc.tracks}
        stats.append(dict(
            dets=len(d), stage1=raw1.shape, stage2=raw2.shape,
            hopeless1=int((raw1 > BIG_P["max_dist"]).all(axis=1).sum()) if raw1.size else 0,
            deleted=len(before - after), born=orc.next_id - first_new, tracks=len(orc.tracks)))
        ntrk.append(len(orc.tracks))
    run = BigRun()
    run.p, run.frames, run.rows, run.ntrk, run.stats, run.oracle = BIG_P, frames, rows, ntrk, \
        stats, orc
    s1 = [s["stage1"] for s in stats]
    s2 = [s["stage2"] for s in stats]
    assert any(r > c and r > 512 and c > 0 for r, c in s1), s1    # transposed, column-major
    assert any(c > r and c > 512 and r > 0 for r, c in s1), s1
    assert any(r > 512 and c > 512 for r, c in s2), s2
    assert any(s["born"] > 256 for s in stats), stats
    assert any(s["deleted"] > 0 and s["born"] > 0 for s in stats), stats
    assert max(s["hopeless1"] for s in stats) >= 50, stats
    assert max(s["dets"] for s in stats) > 512 and min(s["dets"] for s in stats[1:]) > 256
    assert min(ntrk) > 512 and max(ntrk) <= BIG_CAP and max(s["dets"] for s in stats) <= BIG_CAP
    assert sum(len(r) > 256 for r in rows) >= 3                  # output compaction past a trip
    return run
