"""The conservative pre-test in front of k_s1_edges' float64 IoU (csrc/grid.hpp: box_pack16,
box16_meet), evaluated on the host through yta_s1_pretest, which derives origin and scale from the
stream's high detections as the kernel does.  The entry reports two bits per pair; the second
stage (a bound on IoU x score) was measured and not kept, so bit 1 repeats bit 0
today, and the bars below hold for it as they would for a real second stage.

Soundness, against NumPy float64 and the oracle's cost expression (oracle.geometry: fuse_score of
iou_distance, i.e. 1 - (1 - (1 - IoU)) * w): every pair whose cost is below thresh has both bits
set, and every pair that intersects in float64 has bit 0 set.  Nothing else is required of the
bits: false positives only cost time.  Selectivity is checked on the synthetic frames only: the
packed test may pass at most 2 % more pairs than really intersect (the 16-bit step is ~0.03 px
there against ~40 px boxes); the second bit's count is printed, not gated.

The GPU side is tests/test_gpu_s1_pretest.py.
"""
import numpy as np
import pytest

from oracle.geometry import fuse_score, iou_distance
from yolo_tracking_amd.synth import make_frames

THRESHES = (0.8, 1.0)


def pretest(rows, high, score, thresh):
    from yolo_tracking_amd import _lib
    lib = _lib.load_library()
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 4)
    high = np.ascontiguousarray(high, np.float64).reshape(-1, 4)
    score = np.ascontiguousarray(score, np.float64)
    assert len(score) == len(high)
    out = np.full((len(rows), len(high)), 0xFF, np.uint8)
    _lib.check(lib.yta_s1_pretest(len(rows), _lib.ptr(rows), len(high), _lib.ptr(high),
                                  _lib.ptr(score), float(thresh), _lib.ptr(out)))
    assert out.max(initial=0) <= 3
    return out


def intersects(rows, high):
    """geometry.hpp intersects(): plain float64 comparisons, false with any NaN."""
    a, b = rows[:, None, :], high[None, :, :]
    with np.errstate(invalid="ignore"):
        return ((a[..., 2] > a[..., 0]) & (a[..., 2] > b[..., 0]) & (b[..., 2] > a[..., 0]) &
                (b[..., 2] > b[..., 0]) & (a[..., 3] > a[..., 1]) & (a[..., 3] > b[..., 1]) &
                (b[..., 3] > a[..., 1]) & (b[..., 3] > b[..., 1]))


def cost_of(rows, high, score):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return fuse_score(iou_distance(rows, high), score)


def check_sound(rows, high, score, thresh, tag=""):
    """The two soundness bars; returns (bits, intersecting pairs, pairs below thresh)."""
    rows, high = np.asarray(rows, np.float64), np.asarray(high, np.float64)
    bits = pretest(rows, high, score, thresh)
    meet = intersects(rows, high)
    with np.errstate(invalid="ignore"):
        below = cost_of(rows, high, score) < thresh
    assert np.all(bits[meet] & 1), (tag, thresh, "an intersecting pair failed the packed test",
                                    np.argwhere(meet & ((bits & 1) == 0))[:4])
    assert np.all(bits[below] == 3), (tag, thresh, "an edge was dropped",
                                      np.argwhere(below & (bits != 3))[:4])
    return bits, meet, below


def synth_case(seed, n=1024):
    fr = [d for d, _ in make_frames(n, 2, seed=seed)]
    hi = fr[1][fr[1][:, 4] > 0.5]
    return fr[0][:, :4].copy(), hi[:, :4].copy(), hi[:, 4].copy()


def lattice(one_ulp, offset=0.0, nx=12, ny=8, size=40.0):
    """96 boxes edge to edge: x2 == x1 of the right neighbour exactly (they do not intersect), or
    one ulp beyond it (they do).  Every coordinate is an integer below 2^53: no sum rounds."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
    x1, y1 = offset + (size * ix).ravel(), offset + (size * iy).ravel()
    x2, y2 = x1 + size, y1 + size
    assert np.array_equal(x2.reshape(ny, nx)[:, :-1], x1.reshape(ny, nx)[:, 1:])
    if one_ulp:
        x2, y2 = np.nextafter(x2, np.inf), np.nextafter(y2, np.inf)
    return np.stack([x1, y1, x2, y2], axis=1)


@pytest.mark.parametrize("thresh", THRESHES)
def test_synth_frames_sound_and_selective(thresh):
    n_meet = n_s1 = n_s2 = n_below = 0
    for seed in range(1000, 1006):
        rows, high, score = synth_case(seed)
        bits, meet, below = check_sound(rows, high, score, thresh, f"seed {seed}")
        n_meet += int(meet.sum())
        n_below += int(below.sum())
        n_s1 += int(np.count_nonzero(bits & 1))
        n_s2 += int(np.count_nonzero(bits == 3))
    print(f"thresh {thresh}: intersecting {n_meet}, packed test passes {n_s1} "
          f"(+{100.0 * (n_s1 / n_meet - 1):.3f} %), both bits {n_s2}, edges {n_below}")
    assert n_meet > 6 * 1500
    assert n_s1 <= 1.02 * n_meet
    if thresh == 1.0:   # 1 - thresh <= 0: a second stage has to be off
        assert n_s2 == n_s1


@pytest.mark.parametrize("thresh", THRESHES)
@pytest.mark.parametrize("offset", [0.0, 1e6, 3e7])
@pytest.mark.parametrize("one_ulp", [False, True])
def test_lattices(one_ulp, offset, thresh):
    high = lattice(one_ulp, offset)
    score = np.full(len(high), 0.9)
    # rows: the boxes themselves, and copies shifted by half a box and by one ulp
    rows = np.concatenate([high, high + 20.0, np.nextafter(high, np.inf),
                           np.nextafter(high, -np.inf)])
    bits, meet, below = check_sound(rows, high, score, thresh, f"lattice ulp={one_ulp} +{offset}")
    assert meet[:96].sum() == (96 if not one_ulp else 96 + 2 * (11 * 8) + 2 * (12 * 7) + 4 * 77)
    assert below.sum() >= 96


@pytest.mark.parametrize("thresh", THRESHES)
def test_outlier_outside_rows_and_infinities(thresh):
    rows, high, score = synth_case(1003, n=96)
    high = np.concatenate([high, [[1e5, 1e5, 1e5 + 30.0, 1e5 + 50.0]]])   # the extent becomes 1e5
    score = np.concatenate([score, [0.8]])
    lo, hi_ = high[:, :2].min(), high[:, 2:].max()
    span = hi_ - lo
    outside = np.array([[lo - 2 * span, lo, lo - span, hi_],          # left of everything
                        [hi_ + span, lo, hi_ + 2 * span, hi_],        # right
                        [lo, lo - 2 * span, hi_, lo - span],          # above
                        [lo, hi_ + span, hi_, hi_ + 2 * span],        # below
                        [lo - span, lo - span, hi_ + span, hi_ + span],   # around everything
                        [-1e300, -1e300, 1e300, 1e300]])
    inf = np.array([[100.0, 100.0, np.inf, 150.0], [100.0, 100.0, 150.0, np.inf],
                    [-np.inf, 50.0, 200.0, np.inf], [-np.inf, -np.inf, np.inf, np.inf],
                    [np.nan, 0.0, 50.0, 50.0], [60.0, 60.0, 20.0, 20.0]])
    rows = np.concatenate([rows, high[-1:] + 3.0, outside, inf])
    bits, meet, below = check_sound(rows, high, score, thresh, "outlier")
    assert len(rows) == 96 + 1 + 6 + 6
    assert below[96, -1]                                  # the outlier's own row matches it
    assert not meet[97:101].any() and meet[101].all() and meet[102].all()
    assert meet[103:].sum() > 96


@pytest.mark.parametrize("thresh", THRESHES)
@pytest.mark.parametrize("w", [1.0, 0.51, 1.5, "mixed", "nan"])
def test_iou_times_score_sweep(w, thresh):
    """Pairs whose IoU x w lies within 1e-9 (relative) of 1 - 0.8 on both sides, at least 64 on
    each: equal boxes shifted along x by dx have IoU = (W - dx) / (W + dx).  They are evaluated at
    both thresholds (at 1.0 every intersecting pair is an edge)."""
    k = 1.0 - 0.8
    rng = np.random.default_rng(5)
    n = 192
    W, H = rng.uniform(20.0, 90.0, n), rng.uniform(20.0, 90.0, n)
    ws = np.resize([1.0, 0.51, 1.5], n) if isinstance(w, str) else np.full(n, w)
    side = np.resize([1.0 + 5e-10, 1.0 - 5e-10], n)   # IoU x w just above / just below k
    t = k * side / ws
    dx = W * (1.0 - t) / (1.0 + t)
    ox, oy = 200.0 * (np.arange(n) % 16), 200.0 * (np.arange(n) // 16)
    rows = np.stack([ox, oy, ox + W, oy + H], axis=1)
    high = rows + np.stack([dx, 0 * dx, dx, 0 * dx], axis=1)
    own = np.arange(n)
    with np.errstate(invalid="ignore"):
        prod = (1.0 - iou_distance(rows, high)[own, own]) * ws
    assert np.all(np.abs(prod / k - 1.0) <= 1e-9)
    c = cost_of(rows, high, ws)[own, own]
    assert (c < 0.8).sum() >= 64 and (c >= 0.8).sum() >= 64
    score = ws.copy()
    if w == "nan":
        score[7] = np.nan
    bits, meet, below = check_sound(rows, high, score, thresh, f"sweep w={w}")
    assert meet[own, own].all()
    if w == "nan" or thresh == 1.0:   # a second stage must be off: all that meet pass
        assert np.array_equal(bits == 3, (bits & 1) == 1)


def test_degenerate_inputs():
    from yolo_tracking_amd import _lib
    lib = _lib.load_library()
    rows = lattice(False)[:5]
    assert pretest(rows, np.zeros((0, 4)), np.zeros(0), 0.8).shape == (5, 0)
    assert pretest(np.zeros((0, 4)), rows, np.ones(5), 0.8).shape == (0, 5)
    # nothing usable among the detections: they are not binned, every pair reports 3
    bad = np.array([[0.0, 0.0, 0.0, 10.0], [np.nan, 0.0, 1.0, 1.0], [0.0, 0.0, np.inf, 5.0]])
    assert np.all(pretest(rows, bad, np.ones(3), 0.8) == 3)
    # one detection far larger than the others goes to the big list
    high = np.concatenate([lattice(False), [[0.0, 0.0, 4000.0, 4000.0]]])
    bits, meet, below = check_sound(high, high, np.full(len(high), 0.9), 0.8, "big")
    assert np.all(bits[:, -1] == 3) and meet[:, -1].all()
    out = np.zeros(4, np.uint8)
    assert lib.yta_s1_pretest(-1, None, 0, None, None, 0.8, _lib.ptr(out)) == _lib.YTA_ERR_INVALID
    assert lib.yta_s1_pretest(2, None, 2, None, None, 0.8, _lib.ptr(out)) == _lib.YTA_ERR_INVALID
