"""Scenes and references of tests/test_gpu_oc_costs.py (no GPU needed to import or run these).

A scene births N trackers in frames 1-3 and presents M detections from frame 4 on, so frame 4's
stage-1 matrix is M x N.  Trackers have non-zero velocities from frame 4 on (an observation in
each of three frames), which is where the angle term starts to say something; the frames from
`SHAPE_FRAME` on are the ones the tests put their conditions on.

References are evaluated on np.longdouble (64-bit mantissa) from the values the oracle recorded
(oracle/*.py `recorder`); every bar comes from the reference and the number formats alone.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble is not the x87 extended format on this machine"

SHAPE_FRAME = 3                    # index of the first M x N frame
STEPS = (0, 1, 2, 3, 0, 1)         # positions along the velocity: frame 5 comes back to the
                                   # start, so a 1 x 1 case sees both signs of the angle term
PI = LD(np.pi)                     # the float64 constant both the oracle and the device use
EPS = LD(2) ** -52


def _unit_rows(e):
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)


def frames_from(ctr, wh, vel, base, present, seed, nf=5, far=0, twins=False, flip=None):
    """nf frames of (dets (k, 6) float64, feats (k, D) float32 unit rows): object o stands at
    ctr[o] + STEPS[f] vel[o] (+ 0.3 px jitter) in frame f when present(f) lists it; `far` more
    detections stand where nothing else is from SHAPE_FRAME on (counted in M).  twins: objects 0
    and 1 get the same feature rows and confidences in every frame.  flip: this object's feature
    row changes sign from SHAPE_FRAME on."""
    rng = np.random.default_rng(seed)
    K, D = base.shape
    noise = 0.05 * rng.standard_normal((nf, K, D))
    jit = rng.normal(0.0, 0.3, (nf, K, 2))
    conf = rng.uniform(0.5, 0.99, (nf, K))
    if twins and K >= 2:
        noise[:, 1], conf[:, 1] = noise[:, 0], conf[:, 0]
    out = []
    for f in range(nf):
        idx = np.asarray(present(f), dtype=np.int64)
        idx = idx[rng.permutation(len(idx))]
        c = ctr[idx] + vel[idx] * STEPS[f] + jit[f, idx]
        d = np.zeros((len(idx), 6))
        d[:, :2], d[:, 2:4], d[:, 4] = c - wh[idx] / 2, c + wh[idx] / 2, conf[f, idx]
        e = base[idx] + noise[f, idx]
        if flip is not None and f >= SHAPE_FRAME:
            e[idx == flip] *= -1.0
        if far and f >= SHAPE_FRAME:
            fc = 5000.0 + 200.0 * np.arange(far)[:, None] + np.zeros((far, 2))
            fd = np.zeros((far, 6))
            fd[:, :2], fd[:, 2:4], fd[:, 4] = fc - 15, fc + 15, 0.9
            d = np.vstack([d, fd])
            e = np.vstack([e, np.random.default_rng(seed + 77).standard_normal((far, D))])
        out.append((d, _unit_rows(e) if len(d) else np.zeros((0, D), np.float32)))
    return out


def scene(N, M, seed, D=1, canvas=150.0, size=(28.0, 44.0), nf=5, speed=2.0, far=0, twins=False,
          flip=False):
    """N objects in frames 1-3, M (the first M objects, `far` of them far away) from frame 4 on.
    twins: objects 0 and 1 stand 4 px apart with the same motion and the same features, so two
    trackers are born from identical feature rows.  flip: object N - 1 stands alone, and its
    detections' feature rows change sign from frame 4 on, so its row's only positive-IoU dot
    product is negative."""
    rng = np.random.default_rng(seed)
    K = max(N, M - far, 1)
    ctr = 200.0 + rng.uniform(0.0, canvas, (K, 2))
    wh = rng.uniform(*size, (K, 2))
    vel = rng.normal(0.0, speed, (K, 2))
    base = rng.standard_normal((K, max(D, 1)))
    if twins and K >= 2:
        ctr[1], wh[1], vel[1], base[1] = ctr[0] + 4.0, wh[0], vel[0], base[0]
    if flip:
        assert N - 1 < M - far
        ctr[N - 1] = 3000.0
    return frames_from(ctr, wh, vel, base,
                       lambda f: np.arange(N if f < SHAPE_FRAME else M - far), seed + 1, nf, far,
                       twins, N - 1 if flip else None)


def column_overflow_scene(seed, D):
    """One 400 px tracker box over a 5 x 4 grid of 20 px boxes 15 px apart (N = 21); from frame 4
    on only the 20 small boxes are detected: the large tracker's column lists 20 > 16 pairs while
    no detection overlaps more than 10 trackers."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(5), np.arange(4))
    small = 400.0 + 15.0 * np.column_stack([gx.ravel(), gy.ravel()])
    ctr = np.vstack([[[430.0, 422.0]], small])
    wh = np.vstack([[[400.0, 400.0]], np.full((20, 2), 20.0)])
    vel = np.vstack([[[0.0, 0.0]], rng.normal(0.0, 0.7, (20, 2))])
    base = rng.standard_normal((21, D))
    return frames_from(ctr, wh, vel, base,
                       lambda f: np.arange(21) if f < SHAPE_FRAME else np.arange(1, 21), seed + 1)


# ------------------------------------------------------------------ references
def angle_ref(cos, valid, scores, inertia):
    """(pi/2 - |acos(cos)|) / pi * valid * inertia * score in longdouble from the oracle's float64
    clipped cosine (detections x trackers); valid per tracker, scores per detection."""
    ang = (PI / 2 - np.abs(np.arccos(cos.astype(LD)))) / PI
    return ((valid.astype(LD)[None, :] * ang) * LD(inertia)) * scores.astype(LD)[:, None]


def angle_bar(ref, oracle_term):
    """4 x the oracle's own largest float64 deviation from the reference, floored at 2^-52."""
    dev = np.abs(oracle_term.astype(LD) - ref).max() if ref.size else LD(0)
    return max(4 * dev, EPS)


def dot_ref(det_rows, trk_rows):
    """The dot products of the rows as stored, in longdouble (detections x trackers)."""
    return det_rows.astype(LD) @ np.asarray(trk_rows).astype(LD).T


def cosine_ref(det_rows, trk_rows):
    """max(0, 1 - u.v / (|u| |v|)) in longdouble."""
    u, v = det_rows.astype(LD), np.asarray(trk_rows).astype(LD)
    nu, nv = np.sqrt((u * u).sum(1)), np.sqrt((v * v).sum(1))
    return np.maximum(LD(0), 1 - (u @ v.T) / (nu[:, None] * nv[None, :]))


def ulp4(x):
    """4 ulp (float64) of the largest magnitude in x."""
    return 4 * LD(np.spacing(np.float64(np.abs(x).max()))) if x.size else LD(0)


def maxabs(a):
    return np.abs(a).max() if a.size else LD(0)


EXACT_ASSO = ("iou", "giou", "diou")   # bit-equal to the oracle; ciou and centroid to 1e-12
ASSO_ATOL = 1e-12                      # test_gpu_kat.py's bar for the two
