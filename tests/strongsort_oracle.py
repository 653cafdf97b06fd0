"""NumPy restatement of StrongSORT as the device engine computes it (strongsort.hip).

The reference (boxmot/trackers/strongsort/, motion/kalman_filters/strongsort_kf.py,
utils/matching.py:224-378) fixes every float64 operation but not the summation order of its
float32 parts (np.dot / np.linalg.norm).  The device fixes its own order for those, and this
module restates exactly that order, so the device is compared with it bit for bit, while the
reference's goldens are matched exactly on ids / conf / cls / det_ind and to 1e-9 on the boxes.

Pinned float32 order
  norm(x)      64 partial sums p[l] = sum over k = l, l + 64, ... of x[k] * x[k] (each product
               rounded, added in increasing k), then p[l] += p[l ^ 32], ^16, ^8, ^4, ^2, ^1;
               sqrt correctly rounded; x / norm correctly rounded.
  dot(g, f)    a float32 fmaf chain from +0 over k in the order of the MFMA steps: within every
               block of 16, k = 0, 8, 1, 9, ..., 7, 15 (one rounding per step).
  cost         1 - dot, minimum over the gallery rows; the gallery rows are g / norm(g).
  EMA          s = float32(alpha) * last + float32(1 - alpha) * f  (three roundings), s / norm(s).

Stage 2's rows are the unconfirmed tracks followed by stage 1's unmatched tracks with
time_since_update == 1 in ascending list position (the reference iterates a Python set there).
"""
import numpy as np

CHI2INV95_4 = 9.4877
INFTY_COST = 1e5
W_POS = 1.0 / 20
W_VEL = 1.0 / 160


# ------------------------------------------------------------------------------- float32 order
def fmaf(a, b, c):
    """Correctly rounded float32 fma(a, b, c), vectorised: the product is exact in float64; the
    sum is rounded to odd in float64 (TwoSum residual), which makes the final rounding to
    float32 the single rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = even & (e != 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def norm_rows(x):
    """Pinned-order Euclidean norm of every row of x (n, D) float32 -> (n,) float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, D = x.shape
    pad = (-D) % 64
    sq = x * x
    if pad:
        sq = np.concatenate([sq, np.zeros((n, pad), np.float32)], axis=1)
    sq = sq.reshape(n, -1, 64)
    p = np.zeros((n, 64), np.float32)
    for c in range(sq.shape[1]):
        p = p + sq[:, c, :]
    w = 64
    while w > 1:
        w //= 2
        p = p[:, :w] + p[:, w:2 * w]
    return np.sqrt(p[:, 0])


def normalize_rows(x):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(len(x), -1)
    if len(x) == 0:
        return x.copy()
    return x / norm_rows(x)[:, None]


def k_order(D):
    """Order in which the fmaf chain visits k (see the module docstring)."""
    Dp = -(-D // 16) * 16
    base = np.arange(0, Dp, 16)[:, None, None]
    u = np.arange(8)[None, :, None]
    h = np.arange(2)[None, None, :]
    return (base + 8 * h + u).reshape(-1)


def dot_rows(g, f):
    """(n, D) x (m, D) float32 -> (n, m) float32 dot products in the pinned fmaf order."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    f = np.ascontiguousarray(f, dtype=np.float32)
    D = g.shape[1]
    acc = np.zeros((len(g), len(f)), np.float32)
    for k in k_order(D):
        if k < D:
            acc = fmaf(g[:, k][:, None], f[:, k][None, :], acc)
    return acc


def nn_cosine_min(gallery, lens, feats, fast=False):
    """gallery (T, B, D) float32 raw rows, lens (T,) valid rows each, feats (M, D) raw ->
    (T, M) float32: min over the track's rows of 1 - <g / |g|, f / |f|>."""
    gallery = np.asarray(gallery, dtype=np.float32)
    T, B, D = gallery.shape
    fn = normalize_rows(np.asarray(feats, dtype=np.float32).reshape(-1, D))
    out = np.empty((T, len(fn)), np.float32)
    for t in range(T):
        gn = normalize_rows(gallery[t, :lens[t]])
        d = gn @ fn.T if fast else dot_rows(gn, fn)
        out[t] = (np.float32(1.0) - d).min(axis=0)
    return out


# ---------------------------------------------------------------------------------- assignment
def lsa_replay(cost):
    """scipy.optimize.linear_sum_assignment(cost) replayed: same rows, same columns, the same
    choice among equal costs (SciPy's rectangular shortest-augmenting-path solver)."""
    cost = np.asarray(cost, dtype=np.float64)
    nr0, nc0 = cost.shape
    transpose = nc0 < nr0
    c = np.ascontiguousarray(cost.T if transpose else cost)
    nr, nc = c.shape
    u = np.zeros(nr)
    v = np.zeros(nc)
    col4row = np.full(nr, -1, np.int64)
    row4col = np.full(nc, -1, np.int64)
    path = np.full(nc, -1, np.int64)
    for cur in range(nr):
        min_val = 0.0
        remaining = list(range(nc - 1, -1, -1))
        SR = np.zeros(nr, bool)
        SC = np.zeros(nc, bool)
        sp = np.full(nc, np.inf)
        i = cur
        sink = -1
        while sink == -1:
            SR[i] = True
            rem = np.asarray(remaining, dtype=np.int64)
            r = ((min_val + c[i, rem]) - u[i]) - v[rem]
            better = r < sp[rem]
            path[rem[better]] = i
            sp[rem[better]] = r[better]
            vals = sp[rem]
            lowest = vals.min()
            assert lowest != np.inf, "infeasible cost matrix"
            at = np.nonzero(vals == lowest)[0]
            free = at[row4col[rem[at]] == -1]
            index = int(free[-1]) if len(free) else int(at[0])
            min_val = lowest
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            remaining[index] = remaining[-1]
            remaining.pop()
        u[cur] += min_val
        for r_ in np.nonzero(SR)[0]:
            if r_ != cur:
                u[r_] += min_val - sp[col4row[r_]]
        idx = np.nonzero(SC)[0]
        v[idx] -= min_val - sp[idx]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transpose:
        order = np.argsort(col4row, kind="stable")
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.copy()


def min_cost_matching(cost, max_distance):
    """linear_assignment.py:59-78 on a cost matrix (clamped in place) -> (matches [(row, col)],
    unmatched rows, unmatched columns in the reference's order)."""
    nr, nc = cost.shape
    if nr == 0 or nc == 0:
        return [], list(range(nr)), list(range(nc))
    cost[cost > max_distance] = max_distance + 1e-5
    rows, cols = lsa_replay(cost)
    cs, rs = set(cols.tolist()), set(rows.tolist())
    un_c = [j for j in range(nc) if j not in cs]
    un_r = [i for i in range(nr) if i not in rs]
    matches = []
    for i, j in zip(rows.tolist(), cols.tolist()):
        if cost[i, j] > max_distance:
            un_r.append(i)
            un_c.append(j)
        else:
            matches.append((i, j))
    return matches, un_r, un_c


# -------------------------------------------------------------------------------------- Kalman
def kf_initiate(z):
    """strongsort_kf.py:54-85."""
    h = z[3]
    std = np.array([2 * W_POS * h, 2 * W_POS * h, 1e-2, 2 * W_POS * h,
                    10 * W_VEL * h, 10 * W_VEL * h, 1e-5, 10 * W_VEL * h])
    return np.r_[z, np.zeros(4)], np.diag(std * std)


def kf_predict(mean, cov):
    """strongsort_kf.py:87-122 on the 2x2 blocks {i, i + 4} (every other entry is an exact zero)."""
    h = mean[3]
    sp = np.array([W_POS * h, W_POS * h, 1e-2, W_POS * h])
    sv = np.array([W_VEL * h, W_VEL * h, 1e-5, W_VEL * h])
    m = mean.copy()
    P = cov.copy()
    for i in range(4):
        pp, pv, vp, vv = cov[i, i], cov[i, i + 4], cov[i + 4, i], cov[i + 4, i + 4]
        P[i, i] = ((pp + vp) + (pv + vv)) + sp[i] * sp[i]
        P[i, i + 4] = pv + vv
        P[i + 4, i] = vp + vv
        P[i + 4, i + 4] = vv + sv[i] * sv[i]
        m[i] = mean[i] + mean[i + 4]
    return m, P


def _proj_std(mean, conf):
    h = mean[3]
    return np.array([(1 - conf) * (W_POS * h), (1 - conf) * (W_POS * h), (1 - conf) * 1e-1,
                     (1 - conf) * (W_POS * h)])


def kf_nsa_update(mean, cov, z, conf):
    """strongsort_kf.py:124-189: the NSA update (measurement std scaled by 1 - conf)."""
    r = _proj_std(mean, conf)
    m = mean.copy()
    P = cov.copy()
    for i in range(4):
        pp, pv, vp, vv = cov[i, i], cov[i, i + 4], cov[i + 4, i], cov[i + 4, i + 4]
        S = pp + r[i] * r[i]
        il = 1.0 / np.sqrt(S)
        kp = (pp * il) * il
        kv = (vp * il) * il
        innov = z[i] - mean[i]
        m[i] = mean[i] + innov * kp
        m[i + 4] = mean[i + 4] + innov * kv
        P[i, i] = pp - kp * (S * kp)
        P[i, i + 4] = pv - kp * (S * kv)
        P[i + 4, i] = vp - kv * (S * kp)
        P[i + 4, i + 4] = vv - kv * (S * kv)
    return m, P


def kf_gating(mean, cov, zs):
    """strongsort_kf.py:191-233 with project(confidence=0): squared Mahalanobis distance of every
    measurement row (the projected covariance is diagonal)."""
    r = _proj_std(mean, 0.0)
    zs = np.asarray(zs, dtype=np.float64).reshape(-1, 4)
    acc = None
    for i in range(4):
        l = np.sqrt(cov[i, i] + r[i] * r[i])
        z = (zs[:, i] - mean[i]) / l
        acc = z * z if acc is None else acc + z * z
    return acc


def camera_update(mean, warp):
    """track.py:129-138."""
    w_ = mean[2] * mean[3]
    x1 = mean[0] - w_ / 2
    y1 = mean[1] - mean[3] / 2
    x2 = x1 + w_
    y2 = y1 + mean[3]
    a = np.asarray(warp, dtype=np.float64).reshape(2, 3)
    x1_ = (a[0, 0] * x1 + a[0, 1] * y1) + a[0, 2]
    y1_ = (a[1, 0] * x1 + a[1, 1] * y1) + a[1, 2]
    x2_ = (a[0, 0] * x2 + a[0, 1] * y2) + a[0, 2]
    y2_ = (a[1, 0] * x2 + a[1, 1] * y2) + a[1, 2]
    w, h = x2_ - x1_, y2_ - y1_
    out = mean.copy()
    out[:4] = [x1_ + w / 2, y1_ + h / 2, w / h, h]
    return out


def iou_cost(tlwh, cand):
    """iou_matching.py:10-46 -> 1 - IoU of one tlwh box against candidate tlwh rows."""
    tl = tlwh[:2]
    br = tlwh[:2] + tlwh[2:]
    ctl = cand[:, :2]
    cbr = cand[:, :2] + cand[:, 2:]
    w = np.maximum(0.0, np.minimum(br[0], cbr[:, 0]) - np.maximum(tl[0], ctl[:, 0]))
    h = np.maximum(0.0, np.minimum(br[1], cbr[:, 1]) - np.maximum(tl[1], ctl[:, 1]))
    ai = w * h
    return 1.0 - ai / (tlwh[2] * tlwh[3] + cand[:, 2] * cand[:, 3] - ai)


# ------------------------------------------------------------------------------------- tracker
class _Track:
    __slots__ = ("id", "mean", "cov", "conf", "cls", "det_ind", "hits", "age", "tsu", "confirmed",
                 "feat", "gallery")

    def tlwh(self):
        w = self.mean[2] * self.mean[3]
        return np.array([self.mean[0] - w / 2, self.mean[1] - self.mean[3] / 2, w, self.mean[3]])


class StrongSortOracle:
    def __init__(self, max_dist=0.2, max_iou_dist=0.7, max_age=30, n_init=1, nn_budget=100,
                 mc_lambda=0.995, ema_alpha=0.9, fast=False):
        self.max_dist, self.max_iou_dist, self.max_age = max_dist, max_iou_dist, max_age
        self.n_init, self.nn_budget = n_init, nn_budget
        self.mc_lambda, self.ema_alpha = mc_lambda, ema_alpha
        self.fast = fast            # plain sgemm for the gallery product (timing only)
        self.tracks = []
        self.next_id = 1
        self.trace = None           # set to a list to record the cost matrices of both stages

    def has_tracks(self):
        """True when update() applies a warp (the estimator runs only on those frames)."""
        return len(self.tracks) >= 1

    def update(self, dets, feats, warp=None):
        dets = np.asarray(dets, dtype=np.float64).reshape(-1, 6)
        M = len(dets)
        feats = np.asarray(feats, dtype=np.float32)
        feats = feats.reshape(M, feats.size // M if M else (feats.shape[-1] if feats.ndim == 2 else 0))
        tr = self.tracks
        if tr and warp is not None:
            for t in tr:
                t.mean = camera_update(t.mean, warp)
        fn = normalize_rows(feats) if M else feats
        tlwh = np.stack([dets[:, 0], dets[:, 1], dets[:, 2] - dets[:, 0], dets[:, 3] - dets[:, 1]],
                        axis=1)
        xyah = np.stack([tlwh[:, 0] + tlwh[:, 2] / 2, tlwh[:, 1] + tlwh[:, 3] / 2,
                         tlwh[:, 2] / tlwh[:, 3], tlwh[:, 3]], axis=1)
        for t in tr:
            t.mean, t.cov = kf_predict(t.mean, t.cov)
            t.age += 1
            t.tsu += 1
        # stage 1: confirmed tracks, appearance + gate
        conf_rows = [k for k, t in enumerate(tr) if t.confirmed]
        unconf = [k for k, t in enumerate(tr) if not t.confirmed]
        c1 = np.zeros((len(conf_rows), M))
        if len(conf_rows) and M:
            for r, k in enumerate(conf_rows):
                t = tr[k]
                d = t.gallery @ fn.T if self.fast else dot_rows(t.gallery, fn)
                c = (np.float32(1.0) - d).min(axis=0).astype(np.float64)
                gd = kf_gating(t.mean, t.cov, xyah)
                c[gd > CHI2INV95_4] = INFTY_COST
                c1[r] = self.mc_lambda * c + (1 - self.mc_lambda) * gd
        raw1 = c1.copy()
        m1, _, un_d = min_cost_matching(c1, self.max_dist)
        matched_rows = {i for i, _ in m1}
        un_a = [conf_rows[i] for i in range(len(conf_rows)) if i not in matched_rows]
        # stage 2: IoU
        rows2 = unconf + [k for k in un_a if tr[k].tsu == 1]
        un_a = [k for k in un_a if tr[k].tsu != 1]
        c2 = np.zeros((len(rows2), len(un_d)))
        if len(rows2) and len(un_d):
            cand = tlwh[un_d]
            for r, k in enumerate(rows2):
                c2[r] = INFTY_COST if tr[k].tsu > 1 else iou_cost(tr[k].tlwh(), cand)
        raw2 = c2.copy()
        m2, un_r2, un_c2 = min_cost_matching(c2, self.max_iou_dist)
        if self.trace is not None:
            self.trace.append((raw1, raw2))
        matches = [(conf_rows[i], j) for i, j in m1] + [(rows2[i], un_d[j]) for i, j in m2]
        unmatched_tracks = un_a + [rows2[i] for i in un_r2]
        births = [un_d[j] for j in un_c2]
        af, bf = np.float32(self.ema_alpha), np.float32(1 - self.ema_alpha)
        dead = set()
        for k, j in matches:
            t = tr[k]
            t.conf, t.cls, t.det_ind = dets[j, 4], dets[j, 5], float(j)
            t.mean, t.cov = kf_nsa_update(t.mean, t.cov, xyah[j], dets[j, 4])
            s = (af * t.feat + bf * fn[j])[None, :]
            t.feat = (s / norm_rows(s)[:, None])[0]
            t.hits += 1
            t.tsu = 0
            if not t.confirmed and t.hits >= self.n_init:
                t.confirmed = True
        for k in unmatched_tracks:
            t = tr[k]
            if not t.confirmed or t.tsu > self.max_age:
                dead.add(k)
        for j in births:
            t = _Track()
            t.id = self.next_id
            self.next_id += 1
            t.mean, t.cov = kf_initiate(xyah[j])
            t.conf, t.cls, t.det_ind = dets[j, 4], dets[j, 5], float(j)
            t.hits, t.age, t.tsu, t.confirmed = 1, 1, 0, False
            t.feat = fn[j].copy()
            t.gallery = np.zeros((0, feats.shape[1]), np.float32)
            tr.append(t)
        self.tracks = tr = [t for k, t in enumerate(tr) if k not in dead]
        for t in tr:
            if t.confirmed:
                g = normalize_rows(t.feat[None, :])
                t.gallery = np.concatenate([t.gallery, g])[-self.nn_budget:]
        out = []
        for t in tr:
            if not t.confirmed or t.tsu >= 1:
                continue
            b = t.tlwh()
            out.append([b[0], b[1], b[0] + b[2], b[1] + b[3], t.id, t.conf, t.cls, t.det_ind])
        return np.asarray(out, dtype=np.float64).reshape(-1, 8)


# ------------------------------------------------------------------------------------ goldens
PARAM_KEYS = ("max_dist", "max_iou_dist", "max_age", "n_init", "nn_budget", "mc_lambda",
              "ema_alpha")


def golden_stream(z, name):
    """One stream of tests/golden/strongsort_synth.npz -> (params, frames, expected rows) with
    frames = [(dets (M, 6), feats (M, D) float32, warp (2, 3))]."""
    p = dict(zip(PARAM_KEYS, z[name + "_params"].tolist()))
    for k in ("max_age", "n_init", "nn_budget"):
        p[k] = int(p[k])
    cnt = z[name + "_counts"]
    frames = [(z[name + "_dets"][f, :cnt[f]].copy(), z[name + "_feats"][f, :cnt[f]].copy(),
               z[name + "_warps"][f].copy()) for f in range(len(cnt))]
    off = np.concatenate([[0], np.cumsum(z[name + "_row_counts"])])
    rows = [z[name + "_rows"][off[f]:off[f + 1]] for f in range(len(cnt))]
    return p, frames, rows


def run_oracle(params, frames):
    """The restatement over a stream -> (per-frame rows, the oracle)."""
    o = StrongSortOracle(**params)
    return [o.update(d, f, w) for d, f, w in frames], o
