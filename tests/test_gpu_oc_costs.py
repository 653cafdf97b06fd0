"""GPU: the OC-SORT family's stage-1 matrices, entry by entry, against the oracles' record.

The other OC-family GPU files compare output rows and Kalman state, which a slightly wrong cost
changes only when it flips an assignment.  Here every entry of the matrices the engines build for
the first association round is read back (debug_costs, a test-only snapshot) and compared on
every frame of short scenes (tests/oc_costs.py) with what the oracle computed for the same frame
(oracle/*.py `recorder`), the output rows as well, so the snapshot is shown to change nothing.

References and bars (all from the reference and the number formats, on np.longdouble):
  rows / columns   the oracle's kept-detection order and tracker ids after prediction: exact
  asso             iou, giou, diou bit-equal to the oracle; ciou, centroid within 1e-12
                   (test_gpu_kat.py's bar).  The tracker boxes are read back too: where the
                   device's predicted boxes are not the oracle's bit for bit (DeepOCSORT's filter
                   squares exactly where the reference calls pow, test_gpu_deepocsort.py: 1e-10
                   relative on the state), the oracle's asso function is evaluated on the device's
                   boxes, so the bar is the kernel's and not the filter's
  angle term       (pi/2 - |acos(cos)|) / pi * valid * inertia * score in longdouble from the
                   oracle's float64 clipped cosine (the operations up to it are correctly rounded
                   and contraction is off, so both sides share that value; acos is ill-conditioned
                   near +-1, so a longdouble cosine would say nothing).  Bar: 4 x the oracle's own
                   largest float64 deviation from it on the frame, floored at 2^-52
  DeepOCSORT emb   where asso > 0: the dot product in longdouble of the float32 detection row and
                   the oracle's tracker embedding as stored; bar D 2^-53 + sqrt(D) 1e-12 (float64
                   accumulation of unit vectors; test_gpu_deepocsort.py's EMB_ATOL through a unit
                   row).  The oracle's own float32 product is not the reference
  DeepOCSORT term  the oracle's aw_max_metric on the device's own emb (0 where asso <= 0) equals
                   ((w_emb rw) cw) emb from the read-back bit for bit: the engine evaluates the
                   same aw_weight expression, so any difference is a scan bug; aw_off: emb * w_emb
  HybridSORT emb   max(0, 1 - u.v / (|u| |v|)) in longdouble from the float32 rows: the
                   detection rows as given and the tracker rows as the device holds them (read
                   before the frame; they agree with the oracle's to test_gpu_hybridsort.py's
                   FEAT_ATOL, a float32 norm summed in another order); bar (D + 4) 2^-52
  final cost       -((asso + angle) + term), HybridSORT -(asso + angle) + 1.3 emb, in longdouble
                   from the pieces above (the term is the device's own, verified bit for bit, so
                   it adds no bar); bar: the pieces' bars + 4 ulp of the frame's largest |cost|

The conditions on "the frames compared" hold on the frames from oc_costs.SHAPE_FRAME on: frame 4 is
M x N exactly, at least 10 % of the entries have asso > 0 on each, and the angle term takes both
signs over them (earlier frames have no velocities: the term is identically 0 there; they are
compared all the same).  Every test prints its largest error over its bar (profiles/oc_costs).

Breaking one line in a scratch build makes these cases fail: without k_doc_emb's
fetch(k0 + DE_KC), doc_dense_*_D40 and _D96 (emb); with k_doc_aw's column chunks one row short,
doc_dense_*_D24 and _D32, doc_dense_140x530, doc_crowded (AW term); without stash(buf ^ 1) in
k_hs_emb, hybridsort_*_D40, _D64 and _D96 (emb); without the implicit-zero pushes of
k_doc_emb_pairs, doc_listed_* and doc_aw_34x30_D24_listed (AW term).  The second of those two
pushes (n_trk - cnt >= 2) alone cannot fail anything: after the first the row's top value is >= 0,
a top value of 0 gives weight 0 whatever the second is, and a positive top value is a listed one,
so the one zero already bounds the second from below.
"""
import numpy as np
import pytest

import oc_costs as oc
from oc_costs import LD
from oracle.deepocsort import DeepOCSortOracle, aw_max_metric
from oracle.hybridsort import HybridSortOracle, get_features_norm
from oracle.ocsort import ASSO, OCSortOracle
from oracle.ocsort import _asso as oracle_asso
from yolo_tracking_amd import _lib
from yolo_tracking_amd.trackers.deepocsort import DeepOCSortEngine
from yolo_tracking_amd.trackers.hybridsort import HybridSortEngine
from yolo_tracking_amd.trackers.ocsort import OCSortEngine

pytestmark = pytest.mark.gpu

IMG = (1000, 1000, 3)
DOC_KW = dict(det_thresh=0.3, max_age=30, min_hits=1, iou_threshold=0.3, delta_t=3, inertia=0.2,
              w_association_emb=0.5, alpha_fixed_emb=0.95, aw_param=0.5)
OC_KW = dict(det_thresh=0.2, max_age=30, min_hits=1, asso_threshold=0.3, delta_t=3, inertia=0.2)
HS_KW = dict(det_thresh=0.0, max_age=30, min_hits=1, iou_threshold=0.3, delta_t=3, inertia=0.2)


def _pow2(n):
    return 1 << max(4, int(n - 1).bit_length())


class Worst:
    """The largest error / bar per quantity over a case, printed as one line."""

    def __init__(self, name):
        self.name, self.r, self.flags = name, {}, {}

    def check(self, what, err, bar, where):
        err, bar = LD(err), LD(bar)
        k = self.r.get(what, (LD(0), bar))
        if err >= k[0]:
            self.r[what] = (err, bar)
        assert err <= bar, (f"{self.name} {where}: {what} error {float(err):.3e} > "
                            f"bar {float(bar):.3e}")

    def flag(self, what, v):
        self.flags.setdefault(what, []).append(v)

    def report(self):
        parts = [f"{k} {float(e):.2e}/{float(b):.2e}" for k, (e, b) in self.r.items()]
        parts += [f"{k}={''.join(str(int(x)) for x in v)}" for k, v in self.flags.items()]
        print(f"{self.name}: " + "  ".join(parts))


def _head(w, got, rec, f, out, ref):
    """Output rows, sizes, row and column order; returns (m, n)."""
    assert np.array_equal(out, ref), (w.name, f, "output rows")
    m, n = len(rec["det_rows"]), len(rec["trk_ids"])
    assert (got["n_high"], got["n_trk"]) == (m, n), (w.name, f)
    assert np.array_equal(got["rows"], rec["det_rows"]), (w.name, f, "row order")
    assert np.array_equal(got["ids"], rec["trk_ids"]), (w.name, f, "column ids")
    for k, v in got.items():
        if isinstance(v, np.ndarray) and v.ndim == 2:
            assert v.shape == ((n, 4) if k == "boxes" else (m, n)), (w.name, f, k)
    return m, n


BOX_RTOL = 1e-9      # test_gpu_deepocsort.py's KF_RTOL


def _asso_ref(w, got, rec, func, f, centroid_wh=True):
    """The oracle's asso matrix; on the device's own predicted boxes where those are not the
    oracle's bit for bit (counted in the report as box_diff)."""
    if np.array_equal(got["boxes"], rec["trks"]):
        return rec["iou"]
    np.testing.assert_allclose(got["boxes"], rec["trks"], rtol=BOX_RTOL, atol=BOX_RTOL)
    w.flag("box_diff_frame", f)
    trks = np.column_stack([got["boxes"], np.zeros(len(got["boxes"]))])
    if centroid_wh:
        return oracle_asso(ASSO[func], rec["dets"], trks, IMG[1], IMG[0])
    return ASSO[func](rec["dets"], trks)


def _asso(w, got, rec, func, f):
    """Returns (the asso piece's bar, the reference asso)."""
    ref = _asso_ref(w, got, rec, func, f)
    if func in oc.EXACT_ASSO:
        assert np.array_equal(got["asso"], ref), (w.name, f, "asso not bit-equal",
                                                  float(np.abs(got["asso"] - ref).max()))
        w.check("asso", 0, 0, f)
        return LD(0), ref
    w.check("asso", oc.maxabs(got["asso"].astype(LD) - ref.astype(LD)), oc.ASSO_ATOL, f)
    return LD(oc.ASSO_ATOL), ref


class Conditions:
    """What a case must show on its frames from SHAPE_FRAME on."""

    def __init__(self, w, shape):
        self.w, self.shape, self.pos, self.neg, self.frames = w, shape, False, False, 0

    def frame(self, f, rec, angle):
        if f < oc.SHAPE_FRAME:
            return
        self.frames += 1
        if f == oc.SHAPE_FRAME and self.shape is not None:
            assert rec["iou"].shape == self.shape, (self.w.name, rec["iou"].shape)
        if rec["iou"].size:
            frac = float((rec["iou"] > 0).mean())
            assert frac >= 0.10, (self.w.name, f, f"only {frac:.3f} of the entries have asso > 0")
        self.pos |= bool((angle > 0).any())
        self.neg |= bool((angle < 0).any())

    def done(self):
        assert self.frames >= 2, self.w.name
        assert self.pos and self.neg, (self.w.name, "the angle term does not take both signs")


# ------------------------------------------------------------------ DeepOCSORT
def _doc_frame(w, got, rec, f, kw, D, seen):
    """One frame of one DeepOCSORT stream: asso, emb, AW term, final cost."""
    if "iou" not in rec:                       # no trackers: M x 0
        return None
    func = kw["asso_func"]
    asso_bar, ref_asso = _asso(w, got, rec, func, f)
    ref_ang = oc.angle_ref(rec["cos"], rec["valid"], rec["scores"], kw["inertia"])
    a_bar = oc.angle_bar(ref_ang, rec["angle_cost"])
    emb_on = not kw.get("embedding_off") and rec["iou"].size > 0
    term = np.zeros(rec["iou"].shape)
    if emb_on:
        keep = got["asso"] > 0
        ref = oc.dot_ref(rec["dets_embs"], rec["trk_embs"])
        bar = D * LD(2) ** -53 + np.sqrt(LD(D)) * LD(1e-12)
        w.check("emb", oc.maxabs((got["emb"].astype(LD) - ref)[keep]), bar, f)
        assert not got["emb"][~keep].any()     # the wrapper's zeros (association.py:165)
        if kw.get("aw_off"):
            term = got["emb"] * kw["w_association_emb"]
        else:
            w_emb = kw["w_association_emb"]
            term = ((w_emb * got["rw"])[:, None] * got["cw"][None, :]) * got["emb"]
            exp = aw_max_metric(got["emb"].copy(), kw["w_association_emb"], bottom=kw["aw_param"])
            same = np.array_equal(np.asarray(exp, np.float64).view(np.int64), term.view(np.int64)) \
                or np.array_equal(exp, term)   # -0.0 == 0.0
            assert same, (w.name, f, "AW term differs from aw_max_metric on the device's emb",
                          float(np.abs(exp - term).max()))
            w.check("aw_term", 0, 0, f)
            e = got["emb"]
            m, n = e.shape
            if n >= 2:
                top = -np.sort(-e, axis=1)[:, :2]
                seen["zero_row"] |= bool(((top[:, 0] == 0) & (got["rw"] == 0)).any())
                seen["ratio_one"] |= bool(((top[:, 0] == top[:, 1]) & (top[:, 0] > 0)).any())
            seen["neg_dot"] |= bool((e < 0).any())
            if n >= 2:                         # every kept dot product of a row negative: the
                kept = np.where(keep, e, -np.inf).max(1)      # implicit zeros are its top two
                seen["neg_top"] |= bool(((kept < 0) & np.isfinite(kept) & (got["rw"] == 0)).any())
            seen["single"] |= (m == 1 or n == 1)
    ref_cost = -((ref_asso.astype(LD) + ref_ang) + term.astype(LD))
    w.check("cost", oc.maxabs(got["cost"].astype(LD) - ref_cost),
            asso_bar + a_bar + oc.ulp4(ref_cost), f)
    return ref_ang


def _run_doc(name, streams, kw, D, shapes=None, flags=None, img=IMG):
    """streams: one list of frames per stream.  flags(f, got) asserts the path flags of a frame."""
    S = len(streams)
    ekw = dict(kw)
    cap = _pow2(2 * max(len(d) for fr in streams for d, _ in fr))
    eng = DeepOCSortEngine(S, feat_dim=max(D, 1), track_capacity=cap, max_dets=cap // 2, **ekw)
    eng.debug_costs_enable()
    ors = [DeepOCSortOracle(**kw) for _ in range(S)]
    for o in ors:
        o.recorder = []
    ws = [Worst(f"{name}[s{s}]" if S > 1 else name) for s in range(S)]
    conds = [Conditions(ws[s], None if shapes is None else shapes[s]) for s in range(S)]
    seen = dict(zero_row=False, ratio_one=False, neg_dot=False, neg_top=False, single=False)
    emb_off = bool(kw.get("embedding_off"))
    for f in range(len(streams[0])):
        dets = [streams[s][f][0] for s in range(S)]
        feats = None if emb_off else [streams[s][f][1] for s in range(S)]
        outs = eng.update(dets, feats, img_shapes=[img] * S)
        for s in range(S):
            ref = np.asarray(ors[s].update(dets[s], img, None if emb_off else streams[s][f][1]),
                             dtype=np.float64).reshape(-1, 8)
            rec = ors[s].recorder[-1]
            got = eng.debug_costs(s)
            _head(ws[s], got, rec, f, outs[s], ref)
            ang = _doc_frame(ws[s], got, rec, f, kw, D, seen)
            if f >= oc.SHAPE_FRAME:
                ws[s].flag("n_pos", got["n_pos"])
                ws[s].flag("col_ovf", got["col_ovf"])
                if flags is not None:
                    flags(s, f, got)
            if ang is not None:
                conds[s].frame(f, rec, ang)
    for s in range(S):
        conds[s].done()
        ws[s].report()
    eng.close()
    return seen


DENSE_SHAPES = [(1, 1), (1, 70), (70, 1), (63, 65), (130, 129)]
DENSE_WIDTHS = [1, 24, 32, 40, 96]


def _dense_flags(s, f, got):
    assert got["n_pos"] == 1


@pytest.mark.parametrize("D", DENSE_WIDTHS)
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_deepocsort_dense_tiles(monkeypatch, shape, D):
    """k_doc_emb (K below one chunk, ragged, one chunk, a tail of 8, three chunks) at the 64-tile
    edges, k_doc_aw's row and column scans and k_doc_aw_cols' chunk merge, k_doc_final."""
    monkeypatch.setenv("YTA_DOC_DENSE", "1")
    M, N = shape
    kw = dict(DOC_KW, asso_func="iou")
    fr = oc.scene(N, M, 1000 + 7 * M + N + D, D=D)
    _run_doc(f"doc_dense_{M}x{N}_D{D}", [fr], kw, D, shapes=[shape], flags=_dense_flags)


def test_deepocsort_dense_unrolled_scans(monkeypatch):
    """140 x 530: k_doc_aw's unrolled row loop (N >= 512) and unrolled column-chunk loop
    (M / 8 > 16) both run."""
    monkeypatch.setenv("YTA_DOC_DENSE", "1")
    kw = dict(DOC_KW, asso_func="iou")
    fr = oc.scene(530, 140, 4242, D=32, canvas=190.0)
    _run_doc("doc_dense_140x530_D32", [fr], kw, 32, shapes=[(140, 530)], flags=_dense_flags)


@pytest.mark.parametrize("D", [24, 250, 272])
def test_deepocsort_listed_pairs(D):
    """The default switch on an uncrowded stream: k_doc_emb_pairs (tail loop only, ragged tail,
    one unrolled pass plus tail) and k_doc_aw_cols' listed branch."""
    def flags(s, f, got):
        assert got["n_pos"] == 0 and got["col_ovf"] == 0

    kw = dict(DOC_KW, asso_func="iou")
    fr = oc.scene(36, 40, 2000 + D, D=D, canvas=180.0)
    _run_doc(f"doc_listed_40x36_D{D}", [fr], kw, D, shapes=[(40, 36)], flags=flags)


def test_deepocsort_crowded_default_switch():
    """The default switch on a crowded stream: some row lists more than 16 pairs, n_pos == 1."""
    def flags(s, f, got):
        assert got["n_pos"] == 1

    kw = dict(DOC_KW, asso_func="iou")
    fr = oc.scene(96, 96, 2100, D=32, canvas=120.0)
    _run_doc("doc_crowded_96x96_D32", [fr], kw, 32, shapes=[(96, 96)], flags=flags)


def test_deepocsort_column_overflow():
    """More than 16 detections overlap one tracker and no detection more than 16 trackers: row
    weights from the listed pairs, column weights from the dense scan (col_ovf fallback)."""
    def flags(s, f, got):
        assert got["n_pos"] == 0 and got["col_ovf"] == 1

    kw = dict(DOC_KW, asso_func="iou")
    fr = oc.column_overflow_scene(2200, 40)
    _run_doc("doc_colovf_20x21_D40", [fr], kw, 40, shapes=[(20, 21)], flags=flags)


@pytest.mark.parametrize("dense", [False, True], ids=["listed", "dense"])
def test_deepocsort_aw_values(monkeypatch, dense):
    """The AW cases that are easy to get wrong, each present in the data: a row with no
    positive-IoU tracker (top value 0, weight 0), two trackers born from identical features (ratio
    exactly 1), negative dot products on positive-IoU pairs, on one row all of them (the implicit
    zeros are then the row's top two and its weight is 0); N = 1 and M = 1 (the weight stays w_emb)
    in the other two scenes."""
    if dense:
        monkeypatch.setenv("YTA_DOC_DENSE", "1")
    kw = dict(DOC_KW, asso_func="iou")
    fr = oc.scene(30, 34, 2300, D=24, canvas=130.0, far=2, twins=True, flip=True)
    seen = _run_doc(f"doc_aw_34x30_D24_{'dense' if dense else 'listed'}", [fr], kw, 24,
                    shapes=[(34, 30)])
    assert seen["zero_row"] and seen["ratio_one"] and seen["neg_dot"] and seen["neg_top"], seen
    seen = _run_doc(f"doc_aw_1x12_D24_{'dense' if dense else 'listed'}",
                    [oc.scene(12, 1, 2301, D=24, canvas=40.0)], kw, 24, shapes=[(1, 12)])
    assert seen["single"]
    seen = _run_doc(f"doc_aw_12x1_D24_{'dense' if dense else 'listed'}",
                    [oc.scene(1, 12, 2302, D=24, canvas=30.0)], kw, 24, shapes=[(12, 1)])
    assert seen["single"]


@pytest.mark.parametrize("opt", ["aw_off", "embedding_off", "iou", "giou", "diou", "ciou",
                                 "centroid"])
def test_deepocsort_options(opt):
    kw = dict(DOC_KW, asso_func=opt if opt in ("giou", "diou", "ciou", "centroid") else "iou")
    if opt in ("aw_off", "embedding_off"):
        kw[opt] = True
    fr = oc.scene(33, 35, 2400, D=40, canvas=70.0)
    _run_doc(f"doc_opt_{opt}_35x33_D40", [fr], kw, 40, shapes=[(35, 33)])


def test_deepocsort_two_streams():
    """Two streams of different shapes in one engine: the per-stream matrix offsets (doc_mb)."""
    kw = dict(DOC_KW, asso_func="iou")
    a = oc.scene(65, 63, 2500, D=40, canvas=150.0)
    b = oc.scene(20, 31, 2501, D=40, canvas=90.0)
    _run_doc("doc_two_streams_D40", [a, b], kw, 40, shapes=[(63, 65), (31, 20)])


# ------------------------------------------------------------------ OCSORT
OC_FUNCS = ["iou", "giou", "diou", "ciou", "centroid"]


def _run_ocsort(name, streams, func, shapes):
    S = len(streams)
    kw = dict(OC_KW, asso_func=func)
    cap = _pow2(2 * max(len(d) for fr in streams for d, _ in fr))
    eng = OCSortEngine(S, track_capacity=cap, max_dets=cap // 2, **kw)
    eng.debug_costs_enable()
    ors = [OCSortOracle(**kw) for _ in range(S)]
    for o in ors:
        o.recorder = []
    ws = [Worst(f"{name}[s{s}]" if S > 1 else name) for s in range(S)]
    conds = [Conditions(ws[s], shapes[s]) for s in range(S)]
    empty = [0, 0]
    for f in range(len(streams[0])):
        dets = [streams[s][f][0] for s in range(S)]
        outs = eng.update(dets, img_shapes=[IMG] * S)
        for s in range(S):
            w = ws[s]
            ref = np.asarray(ors[s].update(dets[s], IMG), dtype=np.float64).reshape(-1, 8)
            rec = ors[s].recorder[-1]
            got = eng.debug_costs(s)
            m, n = _head(w, got, rec, f, outs[s], ref)
            empty[0] |= n == 0 and m > 0
            empty[1] |= m == 0 and n > 0
            if "iou" not in rec:
                continue
            asso_bar, ref_asso = _asso(w, got, rec, func, f)
            ref_ang = oc.angle_ref(rec["cos"], rec["valid"], rec["scores"], kw["inertia"])
            ref_cost = -(ref_asso.astype(LD) + ref_ang)
            w.check("cost", oc.maxabs(got["cost"].astype(LD) - ref_cost),
                    asso_bar + oc.angle_bar(ref_ang, rec["angle_cost"]) + oc.ulp4(ref_cost), f)
            if m:
                conds[s].frame(f, rec, ref_ang)
    for s in range(S):
        conds[s].done()
        ws[s].report()
    eng.close()
    return empty


@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (130, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("func", OC_FUNCS)
def test_ocsort_costs(func, shape):
    """k_oc_cost: every asso function; a frame without trackers (M x 0) and, last, a frame without
    detections (0 x N) read back cleanly."""
    M, N = shape
    canvas = {"giou": 70.0, "diou": 100.0, "ciou": 100.0}.get(func, 150.0)
    fr = oc.scene(N, M, 3000 + M + N, canvas=canvas if max(shape) > 1 else 10.0, nf=5)
    fr.append((np.zeros((0, 6)), np.zeros((0, 1), np.float32)))
    empty = _run_ocsort(f"ocsort_{func}_{M}x{N}", [fr], func, [shape])
    assert empty == [1, 1]


def test_ocsort_two_streams():
    a = oc.scene(65, 63, 3500, canvas=150.0)
    b = oc.scene(20, 31, 3501, canvas=90.0)
    _run_ocsort("ocsort_two_streams", [a, b], "iou", [(63, 65), (31, 20)])


def test_snapshot_switch_contract():
    """No snapshot before the switch is on and an update has run; the tensor path refuses while it
    is on and runs again once it is off."""
    import torch
    eng = OCSortEngine(1, asso_func="iou", **OC_KW)
    with pytest.raises(_lib.YTAError, match="snapshot"):
        eng.debug_costs(0)
    eng.debug_costs_enable()
    with pytest.raises(_lib.YTAError, match="snapshot"):
        eng.debug_costs(0)                      # on, but nothing has run yet
    d = torch.tensor([[10.0, 10.0, 50.0, 60.0, 0.9, 0.0]], dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.YTAError, match="debug costs"):
        eng.update_tensors([d], img_shapes=[IMG])
    out = eng.update([d.cpu().numpy()], img_shapes=[IMG])[0]
    got = eng.debug_costs(0)
    assert (got["n_high"], got["n_trk"]) == (1, 0) and got["asso"].shape == (1, 0)
    assert np.array_equal(got["rows"], [0]) and len(out) == 1
    eng.debug_costs_enable(False)
    rows, off, _ = eng.update_tensors([d], img_shapes=[IMG])
    torch.cuda.synchronize()
    assert int(off[1]) == 1
    eng.close()


# ------------------------------------------------------------------ HybridSORT
HS_FUNCS = ["iou", "giou", "diou", "ciou"]
FEAT_ATOL = 2e-7     # test_gpu_hybridsort.py's bar on the smooth features


def _run_hybridsort(name, streams, func, D, shapes):
    S = len(streams)
    kw = dict(HS_KW, asso_func=func)
    cap = _pow2(2 * max(len(d) for fr in streams for d, _ in fr))
    eng = HybridSortEngine(S, feat_dim=D, track_capacity=cap, max_dets=cap // 2, **kw)
    eng.debug_costs_enable()
    ors = [HybridSortOracle(**kw) for _ in range(S)]
    for o in ors:
        o.recorder = []
    ws = [Worst(f"{name}[s{s}]" if S > 1 else name) for s in range(S)]
    conds = [Conditions(ws[s], shapes[s]) for s in range(S)]
    new_tracks = False
    for f in range(len(streams[0])):
        dets = [streams[s][f][0] for s in range(S)]
        feats = [get_features_norm(streams[s][f][1]) for s in range(S)]
        assert all((np.abs(x).sum(1) > 0).all() for x in feats)      # no zero-norm rows
        before = [eng.state(s) for s in range(S)]    # the tracker rows the frame will read
        outs = eng.update(dets, feats)
        for s in range(S):
            w = ws[s]
            ref = np.asarray(ors[s].update(dets[s], feats[s]), dtype=np.float64).reshape(-1, 8)
            rec = ors[s].recorder[-1]
            got = eng.debug_costs(s)
            m, n = _head(w, got, rec, f, outs[s], ref)
            if "iou" not in rec:
                continue
            assert all(np.asarray(t).dtype == np.float32 for t in rec["trk_feats"])
            row_of = {int(i): k for k, i in enumerate(before[s]["id"])}
            trk_rows = before[s]["feat"][[row_of[int(i)] for i in rec["trk_ids"]]].reshape(n, D)
            assert trk_rows.dtype == np.float32
            np.testing.assert_allclose(trk_rows, np.array(rec["trk_feats"]).reshape(n, D), rtol=0,
                                       atol=FEAT_ATOL)
            ref_emb = oc.cosine_ref(rec["dets_embs"], trk_rows)
            e_bar = (D + 4) * oc.EPS
            w.check("emb", oc.maxabs(got["emb"].astype(LD) - ref_emb), e_bar, f)
            ref_ang, a_bar = LD(0), LD(0)
            for k in range(4):
                r = oc.angle_ref(rec["cos"][k], rec["valid"], rec["scores"], kw["inertia"])
                a_bar += oc.angle_bar(r, rec["corner_costs"][k])
                ref_ang = r if k == 0 else ref_ang + r
            if f >= oc.SHAPE_FRAME and (rec["valid"] == 0).any():
                new_tracks = True              # placeholder previous observation: all four terms 0
                z = rec["valid"] == 0
                assert all(not c[:, z].any() for c in rec["corner_costs"])
                assert not np.asarray(ref_ang)[:, z].any()
            asso_bar = LD(0) if func in oc.EXACT_ASSO else LD(oc.ASSO_ATOL)
            ref_asso = _asso_ref(w, got, rec, func, f, centroid_wh=False)
            ref_cost = -(ref_asso.astype(LD) + ref_ang) + LD(1.3) * ref_emb
            w.check("cost", oc.maxabs(got["cost"].astype(LD) - ref_cost),
                    asso_bar + a_bar + LD(1.3) * e_bar + oc.ulp4(ref_cost), f)
            conds[s].frame(f, rec, np.asarray(ref_ang))
    for s in range(S):
        conds[s].done()
        ws[s].report()
    eng.close()
    return new_tracks


@pytest.mark.parametrize("D", [8, 32, 40, 64, 96])
@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (130, 129)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hybridsort_emb_widths(shape, D):
    """k_hs_emb: scalar single chunk, vector single chunk, scalar multi-chunk ragged, the vector
    double buffer and its steady state, at the 64-tile edges; the fused epilogue's cost."""
    M, N = shape
    fr = oc.scene(N, M, 5000 + M + N + D, D=D, canvas=70.0 if max(shape) > 1 else 10.0)
    new_tracks = _run_hybridsort(f"hybridsort_giou_{M}x{N}_D{D}", [fr], "giou", D, [shape])
    assert new_tracks or M <= N


@pytest.mark.parametrize("func", HS_FUNCS)
def test_hybridsort_asso_functions(func):
    """Every asso function the engine accepts; frame 5 holds the tracks born in frame 4, whose
    placeholder previous observation makes valid = 0 for all four corner terms."""
    canvas = {"giou": 70.0, "diou": 100.0, "ciou": 100.0}.get(func, 150.0)
    fr = oc.scene(33, 41, 5100, D=40, canvas=canvas)
    assert _run_hybridsort(f"hybridsort_{func}_41x33_D40", [fr], func, 40, [(41, 33)])


def test_hybridsort_two_streams():
    """Two streams of different shapes in one engine: the per-stream matrix offsets (hs_mb)."""
    a = oc.scene(65, 63, 5200, D=40, canvas=150.0)
    b = oc.scene(20, 31, 5201, D=40, canvas=90.0)
    _run_hybridsort("hybridsort_two_streams_D40", [a, b], "iou", 40, [(63, 65), (31, 20)])
