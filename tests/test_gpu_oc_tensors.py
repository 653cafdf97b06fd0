"""GPU: the tensor path of the OC-SORT family (OCSortEngine / DeepOCSortEngine / HybridSortEngine
.update_tensors, the OCSort and DeepOCSort drop-ins fed CUDA tensors): detections, features and
warps read from device tensors, rows written to device tensors, stream-ordered, nothing waited for.

Bar: every frame is bit-identical to update() on a second engine created with the same parameters
and fed the same values: rows compared as int64 views, offsets, row_stream, next_ids(), state(s)
of every stream and stats().  The host engine gets DeepOCSORT's features for the kept rows only
(conf > det_thresh), the tensor engine a row for every detection.  Frames come from
synth.make_frames with max_age = 2 and drop_frac / turnover > 0, so trackers are born after frame
0, lost, re-found and dropped within the 16 frames.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_streams_subset import DOC_KW, HS_KW, OC_KW
from yolo_tracking_amd import _lib
from yolo_tracking_amd.synth import make_frames

pytestmark = pytest.mark.gpu

KINDS = ["ocsort", "deepocsort", "hybridsort"]
D = 8
SYN = dict(drop_frac=0.15, turnover=0.1, low_conf_frac=0.0)
WARP = np.array([[1.0, 1e-3, 0.5], [-1e-3, 1.0, -0.3]])


def _make(kind, S, **over):
    """An engine of `kind` with the subset tests' parameters, max_age = 2 and `over`."""
    if kind == "ocsort":
        from yolo_tracking_amd.trackers.ocsort import OCSortEngine
        return OCSortEngine(S, **{**OC_KW, "max_age": 2, **over})
    if kind == "deepocsort":
        from yolo_tracking_amd.trackers.deepocsort import DeepOCSortEngine
        return DeepOCSortEngine(S, feat_dim=D, **{**DOC_KW, "max_age": 2, **over})
    from yolo_tracking_amd.trackers.hybridsort import HybridSortEngine
    return HybridSortEngine(S, feat_dim=D, **{**HS_KW, "max_age": 2, **over})


def _pair(kind, S, **over):
    return _make(kind, S, **over), _make(kind, S, **over)


_STREAMS = {}


def _streams(S, n, F, seed, **kw):
    """frames[f][s] = (dets (M, 6) float64, embs (M, D) float32 with unit rows).  Computed once
    per argument set and shared by the three trackers' cases: callers do not write into it."""
    key = (S, n, F, seed, tuple(sorted(kw.items())))
    if key not in _STREAMS:
        _STREAMS[key] = _streams_new(S, n, F, seed, **kw)
    return _STREAMS[key]


def _streams_new(S, n, F, seed, **kw):
    per = [make_frames(n, F, seed=seed + s, emb_dim=D, **{**SYN, **kw}) for s in range(S)]
    out = []
    for f in range(F):
        cur = []
        for s in range(S):
            d, e = per[s][f]
            e = (e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)).astype(np.float32)
            cur.append((d, e))
        out.append(cur)
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 8).view(np.int64)


def _host(kind, eng, dets, embs, warps=None, shapes=None, thr=0.0, streams=None, next_id=None):
    """update() of the host engine on float64 values: DeepOCSORT takes the kept rows' features."""
    dets = [np.asarray(d, dtype=np.float64) for d in dets]
    if kind == "ocsort":
        return eng.update(dets, shapes, streams=streams, next_id=next_id)
    if kind == "deepocsort":
        kept = [e[d[:, 4] > thr] for d, e in zip(dets, embs)]
        return eng.update(dets, kept, warps=warps, img_shapes=shapes, streams=streams,
                          next_id=next_id)
    return eng.update(dets, embs, streams=streams, next_id=next_id)


def _tens(kind, eng, dets, feats=None, warps=None, shapes=None, **kw):
    """update_tensors() of `kind`: dets / feats device tensors (lists or packed with counts=)."""
    if kind == "ocsort":
        return eng.update_tensors(dets, img_shapes=shapes, **kw)
    if kind == "deepocsort":
        return eng.update_tensors(dets, feats, warps=warps, img_shapes=shapes, **kw)
    return eng.update_tensors(dets, feats, **kw)


def _same_frame(res, exp, ctx):
    """res: update_tensors' (rows, offsets, row_stream); exp: update()'s list of S arrays."""
    rows, off, rs = (t.cpu().numpy() for t in res)
    lens = [len(e) for e in exp]
    assert off.dtype == np.int32 and rs.dtype == np.int32
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(lens)])), (ctx, off, lens)
    k = int(off[-1])
    want = np.concatenate([_i64(e) for e in exp]) if k else np.zeros((0, 8), np.int64)
    assert np.array_equal(_i64(rows[:k]), want), ctx
    assert np.array_equal(rs[:k], np.repeat(np.arange(len(exp)), lens)), ctx
    assert (rs[k:] == -1).all(), ctx


def _same_engines(tens, host, ctx=""):
    assert np.array_equal(tens.next_ids(), host.next_ids()), ctx
    for s in range(tens.n_streams):
        a, b = tens.state(s), host.state(s)
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), (ctx, s, key)
    assert tens.stats() == host.stats(), ctx


def _both(kind, tens, host, cur, ctx, warps=None, shapes=None, thr=0.0):
    """One frame on both engines from the float64 values `cur` = [(dets, embs)] per stream."""
    dets = [d for d, _ in cur]
    embs = [e for _, e in cur]
    exp = _host(kind, host, dets, embs, warps, shapes, thr)
    res = _tens(kind, tens, [_dev(d) for d in dets], [_dev(e) for e in embs],
                None if warps is None else _dev(warps), shapes)
    _same_frame(res, exp, ctx)
    return res


# ---------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.float16])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_per_dtype(kind, dtype):
    """S = 3, 24 objects, 16 frames; stream 1 is empty every fourth frame; DeepOCSORT gets
    alternating non-identity warps and the image sizes.  float32 / float16 inputs are the cast
    arrays, the host engine is fed their promoted float64 values."""
    S, F = 3, 16
    frames = _streams(S, 24, F, seed=100)
    shapes = [(320, 320, 3)] * S
    tens, host = _pair(kind, S, track_capacity=128, max_dets=32)
    births_late = deaths = prev_trk = 0
    for f in range(F):
        cur = [(d.astype(dtype), e) for d, e in frames[f]]
        if f % 4 == 2:
            cur[1] = (cur[1][0][:0], cur[1][1][:0])
        warps = np.stack([WARP if (s + f) % 2 else np.eye(2, 3) for s in range(S)])
        exp = _host(kind, host, [d for d, _ in cur], [e for _, e in cur], warps, shapes)
        res = _tens(kind, tens, [_dev(d) for d, _ in cur], [_dev(e) for _, e in cur],
                    _dev(warps), shapes)
        _same_frame(res, exp, (kind, dtype, f))
        assert f % 4 == 2 or all(len(e) > 0 for e in exp), (kind, dtype, f)   # rows came out
        st = host.stats()
        deaths += prev_trk + st["births"] - st["trackers"]
        births_late += st["births"] if f else 0
        prev_trk = st["trackers"]
    assert deaths > 0 and births_late > 0, (deaths, births_late)
    _same_engines(tens, host)
    assert tens.tensor_stats()["frames"] == F
    tens.sync()


# ------------------------------------------------------------------- 2. shapes that break kernels
@pytest.mark.parametrize("kind", KINDS)
def test_awkward_shapes(kind):
    import torch
    # one stream, one detection, then an empty frame
    tens, host = _pair(kind, 1, track_capacity=16, max_dets=8)
    one = np.array([[10.0, 20.0, 50.0, 90.0, 0.9, 0.0]])
    emb = np.full((1, D), 1.0 / np.sqrt(D), np.float32)
    for f, k in enumerate([0.0, 1.0, None, 2.0]):
        cur = [(one[:0], emb[:0])] if k is None else [(one + k, emb)]
        _both(kind, tens, host, cur, ("one", f))
    _same_engines(tens, host)

    # zero-count first and last streams, an odd total, an all-empty frame
    S, F = 4, 8
    frames = _streams(S, 13, F, seed=200)
    tens, host = _pair(kind, S, track_capacity=64, max_dets=16)
    for f in range(F):
        cur = list(frames[f])
        cur[0] = (cur[0][0][:0], cur[0][1][:0])
        cur[3] = (cur[3][0][:0], cur[3][1][:0])
        if (len(cur[1][0]) + len(cur[2][0])) % 2 == 0:
            cur[2] = (cur[2][0][:-1], cur[2][1][:-1])
        if f == 5:
            cur = [(d[:0], e[:0]) for d, e in cur]
        assert f == 5 or sum(len(d) for d, _ in cur) % 2 == 1
        _both(kind, tens, host, cur, ("odd", f))
    _same_engines(tens, host)

    # a float32 (total, 7)[:, :6] view (row stride 7 breaks 8-byte alignment of the rows), with
    # the features a column slice of a wider tensor whose padding is NaN
    frames = _streams(2, 21, 6, seed=210)
    tens, host = _pair(kind, 2, track_capacity=64, max_dets=32)
    for f in range(6):
        dets = [d.astype(np.float32) for d, _ in frames[f]]
        embs = [e for _, e in frames[f]]
        n = sum(len(d) for d in dets)
        wide = torch.full((n, 7), float("nan"), dtype=torch.float32, device="cuda:0")
        wide[:, :6] = _dev(np.concatenate(dets))
        view = wide[:, :6]
        fwide = torch.full((n, D + 3), float("nan"), dtype=torch.float32, device="cuda:0")
        fwide[:, :D] = _dev(np.concatenate(embs))
        assert view.stride(0) == 7 and fwide[:, :D].stride(0) == D + 3
        res = _tens(kind, tens, view, fwide[:, :D], counts=[len(d) for d in dets])
        _same_frame(res, _host(kind, host, dets, embs), ("stride7", f))
    assert tens.tensor_stats()["ingest_skipped"] == 0
    _same_engines(tens, host)

    # float64 contiguous: used in place
    tens, host = _pair(kind, 2, track_capacity=64, max_dets=32)
    for f in range(6):
        dets = [d for d, _ in frames[f]]
        embs = [e for _, e in frames[f]]
        res = _tens(kind, tens, _dev(np.concatenate(dets)), _dev(np.concatenate(embs)),
                    counts=[len(d) for d in dets])
        _same_frame(res, _host(kind, host, dets, embs), ("inplace", f))
    assert tens.tensor_stats()["ingest_skipped"] == 6
    _same_engines(tens, host)


def test_deepocsort_rows_at_or_below_det_thresh_are_not_read():
    """det_thresh = 0.3 with a third of the detections below it: the tensor engine's feature rows
    of those detections hold NaN, the host engine never gets them."""
    kind, thr = "deepocsort", 0.3
    frames = _streams(2, 24, 8, seed=220, low_conf_frac=0.35)
    tens, host = _pair(kind, 2, det_thresh=thr, track_capacity=64, max_dets=32)
    low = 0
    for f in range(8):
        dets = [d for d, _ in frames[f]]
        embs = [e for _, e in frames[f]]
        full = []
        for d, e in zip(dets, embs):
            e = e.copy()
            e[~(d[:, 4] > thr)] = np.nan
            low += int((~(d[:, 4] > thr)).sum())
            full.append(_dev(e))
        res = tens.update_tensors([_dev(d) for d in dets], full)
        _same_frame(res, _host(kind, host, dets, embs, thr=thr), f)
    assert low > 0
    _same_engines(tens, host)
    tens.sync()


# ---------------------------------------------------------------------------- 3. many streams
@pytest.mark.parametrize("kind", KINDS)
def test_many_streams(kind):
    """S = 1030: the offset scans give more than one stream per thread."""
    S, F = 1030, 6
    frames = _streams(S, 2, F, seed=3000)
    tens, host = _pair(kind, S, track_capacity=16, max_dets=8)
    for f in range(F):
        dets = [d for d, _ in frames[f]]
        embs = [e for _, e in frames[f]]
        res = _tens(kind, tens, _dev(np.concatenate(dets)), _dev(np.concatenate(embs)),
                    counts=[len(d) for d in dets])
        _same_frame(res, _host(kind, host, dets, embs), f)
    _same_engines(tens, host)


# ----------------------------------------------------------------------------------- 4. growth
@pytest.mark.parametrize("kind", KINDS)
def test_growth(kind):
    S, F = 2, 10
    frames = _streams(S, 30, F, seed=400)
    tens, host = _pair(kind, S, track_capacity=4, max_dets=4)
    for f in range(F):
        _both(kind, tens, host, frames[f], f)
    st = tens.tensor_stats()
    assert st["reserves"] >= 1, st
    cap, maxd = tens.capacity()
    assert cap > 4 and maxd >= max(len(d) for fr in frames for d, _ in fr)
    # every frame was waited for here, so the bound used the previous frame's exact live counts
    # (stored by its kernels) and the engine grew exactly when, and as far as, the host path did
    assert (cap, maxd) == host.capacity()
    tens.sync()   # raises on a device error flag
    _same_engines(tens, host)


# ------------------------------------------------------------------------------ 5. no host wait
@pytest.mark.parametrize("kind", KINDS)
def test_no_host_wait(kind):
    """track_capacity = 512 exceeds every detection of the run (12 x 24 a stream), so no call may
    block on the device; nothing is read between the frames."""
    S, F = 3, 12
    frames = _streams(S, 24, F, seed=500)
    tens, host = _pair(kind, S, track_capacity=512, max_dets=32)
    dev = [([_dev(d) for d, _ in fr], [_dev(e) for _, e in fr]) for fr in frames]
    res = [_tens(kind, tens, *dev[f]) for f in range(F)]   # no synchronisation in between
    st = tens.tensor_stats()
    assert st["host_waits"] == 0 and st["frames"] == F and st["reserves"] == 0, st
    for f in range(F):
        exp = _host(kind, host, [d for d, _ in frames[f]], [e for _, e in frames[f]])
        _same_frame(res[f], exp, f)
    _same_engines(tens, host)


# ----------------------------------------------------------------------------- 6. foreign stream
@pytest.mark.parametrize("kind", KINDS)
def test_foreign_stream(kind):
    """On a side stream, each frame's detections (and features) come out of matmuls queued just
    before the call; the stream is synchronised once, after the last frame."""
    import torch
    S, F = 2, 8
    frames = _streams(S, 24, F, seed=600)
    tens, host = _pair(kind, S, track_capacity=256, max_dets=32)
    up = [([_dev(d) for d, _ in fr], [_dev(e) for _, e in fr]) for fr in frames]
    a = torch.full((1024, 1024), 1.0 / 1024, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device="cuda:0")
    res = []
    with torch.cuda.stream(side):
        for f in range(F):
            x = a
            for _ in range(4):
                x = x @ a
            zero = x[0, 0] * 0   # ready only when the matmuls are
            dets = [u + zero.double() for u in up[f][0]]
            feats = [u + zero for u in up[f][1]]
            r = _tens(kind, tens, dets, feats, stream=side)
            res.append(tuple(t.clone() for t in r))
            del dets, feats, r   # back to the allocator while the frame may still be queued
    side.synchronize()
    for f in range(F):
        exp = _host(kind, host, [d for d, _ in frames[f]], [e for _, e in frames[f]])
        _same_frame(res[f], exp, f)
    _same_engines(tens, host)


# ------------------------------------------------------------------------------------- 7. mask
@pytest.mark.parametrize("kind", KINDS)
def test_mask(kind):
    S, F = 4, 10
    per = _streams(S, 16, F, seed=700)   # per[f][s]
    tens, host = _pair(kind, S, track_capacity=64, max_dets=32)
    rng = np.random.default_rng(5)
    pos = [0] * S
    none = (np.zeros((0, 6)), np.zeros((0, D), np.float32))
    for step in range(2 * F):
        ids = sorted(int(i) for i in rng.permutation(S)[:int(rng.integers(1, S + 1))]
                     if pos[i] < F)
        if not ids:
            continue
        skipped = [s for s in range(S) if s not in ids]
        before = {s: tens.state(s) for s in skipped}
        sub = [per[pos[s]][s] for s in ids]
        outs = _host(kind, host, [d for d, _ in sub], [e for _, e in sub], streams=ids)
        mask = np.zeros(S, np.int32)
        mask[ids] = 1
        cur = [per[pos[s]][s] if s in ids else none for s in range(S)]
        exp = [outs[ids.index(s)] if s in ids else np.zeros((0, 8)) for s in range(S)]
        res = _tens(kind, tens, [_dev(d) for d, _ in cur], [_dev(e) for _, e in cur],
                    active=_dev(mask))
        _same_frame(res, exp, step)
        off = res[1].cpu().numpy()
        for s in skipped:   # 0 rows, state untouched
            assert off[s + 1] == off[s], (step, s)
            after = tens.state(s)
            assert all(np.array_equal(before[s][k], after[k]) for k in after), (step, s)
        for s in ids:
            pos[s] += 1
    assert min(pos) > 3
    _same_engines(tens, host)


# ------------------------------------------------------------------------------ 8. mixed paths
def _raw_update_device(kind, eng, dets, embs, d_out, d_cnt):
    """One raw yta_<t>_update_device call on float64 rows; returns the tensors it must keep."""
    import torch
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    off = np.zeros(len(dets) + 1, np.int32)
    np.cumsum([len(d) for d in dets], out=off[1:])
    keep = [_dev(np.concatenate(dets)), _dev(off), _dev(np.concatenate(embs))]
    torch.cuda.synchronize()
    if kind == "ocsort":
        rc = eng.lib.yta_ocsort_update_device(eng.handle, p(keep[0]), p(keep[1]), None, p(d_out),
                                              p(d_cnt))
    elif kind == "deepocsort":
        rc = eng.lib.yta_deepocsort_update_device(eng.handle, p(keep[0]), p(keep[1]), p(keep[2]),
                                                  None, None, p(d_out), p(d_cnt))
    else:
        rc = eng.lib.yta_hybridsort_update_device(eng.handle, p(keep[0]), p(keep[1]), p(keep[2]),
                                                  p(d_out), p(d_cnt))
    _lib.check(rc)
    return keep


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_paths(kind):
    """One engine alternates update_tensors and update(); frame 5, a host frame right after a
    tensor frame, brings more detections than either capacity holds; stream 1 is reset in
    between.  Then the aliasing fix: after one raw update_device call into a caller's buffer, a
    host update() leaves that buffer alone and returns the right rows."""
    import torch
    S, F = 2, 12
    frames = _streams(S, 12, 5, seed=800) + _streams(S, 40, F - 5, seed=810)
    mix, host = _pair(kind, S, track_capacity=16, max_dets=16)
    for f in range(F):
        if f == 8:
            mix.reset_stream(1)
            host.reset_stream(1)
            assert len(mix.state(1)["id"]) == 0
        dets = [d for d, _ in frames[f]]
        embs = [e for _, e in frames[f]]
        exp = _host(kind, host, dets, embs)
        if f % 2 == 0:
            res = _tens(kind, mix, [_dev(d) for d in dets], [_dev(e) for e in embs])
            _same_frame(res, exp, f)
        else:
            got = _host(kind, mix, dets, embs)
            for s in range(S):
                assert np.array_equal(_i64(got[s]), _i64(exp[s])), (f, s)
    assert mix.capacity()[1] >= 40 and mix.capacity() == host.capacity()
    _same_engines(mix, host)
    mix.sync()

    # a.out used to stay the caller's buffer after update_device (fresh, roomy engines: the raw
    # call's capacities are hard limits)
    more = _streams(S, 40, 2, seed=820)
    mix, host = _pair(kind, S, track_capacity=256, max_dets=64)
    cap, _ = mix.capacity()
    d_out = torch.zeros((S * cap, 8), dtype=torch.float64, device="cuda:0")
    d_cnt = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    for eng in (mix, host):
        keep = _raw_update_device(kind, eng, [d for d, _ in more[0]], [e for _, e in more[0]],
                                  d_out, d_cnt)
        eng.sync()
        del keep
    sentinel = -12345.0
    d_out.fill_(sentinel)
    torch.cuda.synchronize()
    dets = [d for d, _ in more[1]]
    embs = [e for _, e in more[1]]
    got = _host(kind, mix, dets, embs)
    assert sum(len(g) for g in got) > 0
    torch.cuda.synchronize()
    assert bool((d_out == sentinel).all()), "update() wrote the rows into update_device's buffer"
    # the same frame through the tensor path of the other engine: same rows
    res = _tens(kind, host, [_dev(d) for d in dets], [_dev(e) for e in embs])
    _same_frame(res, got, "after update_device")
    _same_engines(mix, host)


# --------------------------------------------------------------------------------- 9. drop-ins
def test_dropin_ocsort():
    import torch
    from yolo_tracking_amd.trackers.ocsort import KalmanBoxTracker, OCSort
    frames = [fr[0][0] for fr in _streams(1, 24, 10, seed=1000)]
    frames.insert(5, frames[0][:0])
    img = np.zeros((320, 320, 3), np.uint8)
    kw = dict(det_thresh=0.2, max_age=2, min_hits=1, asso_func="giou")
    t = OCSort(**kw)
    exp = [np.asarray(t.update(d, img)).reshape(-1, 8) for d in frames]
    end = KalmanBoxTracker.count
    t = OCSort(**kw)
    assert KalmanBoxTracker.count == 0
    for f, d in enumerate(frames):
        got = t.update(_dev(d), img)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape[1] == 8, f
        assert np.array_equal(_i64(got.cpu().numpy()), _i64(exp[f])), f
    assert KalmanBoxTracker.count == end > 0 and t.frame_count == len(frames)
    # the ndarray path is as it was: np.array([]) for no tracks
    assert OCSort(**kw).update(np.zeros((0, 6)), img).shape == (0,)


def test_dropin_deepocsort():
    import torch
    from yolo_tracking_amd.motion import IdentityCMC
    from yolo_tracking_amd.trackers.deepocsort import DeepOCSort, KalmanBoxTracker
    frames = [fr[0] for fr in _streams(1, 24, 10, seed=1100, low_conf_frac=0.2)]
    img = np.zeros((320, 320, 3), np.uint8)
    kw = dict(det_thresh=0.3, max_age=2, min_hits=1, asso_func="giou", cmc=IdentityCMC(),
              feat_dim=D)
    a = DeepOCSort(None, "cuda:0", False, **kw)
    exp = [np.asarray(a.update(d, img, embs=e)).reshape(-1, 8) for d, e in frames]
    end = KalmanBoxTracker.count
    b = DeepOCSort(None, "cuda:0", False, **kw)
    assert KalmanBoxTracker.count == 1
    for f, (d, e) in enumerate(frames):
        got = b.update(_dev(d), img, embs=_dev(e))
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.shape[1] == 8, f
        assert np.array_equal(_i64(got.cpu().numpy()), _i64(exp[f])), f
    assert KalmanBoxTracker.count == end > 1 and b.frame_count == len(frames)


# --------------------------------------------------------------------------------- 10. refusals
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    import torch
    S, F = 2, 6
    frames = _streams(S, 16, F, seed=1200)
    tens, host = _pair(kind, S, track_capacity=128, max_dets=32)
    for f in range(F):
        dets = [d for d, _ in frames[f]]
        embs = [e for _, e in frames[f]]
        dd, de = [_dev(d) for d in dets], [_dev(e) for e in embs]
        if f == 3:
            before = [tens.state(s) for s in range(S)]
            with pytest.raises(ValueError):   # a tensor on the CPU
                _tens(kind, tens, [torch.from_numpy(dets[0]), dd[1]], de)
            with pytest.raises(ValueError):   # a wrong column count
                _tens(kind, tens, [dd[0][:, :5], dd[1]], de)
            with pytest.raises(ValueError):   # an unsupported dtype
                _tens(kind, tens, [d.long() for d in dd], de)
            with pytest.raises(ValueError):   # a wrong counts sum
                _tens(kind, tens, torch.cat(dd), torch.cat(de),
                      counts=[len(dets[0]), len(dets[1]) + 1])
            with pytest.raises(ValueError):   # a list with counts
                _tens(kind, tens, dd, de, counts=[len(d) for d in dets])
            if kind != "ocsort":
                with pytest.raises(ValueError):   # feature rows != detection rows
                    _tens(kind, tens, dd, [de[0][:-1], de[1]])
                with pytest.raises(ValueError):   # features of the wrong dtype
                    _tens(kind, tens, dd, [e.double() for e in de])
            # a capturing stream: the cross-stream waits must not end up in a graph
            cs = torch.cuda.Stream(device="cuda:0")
            packed, pfe, counts = torch.cat(dd), torch.cat(de), [len(d) for d in dets]
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=cs):
                y = packed * 1.0
                with pytest.raises(_lib.YTAError):
                    _tens(kind, tens, packed, pfe, counts=counts, stream=cs)
            del g, y
            torch.cuda.synchronize()
            # raw ctypes: rows_capacity smaller than the frame's detections
            n = int(sum(counts))
            rows = torch.empty((n, 8), dtype=torch.float64, device="cuda:0")
            offs = torch.empty(S + 1, dtype=torch.int32, device="cuda:0")
            cnt = np.asarray(counts, np.int32)
            p = lambda t: ctypes.c_void_p(t.data_ptr())
            head = (tens.handle, None, p(packed), _lib.YTA_F64, 6, _lib.ptr(cnt))
            tail = (None, None, p(rows), n - 1, p(offs), None)
            if kind == "ocsort":
                rc = tens.lib.yta_ocsort_update_tensors(*head, None, *tail)
            elif kind == "deepocsort":
                rc = tens.lib.yta_deepocsort_update_tensors(*head, p(pfe), D, None, None, *tail)
            else:
                rc = tens.lib.yta_hybridsort_update_tensors(*head, p(pfe), D, *tail)
            assert rc == _lib.YTA_ERR_CAPACITY
            with pytest.raises(_lib.CapacityError):
                _lib.check(rc)
            if kind != "ocsort":   # feat_stride < feat_dim
                tail_ok = (None, None, p(rows), n, p(offs), None)
                if kind == "deepocsort":
                    rc = tens.lib.yta_deepocsort_update_tensors(*head, p(pfe), D - 1, None, None,
                                                                *tail_ok)
                else:
                    rc = tens.lib.yta_hybridsort_update_tensors(*head, p(pfe), D - 1, *tail_ok)
                assert rc == _lib.YTA_ERR_INVALID
            assert tens.tensor_stats()["frames"] == 3
            for s in range(S):
                after = tens.state(s)
                assert all(np.array_equal(before[s][k], after[k]) for k in after), s
        _same_frame(_tens(kind, tens, dd, de), _host(kind, host, dets, embs), f)
    _same_engines(tens, host)


@pytest.mark.parametrize("kind", ["ocsort", "deepocsort"])
def test_centroid_needs_img_shapes(kind):
    S = 2
    frames = _streams(S, 8, 3, seed=1300)
    tens, host = _pair(kind, S, asso_func="centroid", track_capacity=32, max_dets=16)
    shapes = [(240, 240, 3), (200, 260, 3)]
    for f in range(3):
        dets = [d for d, _ in frames[f]]
        embs = [e for _, e in frames[f]]
        dd, de = [_dev(d) for d in dets], [_dev(e) for e in embs]
        if f == 1:
            with pytest.raises(ValueError):
                _tens(kind, tens, dd, de)
            assert tens.tensor_stats()["frames"] == 1
        res = _tens(kind, tens, dd, de, shapes=shapes)
        _same_frame(res, _host(kind, host, dets, embs, shapes=shapes), f)
    _same_engines(tens, host)
