"""k_apply's block placement (xcd_stream_blocks, csrc/common.hpp): the hardware block id is
remapped to a logical (stream, block) pair so that the blocks of one stream share an XCD.  The map
is only a permutation of block ids, so every result must stay what launch order gives.

The map itself is checked on the CPU (tests/test_apply_block_map.py).  Here: small shapes that
reach every path of the map: N = 96 objects, track capacities 192 and 384 (gx = 2 and 3 blocks
per stream), S in {1, 5, 8, 16, 24} (launch order only / a tail after one group of 8 / 1, 2 and
3 streams per XCD), 40 frames of SyntheticStream (2 % turnover, 10 %
low-confidence rows: Lost tracks appear, are re-found from the pool tail and expire after frame 30,
unconfirmed tracks are confirmed or removed), plus one case with non-uniform detection offsets (a
stream with no detections in some frames, a stream short by a third: the streams' items end in
different blocks and whole blocks exit early).  Bar, as in test_gpu_headline_shape.py:
* every stream's rows in every frame (int64 bit patterns) and every final ID counter equal a
  one-stream engine fed the same frames through yta_bytetrack_update_device;
* two sampled streams per case against oracle.bytetrack.ByteTrackOracle(0.5, 0.8, 30, 30): ids,
  scores, classes and det_ind exact, boxes within 1e-9 relative;
* no error flag (yta_bytetrack_sync) and no fallback counted in any frame.
BoT-SORT (k_apply<1>): S = 8, N = 96, no ReID (D = 0), a camera warp per stream, against its
one-stream engines the same way.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 96
FRAMES = 40
S_MAX = 24
SEED = 7000
KW = dict(track_thresh=0.5, match_thresh=0.8, track_buffer=30, frame_rate=30)
GAP_STREAM, GAP_FRAMES = 3, (12, 13, 25)     # no detections in these frames
SHORT_STREAM = 5                             # two thirds of every frame's detections


def _stream_frames(s, variant):
    from yolo_tracking_amd.synth import SyntheticStream
    g = SyntheticStream(N, SEED + s)
    fr = [g.next_frame()[0] for _ in range(FRAMES)]
    if variant == "gap":
        fr = [d[:0] if f in GAP_FRAMES else d for f, d in enumerate(fr)]
    elif variant == "short":
        fr = [d[:2 * N // 3] for d in fr]
    return fr


class Staged:
    """Frames of some streams in HBM: every frame's rows packed stream after stream."""

    def __init__(self, keys, frames_of):
        import torch
        self.keys = keys                                   # per stream: (stream seed index, variant)
        self.host = [frames_of(k) for k in keys]           # [stream][frame] -> (M, 6)
        S = len(keys)
        cnt = np.array([[len(self.host[s][f]) for s in range(S)] for f in range(FRAMES)], np.int64)
        off = np.zeros((FRAMES, S + 1), np.int32)
        off[:, 1:] = np.cumsum(cnt, axis=1)
        self.row0 = np.concatenate([[0], np.cumsum(off[:, -1])])      # first row of frame f
        packed = np.concatenate([self.host[s][f] for f in range(FRAMES) for s in range(S)])
        self.dets = torch.from_numpy(np.ascontiguousarray(packed)).cuda()
        self.off = torch.from_numpy(off).cuda()
        self.off_host = off
        one = np.zeros((FRAMES, S, 2), np.int32)
        one[:, :, 1] = cnt
        self.off1 = torch.from_numpy(one).cuda()

    def frame_ptr(self, f, s=0):
        return self.dets.data_ptr() + (int(self.row0[f]) + int(self.off_host[f, s])) * 48


@pytest.fixture(scope="module")
def ctx():
    """Staged frames, and the caches of the one-stream engine runs and the oracle runs (computed
    once per (capacity, stream) / per stream and shared by the cases)."""
    cache = {}

    def frames_of(key):
        if key not in cache:
            cache[key] = _stream_frames(*key)
        return cache[key]

    uniform = Staged([(s, "full") for s in range(S_MAX)], frames_of)
    keys = [(s, "full") for s in range(16)]
    keys[GAP_STREAM] = (GAP_STREAM, "gap")
    keys[SHORT_STREAM] = (SHORT_STREAM, "short")
    ragged = Staged(keys, frames_of)
    return dict(uniform=uniform, ragged=ragged, solo={}, oracle={}, solo_engines={})


def _solo(ctx, cap, staged, s):
    """Stream s of `staged` through a one-stream engine of the same capacity."""
    import torch

    from yolo_tracking_amd import ByteTrackEngine, _lib
    key = (cap,) + staged.keys[s]
    if key in ctx["solo"]:
        return ctx["solo"][key]
    if cap not in ctx["solo_engines"]:
        ctx["solo_engines"][cap] = ByteTrackEngine(1, device=0, track_capacity=cap, max_dets=N, **KW)
    e = ctx["solo_engines"][cap]
    e.reset()
    out = torch.zeros((FRAMES, cap, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    for f in range(FRAMES):
        _lib.check(e.lib.yta_bytetrack_update_device(
            e.handle, ctypes.c_void_p(staged.frame_ptr(f, s)),
            ctypes.c_void_p(staged.off1[f, s].data_ptr()), ctypes.c_void_p(out[f].data_ptr()),
            ctypes.c_void_p(cnt.data_ptr() + 4 * f)))
    _lib.check(e.lib.yta_bytetrack_sync(e.handle))
    nid = np.zeros(1, np.int64)
    _lib.check(e.lib.yta_bytetrack_next_ids(e.handle, nid.ctypes.data))
    ctx["solo"][key] = (out, cnt, int(nid[0]))
    return ctx["solo"][key]


def _oracle(ctx, staged, s):
    from oracle.bytetrack import ByteTrackOracle
    key = staged.keys[s]
    if key not in ctx["oracle"]:
        o = ByteTrackOracle(0.5, 0.8, 30, 30)
        rows = [np.asarray(o.update(d), np.float64).reshape(-1, 8) for d in staged.host[s]]
        ctx["oracle"][key] = (rows, int(o.next_id))
    return ctx["oracle"][key]


def _run_case(ctx, staged, S, cap, sampled):
    import torch

    from yolo_tracking_amd import ByteTrackEngine, _lib
    eng = ByteTrackEngine(S, device=0, track_capacity=cap, max_dets=N, **KW)
    assert eng.capacity() == (cap, N)
    lib = eng.lib
    out = torch.zeros((FRAMES, S, cap, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros((FRAMES, S), dtype=torch.int32, device="cuda")
    seen = dict(lazy=0, unc=0, lost=0, second=0, births=0)
    for f in range(FRAMES):
        _lib.check(lib.yta_bytetrack_update_device(
            eng.handle, ctypes.c_void_p(staged.frame_ptr(f)), ctypes.c_void_p(staged.off[f].data_ptr()),
            ctypes.c_void_p(out[f].data_ptr()), ctypes.c_void_p(cnt[f].data_ptr())))
        _lib.check(lib.yta_bytetrack_sync(eng.handle))          # raises on a device error flag
        st = eng.stats()
        assert st["fallback1"] == 0 and st["fallback23"] == 0 and st["fallback_f"] == 0, (f, st)
        assert st["dets"] == int(staged.off_host[f, S]), (f, st)
        for k in seen:
            seen[k] += st[k]
    # the workload reached every branch of k_apply: lazy Lost rows, stage-2 updates, unconfirmed
    # tracks (confirmed or removed), births
    assert all(v > 0 for v in seen.values()), seen
    nid = np.zeros(S, np.int64)
    _lib.check(lib.yta_bytetrack_next_ids(eng.handle, nid.ctypes.data))
    eng.close()
    rows = torch.arange(cap, device="cuda")
    for s in range(S):
        r_out, r_cnt, r_nid = _solo(ctx, cap, staged, s)
        assert torch.equal(cnt[:, s], r_cnt), (s, cnt[:, s].tolist(), r_cnt.tolist())
        live = (rows[None, :] < r_cnt[:, None].long())[:, :, None]
        diff = ((out[:, s].view(torch.int64) != r_out.view(torch.int64)) & live).any(dim=2).any(dim=1)
        assert not bool(diff.any()), (s, torch.nonzero(diff).flatten()[:8].tolist())
        assert int(r_cnt.sum()) > 0.5 * sum(len(d) for d in staged.host[s])
        assert nid[s] == r_nid, (s, int(nid[s]), r_nid)
    h_out, h_cnt = out.cpu().numpy(), cnt.cpu().numpy()
    for s in sampled:
        exp_rows, exp_nid = _oracle(ctx, staged, s)
        for f in range(FRAMES):
            exp = exp_rows[f]
            assert h_cnt[f, s] == len(exp), (s, f, int(h_cnt[f, s]), len(exp))
            got = h_out[f, s, :len(exp)]
            assert np.array_equal(got[:, 4:], exp[:, 4:]), (s, f)
            np.testing.assert_allclose(got[:, :4], exp[:, :4], rtol=1e-9, atol=1e-9,
                                       err_msg=f"stream {s} frame {f}")
        assert nid[s] == exp_nid, (s, int(nid[s]), exp_nid)


@pytest.mark.parametrize("cap", [192, 384])
@pytest.mark.parametrize("S", [1, 5, 8, 16, 24])
def test_streams_equal_one_stream_engine(ctx, S, cap):
    assert (cap + 127) // 128 == {192: 2, 384: 3}[cap]
    _run_case(ctx, ctx["uniform"], S, cap, sorted({0, S - 1}))


@pytest.mark.parametrize("cap", [192, 384])
def test_non_uniform_offsets(ctx, cap):
    """A stream with no detections in some frames and one short by a third: the streams' items
    end in different blocks of the launch."""
    st = ctx["ragged"]
    assert st.off_host[GAP_FRAMES[0], GAP_STREAM] == st.off_host[GAP_FRAMES[0], GAP_STREAM + 1]
    assert st.off_host[0, SHORT_STREAM + 1] - st.off_host[0, SHORT_STREAM] == 2 * N // 3
    _run_case(ctx, st, 16, cap, [GAP_STREAM, SHORT_STREAM])


def test_botsort_equals_one_stream_engines(ctx):
    """k_apply<1> (BoT-SORT: xywh filter, class votes, camera warp) at S = 8, gx = 3."""
    from yolo_tracking_amd.trackers.botsort import BoTSORTEngine
    S, cap = 8, 384
    P = dict(with_reid=False, device=0, track_capacity=cap, max_dets=N)
    host = ctx["uniform"].host
    eng = BoTSORTEngine(S, **P)
    solo = [BoTSORTEngine(1, **P) for _ in range(S)]
    assert eng.capacity() == (cap, N)
    nid, nid1 = np.zeros(S, np.int64), np.zeros((S, 1), np.int64)
    rng = np.random.default_rng(5)
    rows = 0
    for f in range(FRAMES):
        # a small camera motion per stream from frame 10 on (kf_gmc and the cross terms)
        warps = np.tile(np.eye(2, 3), (S, 1, 1))
        if f >= 10:
            warps[:, :, 2] = rng.normal(0.0, 1.5, size=(S, 2))
            warps[:, 0, 0] = warps[:, 1, 1] = 1.0 + rng.normal(0.0, 1e-3, size=S)
        got = eng.update([host[s][f] for s in range(S)], warps=warps, next_id=nid)
        st = eng.stats()
        assert st["fallback1"] == 0 and st["fallback23"] == 0 and st["fallback_f"] == 0, (f, st)
        for s in range(S):
            exp = solo[s].update([host[s][f]], warps=warps[s:s + 1], next_id=nid1[s])[0]
            assert got[s].shape == exp.shape, (f, s, got[s].shape, exp.shape)
            assert np.array_equal(got[s].view(np.int64), exp.view(np.int64)), (f, s)
            rows += len(exp)
        assert np.array_equal(nid, nid1[:, 0]), (f, nid, nid1[:, 0])
    assert rows > 0.5 * S * N * FRAMES
    eng.close()
    for e in solo:
        e.close()
