"""The detection pass at the top of k_s1_edges (csrc/bytetrack.hip, s1_dets_fused):
thread t classifies detection rows t and t + blockDim from registers, one packed block scan gives
the order-preserving high / second list positions, the lists go to HBM and the high boxes reach
the grid build through LDS.  More than 2 * blockDim detections take the chunked form and the
lists are read back.  Both instantiations are driven: 512 threads (many streams; forced with
YTA_SPLIT23=0) and 1024 threads (few streams, the default up to 64 streams).

Bars, as in test_gpu_apply_placement.py (whose staging and comparison this file reuses): rows as
int64 bit patterns and final ID counters of a multi-stream engine against one-stream engines;
sampled streams against oracle.bytetrack.ByteTrackOracle(0.5, 0.8, 30, 30) (ids, scores, classes,
det_ind exact, boxes within 1e-9 relative); no error flag, no fallback counted.

* multi-stream, both modes: S = 5 and 16, N = 96, 40 frames, and the ragged offsets (a stream
  with no detections in some frames, a stream short by a third);
* the fast path's boundary, one stream: nd = 1024 / 1025 under the 512-thread kernel, 2048 / 2049
  under the 1024-thread one, with few enough high rows for the LDS grid (the hand-off) and with
  the synthetic default (90 % high: the HBM grid, lists read back after the block's own stores);
  the engine's high and second counts equal the oracle's split in every frame;
* confidence KAT: exactly at / one ulp around track_thresh and the low threshold 0.1, a NaN; all
  rows high; no row high (a grid over nothing); nd = 0; nd = 1;
* ERR_DET_CAPACITY from a frame with more detections than max_dets through
  yta_bytetrack_update_device (no earlier test asserts the flag on that path).
"""
import ctypes

import numpy as np
import pytest

from test_gpu_apply_placement import FRAMES, GAP_STREAM, N, SHORT_STREAM, Staged, _run_case
from test_gpu_apply_placement import _stream_frames

pytestmark = pytest.mark.gpu

KW = dict(track_thresh=0.5, match_thresh=0.8, track_buffer=30, frame_rate=30)
LOW = 0.1   # byte_tracker.py:153
CAP = 192


@pytest.fixture(scope="module")
def ctx():
    cache = {}

    def frames_of(key):
        if key not in cache:
            cache[key] = _stream_frames(*key)
        return cache[key]

    uniform = Staged([(s, "full") for s in range(16)], frames_of)
    keys = [(s, "full") for s in range(16)]
    keys[GAP_STREAM] = (GAP_STREAM, "gap")
    keys[SHORT_STREAM] = (SHORT_STREAM, "short")
    ragged = Staged(keys, frames_of)
    # the one-stream engines (created on first use, in the default few-stream mode: 1024-thread
    # blocks) and the oracle runs are shared by every case
    return dict(uniform=uniform, ragged=ragged, solo={}, oracle={}, solo_engines={})


def _solo_first(ctx):
    """Create the shared one-stream engine before a case changes the mode variables."""
    from yolo_tracking_amd import ByteTrackEngine
    if CAP not in ctx["solo_engines"]:
        ctx["solo_engines"][CAP] = ByteTrackEngine(1, device=0, track_capacity=CAP, max_dets=N, **KW)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("S", [5, 16])
def test_streams_both_modes(ctx, monkeypatch, S, split):
    assert FRAMES == 40 and N == 96
    _solo_first(ctx)
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    _run_case(ctx, ctx["uniform"], S, CAP, sorted({0, S - 1}))


@pytest.mark.parametrize("split", [0, 1])
def test_ragged_offsets_both_modes(ctx, monkeypatch, split):
    _solo_first(ctx)
    st = ctx["ragged"]
    assert st.off_host[12, GAP_STREAM] == st.off_host[12, GAP_STREAM + 1]
    assert st.off_host[0, SHORT_STREAM + 1] - st.off_host[0, SHORT_STREAM] == 2 * N // 3
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    _run_case(ctx, st, 16, CAP, [GAP_STREAM, SHORT_STREAM])


def _drive_one_stream(frames, split, cap, maxd):
    """One stream through yta_bytetrack_update_device against the oracle, frame by frame; the
    engine's confidence split is checked against the oracle's in every frame."""
    import torch

    from oracle.bytetrack import ByteTrackOracle
    from yolo_tracking_amd import ByteTrackEngine, _lib
    from test_gpu_engine_modes import modes
    eng = ByteTrackEngine(1, device=0, track_capacity=cap, max_dets=maxd, **KW)
    assert modes(eng)["split23"] == split
    ora = ByteTrackOracle(0.5, 0.8, 30, 30)
    out = torch.zeros((cap, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    for f, d in enumerate(frames):
        d = np.ascontiguousarray(d, np.float64).reshape(-1, 6)
        dev = torch.from_numpy(d if len(d) else np.zeros((1, 6))).cuda()
        off = torch.tensor([0, len(d)], dtype=torch.int32, device="cuda")
        _lib.check(eng.lib.yta_bytetrack_update_device(
            eng.handle, ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(off.data_ptr()),
            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(cnt.data_ptr())))
        _lib.check(eng.lib.yta_bytetrack_sync(eng.handle))     # raises on a device error flag
        st = eng.stats()
        assert st["fallback1"] == 0 and st["fallback23"] == 0 and st["fallback_f"] == 0, (f, st)
        conf = d[:, 4]
        n_high = int(np.count_nonzero(conf > KW["track_thresh"]))
        n_second = int(np.count_nonzero((conf > LOW) & (conf < KW["track_thresh"])))
        assert (st["dets"], st["high"], st["second"]) == (len(d), n_high, n_second), (f, st)
        exp = np.asarray(ora.update(d), np.float64).reshape(-1, 8)
        k = int(cnt.item())
        assert k == len(exp), (f, k, len(exp))
        got = out[:k].cpu().numpy()
        assert np.array_equal(got[:, 4:], exp[:, 4:]), f
        np.testing.assert_allclose(got[:, :4], exp[:, :4], rtol=1e-9, atol=1e-9,
                                   err_msg=f"frame {f}")
    assert int(eng.next_ids()[0]) == ora.next_id
    assert (eng.capacity()) == (cap, maxd)     # nothing grew: the shapes are the ones asked for
    eng.close()


# nd on either side of 2 * blockDim.  sparse = False: the synthetic default (nine rows in ten high:
# at these sizes the grid goes to HBM); True: two objects in five high in every frame, the others
# below the low threshold but for one in twenty (n_high small enough for the LDS grid, and the
# high rows scattered among the others, while stages 2 and 3 stay small: a large second list or
# many unconfirmed tracks would send them to their global arena, a counted fallback)
@pytest.mark.parametrize("split,nd,sparse", [(0, 1024, False), (0, 1025, False), (0, 1025, True),
                                             (1, 2048, False), (1, 2048, True), (1, 2049, False),
                                             (1, 2049, True)])
def test_fast_path_boundary(monkeypatch, split, nd, sparse):
    from yolo_tracking_amd.synth import make_frames
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    n_frames = 4 if nd <= 1025 else 3
    if sparse:   # row k is object k in every frame
        frames = [d for d, _ in make_frames(nd, n_frames, seed=4100 + nd, low_conf_frac=0.0,
                                            shuffle=False)]
        k = np.arange(nd)
        for d in frames:
            d[k % 5 >= 2, 4] = 0.05
            d[k % 20 == 19, 4] = 0.3
        assert 0 < np.count_nonzero(frames[0][:, 4] > KW["track_thresh"]) < 0.45 * nd
    else:
        frames = [d for d, _ in make_frames(nd, n_frames, seed=4100 + nd)]
    assert all(len(d) == nd for d in frames)
    _drive_one_stream(frames, split, cap=2 * nd, maxd=nd)


def _kat_frames():
    thr = KW["track_thresh"]
    up, dn = (lambda x: np.nextafter(x, 1.0)), (lambda x: np.nextafter(x, 0.0))
    edge = [thr, up(thr), dn(thr), LOW, up(LOW), dn(LOW), np.nan, 0.9, 0.3, 0.05]
    n = 30
    rng = np.random.default_rng(77)
    ctr = np.stack([60.0 + 120.0 * (np.arange(n) % 6), 60.0 + 120.0 * (np.arange(n) // 6)], axis=1)
    wh = rng.uniform(30.0, 60.0, size=(n, 2))

    def frame(conf, keep=None):
        c = ctr + rng.normal(0.0, 0.5, size=ctr.shape)
        d = np.concatenate([c - wh / 2, c + wh / 2, np.asarray(conf, np.float64)[:, None],
                            np.zeros((n, 1))], axis=1)
        return d if keep is None else d[keep]
    hi = rng.uniform(0.6, 0.95, size=n)
    lo = rng.uniform(0.2, 0.4, size=n)
    cyc = np.array([edge[k % len(edge)] for k in range(n)])
    return [frame(hi),                       # every row high: tracks are born
            frame(cyc),                      # the thresholds, one ulp around them, a NaN
            frame(hi),
            frame(lo),                       # no row high: n_high = 0, the grid is over nothing
            frame(hi)[:0],                   # nd = 0
            frame(hi, keep=[7]),             # nd = 1
            frame(np.roll(cyc, 3)),
            frame(hi)]


@pytest.mark.parametrize("split", [0, 1])
def test_confidence_kat(monkeypatch, split):
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    frames = _kat_frames()
    assert np.isnan(frames[1][:, 4]).sum() == 3 and len(frames[4]) == 0 and len(frames[5]) == 1
    assert (frames[1][:, 4] == KW["track_thresh"]).sum() == 3 and (frames[1][:, 4] == LOW).sum() == 3
    _drive_one_stream(frames, split, cap=128, maxd=32)


@pytest.mark.parametrize("split", [0, 1])
def test_det_capacity_flag(monkeypatch, split):
    """More detections than max_dets through yta_bytetrack_update_device (which cannot see the
    count on the host): the frame runs on the first max_dets rows and the flag is raised."""
    import torch

    from yolo_tracking_amd import ByteTrackEngine, _lib
    from yolo_tracking_amd.synth import make_frames
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    maxd = 16
    d = make_frames(maxd + 5, 1, seed=4300)[0][0]
    eng = ByteTrackEngine(1, device=0, track_capacity=64, max_dets=maxd, **KW)
    dev = torch.from_numpy(np.ascontiguousarray(d)).cuda()
    off = torch.tensor([0, len(d)], dtype=torch.int32, device="cuda")
    out = torch.zeros((64, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(eng.lib.yta_bytetrack_update_device(
        eng.handle, ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(off.data_ptr()),
        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(cnt.data_ptr())))
    with pytest.raises(_lib.CapacityError, match="too many detections"):
        _lib.check(eng.lib.yta_bytetrack_sync(eng.handle))
    assert eng.capacity() == (64, maxd)
    eng.close()
