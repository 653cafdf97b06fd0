"""k_s1_edges with the packed pre-test in front of its float64 IoU (csrc/bytetrack.hip,
s1_edges_rows_wave; csrc/grid.hpp, box_pack16 / box16_meet): frames built to sit on the test's
edges, one stream through yta_bytetrack_update_device against ByteTrackOracle(0.5, 0.8, 30, 30)
frame by frame, as tests/test_gpu_fused_dets.py drives its boundary cases (ids, scores, classes
and det_ind exact, boxes to 1e-9, no fallback counted), under both instantiations of the kernel
(YTA_SPLIT23=0: 512 threads, 1: 1024 threads).

* boxes edge to edge (x2 == the neighbour's x1: no intersection) and one ulp into each other;
* the same geometry 1e6 and 3e7 away from the origin (the packed coordinates are relative to the
  grid's origin, the float64 ones are not);
* one far detection that stretches the stream's extent, and with it the 16-bit step, to 1e5;
* pairs whose IoU x score lies within 1e-9 of 1 - match_thresh, on both sides, with scores 1.0,
  0.51 and 1.5;
* 1, 64, 65 and 1024 high detections (a wave, a wave and one, the LDS grid at its largest under
  the 512-thread kernel);
* 200 mutually overlapping boxes: a wave's candidate total is far beyond its queue and every row
  has more edges than slots, so the frame may take the counted fallbacks (not asserted there).

The predicates themselves, non-finite and degenerate boxes included, are checked on the host in
tests/test_s1_pretest_cpu.py.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_fused_dets import KW, _drive_one_stream
from test_s1_pretest_cpu import lattice

pytestmark = pytest.mark.gpu

SPLITS = [0, 1]


def _dets(boxes, conf):
    d = np.zeros((len(boxes), 6))
    d[:, :4] = boxes
    d[:, 4] = conf
    return d


def _jittered(boxes, conf, n_frames, seed, sigma=0.25):
    """The same objects in every frame, corners jittered from the second frame on."""
    rng = np.random.default_rng(seed)
    return [_dets(boxes + (rng.normal(0.0, sigma, boxes.shape) if f else 0.0), conf)
            for f in range(n_frames)]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("offset", [0.0, 1e6, 3e7])
@pytest.mark.parametrize("one_ulp", [False, True])
def test_lattices(monkeypatch, one_ulp, offset, split):
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    boxes = lattice(one_ulp, offset)
    assert len(boxes) == 96
    conf = np.random.default_rng(3).uniform(0.6, 0.95, 96)
    # two frames exactly on the lattice (the predicted boxes then differ from it by roundings
    # only: touching stays within an ulp or two of touching), then jitter
    frames = [_dets(boxes, conf), _dets(boxes, conf)] + _jittered(boxes, conf, 3, 11)[1:]
    _drive_one_stream(frames, split, cap=384, maxd=96)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("offset", [1e6, 3e7])
def test_synth_far_from_origin(monkeypatch, offset, split):
    from yolo_tracking_amd.synth import make_frames
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    frames = [d for d, _ in make_frames(96, 5, seed=4400)]
    for d in frames:
        d[:, :4] += offset
    _drive_one_stream(frames, split, cap=384, maxd=96)


@pytest.mark.parametrize("split", SPLITS)
def test_outlier_stretches_the_extent(monkeypatch, split):
    from yolo_tracking_amd.synth import make_frames
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    frames = []
    for f, (d, _) in enumerate(make_frames(96, 5, seed=4401)):
        far = np.array([[1e5 + f, 1e5 - f, 1e5 + f + 30.0, 1e5 - f + 50.0, 0.8, 0.0]])
        frames.append(np.concatenate([d[:40], far, d[40:]]))
    _drive_one_stream(frames, split, cap=388, maxd=97)


def _sweep_frames():
    k = 1.0 - KW["match_thresh"]
    n = 96
    rng = np.random.default_rng(9)
    W, H = rng.uniform(20.0, 90.0, n), rng.uniform(20.0, 90.0, n)
    ws = np.resize([1.0, 0.51, 1.5], n)
    side = np.resize([1.0 + 5e-10, 1.0 - 5e-10], n)
    t = k * side / ws
    dx = W * (1.0 - t) / (1.0 + t)      # equal boxes dx apart: IoU = (W - dx) / (W + dx) = t
    ox, oy = 200.0 * (np.arange(n) % 12), 200.0 * (np.arange(n) // 12)
    a = np.stack([ox, oy, ox + W, oy + H], axis=1)
    b = a + np.stack([dx, 0 * dx, dx, 0 * dx], axis=1)
    # tracks are born on a, meet their detection dx away at IoU x score ~ 1 - match_thresh (the
    # oracle decides which side each pair falls on), then the scene stays where it is
    return [_dets(a, 0.9), _dets(b, ws), _dets(b, ws), _dets(b, ws)]


@pytest.mark.parametrize("split", SPLITS)
def test_iou_times_score_at_the_threshold(monkeypatch, split):
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    _drive_one_stream(_sweep_frames(), split, cap=384, maxd=96)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("n", [1, 64, 65, 1024])
def test_high_counts(monkeypatch, n, split):
    from yolo_tracking_amd.synth import make_frames
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    frames = [d for d, _ in make_frames(n, 4, seed=4500 + n, low_conf_frac=0.0)]
    assert all(np.count_nonzero(d[:, 4] > KW["track_thresh"]) == n for d in frames)
    _drive_one_stream(frames, split, cap=max(2 * n, 16), maxd=n)


@pytest.mark.parametrize("split", SPLITS)
def test_cluster_beyond_queue_and_slots(monkeypatch, split):
    """200 boxes that all overlap each other: like _drive_one_stream, without its fallback bar."""
    import torch

    from oracle.bytetrack import ByteTrackOracle
    from yolo_tracking_amd import ByteTrackEngine, _lib
    monkeypatch.setenv("YTA_SPLIT23", str(split))
    n, cap = 200, 800
    rng = np.random.default_rng(21)
    ctr = rng.uniform(0.0, 30.0, (n, 2)) + 500.0
    wh = rng.uniform(60.0, 80.0, (n, 2))
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], axis=1)
    conf = rng.uniform(0.6, 0.95, n)
    frames = _jittered(boxes, conf, 4, 22)
    eng = ByteTrackEngine(1, device=0, track_capacity=cap, max_dets=n, **KW)
    ora = ByteTrackOracle(0.5, 0.8, 30, 30)
    out = torch.zeros((cap, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    for f, d in enumerate(frames):
        dev = torch.from_numpy(np.ascontiguousarray(d)).cuda()
        off = torch.tensor([0, len(d)], dtype=torch.int32, device="cuda")
        _lib.check(eng.lib.yta_bytetrack_update_device(
            eng.handle, ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(off.data_ptr()),
            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(cnt.data_ptr())))
        _lib.check(eng.lib.yta_bytetrack_sync(eng.handle))
        exp = np.asarray(ora.update(d), np.float64).reshape(-1, 8)
        k = int(cnt.item())
        assert k == len(exp), (f, k, len(exp))
        got = out[:k].cpu().numpy()
        assert np.array_equal(got[:, 4:], exp[:, 4:]), f
        np.testing.assert_allclose(got[:, :4], exp[:, :4], rtol=1e-9, atol=1e-9,
                                   err_msg=f"frame {f}")
    assert int(eng.next_ids()[0]) == ora.next_id
    eng.close()
