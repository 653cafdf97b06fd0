"""CPU: k_apply's block placement (xcd_stream_blocks, csrc/common.hpp) evaluated on the host
through yta_apply_block_map: hardware block lin of a (gx blocks per stream) x (S streams) launch
works on logical (stream, block).  The map must visit every pair exactly once whatever gx and S
are; for the streams of whole groups of 8 it keeps a stream's blocks on XCD s & 7 (workgroups go
to the 8 XCDs round-robin by linear id), consecutive and in order there; the tail keeps the launch
order.  The GPU side is tests/test_gpu_apply_placement.py.
"""
import numpy as np


def test_block_map_is_a_bijection():
    from yolo_tracking_amd import _lib
    lib = _lib.load_library()
    for gx in range(1, 18):
        for S in range(1, 41):
            st = np.full(gx * S, -1, np.int32)
            bl = np.full(gx * S, -1, np.int32)
            _lib.check(lib.yta_apply_block_map(gx, S, _lib.ptr(st), _lib.ptr(bl)))
            assert st.min() >= 0 and st.max() < S and bl.min() >= 0 and bl.max() < gx, (gx, S)
            assert len(np.unique(st.astype(np.int64) * gx + bl)) == gx * S, (gx, S)
            lin = np.arange(gx * S)
            grouped = st < (S & ~7)
            assert np.array_equal(lin[grouped] & 7, st[grouped] & 7), (gx, S)
            assert np.array_equal((lin[grouped] >> 3) % gx, bl[grouped]), (gx, S)
            assert np.array_equal(st[~grouped], lin[~grouped] // gx), (gx, S)
            assert np.array_equal(bl[~grouped], lin[~grouped] % gx), (gx, S)


def test_block_map_rejects_bad_shapes():
    from yolo_tracking_amd import _lib
    lib = _lib.load_library()
    a = np.zeros(4, np.int32)
    assert lib.yta_apply_block_map(0, 4, _lib.ptr(a), _lib.ptr(a)) == _lib.YTA_ERR_INVALID
    assert lib.yta_apply_block_map(2, 2, None, _lib.ptr(a)) == _lib.YTA_ERR_INVALID
