"""CPU: the tensor path's surface (no compute calls): the C ABI declares and exports its entry
points, the dtype codes agree between the header and the binding, the engines have the methods."""
import os
import re

from conftest import REPO

NEW = ("yta_bytetrack_update_tensors", "yta_botsort_update_tensors", "yta_bytetrack_tensor_stats")


def _header():
    return open(os.path.join(REPO, "include", "yolo_tracking_amd.h")).read()


def test_header_declares_the_entry_points():
    src = _header()
    for name in NEW:
        assert re.search(rf"^int {name}\s*\(", src, re.M), name


def test_binding_exports_them():
    from yolo_tracking_amd import _lib
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_dtype_codes_match_the_header():
    from yolo_tracking_amd import _lib
    src = _header()
    for name in ("YTA_F64", "YTA_F32", "YTA_F16"):
        m = re.search(rf"^#define {name} (\d+)\s*$", src, re.M)
        assert m, name
        assert getattr(_lib, name) == int(m.group(1)), name
    assert len({_lib.YTA_F64, _lib.YTA_F32, _lib.YTA_F16}) == 3


def test_engines_have_the_methods():
    from yolo_tracking_amd import ByteTrackEngine
    from yolo_tracking_amd.trackers.botsort import BoTSORTEngine
    for cls in (ByteTrackEngine, BoTSORTEngine):
        assert callable(getattr(cls, "update_tensors", None)), cls
        assert callable(getattr(cls, "tensor_stats", None)), cls
    assert BoTSORTEngine.update_tensors is not ByteTrackEngine.update_tensors


def test_cuda_tensor_detection_needs_no_torch():
    import numpy as np

    from yolo_tracking_amd.trackers._tensors import is_cuda_tensor
    assert not is_cuda_tensor(np.zeros((2, 6))) and not is_cuda_tensor(None)
    import torch
    assert not is_cuda_tensor(torch.zeros(2, 6))
