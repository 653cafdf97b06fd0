"""CPU: the surface of StrongSORT's tensor path, stream subsets and per-stream reset: the header
declares the entry points (each under a comment), the library exports them, the ctypes signatures
agree with the header, and StrongSortEngine has the methods.  No compute calls (no GPU here)."""
import os
import re

import pytest

from conftest import REPO

ENTRY_POINTS = ["yta_strongsort_update_tensors", "yta_strongsort_tensor_stats",
                "yta_strongsort_next_ids", "yta_strongsort_update_streams",
                "yta_strongsort_update_device_masked", "yta_strongsort_reset_stream"]


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(REPO, "include", "yolo_tracking_amd.h")).read()


def _declaration(header, name):
    """(text before the declaration, its argument list) of `int name(...);`."""
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.M)
    assert m, f"{name} is not declared"
    return header[:m.start()], m.group(1)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_header_declares_it_under_a_comment(header, name):
    before, _ = _declaration(header, name)
    assert before.rstrip().endswith("*/"), f"{name}: no comment right above the declaration"
    comment = before[before.rindex("/*"):]
    assert len(comment.split()) >= 10, f"{name}: the comment says nothing"


@pytest.mark.parametrize("name", ENTRY_POINTS + ["yta_strongsort_n_tracks"])
def test_library_exports_it_with_the_headers_argument_count(header, name):
    from yolo_tracking_amd import _lib
    assert name in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.load_library(), name)
    _, args = _declaration(header, name)
    n_args = len([a for a in args.split(",") if a.strip()])
    assert len(_lib._SIGS[name][0]) == n_args, name


def test_update_tensors_signature_is_the_issues(header):
    _, args = _declaration(header, "yta_strongsort_update_tensors")
    names = [re.sub(r"[\s*]+", " ", a).strip().split(" ")[-1] for a in args.split(",")]
    assert names == ["engine", "caller_stream", "d_dets", "dtype", "row_stride", "det_counts",
                     "d_feats", "feat_stride", "d_warps", "d_active", "next_id", "d_rows",
                     "rows_capacity", "d_row_offsets", "d_row_stream"]


def test_engine_surface():
    from yolo_tracking_amd import StrongSortEngine
    from yolo_tracking_amd.trackers._streams import StreamSubset
    from yolo_tracking_amd.trackers._tensors import TensorPath
    assert issubclass(StrongSortEngine, StreamSubset) and issubclass(StrongSortEngine, TensorPath)
    assert StrongSortEngine._abi == "strongsort"
    for m in ("update_tensors", "update_streams", "reset_stream", "tensor_stats", "next_ids",
              "sync", "n_tracks"):
        assert callable(getattr(StrongSortEngine, m, None)), m


def test_makefile_lists_the_new_header():
    csrc = os.path.join(REPO, "yolo_tracking_amd", "csrc")
    # the tensor path's kernels and slots: tensor_path.hpp, shared by every engine
    assert os.path.isfile(os.path.join(csrc, "tensor_path.hpp"))
    mk = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    assert "tensor_path.hpp" in re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    assert '#include "tensor_path.hpp"' in open(os.path.join(csrc, "strongsort.hip")).read()
