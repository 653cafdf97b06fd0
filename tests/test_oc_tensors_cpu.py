"""CPU: the surface of the OC-SORT family's tensor path (no compute calls): the C ABI declares and
exports its nine entry points, the binding lists them, the three engines have the methods."""
import os
import re

from conftest import REPO

NEW = tuple(f"yta_{t}_{f}" for t in ("ocsort", "deepocsort", "hybridsort")
            for f in ("update_tensors", "tensor_stats", "next_ids"))


def _header():
    return open(os.path.join(REPO, "include", "yolo_tracking_amd.h")).read()


def test_header_declares_the_nine_entry_points():
    src = _header()
    assert len(NEW) == 9
    for name in NEW:
        assert re.search(rf"^int {name}\s*\(", src, re.M), name


def test_every_declaration_has_a_comment_before_it():
    """The header's style: a /* ... */ block ends on the line before a declaration, or before
    the run of declarations the block names (tensor_stats / next_ids share one)."""
    lines = _header().split("\n")
    for name in NEW:
        k = next(i for i, ln in enumerate(lines) if re.match(rf"int {name}\s*\(", ln))
        j = k - 1
        while j >= 0 and not lines[j].rstrip().endswith("*/"):
            assert lines[j].strip(), name   # no blank line between the comment and its run
            j -= 1
        assert j >= 0, name


def test_binding_exports_them():
    from yolo_tracking_amd import _lib
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_signatures_match_the_header_argument_counts():
    from yolo_tracking_amd import _lib
    src = _header()
    for name in NEW:
        m = re.search(rf"^int {name}\s*\(([^;]*)\);", src, re.M | re.S)
        assert m, name
        assert len(_lib._SIGS[name][0]) == m.group(1).count(",") + 1, name


def test_engines_have_the_methods():
    from yolo_tracking_amd.trackers.deepocsort import DeepOCSortEngine
    from yolo_tracking_amd.trackers.hybridsort import HybridSortEngine
    from yolo_tracking_amd.trackers.ocsort import OCSortEngine
    for cls in (OCSortEngine, DeepOCSortEngine, HybridSortEngine):
        for m in ("update_tensors", "tensor_stats", "next_ids", "sync"):
            assert callable(getattr(cls, m, None)), (cls, m)
    assert len({c.update_tensors for c in (OCSortEngine, DeepOCSortEngine, HybridSortEngine)}) == 3
    assert len({c._abi for c in (OCSortEngine, DeepOCSortEngine, HybridSortEngine)}) == 3


def test_makefile_lists_the_kernels_header():
    mk = open(os.path.join(REPO, "yolo_tracking_amd", "csrc", "Makefile")).read()
    # the family's tensor kernels are tensor_path.hpp's, which oc_host.hpp includes
    assert re.search(r"^HDRS\s*=.*\btensor_path\.hpp\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\boc_host\.hpp\b", mk, re.M)
    host = open(os.path.join(REPO, "yolo_tracking_amd", "csrc", "oc_host.hpp")).read()
    assert '#include "tensor_path.hpp"' in host
