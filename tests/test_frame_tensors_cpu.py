"""No GPU: the surface of the frame-tensor path (yta_sof_apply_tensors, yta_ecc_apply_tensors,
yta_reid_preprocess_tensors and the two accounting entries) is declared, documented, exported and
bound with matching arity; the engines carry the Python front ends; the shared header is a build
dependency."""
import os
import re

from yolo_tracking_amd import _lib
from yolo_tracking_amd.motion.ecc import EccEngine
from yolo_tracking_amd.motion.sof import SofEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["yta_sof_apply_tensors", "yta_sof_tensor_stats", "yta_ecc_apply_tensors",
       "yta_ecc_tensor_stats", "yta_reid_preprocess_tensors"]


def _header():
    with open(os.path.join(REPO, "include", "yolo_tracking_amd.h")) as f:
        return f.read()


def test_header_declares_the_entries_with_a_comment_block():
    text = _header()
    for name in NEW:
        m = re.search(r"\*/\s*\nint %s\(" % name, text)
        assert m, f"{name}: no declaration directly after a comment block"


def test_exports_and_arity_match_the_header():
    text = _header()
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS, name
        m = re.search(r"\nint %s\(([^;]*?)\);" % name, text, re.S)
        assert m, name
        assert len(_lib._SIGS[name][0]) == m.group(1).count(",") + 1, name


def test_engines_have_the_front_ends():
    for cls in (SofEngine, EccEngine):
        assert callable(getattr(cls, "apply_tensors", None)), cls.__name__
        assert callable(getattr(cls, "tensor_stats", None)), cls.__name__


def test_shared_header_is_a_build_dependency():
    csrc = os.path.join(REPO, "yolo_tracking_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        hdrs = re.search(r"^HDRS\s*=(.*)$", f.read(), re.M).group(1).split()
    assert "cmc_tensors.hpp" in hdrs and os.path.isfile(os.path.join(csrc, "cmc_tensors.hpp"))
    for src in ("cmc.hip", "ecc.hip"):
        with open(os.path.join(csrc, src)) as f:
            assert '#include "cmc_tensors.hpp"' in f.read(), src
    # the protocol itself (slots, hand-off) is tensor_path.hpp's
    assert "tensor_path.hpp" in hdrs and os.path.isfile(os.path.join(csrc, "tensor_path.hpp"))
    with open(os.path.join(csrc, "cmc_tensors.hpp")) as f:
        assert '#include "tensor_path.hpp"' in f.read()
