"""CPU: the OC-SORT family oracles' recorder (oracle/{ocsort,deepocsort,hybridsort}.py).

tests/test_gpu_oc_costs.py compares the engines' stage-1 matrices with what the oracles record, so
the record has to be what the oracle acted on.  For every frame of one golden case per tracker:
the recorded cost, solved again with oracle.lap, gives the pairs the oracle's association got
(on the frames that took the unique-match shortcut, where no cost was solved: the pairs above the
threshold), the recorded pieces add up to it bit for bit, and recording leaves the outputs and the
final tracker states bit-identical to a run without it.
"""
import os

import numpy as np
import pytest

from oracle.lap import linear_assignment_padded
from test_oracle_golden import deepocsort_case, hybridsort_case, ocsort_case


def _run_ocsort(g, name, record):
    from oracle.ocsort import OCSortOracle
    frames, img_shape, kw = ocsort_case(g, name)
    t = OCSortOracle(**kw)
    if record:
        t.recorder = []
    out = [np.asarray(t.update(d, img_shape), dtype=np.float64).reshape(-1, 8) for d in frames]
    return t, out, kw["asso_threshold"]


def _run_deepocsort(g, name, record):
    from oracle.deepocsort import DeepOCSortOracle
    frames, img_shape, kw, warp, _ = deepocsort_case(g, name)
    t = DeepOCSortOracle(**kw)
    if record:
        t.recorder = []
    out = [np.asarray(t.update(d, img_shape, f, warp), dtype=np.float64).reshape(-1, 8)
           for d, f in frames]
    return t, out, kw["iou_threshold"]


def _run_hybridsort(g, name, record):
    from oracle.hybridsort import HybridSortOracle, get_features_norm
    frames, kw, _ = hybridsort_case(g, name)
    t = HybridSortOracle(**kw)
    if record:
        t.recorder = []
    out = [np.asarray(t.update(d, get_features_norm(e)), dtype=np.float64).reshape(-1, 8)
           for d, e in frames]
    return t, out, kw["iou_threshold"]


CASES = [("ocsort_synth.npz", "oc_n128_iou_mh3", _run_ocsort),
         ("deepocsort_synth.npz", "dos_n64_d32", _run_deepocsort),
         ("deepocsort_synth.npz", "dos_n96_d32_awoff", _run_deepocsort),
         ("hybridsort_synth.npz", "hs_n64_d32", _run_hybridsort)]


def _state(t):
    return [(k.id, k.kf.x.copy(), k.kf.P.copy()) for k in t.trackers]


@pytest.mark.parametrize("npz,name,run", CASES, ids=[c[1] for c in CASES])
def test_recorded_cost_reproduces_the_matches(golden_dir, npz, name, run):
    g = np.load(os.path.join(golden_dir, npz))
    plain, out_plain, thr = run(g, name, False)
    rec, out_rec, _ = run(g, name, True)
    assert len(out_plain) == len(out_rec)
    for a, b in zip(out_plain, out_rec):        # recording changes nothing, bit for bit
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    for (ia, xa, Pa), (ib, xb, Pb) in zip(_state(plain), _state(rec), strict=True):
        assert ia == ib and np.array_equal(xa, xb) and np.array_equal(Pa, Pb)
    assert len(rec.recorder) == len(out_rec)
    solved = shortcuts = 0
    for f, r in enumerate(rec.recorder):
        if "cost" not in r:                     # no trackers yet
            assert len(r["trk_ids"]) == 0
            continue
        m, n = len(r["det_rows"]), len(r["trk_ids"])
        assert r["cost"].shape == r["iou"].shape == r["angle_cost"].shape == (m, n)
        if min(m, n) == 0:
            assert r["matched"].shape == (0, 2)
            continue
        if "emb_cost" in r:                     # HybridSORT
            again = 1.0 * (-(r["iou"] + r["angle_cost"])) + 1.3 * r["emb_cost"] + 0.0
        else:
            again = -(r["iou"] + r["angle_cost"] + r.get("emb_term", 0))
        assert np.array_equal(again, r["cost"]), f
        pairs = np.asarray(linear_assignment_padded(r["cost"].copy()), dtype=np.int64)
        pairs = pairs.reshape(-1, 2)
        if r.get("shortcut"):
            shortcuts += 1
            pairs = pairs[r["iou"][pairs[:, 0], pairs[:, 1]] > thr]
            pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
        else:
            solved += 1
        assert np.array_equal(pairs, r["matched"]), f
    assert solved > 0
    print(f"{name}: {solved} frames solved, {shortcuts} took the unique-match shortcut")
