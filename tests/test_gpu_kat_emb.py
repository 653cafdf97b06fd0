"""Known-answer tests of the appearance-cost primitives the engines use (cost_cosine,
aw_metric), through the C ABI.

* yta_embedding_distance (matching.py:145-167, the BoT-SORT engine's cosine_dist16) against SciPy's
  own cdist(..., 'cosine') — the reference's call: float64 over float32 rows, within EMB_ATOL (the
  dot products are summed in a different order than SciPy's loop).
* yta_aw_max_metric (association.py:79-108, the DeepOCSORT engine's top2_push / aw_weight) against
  oracle/deepocsort.aw_max_metric: bit-exact (top-2 selection is order-free and the weight
  expression is the reference's).

These are kat.hip's stand-alone kernels (k_emb_dist, k_aw_weights, k_aw_apply): serial, one thread
per row or column, sharing only top2_push, aw_weight and cosine_dist16 with the engines.  The
kernels the engines run (k_doc_emb, k_doc_emb_pairs, k_doc_aw, k_doc_aw_cols, k_doc_final,
k_doc_cost, k_oc_cost, k_hs_emb) are compared entry by entry in tests/test_gpu_oc_costs.py."""
import numpy as np
import pytest
from scipy.spatial.distance import cdist

from oracle.deepocsort import aw_max_metric as aw_oracle
from yolo_tracking_amd import _lib

pytestmark = pytest.mark.gpu

EMB_ATOL = 1e-12


@pytest.mark.parametrize("n,m,d", [(1, 1, 512), (7, 13, 512), (64, 33, 128), (5, 3, 1), (40, 40, 17)])
def test_embedding_distance(n, m, d):
    rng = np.random.default_rng(n * 100 + m)
    t = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((m, d)).astype(np.float32)
    if m > 1:
        q[0] = t[0]                 # identical rows: distance 0 (clamped at 0 if slightly < 0)
        q[1] = -t[0]                # opposite: 2
    got = _lib.embedding_distance(t, q)
    exp = np.maximum(0.0, cdist(t, q, "cosine"))
    np.testing.assert_allclose(got, exp, rtol=0, atol=EMB_ATOL)
    assert (got >= 0).all()
    assert _lib.embedding_distance(np.zeros((0, d), np.float32), q).shape == (0, m)


@pytest.mark.parametrize("shape", [(1, 5), (5, 1), (2, 2), (30, 17), (128, 200)])
def test_aw_max_metric_bit_exact(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    e = rng.uniform(-0.3, 1.0, shape)
    e[rng.random(shape) < 0.2] = 0.0                       # emb[iou <= 0] = 0 in the caller
    if shape[0] > 2 and shape[1] > 2:
        e[1, :] = 0.0                                       # all-zero row: weight 0
        e[2, 0] = e[2, 1] = e[2].max() + 0.5                # tied maximum: second == top
        e[:, 2] = -0.25                                     # negative column
    for w, bottom in [(0.5, 0.5), (0.75, 0.2)]:
        got = _lib.aw_max_metric(e, w, bottom)
        exp = aw_oracle(e, w, bottom)
        assert np.array_equal(got, exp), np.abs(got - exp).max()
