"""CPU: the StrongSORT restatement (tests/strongsort_oracle.py) against SciPy's solver and against
the reference's goldens (tests/golden/strongsort_synth.npz, made by
tests/golden/make_goldens_strongsort.py), and the plugin surface that needs no device."""
import os

import numpy as np
import pytest

import strongsort_big as big
import strongsort_oracle as so
from conftest import GOLDEN

SHAPES = [(1, 1), (3, 5), (5, 3), (13, 13), (17, 64)]


def clamped_cases(nr, nc, seed):
    """Cost matrices as min_cost_matching hands them to the solver: random costs clamped at
    max_distance + 1e-5, with all-clamped rows and an all-clamped matrix among them."""
    rng = np.random.default_rng(seed)
    top = 0.2 + 1e-5
    out = []
    for frac in (0.3, 0.6, 0.9):
        c = rng.random((nr, nc)) * 0.2 / (1 - frac)
        c[c > 0.2] = top
        out.append(c)
    c = rng.random((nr, nc)) * 0.25
    c[c > 0.2] = top
    c[rng.random(nr) < 0.5] = top                  # hopeless rows
    c[0] = top
    out.append(c)
    c = rng.random((nr, nc)) * 0.25
    c[c > 0.2] = top
    c[:, rng.random(nc) < 0.5] = top               # hopeless columns
    out.append(c)
    out.append(np.full((nr, nc), top))             # all clamped
    q = np.round(rng.random((nr, nc)) * 4) / 4     # few distinct values: ties everywhere
    out.append(q)
    return out


# above the device solver's block size (512), where the GPU tests lean on the restatement
BIG_SHAPES = [(513, 513), (700, 600), (600, 700)]


@pytest.mark.parametrize("shape", SHAPES + BIG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lsa_replay_equals_scipy(shape):
    scipy_optimize = pytest.importorskip("scipy.optimize")
    if shape in BIG_SHAPES:
        for k, quant in ((3, 0), (3, 8), (12, 4)):
            c = big.sparse_clamped(*shape, seed=100 * k + quant, k=k, quant=quant)
            r, q = scipy_optimize.linear_sum_assignment(c)
            assert big.is_decisive(c, r, q), (shape, k, quant)   # the ties place the pairs
            r2, q2 = so.lsa_replay(c)
            assert np.array_equal(r, r2) and np.array_equal(q, q2), (shape, k, quant)
        return
    for seed in range(6):
        for c in clamped_cases(*shape, seed):
            r, k = scipy_optimize.linear_sum_assignment(c)
            r2, k2 = so.lsa_replay(c)
            assert np.array_equal(r, r2) and np.array_equal(k, k2), (shape, seed, c)


@pytest.mark.parametrize("shape", big.GALLERY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nn_cosine_min_against_float64(shape):
    """The restatement's pinned float32 order against min(1 - g.f) over float64-normalised rows,
    at the shapes of the GPU test that is bit-exact against the restatement.  Bound (D + 16) *
    2^-24: unit vectors, so each of the D fma steps rounds a partial sum of magnitude <= 1 (half
    an ulp of 1 = 2^-24 at most), plus a few roundings for the two normalisations and 1 - dot."""
    T, B, D, M = shape
    gal, lens, feats, _ = big.gallery_case(*shape)
    got = so.nn_cosine_min(gal, lens, feats)
    err = float(np.abs(got.astype(np.float64) - big.nn_cosine_min_f64(gal, lens, feats)).max())
    print(f"nn_cosine_min {shape}: max |float32 order - float64| = {err:.3g}, "
          f"bound {(D + 16) * 2.0 ** -24:.3g}")
    assert err <= (D + 16) * 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "strongsort_synth.npz")) as z:
        return {k: z[k] for k in z.files}


def test_goldens_cover_the_paths(golden):
    names = [str(s) for s in golden["streams"]]
    assert names == ["a", "b", "c", "y"]
    for name in "abc":
        p, frames, rows = so.golden_stream(golden, name)
        assert len(frames) >= 40 and max(len(d) for d, _, _ in frames) <= 40
        assert frames[0][1].shape[1] == 32 and p["nn_budget"] == 5 and p["max_age"] == 5
        assert any(len(d) == 0 for d, _, _ in frames[1:])            # a frame without detections
        assert any(not np.array_equal(w, np.eye(2, 3)) for _, _, w in frames)
        ids = np.concatenate([r[:, 4] for r in rows])
        last = rows[-1][:, 4]
        assert len(set(ids.tolist()) - set(last.tolist())) > 0         # tracks ended
    assert so.golden_stream(golden, "b")[0]["n_init"] == 3
    assert len(so.golden_stream(golden, "b")[1][0][0]) == 0           # starts with no track at all
    # recorded solver problems: clamped ties, rows > columns and rows < columns
    shapes = golden["kat_shapes"]
    assert len(shapes) >= 8 and np.any(shapes[:, 0] > shapes[:, 1]) and np.any(
        shapes[:, 0] < shapes[:, 1])


@pytest.mark.parametrize("name", ["a", "b", "c", "y"])
def test_restatement_matches_goldens(golden, name):
    p, frames, rows = so.golden_stream(golden, name)
    got, _ = so.run_oracle(p, frames)
    for f, (g, e) in enumerate(zip(got, rows)):
        assert g.shape == e.shape, f"frame {f}"
        assert np.array_equal(g[:, 4:], e[:, 4:]), f"frame {f}: id / conf / cls / det_ind"
        assert np.allclose(g[:, :4], e[:, :4], rtol=1e-9, atol=0), f"frame {f}: boxes"


def test_recorded_solver_problems(golden):
    off = oc = 0
    for nr, nc in golden["kat_shapes"]:
        c = golden["kat_cost"][off:off + nr * nc].reshape(nr, nc)
        k = min(nr, nc)
        r, q = so.lsa_replay(c)
        assert np.array_equal(r, golden["kat_rows"][oc:oc + k])
        assert np.array_equal(q, golden["kat_cols"][oc:oc + k])
        off += nr * nc
        oc += k


def test_plugin_surface():
    import boxmot
    import yolo_tracking_amd as y
    from boxmot.trackers.strongsort.strong_sort import StrongSORT
    assert StrongSORT is y.StrongSORT and boxmot.StrongSORT is y.StrongSORT
    with pytest.raises(ValueError):
        y.StrongSORT(None, 0, False, nn_budget=None)
    with pytest.raises(ValueError):
        y.StrongSortEngine(1, nn_budget=None)
    for name in ("yta_strongsort_create", "yta_strongsort_update", "yta_strongsort_update_device",
                 "yta_strongsort_get_state", "yta_lsa_replay", "yta_nn_cosine_min",
                 "yta_kf_nsa_update", "yta_kf_xyah_gating"):
        assert name in y._lib.EXPORTED_SYMBOLS


def test_fmaf_is_a_single_rounding():
    """The float32 fma the restatement chains (the MFMA's numerics) against exact rational
    arithmetic, on operands chosen to sit on float32 rounding boundaries."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(300).astype(np.float32)
    b = rng.standard_normal(300).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)   # heavy cancellation
    c[::3] = rng.standard_normal(100).astype(np.float32)
    # ties of the double-rounded sum: c = 1, a * b = 2^-24 + 2^-60 (just above half an ulp)
    a = np.concatenate([a, np.float32([2.0 ** -12 + 2.0 ** -35])])
    b = np.concatenate([b, np.float32([2.0 ** -12])])
    c = np.concatenate([c, np.float32([1.0])])
    got = so.fmaf(a, b, c)
    for x, y_, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y_)) + Fraction(float(z))
        lo = np.float32(float(exact))        # float(Fraction) is correctly rounded to float64
        # round the exact value to float32 directly: compare the two neighbours
        cand = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cand, key=lambda v: (abs(Fraction(float(v)) - exact),
                                        int(np.float32(v).view(np.uint32)) & 1))
        assert g == best, (x, y_, z)
