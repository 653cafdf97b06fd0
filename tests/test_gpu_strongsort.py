"""GPU: StrongSORT on the device (csrc/strongsort.hip, csrc/lsa_replay.hpp through the C ABI)
against its restatement (tests/strongsort_oracle.py), bit for bit, and against the reference's
goldens (tests/golden/strongsort_synth.npz: ids / conf / cls / det_ind exact, boxes 1e-9); above
one block, one tile and one loop trip on the inputs of tests/strongsort_big.py, with SciPy itself
as the solver's reference."""
import os

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import strongsort_big as big
import strongsort_oracle as so
from conftest import GOLDEN
from yolo_tracking_amd import _lib

pytestmark = pytest.mark.gpu

STREAMS = ["a", "b", "c"]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "strongsort_synth.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(golden):
    """name -> (params, frames, golden rows, restatement rows, restatement tracker); computed
    once and left unchanged."""
    out = {}
    for name in STREAMS + ["y"]:
        p, frames, rows = so.golden_stream(golden, name)
        got, orc = so.run_oracle(p, frames)
        out[name] = (p, frames, rows, got, orc)
    return out


# ------------------------------------------------------------------------------------- solver
def test_lsa_replay_recorded_scipy_results(golden):
    off = oc = 0
    for nr, nc in golden["kat_shapes"]:
        c = golden["kat_cost"][off:off + nr * nc].reshape(nr, nc)
        k = min(nr, nc)
        r, q = _lib.lsa_replay(c)
        assert np.array_equal(r, golden["kat_rows"][oc:oc + k]), (nr, nc)
        assert np.array_equal(q, golden["kat_cols"][oc:oc + k]), (nr, nc)
        off += nr * nc
        oc += k


def _clamped(nr, nc, seed, frac):
    rng = np.random.default_rng(seed)
    c = rng.random((nr, nc)) * 0.2 / (1 - frac)
    c[c > 0.2] = 0.2 + 1e-5
    return c


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (64, 17), (130, 130)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_lsa_replay_against_restatement(shape):
    nr, nc = shape
    cases = [_clamped(nr, nc, 1, 0.5), _clamped(nr, nc, 2, 0.9), np.full((nr, nc), 0.7 + 1e-5)]
    c = _clamped(nr, nc, 3, 0.7)
    c[::3] = 0.2 + 1e-5                                    # hopeless rows
    cases.append(c)
    for c in cases:
        r, q = _lib.lsa_replay(c)
        er, eq = so.lsa_replay(c)
        assert np.array_equal(r, er) and np.array_equal(q, eq), shape


# ---------------------------------------------------------------- solver above one block (512)
# Every thread of lsa_replay_block takes several trips of the relax / select, init and dual-update
# loops and merges candidates into its own (value, rank) key before the butterfly; from 1365 rows
# or columns on the work arrays need the opt-in dynamic LDS.
BIG_SHAPES = [(513, 513), (600, 700), (700, 600), (1100, 900), (1000, 1600), (3072, 3072)]
KQ = [(3, 0), (3, 8), (12, 4)]


def _solver_case(c, decisive=True):
    """The device against SciPy itself and, up to 1100 x 900, against the restatement.  With
    `decisive` the expected answer must have been placed by the tie-breaking rule
    (strongsort_big.is_decisive)."""
    refs = [linear_sum_assignment(c)]
    if max(c.shape) <= 1100:
        refs.append(so.lsa_replay(c))
    r, q = _lib.lsa_replay(c)
    for er, eq in refs:
        if decisive:
            assert big.is_decisive(c, er, eq), c.shape
        assert np.array_equal(r, er), c.shape
        assert np.array_equal(q, eq), (c.shape, int((q != eq).sum()))


@pytest.mark.parametrize("shape,kq", [(s, kq) for s in BIG_SHAPES for kq in KQ
                                      if s[0] < 3072 or kq[0] == 3],    # 3072: k = 3 only
                         ids=lambda v: f"{v[0]}x{v[1]}")
def test_lsa_replay_sparse_clamped(shape, kq):
    k, quant = kq
    _solver_case(big.sparse_clamped(*shape, seed=100 * k + quant, k=k, quant=quant))


@pytest.mark.parametrize("shape", [(700, 600), (600, 700)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lsa_replay_structured(shape):
    _solver_case(big.last_columns(*shape, seed=7))
    _solver_case(big.first_rows_hopeless(*shape, seed=8))
    # all equal: nothing but the tie rule produces the answer, yet SciPy's is the identity, whose
    # columns ascend, so the decisiveness check does not apply to this one case
    _solver_case(np.full(shape, big.TOP), decisive=False)


@pytest.mark.parametrize("shape", [(3073, 4), (4, 3073)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_lsa_replay_refuses_more_than_3072(shape):
    with pytest.raises(_lib.YTAError) as e:
        _lib.lsa_replay(np.zeros(shape))
    assert e.value.code == _lib.YTA_ERR_INVALID and "3072" in str(e.value)


def test_lsa_replay_infeasible_then_valid():
    c = big.sparse_clamped(600, 700, seed=5, k=3)
    bad = c.copy()
    bad[301] = np.inf
    with pytest.raises(_lib.YTAError) as e:
        _lib.lsa_replay(bad)
    assert e.value.code == _lib.YTA_ERR_INVALID and "infeasible" in str(e.value)
    r, q = _lib.lsa_replay(c)                     # the next call is not affected
    er, eq = so.lsa_replay(c)
    assert np.array_equal(r, er) and np.array_equal(q, eq)


# -------------------------------------------------------------------- gallery distance, Kalman
@pytest.mark.parametrize("shape", big.GALLERY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nn_cosine_min_across_tiles(shape):
    """More than one block of detections (128), all four waves of a block, gallery lengths on,
    one below and one above the 32-row tile, D off the 16-wide k step; the rows past a track's
    length would win the minimum with cost 0 if they were read."""
    gal, lens, feats, poisoned = big.gallery_case(*shape)
    exp = so.nn_cosine_min(gal, lens, feats)
    assert poisoned and min(exp[t, j] for t, j in poisoned) > 0.1
    got = _lib.nn_cosine_min(gal, lens, feats)
    assert got.dtype == np.float32 and got.shape == exp.shape
    bad = np.argwhere(got != exp)
    assert len(bad) == 0, (shape, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("D", [1, 96, 512])
@pytest.mark.parametrize("B", [1, 7, 100])
def test_nn_cosine_min_bit_exact(B, D):
    rng = np.random.default_rng(100 * B + D)
    T, M = 3, 5
    gal = rng.standard_normal((T, B, D)).astype(np.float32)
    feats = (rng.standard_normal((M, D)) * rng.uniform(0.5, 3, (M, 1))).astype(np.float32)
    if D > 1:
        feats[1] = gal[0, B // 2] * np.float32(1.7) + np.float32(0.01) * feats[1]   # a near match
    lens = np.array([B, max(1, B // 2), B], np.int32)
    gal[2, :] = gal[2, 0]                                   # a gallery of duplicates
    gal[1, lens[1]:] = np.nan                               # rows past the length are not read
    got = _lib.nn_cosine_min(gal, lens, feats)
    exp = so.nn_cosine_min(gal, lens, feats)
    assert got.dtype == np.float32 and np.array_equal(got, exp)


def _kf_states(n, seed):
    """States a few predicts / updates into their life (block-structured covariances)."""
    rng = np.random.default_rng(seed)
    ms, Ps = [], []
    for _ in range(n):
        z = np.array([rng.uniform(100, 1800), rng.uniform(100, 1000), rng.uniform(0.3, 0.8),
                      rng.uniform(60, 300)])
        m, P = so.kf_initiate(z)
        for _ in range(rng.integers(1, 5)):
            m, P = so.kf_predict(m, P)
            m, P = so.kf_nsa_update(m, P, z + rng.normal(0, 2, 4) * [1, 1, 0.001, 1], 0.4)
        m, P = so.kf_predict(m, P)
        ms.append(m)
        Ps.append(P)
    return np.stack(ms), np.stack(Ps)


@pytest.mark.parametrize("conf", [0.0, 0.5, 0.999])
def test_kf_nsa_update_kat(conf):
    m, P = _kf_states(9, 4)
    rng = np.random.default_rng(5)
    z = m[:, :4] + rng.normal(0, 3, (9, 4)) * [1, 1, 0.002, 1]
    gm, gP = _lib.kf_nsa_update(m, P, z, conf)
    for i in range(9):
        em, eP = so.kf_nsa_update(m[i], P[i], z[i], conf)
        assert np.array_equal(gm[i], em) and np.array_equal(gP[i], eP), i


def test_kf_gating_kat():
    m, P = _kf_states(7, 6)
    rng = np.random.default_rng(7)
    zs = np.concatenate([m[:, :4] + rng.normal(0, 4, (7, 4)) * [1, 1, 0.002, 1],
                         m[:3, :4] + [300, -200, 0.1, 40]])
    got = _lib.kf_xyah_gating(m, P, zs)
    for i in range(7):
        assert np.array_equal(got[i], so.kf_gating(m[i], P[i], zs)), i
    assert (got < so.CHI2INV95_4).any() and (got > so.CHI2INV95_4).any()


# --------------------------------------------------------------------------------------- engine
def _engine(n_streams, p, D=32, cap=96, maxd=48):
    from yolo_tracking_amd import StrongSortEngine
    return StrongSortEngine(n_streams, feat_dim=D, device=0, track_capacity=cap, max_dets=maxd, **p)


def _check_state(eng, stream, orc):
    st = eng.state(stream)
    assert np.array_equal(st["id"], [t.id for t in orc.tracks])
    assert np.array_equal(st["hits"], [t.hits for t in orc.tracks])
    assert np.array_equal(st["age"], [t.age for t in orc.tracks])
    assert np.array_equal(st["time_since_update"], [t.tsu for t in orc.tracks])
    assert np.array_equal(st["state"], [2 if t.confirmed else 1 for t in orc.tracks])
    for k, t in enumerate(orc.tracks):
        assert np.array_equal(st["mean"][k], t.mean), k
        assert np.array_equal(st["covariance"][k], t.cov), k
        assert np.array_equal(st["feat"][k], t.feat), k
        n = st["gallery_len"][k]
        assert n == len(t.gallery)
        if n:   # the ring keeps the same rows in another order
            a = st["gallery"][k][:n]
            assert np.array_equal(a[np.lexsort(a.T)], t.gallery[np.lexsort(t.gallery.T)]), k


def _run_single(eng, frames, exp_rows, gold_rows):
    for f, (d, ft, w) in enumerate(frames):
        warp = [w] if eng.n_tracks()[0] >= 1 else None
        got = eng.update([d], [ft], warp)[0]
        assert got.shape == exp_rows[f].shape and np.array_equal(got, exp_rows[f]), f"frame {f}"
        e = gold_rows[f]
        assert np.array_equal(got[:, 4:], e[:, 4:]), f"frame {f}: golden ids"
        assert np.allclose(got[:, :4], e[:, :4], rtol=1e-9, atol=0), f"frame {f}: golden boxes"


@pytest.mark.parametrize("name", STREAMS)
def test_engine_one_stream_bit_exact_and_after_reset(runs, name):
    p, frames, rows, exp, orc = runs[name]
    eng = _engine(1, p)
    _run_single(eng, frames, exp, rows)
    _check_state(eng, 0, orc)
    eng.reset()                                   # ids restart at 1, galleries are empty
    assert eng.n_tracks()[0] == 0 and len(eng.state(0)["id"]) == 0
    _run_single(eng, frames[:12], exp, rows)


def test_engine_three_streams_in_one_engine(runs):
    """S = 3 in the same launches; the streams have different lengths (a finished stream gets
    empty frames), the shared hyper-parameters are stream a's."""
    p = runs["a"][0]
    names = ["a", "b", "c"]
    streams = []
    for n in names:
        frames = runs[n][1]
        if runs[n][0] == p:
            exp = runs[n][3]
        else:                                     # other golden parameters: restate under a's
            exp = so.run_oracle(p, frames)[0]
        streams.append((frames, exp))
    nf = max(len(fr) for fr, _ in streams)
    eng = _engine(3, p)
    for f in range(nf):
        dets, feats, warps = [], [], []
        nt = eng.n_tracks()
        for s, (frames, _) in enumerate(streams):
            d, ft, w = frames[f] if f < len(frames) else (np.zeros((0, 6)),
                                                          np.zeros((0, 32), np.float32), None)
            dets.append(d)
            feats.append(ft)
            warps.append(w if nt[s] >= 1 else None)
        got = eng.update(dets, feats, warps)
        for s, (frames, exp) in enumerate(streams):
            if f < len(frames):
                assert np.array_equal(got[s], exp[f]), (names[s], f)
            else:
                assert len(got[s]) == 0, (names[s], f)   # no detection, no output row
    assert eng.n_tracks().tolist() == [len(eng.state(s)["id"]) for s in range(3)]


# ------------------------------------------------------------------------------ engine at size
@pytest.fixture(scope="module")
def bigrun():
    """The restatement over strongsort_big's stream (shared with the tensor-path tests); its
    property assertions (both stage-1 orientations and a stage 2 above 512, more than 256 births,
    deletions beside births, hopeless rows) run inside."""
    return big.big_run()


def _big_engine(n_streams):
    return _engine(n_streams, big.BIG_P, D=big.BIG_D, cap=big.BIG_CAP, maxd=big.BIG_CAP)


def test_engine_big_stream_bit_exact(bigrun):
    eng = _big_engine(1)
    for again, frames in enumerate((bigrun.frames, bigrun.frames[:3])):
        for f, (d, ft, w) in enumerate(frames):
            got = eng.update([d], [ft], [w] if eng.n_tracks()[0] >= 1 else None)[0]
            exp = bigrun.rows[f]
            assert got.shape == exp.shape, (again, f, got.shape, exp.shape)
            assert np.array_equal(got, exp), (again, f, np.argwhere(got != exp)[:4].tolist())
            assert eng.n_tracks()[0] == bigrun.ntrk[f], (again, f)
        if not again:
            _check_state(eng, 0, bigrun.oracle)
            eng.reset()
            assert eng.n_tracks()[0] == 0 and len(eng.state(0)["id"]) == 0


def test_engine_big_stream_two_streams(bigrun):
    """S = 2: stream 1 is the same stream two frames late (empty frames first), so at every
    launch the two streams are at different sizes; ids restart per stream.  A wrong s * CAP *
    MAXD stride lands inside the other stream's data at this size, and with max_dets below
    track_capacity so does one stride taken for the other."""
    fr, nf, lag = bigrun.frames, len(bigrun.frames), 2
    empty = (np.zeros((0, 6)), np.zeros((0, big.BIG_D), np.float32), None)
    maxd = 768
    assert 512 < max(len(d) for d, _, _ in fr) <= maxd < big.BIG_CAP
    eng = _engine(2, big.BIG_P, D=big.BIG_D, cap=big.BIG_CAP, maxd=maxd)
    for f in range(nf + lag):
        at = (f, f - lag)
        ins = [fr[g] if 0 <= g < nf else empty for g in at]
        nt = eng.n_tracks()
        got = eng.update([d for d, _, _ in ins], [ft for _, ft, _ in ins],
                         [w if w is not None and nt[s] >= 1 else None
                          for s, (_, _, w) in enumerate(ins)])
        for s, g in enumerate(at):
            if 0 <= g < nf:
                assert np.array_equal(got[s], bigrun.rows[g]), (s, g)
                assert eng.n_tracks()[s] == bigrun.ntrk[g], (s, g)
            else:
                assert len(got[s]) == 0, (s, g)              # no detection, no output row
        if f == nf - 1:
            _check_state(eng, 0, bigrun.oracle)
    _check_state(eng, 1, bigrun.oracle)


def test_engine_at_the_solver_limit(runs):
    """track_capacity = max_dets = 3072: k_ss_match runs with the solver's largest work arrays
    (about 147 KB of opt-in dynamic LDS); the answers are stream a's."""
    p, frames, rows, exp, orc = runs["a"]
    eng = _engine(1, p, cap=3072, maxd=3072)
    assert eng.capacity() == (3072, 3072)
    _run_single(eng, frames, exp, rows)
    _check_state(eng, 0, orc)


class _FakeReID:
    """get_features(xyxys, img) serving the golden feature rows of the current frame."""

    def __init__(self, frames):
        self.frames = frames
        self.f = 0

    def get_features(self, xyxys, img):
        d, ft, _ = self.frames[self.f]
        assert np.array_equal(np.asarray(xyxys), d[:, :4])
        return ft


class _ScriptedCMC:
    def __init__(self, frames, reid):
        self.frames, self.reid, self.calls = frames, reid, 0

    def apply(self, img, dets):
        self.calls += 1
        return self.frames[self.reid.f][2]


def test_create_tracker_against_goldens(runs):
    from yolo_tracking_amd import StrongSORT, create_tracker, get_tracker_config
    p, frames, rows, exp, _ = runs["y"]
    reid = _FakeReID(frames)
    trk = create_tracker("strongsort", get_tracker_config("strongsort"), reid, "cuda:0", False,
                         False)
    assert isinstance(trk, StrongSORT) and trk.model is reid
    trk.cmc = cmc = _ScriptedCMC(frames, reid)
    img = np.zeros((8, 8, 3), np.uint8)
    with_tracks = 0
    for f, (d, _, _) in enumerate(frames):
        reid.f = f
        with_tracks += trk.tracks is not None and len(trk.tracks["id"]) >= 1
        got = trk.update(d, img)
        got = np.asarray(got, dtype=np.float64).reshape(-1, 8)
        assert np.array_equal(got, exp[f]), f"frame {f}"
        assert np.array_equal(got[:, 4:], rows[f][:, 4:]), f"frame {f}"
        assert np.allclose(got[:, :4], rows[f][:, :4], rtol=1e-9, atol=0), f"frame {f}"
    assert cmc.calls == with_tracks < len(frames)   # strong_sort.py:62: only with >= 1 track
    assert trk.update(np.zeros((0, 6)), img).shape == (0,)      # strong_sort.py:99


def test_real_ecc_against_the_ecc_oracle():
    """The drop-in with its own ECC (device) against the restatement fed oracle.cmc_ecc's warps."""
    import cmc_frames
    from oracle import cmc_ecc as ce
    from yolo_tracking_amd import StrongSORT
    h, w, n, D = 240, 320, 7, 16
    imgs, _ = cmc_frames.sequence(h, w, n, seed=3)
    rng = np.random.default_rng(9)
    base = rng.standard_normal((4, D)).astype(np.float32)
    box = np.array([[30, 40, 90, 160], [150, 60, 200, 190], [220, 20, 300, 150],
                    [100, 120, 170, 230]], dtype=np.float64)
    frames = []
    for f in range(n):
        b = box + [6.0 * f, -4.0 * f, 6.0 * f, -4.0 * f]
        d = np.concatenate([b, rng.uniform(0.4, 0.95, (4, 1)), np.zeros((4, 1))], axis=1)
        frames.append((d, base + np.float32(0.02) * rng.standard_normal((4, D)).astype(np.float32)))
    reid = _FakeReID([(d, ft, None) for d, ft in frames])
    trk = StrongSORT(reid, "cuda:0", False, n_init=2, nn_budget=3, max_age=3)
    orc = so.StrongSortOracle(n_init=2, nn_budget=3, max_age=3)
    ecc = ce.ECCOracle()
    rows = 0
    for f, (d, ft) in enumerate(frames):
        reid.f = f
        warp = np.asarray(ecc.apply(imgs[f], None), np.float64) if orc.has_tracks() else None
        exp = orc.update(d, ft, warp)
        got = np.asarray(trk.update(d, imgs[f]), dtype=np.float64).reshape(-1, 8)
        assert np.array_equal(got, exp), f"frame {f}"
        rows += len(got)
    assert rows >= 4 * (n - 2)


def test_create_refuses_a_gallery_larger_than_the_device():
    from yolo_tracking_amd import StrongSortEngine
    with pytest.raises(_lib.YTAError) as e:
        StrongSortEngine(64, feat_dim=2048, nn_budget=4096, track_capacity=3072, max_dets=64)
    assert e.value.code == _lib.YTA_ERR_NOMEM and "galleries need" in str(e.value)
    eng = StrongSortEngine(1, feat_dim=8, nn_budget=2, track_capacity=4, max_dets=4)   # still usable
    assert eng.capacity() == (4, 4)


def test_capacity_error_and_odd_feature_width():
    """D = 8 takes the guarded (non-float4) loads of the gallery product; more tracks than
    track_capacity is a CapacityError, and the engine works again after reset."""
    from yolo_tracking_amd import StrongSortEngine
    p = dict(max_dist=0.2, max_iou_dist=0.7, max_age=2, n_init=1, nn_budget=2, mc_lambda=0.995,
             ema_alpha=0.9)
    rng = np.random.default_rng(21)
    base = rng.standard_normal((3, 8)).astype(np.float32)
    box = np.array([[10, 10, 50, 90], [200, 40, 260, 160], [400, 300, 470, 420]], dtype=np.float64)

    def frame(f):
        d = np.concatenate([box + 2.0 * f, np.full((3, 1), 0.8), np.zeros((3, 1))], axis=1)
        return d, base + np.float32(0.01) * rng.standard_normal((3, 8)).astype(np.float32)

    frames = [frame(f) for f in range(5)]
    eng = StrongSortEngine(1, feat_dim=8, track_capacity=4, max_dets=8, **p)
    for _ in range(2):
        orc = so.StrongSortOracle(**p)
        for d, ft in frames:
            assert np.array_equal(eng.update([d], [ft])[0], orc.update(d, ft))
        assert len(eng.state(0)["id"]) == 3
        far = np.concatenate([box[:2] + 700.0, box + 1200.0])       # five new objects
        d = np.concatenate([far, np.full((5, 1), 0.8), np.zeros((5, 1))], axis=1)
        with pytest.raises(_lib.CapacityError):
            eng.update([d], [rng.standard_normal((5, 8)).astype(np.float32)])
        eng.reset()
