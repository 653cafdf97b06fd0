"""GPU: StrongSORT's tensor path (yta_strongsort_update_tensors), stream subsets and per-stream
reset.  Inputs are the golden streams of tests/golden/strongsort_synth.npz and, for frames of
several hundred detections, the stream of tests/strongsort_big.py; the expected values
come from the host-buffer update() of a second engine on the same (cast) values, from the goldens
and from the restatement (tests/strongsort_oracle.py), never from the tensor path itself."""
import ctypes
import os

import numpy as np
import pytest

import strongsort_big as big
import strongsort_oracle as so
from conftest import GOLDEN
from yolo_tracking_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
NAMES = ["a", "b", "c"]
D = 32
NP_DT = {"f64": np.float64, "f32": np.float32, "f16": np.float16}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "strongsort_synth.npz")) as z:
        return {k: z[k] for k in z.files}


def _engine(n_streams, p, feat_dim=D, **kw):
    from yolo_tracking_amd import StrongSortEngine
    kw = dict(dict(track_capacity=96, max_dets=48), **kw)
    return StrongSortEngine(n_streams, feat_dim=feat_dim, device=0, **kw, **p)


def _sequence(golden, names, dt):
    """Per frame, per stream (dets float64 holding the values cast to dt, feats, warp); a stream
    that has ended gets empty frames.  Parameters: stream a's."""
    p = so.golden_stream(golden, "a")[0]
    streams = [so.golden_stream(golden, n)[1] for n in names]
    seq = []
    for f in range(max(len(fr) for fr in streams)):
        row = []
        for fr in streams:
            d, ft, w = fr[f] if f < len(fr) else (np.zeros((0, 6)), np.zeros((0, D), np.float32),
                                                  np.eye(2, 3))
            row.append((d.astype(NP_DT[dt]).astype(np.float64), ft, w))
        seq.append(row)
    return p, seq


def _host_run(p, seq, eng=None):
    """The host-buffer update() over seq -> per-frame rows, per-frame gates (the streams that held
    a track when the frame came in, so got their warp: strong_sort.py:62), the engine."""
    eng = eng or _engine(len(seq[0]), p, feat_dim=seq[0][0][1].shape[1])
    rows, gates = [], []
    for fr in seq:
        g = eng.n_tracks() >= 1
        rows.append(eng.update([d for d, _, _ in fr], [ft for _, ft, _ in fr],
                               [w if g[s] else None for s, (_, _, w) in enumerate(fr)]))
        gates.append(g)
    return rows, gates, eng


@pytest.fixture(scope="module")
def ref(golden):
    """dtype -> (params, seq, rows, gates, final states, final n_tracks) of streams a / b / c in
    one engine run through update(); computed once per dtype and left unchanged."""
    cache = {}

    def get(dt):
        if dt not in cache:
            p, seq = _sequence(golden, NAMES, dt)
            rows, gates, eng = _host_run(p, seq)
            cache[dt] = (p, seq, rows, gates, [eng.state(s) for s in range(3)], eng.n_tracks())
        return cache[dt]
    return get


def _same_state(a, b):
    for k in ("id", "hits", "age", "time_since_update", "state", "mean", "covariance", "feat",
              "gallery_len"):
        if not np.array_equal(a[k], b[k]):
            return False
    return all(np.array_equal(a["gallery"][k][:n], b["gallery"][k][:n])   # rows past n: never set
               for k, n in enumerate(a["gallery_len"]))


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


TORCH_DT = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16}


def _plain(fr, dt):
    return dict(dets=[_t(d, TORCH_DT[dt]) for d, _, _ in fr], feats=[_t(ft) for _, ft, _ in fr])


def _host_warps(fr, gate):
    return [w if gate[s] else None for s, (_, _, w) in enumerate(fr)]


def _dev_warps(fr, gate):
    w = np.stack([w if gate[s] else np.full((2, 3), np.nan) for s, (_, _, w) in enumerate(fr)])
    return _t(w)


def _check_frame(out, exp, tag):
    rows, off, rs = (t.cpu().numpy() for t in out)
    counts = [len(e) for e in exp]
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(counts)])), tag
    for s, e in enumerate(exp):
        assert np.array_equal(rows[off[s]:off[s + 1]], e), (tag, s)
    exp_rs = np.full(len(rs), -1, np.int32)
    exp_rs[:off[-1]] = np.repeat(np.arange(len(exp)), counts)
    assert np.array_equal(rs, exp_rs), tag


def _tensor_run(eng, seq, rows, gates, dt="f64", layout=_plain, warps=_host_warps):
    for f, fr in enumerate(seq):
        out = eng.update_tensors(warps=warps(fr, gates[f]), **layout(fr, dt))
        _check_frame(out, rows[f], f"frame {f}")


# --------------------------------------------------------------------------- 1. parity per dtype
@pytest.mark.parametrize("dt", ["f64", "f32", "f16"])
def test_parity_per_dtype(golden, ref, dt):
    p, seq, rows, gates, states, _ = ref(dt)
    eng = _engine(3, p)
    _tensor_run(eng, seq, rows, gates, dt)
    for s in range(3):
        assert _same_state(eng.state(s), states[s]), s
    if dt == "f64":   # and the reference's own rows, for the streams recorded under these params
        checked = 0
        for s, n in enumerate(NAMES):
            gp, _, grows = so.golden_stream(golden, n)
            if gp != p:
                continue
            checked += 1
            for f, e in enumerate(grows):
                got = rows[f][s]
                assert np.array_equal(got[:, 4:], e[:, 4:]), (n, f)
                assert np.allclose(got[:, :4], e[:, :4], rtol=1e-9, atol=0), (n, f)
        assert checked >= 1


# --------------------------------------------------------------------------- 2. awkward layouts
def _packed(fr, dt):
    return dict(dets=torch.cat([_t(d, TORCH_DT[dt]) for d, _, _ in fr]),
                feats=torch.cat([_t(ft) for _, ft, _ in fr]), counts=[len(d) for d, _, _ in fr])


def _wide9(fr, dt):
    a = _packed(fr, dt)
    wide = torch.full((len(a["dets"]), 9), float("nan"), dtype=TORCH_DT[dt], device=DEV)
    wide[:, 2:8] = a["dets"]
    return dict(a, dets=wide[:, 2:8])


def _featpad(fr, dt):
    a = _packed(fr, dt)
    wide = torch.full((len(a["feats"]), D + 3), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, 1:D + 1] = a["feats"]
    return dict(a, feats=wide[:, 1:D + 1])


def _offset1(fr, dt):
    """Views one element into their buffers: 8-B but not 16-B aligned float64, 2-B aligned
    float16, 4-B aligned features."""
    a = _packed(fr, dt)
    n = len(a["dets"])
    buf = torch.full((6 * n + 1,), float("nan"), dtype=TORCH_DT[dt], device=DEV)
    fbuf = torch.full((D * n + 1,), float("nan"), dtype=torch.float32, device=DEV)
    dets, feats = buf[1:].view(n, 6), fbuf[1:].view(n, D)
    dets.copy_(a["dets"])
    feats.copy_(a["feats"])
    assert n == 0 or dets.data_ptr() % 16 != 0 or dt != "f64"
    return dict(a, dets=dets, feats=feats)


@pytest.mark.parametrize("layout,dt", [(_packed, "f64"), (_wide9, "f64"), (_wide9, "f16"),
                                       (_featpad, "f32"), (_offset1, "f64"), (_offset1, "f16")],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_awkward_layouts(ref, layout, dt):
    p, seq, rows, gates, states, _ = ref(dt)
    eng = _engine(3, p)
    _tensor_run(eng, seq, rows, gates, dt, layout=layout)
    for s in range(3):
        assert _same_state(eng.state(s), states[s]), s
    assert eng.tensor_stats()["frames"] == len(seq)


# ---------------------------------------------------------------------------- 2b. a big frame
@pytest.fixture(scope="module")
def bigrun():
    """strongsort_big's stream and the restatement's run over it (computed once per process and
    shared with test_gpu_strongsort.py)."""
    return big.big_run()


def _wide_and_padded(fr, dt):
    """dets a column slice of a 9-wide tensor, feats packed rows three floats wider than D."""
    a = _packed(fr, dt)
    n, fd = a["feats"].shape
    wide = torch.full((n, 9), float("nan"), dtype=TORCH_DT[dt], device=DEV)
    wide[:, 2:8] = a["dets"]
    fw = torch.full((n, fd + 3), float("nan"), dtype=torch.float32, device=DEV)
    fw[:, 1:fd + 1] = a["feats"]
    return dict(a, dets=wide[:, 2:8], feats=fw[:, 1:fd + 1])


@pytest.mark.parametrize("layout,dt", [(_plain, "f32"), (_plain, "f16"), (_wide_and_padded, "f32")],
                         ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_big_stream_against_update(bigrun, layout, dt):
    """strongsort_big's stream (several hundred detections a frame: with max_dets = 1024
    k_ss_ingest runs 12 chunk blocks a stream) through update_tensors against update() of a second
    engine on the same cast values; update() itself is pinned to the restatement on this stream by
    test_gpu_strongsort.py::test_engine_big_stream_bit_exact."""
    run = bigrun
    kw = dict(feat_dim=big.BIG_D, track_capacity=big.BIG_CAP, max_dets=big.BIG_CAP)
    seq = [[(d.astype(NP_DT[dt]).astype(np.float64), ft, w)] for d, ft, w in run.frames]
    assert all(np.isfinite(fr[0][0]).all() for fr in seq) and max(len(fr[0][0]) for fr in seq) > 512
    rows, gates, host = _host_run(run.p, seq, _engine(1, run.p, **kw))
    assert sum(len(r[0]) for r in rows) > 2000
    eng = _engine(1, run.p, **kw)
    _tensor_run(eng, seq, rows, gates, dt, layout=layout)
    assert np.array_equal(eng.n_tracks(), host.n_tracks()) and host.n_tracks()[0] > 512
    assert _same_state(eng.state(0), host.state(0))
    eng.sync()                                   # no capacity or solver error was left behind


def test_one_stream_and_a_frame_without_any_detection(golden):
    """S = 1 (stream a against its goldens), then S = 3 with a frame in which no stream has a
    detection spliced in."""
    p, frames, grows = so.golden_stream(golden, "a")
    eng = _engine(1, p)
    for f, (d, ft, w) in enumerate(frames):
        warp = [w if eng.n_tracks()[0] >= 1 else None]
        rows, off, rs = eng.update_tensors([_t(d)], [_t(ft)], warps=warp)
        got = rows.cpu().numpy()[:int(off[1])]
        assert np.array_equal(got[:, 4:], grows[f][:, 4:]), f
        assert np.allclose(got[:, :4], grows[f][:, :4], rtol=1e-9, atol=0), f
    p, seq = _sequence(golden, NAMES, "f64")
    empty = [(np.zeros((0, 6)), np.zeros((0, D), np.float32), np.eye(2, 3))] * 3
    seq = seq[:10] + [empty] + seq[10:20]
    rows, gates, host = _host_run(p, seq)
    eng = _engine(3, p)
    _tensor_run(eng, seq, rows, gates)
    assert all(_same_state(eng.state(s), host.state(s)) for s in range(3))


def _small_frames(n, seed=21):
    """test_capacity_error_and_odd_feature_width's three objects with D = 8."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((3, 8)).astype(np.float32)
    box = np.array([[10, 10, 50, 90], [200, 40, 260, 160], [400, 300, 470, 420]], dtype=np.float64)
    frames = []
    for f in range(n):
        d = np.concatenate([box + 2.0 * f, np.full((3, 1), 0.8), np.zeros((3, 1))], axis=1)
        frames.append((d, base + np.float32(0.01) * rng.standard_normal((3, 8)).astype(np.float32)))
    far = np.concatenate([box[:2] + 700.0, box + 1200.0])       # five new objects
    d5 = np.concatenate([far, np.full((5, 1), 0.8), np.zeros((5, 1))], axis=1)
    return frames, (d5, rng.standard_normal((5, 8)).astype(np.float32))


SMALL_P = dict(max_dist=0.2, max_iou_dist=0.7, max_age=2, n_init=1, nn_budget=2, mc_lambda=0.995,
               ema_alpha=0.9)


def test_feature_width_8_takes_the_guarded_loads():
    frames, _ = _small_frames(6)
    eng = _engine(1, SMALL_P, feat_dim=8, track_capacity=4, max_dets=8)
    orc = so.StrongSortOracle(**SMALL_P)
    for d, ft in frames:
        pad = torch.full((3, 11), float("nan"), dtype=torch.float32, device=DEV)
        pad[:, 2:10] = _t(ft)
        rows, off, _ = eng.update_tensors([_t(d, torch.float32)], [pad[:, 2:10]])
        exp = orc.update(d.astype(np.float32).astype(np.float64), ft)
        assert np.array_equal(rows.cpu().numpy()[:int(off[1])], exp)
    assert len(eng.state(0)["id"]) == 3


def test_many_streams():
    """S = 1030: the output-offset scan (one 1024-thread block) gives some threads two streams and
    the last ones none.  Every stream sees 0..3 of its three objects a frame; update_tensors on one
    engine against update() on a second, bit for bit."""
    S, F = 1030, 4
    rng = np.random.default_rng(1030)
    base = rng.standard_normal((3, 8)).astype(np.float32)
    box = np.array([[10, 10, 50, 90], [200, 40, 260, 160], [400, 300, 470, 420]], dtype=np.float64)
    kw = dict(feat_dim=8, track_capacity=8, max_dets=4)
    ten, host = _engine(S, SMALL_P, **kw), _engine(S, SMALL_P, **kw)
    seen, n_rows = np.zeros(S, bool), 0
    for f in range(F):
        counts = rng.integers(0, 4, size=S)
        counts[[0, 1023, 1024, 1029]] = np.maximum(counts[[0, 1023, 1024, 1029]], 1)
        counts[5 + f] = 0   # at least one stream without a detection in every frame
        dets, feats = [], []
        for s in range(S):
            pick = np.sort(rng.permutation(3)[:counts[s]])
            b = box[pick] + 2.0 * f + 0.25 * (s % 7)
            dets.append(np.concatenate([b, np.full((len(pick), 1), 0.8), np.zeros((len(pick), 1))],
                                       axis=1))
            feats.append(base[pick] + np.float32(0.01) *
                         rng.standard_normal((len(pick), 8)).astype(np.float32))
        seen |= counts > 0
        exp = host.update(dets, feats)
        out = ten.update_tensors(_t(np.concatenate(dets)), _t(np.concatenate(feats)),
                                 counts=counts.tolist())
        _check_frame(out, exp, f"frame {f}")   # rows, offsets, row_stream (-1 from offsets[S] on)
        assert int(out[1][S]) == sum(len(e) for e in exp)
        n_rows += int(out[1][S])
        assert np.array_equal(ten.n_tracks(), host.n_tracks()), f
    assert n_rows > 0   # the first frame's births report no row; the later frames do
    assert seen[[0, 1023, 1024, 1029]].all() and (counts == 0).any()
    ten.sync()   # no stream outgrew track_capacity
    assert host.n_tracks().max() <= 8


# ------------------------------------------------------------------------------------- 3. warps
def test_device_warps_with_nan_rows(ref):
    p, seq, rows, gates, states, _ = ref("f64")
    assert any(not g.all() for g in gates) and any(g.any() for g in gates)
    eng = _engine(3, p)
    _tensor_run(eng, seq, rows, gates, warps=_dev_warps)
    for s in range(3):
        assert _same_state(eng.state(s), states[s]), s


# -------------------------------------------------------------------------------------- 4. mask
def test_device_mask_against_update_streams_and_single_engines(golden):
    p, seq = _sequence(golden, NAMES, "f64")
    streams = [[fr[s] for fr in seq] for s in range(3)]
    tens, sub = _engine(3, p), _engine(3, p)
    single = [_engine(1, p) for _ in range(3)]
    pos = [0, 0, 0]
    skipped = 0
    for f in range(30):
        act = [s for s in range(3) if (f + s) % 3 != 0 and (f // 7 + s) % 2 == 0 or f < 2]
        if not act:
            act = [f % 3]
        gate = [single[s].n_tracks()[0] >= 1 for s in range(3)]
        cur = [streams[s][pos[s]] for s in range(3)]   # a skipped stream's rows are offered too
        before = {s: tens.state(s) for s in range(3) if s not in act}
        nid0 = tens.next_ids()
        mask = torch.tensor([int(s in act) for s in range(3)], dtype=torch.int32, device=DEV)
        out = tens.update_tensors([_t(d) for d, _, _ in cur], [_t(ft) for _, ft, _ in cur],
                                  warps=_dev_warps(cur, gate), active=mask)
        exp = [single[s].update([cur[s][0]], [cur[s][1]], [cur[s][2] if gate[s] else None])[0]
               if s in act else np.zeros((0, 8)) for s in range(3)]
        _check_frame(out, exp, f"frame {f}")
        got = sub.update_streams(act[::-1], [cur[s][0] for s in act[::-1]],
                                 [cur[s][1] for s in act[::-1]],
                                 [cur[s][2] if gate[s] else None for s in act[::-1]])
        for k, s in enumerate(act[::-1]):
            assert np.array_equal(got[k], exp[s]), (f, s)
        nid1 = tens.next_ids()
        for s, st in before.items():
            assert _same_state(tens.state(s), st), (f, s)
            assert nid1[s] == nid0[s], (f, s)
            skipped += 1
        for s in act:
            pos[s] += 1
        nt = [single[s].n_tracks()[0] for s in range(3)]
        assert tens.n_tracks().tolist() == nt and sub.n_tracks().tolist() == nt, f
    assert skipped >= 20
    for s in range(3):
        assert _same_state(tens.state(s), single[s].state(0)), s
        assert _same_state(sub.state(s), single[s].state(0)), s
    assert np.array_equal(tens.next_ids(), sub.next_ids())


# ------------------------------------------------------------------------------ 5. reset_stream
def test_reset_stream_mid_run(golden):
    p, seq = _sequence(golden, NAMES, "f64")
    streams = [[fr[s] for fr in seq] for s in range(3)]
    single = [_engine(1, p) for _ in range(3)]
    eng = _engine(3, p)

    def step(cur):
        gate = [single[s].n_tracks()[0] >= 1 for s in range(3)]
        exp = [single[s].update([cur[s][0]], [cur[s][1]], [cur[s][2] if gate[s] else None])[0]
               for s in range(3)]
        _check_frame(eng.update_tensors(warps=_host_warps(cur, gate), **_plain(cur, "f64")), exp,
                     "")
        return exp

    for f in range(15):
        step([streams[s][f] for s in range(3)])
    assert eng.n_tracks()[1] >= 1
    eng.reset_stream(1)
    single[1].reset()
    assert len(eng.state(1)["id"]) == 0 and eng.next_ids()[1] == 1 and eng.n_tracks()[1] == 0
    assert eng.next_ids()[0] > 1 and eng.n_tracks()[0] >= 1
    restated = so.run_oracle(p, streams[1][:12])[0]
    for f in range(12):
        exp = step([streams[0][15 + f], streams[1][f], streams[2][15 + f]])
        assert np.array_equal(exp[1], restated[f]), f   # ids from 1 again, empty galleries
    assert sum(len(r) for r in restated) > 0
    for s in range(3):
        assert _same_state(eng.state(s), single[s].state(0)), s
    with pytest.raises(_lib.YTAError):
        eng.reset_stream(3)


# ---------------------------------------------------------------------------- 6. foreign stream
def test_foreign_stream_without_synchronisation(ref):
    p, seq, rows, gates, states, _ = ref("f32")
    eng = _engine(3, p)
    st = torch.cuda.Stream(device=DEV)
    base = [(_packed(fr, "f32"), _dev_warps(fr, gates[f])) for f, fr in enumerate(seq)]
    torch.cuda.synchronize()
    kept = []
    with torch.cuda.stream(st):
        for a, w in base:
            dets = (a["dets"] * 2.0) * 0.5       # produced on st immediately before the call
            feats = a["feats"] + 0.0
            out = eng.update_tensors(dets, feats, warps=w * 1.0, counts=a["counts"], stream=st)
            kept.append([t.clone() for t in out])   # consumed on st immediately after
    assert eng.tensor_stats()["host_waits"] == 0
    st.synchronize()
    for f, out in enumerate(kept):
        _check_frame(out, rows[f], f"frame {f}")
    for s in range(3):
        assert _same_state(eng.state(s), states[s]), s


# ------------------------------------------------------------------------------ 7. no host wait
def test_no_host_wait(ref):
    p, seq, rows, gates, _, n_tracks = ref("f64")
    eng = _engine(3, p)
    outs = [eng.update_tensors(warps=_dev_warps(fr, gates[f]), **_plain(fr, "f64"))
            for f, fr in enumerate(seq)]
    st = eng.tensor_stats()
    assert st["host_waits"] == 0 and st["frames"] == len(seq) and st["reserves"] == 0
    assert np.array_equal(eng.n_tracks(), n_tracks)
    assert eng.tensor_stats()["host_waits"] == 1
    for f, out in enumerate(outs):
        _check_frame(out, rows[f], f"frame {f}")


# ------------------------------------------------------------------------------- 8. mixed paths
def test_mixed_paths(ref):
    p, seq, rows, gates, states, _ = ref("f64")
    S, CAP, MAXD = 3, 96, 48
    eng = _engine(S, p)
    _tensor_run(eng, seq[:10], rows[:10], gates[:10])
    for f in range(10, 20):
        fr = seq[f]
        got = eng.update([d for d, _, _ in fr], [ft for _, ft, _ in fr], _host_warps(fr, gates[f]))
        assert all(np.array_equal(got[s], rows[f][s]) for s in range(S)), f
    dd = torch.zeros((S, MAXD, 6), dtype=torch.float64, device=DEV)
    ff = torch.zeros((S, MAXD, D), dtype=torch.float32, device=DEV)
    out = torch.zeros((S, CAP, 8), dtype=torch.float64, device=DEV)
    cnt = torch.zeros(S, dtype=torch.int32, device=DEV)
    nout = torch.zeros(S, dtype=torch.int32, device=DEV)
    ones = torch.ones(S, dtype=torch.int32, device=DEV)
    pp = lambda t: ctypes.c_void_p(t.data_ptr())
    for f in range(20, 30):
        fr = seq[f]
        for s, (d, ft, _) in enumerate(fr):
            dd[s, :len(d)] = _t(d)
            ff[s, :len(d)] = _t(ft)
            cnt[s] = len(d)
        w = _dev_warps(fr, gates[f])
        torch.cuda.synchronize()
        _lib.check(eng.lib.yta_strongsort_update_device_masked(
            eng.handle, pp(ones), pp(dd), pp(cnt), pp(ff), pp(w), pp(out), pp(nout), None))
        eng.sync()
        for s in range(S):
            assert np.array_equal(out[s, :int(nout[s])].cpu().numpy(), rows[f][s]), (f, s)
    _tensor_run(eng, seq[30:], rows[30:], gates[30:])
    for s in range(S):
        assert _same_state(eng.state(s), states[s]), s


# --------------------------------------------------------------------------------- 9. refusals
def test_refusals_before_any_launch(ref):
    p, seq, rows, gates, _, _ = ref("f64")
    eng = _engine(3, p)
    _tensor_run(eng, seq[:8], rows[:8], gates[:8])
    fr = seq[8]
    a = _plain(fr, "f64")
    assert all(len(d) >= 2 for d in a["dets"])
    frames0 = eng.tensor_stats()["frames"]
    state0 = [eng.state(s) for s in range(3)]
    ut = eng.update_tensors
    with pytest.raises(ValueError):   # wrong device
        ut([d.cpu() for d in a["dets"]], a["feats"])
    with pytest.raises(ValueError):   # wrong dtype: detections, features
        ut([d.long() for d in a["dets"]], a["feats"])
    with pytest.raises(ValueError):
        ut(a["dets"], [f.double() for f in a["feats"]])
    with pytest.raises(ValueError):   # wrong shape
        ut([d[:, :5] for d in a["dets"]], a["feats"])
    with pytest.raises(ValueError):
        ut(a["dets"], [f[:, :D - 1] for f in a["feats"]])
    with pytest.raises(ValueError):   # feature rows != detection rows
        ut(a["dets"], [a["feats"][0][:-1]] + a["feats"][1:])
    with pytest.raises(ValueError):   # warps of the wrong size
        ut(a["dets"], a["feats"], warps=torch.zeros((2, 6), dtype=torch.float64, device=DEV))
    big = torch.cat([a["dets"][0]] * 30)[:49]   # above max_dets = 48
    with pytest.raises(_lib.CapacityError):
        ut([big] + a["dets"][1:], [torch.zeros((49, D), device=DEV)] + a["feats"][1:])
    # rows_capacity below the frame's detections (raw ctypes: update_tensors sizes its own rows)
    pk = _packed(fr, "f64")
    n = len(pk["dets"])
    out = torch.empty((n, 8), dtype=torch.float64, device=DEV)
    offs = torch.empty(4, dtype=torch.int32, device=DEV)
    cnt = np.asarray(pk["counts"], np.int32)
    pp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = eng.lib.yta_strongsort_update_tensors(
        eng.handle, None, pp(pk["dets"]), _lib.YTA_F64, 6, _lib.ptr(cnt), pp(pk["feats"]), D, None,
        None, None, pp(out), n - 1, pp(offs), None)
    assert rc == _lib.YTA_ERR_CAPACITY
    # a capturing stream: the cross-stream waits must not end up in a graph
    cs = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        y = pk["dets"] * 1.0
        with pytest.raises(_lib.YTAError):
            ut(pk["dets"], pk["feats"], counts=pk["counts"], stream=cs)
    del g, y
    torch.cuda.synchronize()
    assert eng.tensor_stats()["frames"] == frames0
    for s in range(3):
        assert _same_state(eng.state(s), state0[s]), s
    _tensor_run(eng, seq[8:12], rows[8:12], gates[8:12])   # and the engine goes on as before


# ---------------------------------------------------------------------------- 10. track capacity
def test_track_capacity_is_reported_by_sync():
    frames, (d5, f5) = _small_frames(5)
    eng = _engine(1, SMALL_P, feat_dim=8, track_capacity=4, max_dets=8)

    def run():
        orc = so.StrongSortOracle(**SMALL_P)
        for d, ft in frames:
            rows, off, _ = eng.update_tensors([_t(d)], [_t(ft)])
            assert np.array_equal(rows.cpu().numpy()[:int(off[1])], orc.update(d, ft))
        assert len(eng.state(0)["id"]) == 3

    run()
    eng.update_tensors([_t(d5)], [_t(f5)])   # five new objects beside three tracks: returns
    with pytest.raises(_lib.CapacityError):
        eng.sync()
    eng.reset()
    run()
    eng.sync()


# ------------------------------------------------------------------------------------ 11. drop-in
class _FakeReID:
    """get_features(xyxys, img) serving the feature rows of the current frame (NumPy in and out:
    a foreign producer)."""

    def __init__(self, frames):
        self.frames, self.f = frames, 0

    def get_features(self, xyxys, img):
        assert isinstance(xyxys, np.ndarray) and isinstance(img, np.ndarray)
        d, ft = self.frames[self.f][:2]
        assert np.array_equal(xyxys, d[:, :4])
        return ft


class _ScriptedCMC:
    def __init__(self, frames, reid):
        self.frames, self.reid, self.calls = frames, reid, 0

    def apply(self, img, dets):
        assert isinstance(img, np.ndarray) and isinstance(dets, np.ndarray)
        self.calls += 1
        return self.frames[self.reid.f][2]


def test_dropin_cuda_inputs_against_the_numpy_dropin(golden):
    from yolo_tracking_amd import StrongSORT, create_tracker, get_tracker_config
    p, frames, grows = so.golden_stream(golden, "y")

    def make():
        reid = _FakeReID(frames)
        trk = create_tracker("strongsort", get_tracker_config("strongsort"), reid, DEV, False,
                             False)
        assert isinstance(trk, StrongSORT)
        trk.cmc = _ScriptedCMC(frames, reid)
        return trk, reid

    (host, hreid), (dev, dreid), (emb, ereid) = make(), make(), make()
    img = np.zeros((8, 8, 3), np.uint8)
    img_dev = torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV)
    with_tracks = 0
    for f, (d, ft, _) in enumerate(frames):
        hreid.f = dreid.f = ereid.f = f
        with_tracks += host.tracks is not None and len(host.tracks["id"]) >= 1
        exp = np.asarray(host.update(d, img), dtype=np.float64).reshape(-1, 8)
        assert np.array_equal(exp[:, 4:], grows[f][:, 4:]), f
        got = dev.update(_t(d), img_dev)                    # foreign reid: rows from get_features
        got2 = emb.update(_t(d), img_dev, embs=_t(ft))      # embeddings handed in
        for g in (got, got2):
            assert isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.float64
            assert g.shape == (len(exp), 8) and np.array_equal(g.cpu().numpy(), exp), f
    assert dev.cmc.calls == emb.cmc.calls == host.cmc.calls == with_tracks < len(frames)
    got = dev.update(torch.zeros((0, 6), dtype=torch.float64, device=DEV), img_dev)
    assert got.is_cuda and got.shape == (0, 8)
    assert host.update(np.zeros((0, 6)), img).shape == (0,)   # the NumPy form is as it was


def test_dropin_cuda_inputs_with_the_packages_ecc():
    import cmc_frames
    from yolo_tracking_amd import StrongSORT
    h, w, n, Dd = 240, 320, 7, 16
    imgs, _ = cmc_frames.sequence(h, w, n, seed=3)
    rng = np.random.default_rng(9)
    base = rng.standard_normal((4, Dd)).astype(np.float32)
    box = np.array([[30, 40, 90, 160], [150, 60, 200, 190], [220, 20, 300, 150],
                    [100, 120, 170, 230]], dtype=np.float64)
    frames = []
    for f in range(n):
        b = box + [6.0 * f, -4.0 * f, 6.0 * f, -4.0 * f]
        d = np.concatenate([b, rng.uniform(0.4, 0.95, (4, 1)), np.zeros((4, 1))], axis=1)
        frames.append((d, base + np.float32(0.02) * rng.standard_normal((4, Dd)).astype(np.float32)))
    kw = dict(n_init=2, nn_budget=3, max_age=3)
    host = StrongSORT(None, DEV, False, **kw)
    dev = StrongSORT(None, DEV, False, **kw)
    rows = 0
    for f, (d, ft) in enumerate(frames):
        exp = np.asarray(host.update(d, imgs[f], embs=ft), dtype=np.float64).reshape(-1, 8)
        got = dev.update(_t(d), _t(imgs[f]), embs=_t(ft))
        assert got.is_cuda and np.array_equal(got.cpu().numpy().reshape(-1, 8), exp), f
        rows += len(exp)
    assert rows >= 4 * (n - 2)
