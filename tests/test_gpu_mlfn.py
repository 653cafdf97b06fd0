"""GPU: the MLFN kernels of csrc/mlfn.hip (yta_mlfn_gconv3x3, yta_mlfn_fsm, yta_mlfn_subsample +
yta_osnet_pointwise as the strided downsample, yta_osnet_pointwise's relu = 3, yta_mlfn_mean2)
against PyTorch's float32 operators on the same device inputs, and the network built on them
(appearance/mlfn.py) against the reference's module (tests/golden/mlfn_small.npz), against the
same folded graph on PyTorch's kernels at full size, and through ReIDDetectMultiBackend /
create_tracker from a weight file.

Bars, as in test_gpu_mobilenetv2.py: kernels 1e-5 of the output scale in float32 and 2e-3 in
float16 (one rounding to float16, 2^-11, of a float32 result); output buffers carry one extra
plane of 7.0 that must stay untouched; a second call gives equal bits.  Networks: 1e-4 of the
feature scale in float32 (the fixture's reference float32-versus-float64 deviations
are all below 1e-5, which test_mlfn_cpu.py asserts); float16 is measured against what PyTorch's
float16 graph itself errs."""
import ctypes

import numpy as np
import pytest
import torch

import mlfn_golden
from yolo_tracking_amd import _lib
from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
from yolo_tracking_amd.appearance.mlfn import MLFNReID, random_state_dict

pytestmark = pytest.mark.gpu
F = torch.nn.functional


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bar(half):
    return 2e-3 if half else 1e-5


# ---- yta_mlfn_gconv3x3
def _gconv(x, w, b, scale, G, s, half):
    """Into a buffer with one extra plane of 7.0 -> (whole buffer, (N, C, Ho, Wo) view)."""
    n, c, h, wd = x.shape
    ho, wo = (h - 1) // s + 1, (wd - 1) // s + 1
    buf = torch.full((n * c + 1, ho * wo), 7.0, dtype=x.dtype, device="cuda")
    _lib.check(_lib.load_library().yta_mlfn_gconv3x3(
        _p(x), _p(w), _p(b), _p(scale), scale.stride(0) if scale is not None else 0, n, c, G, h,
        wd, s, int(half), _p(buf), None))
    torch.cuda.synchronize()
    return buf, buf[:n * c].view(n, c, ho, wo)


GC_SHAPES = [(2, 4, 4, 1, 2), (1, 6, 2, 7, 4), (2, 12, 3, 9, 5), (1, 8, 1, 5, 3),
             (1, 128, 32, 17, 33), (1, 64, 2, 8, 4), (2, 16, 4, 64, 32)]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", GC_SHAPES)
def test_gconv3x3_kernel(shape, stride, half):
    """relu(grouped conv + b) * scale[sample][c // n]: the scales differ per sample and group
    and include exactly 0 and exactly 1 (where the shape has two of them), and sit in a wider
    buffer (row stride 16 G + 3); channel 1's bias is large and negative (exact zeros)."""
    n, c, G, h, w = shape
    cg = c // G
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(shape) + stride)
    x = torch.randn((n, c, h, w), generator=g).to(dt).cuda()
    wt = (torch.randn((c, cg, 3, 3), generator=g) * (1.0 / (3 * cg ** 0.5))).cuda()
    b = 0.3 * torch.randn(c, generator=g)
    b[1] = -500.0
    b = b.cuda()
    wide = torch.full((n, 16 * G + 3), 7.0)
    sc = 0.05 + 0.9 * torch.rand((n, G), generator=g)
    sc.view(-1)[0] = 1.0
    if sc.numel() > 1:
        sc.view(-1)[-1] = 0.0
    wide[:, 5:5 + G] = sc
    wide = wide.cuda()
    scale = wide[:, 5:5 + G]
    conv = F.relu(F.conv2d(x.float(), wt, b, stride=stride, padding=1, groups=G))
    ref = conv * scale.repeat_interleave(cg, dim=1)[:, :, None, None]
    buf, y = _gconv(x, wt.view(c, cg * 9), b, scale, G, stride, half)
    err, top = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    print(shape, stride, dt, "error / scale", err / top)
    assert top > 0 and err <= _bar(half) * top
    assert (y[:, 1] == 0).all() and (ref[:, 1] == 0).all()        # the ReLU's exact zeros
    if sc.numel() > 1:
        assert (y[-1, c - cg:] == 0).all()                         # scale exactly 0
    if G > 1 and cg > 1:   # the interleaved order c % G would be off by far more than the bar
        wrong = conv * scale.repeat(1, cg)[:, :, None, None]
        assert (wrong - ref).abs().max().item() > 10 * _bar(half) * top
    assert (buf[n * c] == 7.0).all()                # the plane past N * C stays untouched
    assert torch.equal(buf, _gconv(x, wt.view(c, cg * 9), b, scale, G, stride, half)[0])


def test_gconv3x3_without_scale():
    n, c, G, h, w = 2, 12, 3, 9, 5
    g = torch.Generator().manual_seed(12)
    x = torch.randn((n, c, h, w), generator=g).cuda()
    wt = (torch.randn((c, c // G, 3, 3), generator=g) * 0.2).cuda()
    b = (0.3 * torch.randn(c, generator=g)).cuda()
    ref = F.relu(F.conv2d(x, wt, b, stride=2, padding=1, groups=G))
    buf, y = _gconv(x, wt.view(c, -1), b, None, G, 2, False)
    assert (y - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (buf[n * c] == 7.0).all()
    lib = _lib.load_library()
    assert lib.yta_mlfn_gconv3x3(_p(x), _p(wt), _p(b), None, 0, n, c, 5, h, w, 2, 0, _p(buf),
                                 None) != 0      # 5 does not divide 12
    assert lib.yta_mlfn_gconv3x3(_p(x), _p(wt), _p(b), None, 0, n, c, G, h, w, 3, 0, _p(buf),
                                 None) != 0      # stride 3


# ---- yta_mlfn_fsm
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", [(2, 8, 6, 5, 2), (3, 256, 128, 64, 32)])
def test_fsm_kernel(shape, half):
    """Slot 5 of a 16-slot selection buffer; the other slots keep their 7.0, in the float32
    buffer and in the storage-type one."""
    n, cin, f0, f1, G = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(shape))
    pooled = torch.rand((n, cin), generator=g).to(dt).cuda()
    ws = [(torch.randn((o, i), generator=g) * (2.0 / i) ** 0.5).cuda()
          for i, o in ((cin, f0), (f0, f1), (f1, G))]
    bs = [(0.2 * torch.randn(o, generator=g)).cuda() for o in (f0, f1, G)]
    ref = pooled.float()
    for i in range(3):
        ref = ref @ ws[i].t() + bs[i]
        ref = torch.sigmoid(ref) if i == 2 else F.relu(ref)
    assert ref.max().item() - ref.min().item() > 0.02
    wk = [w.t().contiguous() for w in ws]
    lib = _lib.load_library()

    def run():
        sel = torch.full((n, 16 * G), 7.0, device="cuda")
        sel_t = torch.full((n, 16 * G), 7.0, dtype=dt, device="cuda")
        _lib.check(lib.yta_mlfn_fsm(
            _p(pooled), n, cin, f0, f1, G, _p(wk[0]), _p(bs[0]), _p(wk[1]), _p(bs[1]), _p(wk[2]),
            _p(bs[2]), int(half), ctypes.c_void_p(sel.data_ptr() + 4 * 5 * G), 16 * G,
            ctypes.c_void_p(sel_t.data_ptr() + sel_t.element_size() * 5 * G), 16 * G, None))
        torch.cuda.synchronize()
        return sel, sel_t
    sel, sel_t = run()
    s = sel[:, 5 * G:6 * G]
    err = (s - ref).abs().max().item() / ref.max().item()
    print(shape, dt, "error / scale", err)
    assert err <= _bar(half)
    assert torch.equal(s, sel_t[:, 5 * G:6 * G].float())
    for buf in (sel, sel_t):
        assert (buf[:, :5 * G] == 7.0).all() and (buf[:, 6 * G:] == 7.0).all()
    sel2, sel_t2 = run()
    assert torch.equal(sel, sel2) and torch.equal(sel_t, sel_t2)


# ---- the strided downsample: yta_mlfn_subsample ahead of yta_osnet_pointwise; relu = 3
def _pw(x, wk, bias, res, relu, half, p):
    n, k = x.shape[:2]
    cout = wk.shape[1]
    buf = torch.full((n * cout + 1, p), 7.0, dtype=x.dtype, device="cuda")
    a = _lib.PwArgs()
    a.x1 = x.data_ptr()
    a.x1n, a.x1c, a.x1p = k * p, p, 1
    a.w, a.bias, a.res = wk.data_ptr(), bias.data_ptr(), res.data_ptr()
    a.rn, a.rc, a.rp = cout * p, p, 1
    a.y = buf.data_ptr()
    a.yn, a.yc, a.yp = cout * p, p, 1
    a.k1, a.k2, a.G, a.cout_g, a.P, a.N, a.relu = k, 0, 1, cout, p, n, relu
    _lib.check(_lib.load_library().yta_osnet_pointwise(ctypes.byref(a), int(half), None))
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", [(2, 16, 32, 9, 5), (1, 24, 40, 64, 32)])
def test_strided_downsample(shape, half):
    """downsample = Conv2d(cin, cout, 1, stride=2) + BatchNorm (folded) with fm_conv3's result as
    the residual and the block's last ReLU: the gather, then the GEMM."""
    n, cin, cout, h, w = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((n, cin, h, w), generator=g).to(dt).cuda()
    wt = (torch.randn((cout, cin), generator=g) * cin ** -0.5).cuda()
    b = (0.3 * torch.randn(cout, generator=g)).cuda()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    res = torch.rand((n, cout, ho, wo), generator=g).to(dt).cuda()
    lib = _lib.load_library()

    def run():
        xs = torch.full((n * cin + 1, ho * wo), 7.0, dtype=dt, device="cuda")
        _lib.check(lib.yta_mlfn_subsample(_p(x), n, cin, h, w, 2, int(half), _p(xs), None))
        return xs, _pw(xs[:n * cin].view(n, cin, ho * wo), wt.t().contiguous(), b, res, 1, half,
                       ho * wo)
    xs, buf = run()
    assert torch.equal(xs[:n * cin].view(n, cin, ho, wo), x[:, :, ::2, ::2])
    assert (xs[n * cin] == 7.0).all()
    ref = F.relu(F.conv2d(x.float(), wt[:, :, None, None], b, stride=2) + res.float())
    y = buf[:n * cout].view(n, cout, ho, wo)
    err, top = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    print(shape, dt, "error / scale", err / top)
    assert err <= _bar(half) * top and (ref == 0).any()
    assert (buf[n * cout] == 7.0).all()
    xs2, buf2 = run()
    assert torch.equal(xs, xs2) and torch.equal(buf, buf2)


@pytest.mark.parametrize("half", [False, True])
def test_pointwise_relu_on_both_sides_of_the_residual(half):
    """relu = 3: relu(relu(W x + b) + res) (mlfn.py:87-92) with residuals of both signs; relu = 1
    is still relu(W x + b + res)."""
    n, k, cout, p = 2, 33, 89, 45
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(3)
    x = torch.randn((n, k, p), generator=g).to(dt).cuda()
    w = (torch.randn((cout, k), generator=g) * 0.3).cuda()
    bias = torch.randn(cout, generator=g).cuda()
    res = torch.randn((n, cout, p), generator=g).to(dt).cuda()
    lin = torch.einsum("ok,nkp->nop", w, x.float()) + bias[None, :, None]
    r3, r1 = F.relu(F.relu(lin) + res.float()), F.relu(lin + res.float())
    assert (r3 - r1).abs().max().item() > 0.5
    for relu, ref in ((3, r3), (1, r1)):
        buf = _pw(x, w.t().contiguous(), bias, res, relu, half, p)
        y = buf[:n * cout].view(n, cout, p)
        err, top = (y.float() - ref).abs().max().item(), ref.abs().max().item()
        print("relu", relu, dt, "error / scale", err / top)
        assert err <= _bar(half) * top and (y == 0).any()
        assert (buf[n * cout] == 7.0).all()


@pytest.mark.parametrize("half", [False, True])
def test_mean2_kernel(half):
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(9)
    a = torch.randn(3 * 1024 + 5, generator=g).to(dt).cuda()
    b = torch.randn(3 * 1024 + 5, generator=g).to(dt).cuda()
    y = torch.full((a.numel() + 64,), 7.0, dtype=dt, device="cuda")
    _lib.check(_lib.load_library().yta_mlfn_mean2(_p(a), _p(b), a.numel(), int(half), _p(y), None))
    torch.cuda.synchronize()
    ref = (a.float() + b.float()) * 0.5
    assert (y[:a.numel()].float() - ref).abs().max().item() <= _bar(half) * ref.abs().max().item()
    assert (y[a.numel():] == 7.0).all()


# ---- single blocks and the network against the reference
def _rel(y, ref):
    return np.abs(y.float().cpu().numpy() - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("i", range(mlfn_golden.N_BLOCKS))
def test_block_matches_reference_block(i):
    cfg, bsd, x, y_ref, s_ref = mlfn_golden.load()[3][i]
    xg = torch.from_numpy(x).cuda()
    blk = mlfn_golden.block_graph(cfg, bsd, device="cuda:0")
    assert blk.hip
    y, s = blk(xg)
    ey, es = _rel(y, y_ref), _rel(s, s_ref)
    print("block", cfg, "f32 error / scale: y", ey, "s", es)
    assert y.shape == y_ref.shape and s.shape == s_ref.shape
    assert ey <= 1e-4 and es <= 1e-4
    y2, s2 = blk(xg)
    assert torch.equal(y, y2) and torch.equal(s, s2)
    yh, sh = mlfn_golden.block_graph(cfg, bsd, device="cuda:0", half=True)(xg.half())
    yt, st = mlfn_golden.block_graph(cfg, bsd, device="cuda:0", half=True, hip=False)(xg.half())
    e_hip, e_torch = max(_rel(yh, y_ref), _rel(sh, s_ref)), max(_rel(yt, y_ref), _rel(st, s_ref))
    print("block", cfg, "f16 error / scale: hip", e_hip, "torch graph", e_torch)
    assert yh.dtype == torch.float16 and e_hip <= max(2 * e_torch, 2e-2)


def _golden_net(sd, **kw):
    return MLFNReID("mlfn", sd, device="cuda:0", **mlfn_golden.NET, **kw)


KEYS = [k for k, _ in mlfn_golden.SHAPES]


@pytest.mark.parametrize("key", KEYS)
def test_network_matches_reference_f32(key):
    _, sd, cases, _ = mlfn_golden.load()
    x, ref, dev = cases[key]
    x = torch.from_numpy(x).cuda()
    net = _golden_net(sd)
    assert net.hip
    y = net(x)
    assert y.dtype == torch.float32 and y.shape == ref.shape
    err = _rel(y, ref)
    bar = 1e-4 if dev <= 1e-5 else 10 * dev
    print(key, "f32 error / scale", err, "bar", bar)
    assert err <= bar
    assert torch.equal(y, net(x))


@pytest.mark.parametrize("key", KEYS)
def test_network_matches_reference_f16(key):
    """No fixed number for float16: the HIP forward may err against the golden at most twice
    what the same folded graph on PyTorch's float16 operators (hip=False, on the device) errs
    against it, with a floor of 2e-2, the project's float16 bar."""
    _, sd, cases, _ = mlfn_golden.load()
    x, ref, _ = cases[key]
    x = torch.from_numpy(x).cuda().half()
    y = _golden_net(sd, half=True)(x)
    assert y.dtype == torch.float16
    e_hip = _rel(y, ref)
    e_torch = _rel(_golden_net(sd, hip=False, half=True)(x), ref)
    print(key, "f16 error / scale: hip", e_hip, "torch graph", e_torch)
    assert e_hip <= max(2 * e_torch, 2e-2)


def test_hip_forward_matches_torch_graph_full_size():
    """The real channel counts (32 groups of 4 .. 32 channels, selection layers up to 2048 ->
    512) without trained weights: the HIP forward against the same folded graph on PyTorch's
    kernels."""
    sd = random_state_dict(3, randomise_bn=True)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 256, 128))
                         .astype(np.float32)).cuda()
    b = MLFNReID("mlfn", sd, device="cuda:0", hip=False)(x)
    a = MLFNReID("mlfn", sd, device="cuda:0")(x)
    err = (a - b).abs().max().item() / b.abs().max().item()
    print("mlfn hip vs torch graph, error / scale", err, "feature max", b.max().item())
    assert a.shape == b.shape == (2, 1024) and b.abs().max().item() > 0
    assert err <= 1e-5


def test_weight_file_and_create_tracker(tmp_path):
    """A reference-format mlfn_dukemtmcreid.pt ({'state_dict': ...}, 'module.' prefixes,
    classifier.* present) loads through ReIDDetectMultiBackend; get_features = network(crops) /
    global norm; create_tracker builds the producer from the path, with 1024-d features."""
    from yolo_tracking_amd import create_tracker, get_tracker_config
    from yolo_tracking_amd.synth import make_frames
    sd = random_state_dict(5, randomise_bn=True)
    ck = {"module." + k: torch.from_numpy(v) for k, v in sd.items()}
    ck["module.classifier.weight"] = torch.zeros(702, 1024)
    ck["module.classifier.bias"] = torch.zeros(702)
    w = tmp_path / "mlfn_dukemtmcreid.pt"
    torch.save({"state_dict": ck}, w)
    reid = ReIDDetectMultiBackend(w, device=0, fp16=False)
    assert reid.model.name == "mlfn" and reid.model.feature_dim == 1024 and reid.model.hip
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    boxes = np.array([[10, 20, 110, 300], [300, 50, 380, 250], [500, 100, 639, 479]], np.float64)
    f = reid.get_features(boxes, img)
    raw = MLFNReID("mlfn", sd, device="cuda:0")(reid.preprocess(boxes, img)).cpu().numpy()
    assert f.shape == (3, 1024) and np.abs(raw).max() > 0
    np.testing.assert_allclose(f, raw / np.linalg.norm(raw), rtol=1e-5, atol=1e-7)
    img = rng.integers(0, 256, (640, 640, 3), dtype=np.uint8)
    frames = make_frames(24, 3, 5, canvas=600.0)
    for kind in ("botsort", "deepocsort", "strongsort"):
        t = create_tracker(kind, get_tracker_config(kind), w, "0", False, False)
        assert isinstance(t.model, ReIDDetectMultiBackend), kind
        assert t.model.model.name == "mlfn" and t.model.model.feature_dim == 1024
        rows = 0
        for dets, _ in frames:
            r = np.asarray(t.update(dets, img))
            assert r.size == 0 or (r.ndim == 2 and r.shape[1] == 8), kind
            rows += len(r) if r.size else 0
        print(kind, "rows over three frames:", rows)
    with pytest.warns(RuntimeWarning, match="random"):
        r = ReIDDetectMultiBackend(tmp_path / "mlfn_msmt17.pt", device=0, random_init=True)
    assert r.model.name == "mlfn"
    with pytest.raises(FileNotFoundError):
        ReIDDetectMultiBackend(tmp_path / "mlfn_market1501.pt", device=0)
    with pytest.raises(NotImplementedError, match="mlfn"):
        ReIDDetectMultiBackend(tmp_path / "resnet50_msmt17.pt", device=0)
