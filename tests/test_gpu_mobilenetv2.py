"""GPU: the MobileNetV2 kernels of csrc/mbv2.hip (yta_mbv2_expand_dw, yta_mbv2_dw3x3,
yta_mbv2_stem) and yta_osnet_pointwise's ReLU6 epilogue against PyTorch's float32 operators on the
same device inputs, and the network built on them (appearance/mobilenetv2.py) against the
reference's module (tests/golden/mobilenetv2_x0_25.npz), against the same folded graph on
PyTorch's kernels at the real widths, and through ReIDDetectMultiBackend / create_tracker from a
weight file.

Bars, as in test_gpu_osnet_in.py: kernels 1e-5 of the output scale in float32 and 2e-3 in float16
(one rounding to float16, 2^-11, of a float32 result); output buffers carry one extra plane of
7.0 that must stay untouched; a second call gives equal bits.  Networks: 1e-4 of the feature scale
in float32; float16 is measured against what PyTorch's float16 graph itself errs."""
import ctypes
import os

import numpy as np
import pytest
import torch

from yolo_tracking_amd import _lib
from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
from yolo_tracking_amd.appearance.mobilenetv2 import MobileNetV2ReID, random_state_dict

pytestmark = pytest.mark.gpu
F = torch.nn.functional


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _bar(half):
    return 2e-3 if half else 1e-5


# ---- yta_mbv2_expand_dw
def _expand_dw(x, w1, b1, wd, b2, s, half):
    """Into a buffer with one extra plane of 7.0 -> (N, Cmid, Ho, Wo) view, guard plane."""
    n, cin, h, w = x.shape
    cmid = w1.shape[0]
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    buf = torch.full((n * cmid + 1, ho * wo), 7.0, dtype=x.dtype, device="cuda")
    w1k = w1.t().contiguous()                          # [Cin][Cmid], k-major
    _lib.check(_lib.load_library().yta_mbv2_expand_dw(
        _p(x), _p(w1k), _p(b1), _p(wd.contiguous()), _p(b2), n, cin, cmid, h, w, s, int(half),
        _p(buf), None))
    torch.cuda.synchronize()
    return buf[:n * cmid].view(n, cmid, ho, wo), buf[n * cmid]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 24, 5, 3, 1), (1, 6, 36, 7, 4, 2), (1, 8, 8, 2, 1, 2),
                                   (2, 33, 198, 9, 5, 2), (1, 16, 96, 33, 17, 1),
                                   (1, 32, 32, 128, 64, 1), (1, 89, 534, 16, 8, 1)])
def test_expand_dw_kernel(shape, half):
    """relu6(dw3x3_s(relu6(W1 x + b1)) + b2) with b1 from N(0.5, 0.5^2): relu6(b1) is non-zero, so
    a halo filled with it instead of the filter's zero padding shows.  Channel 0 expands to
    exactly 6 everywhere (its taps are 0.1: the output is 0.6 x the taps inside the image),
    channel 1 to exactly 0, channels 2 and 3 leave the second clamp at 6 and at 0."""
    n, cin, cmid, h, w, s = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((n, cin, h, w), generator=g).to(dt).cuda()
    w1 = torch.randn((cmid, cin), generator=g) * (2.5 / cin ** 0.5)
    b1 = 0.5 + 0.5 * torch.randn(cmid, generator=g)
    wd = torch.randn((cmid, 9), generator=g) * 0.5
    b2 = 0.5 + 0.5 * torch.randn(cmid, generator=g)
    w1[0], b1[0], wd[0], b2[0] = 0.0, 50.0, 0.1, 0.0
    w1[1], b1[1] = 0.0, -50.0
    b2[2], b2[3] = 500.0, -500.0
    w1, b1, wd, b2 = w1.cuda(), b1.cuda(), wd.cuda(), b2.cuda()
    e = F.relu6(F.conv2d(x.float(), w1[:, :, None, None], b1))
    ref = F.relu6(F.conv2d(e, wd.view(cmid, 1, 3, 3), b2, stride=s, padding=1, groups=cmid))
    assert (e == 6).any() and (e == 0).any()
    assert (ref == 6).any() and (ref == 0).any()
    y, guard = _expand_dw(x, w1, b1, wd, b2, s, half)
    err, scale = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    print(shape, dt, "error / scale", err / scale)
    assert scale == 6.0
    assert err <= _bar(half) * scale
    assert (y == 6).any() and (y == 0).any()
    assert (guard == 7.0).all()                     # the plane past N * Cmid stays untouched
    y2, _ = _expand_dw(x, w1, b1, wd, b2, s, half)
    assert torch.equal(y, y2)                       # no atomics: bit-identical


# ---- yta_mbv2_dw3x3
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 5, 1, 2), (3, 7, 5, 3), (2, 4, 33, 17), (1, 3, 128, 64)])
def test_dw3x3_kernel(shape, stride, half):
    n, c, h, w = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(shape) + stride)
    x = (torch.rand(shape, generator=g) * 6).to(dt).cuda()      # a ReLU6 output
    wd = (torch.randn((c, 9), generator=g) * 0.5).cuda()
    b = 0.5 + torch.randn(c, generator=g)
    b[0], b[1] = 50.0, -50.0                                    # both clamps, in every shape
    b = b.cuda()
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    lib = _lib.load_library()

    def run():
        buf = torch.full((n * c + 1, ho * wo), 7.0, dtype=dt, device="cuda")
        _lib.check(lib.yta_mbv2_dw3x3(_p(x), _p(wd), _p(b), n, c, h, w, stride, int(half), _p(buf),
                                      None))
        torch.cuda.synchronize()
        return buf
    buf = run()
    ref = F.relu6(F.conv2d(x.float(), wd.view(c, 1, 3, 3), b, stride=stride, padding=1, groups=c))
    y = buf[:n * c].view(n, c, ho, wo)
    err, scale = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    print(shape, stride, dt, "error / scale", err / scale)
    assert err <= _bar(half) * scale
    assert (ref == 6).any() and (ref == 0).any() and (y == 6).any() and (y == 0).any()
    assert (buf[n * c] == 7.0).all()
    assert torch.equal(buf, run())


# ---- yta_mbv2_stem
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", [(2, 64, 32, 8), (1, 37, 29, 44), (1, 2, 1, 5)])
def test_stem_kernel(shape, half):
    n, h, w, c0 = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(h + w)
    x = torch.randn((n, 3, h, w), generator=g).to(dt).cuda()
    wt = (torch.randn((c0, 3, 3, 3), generator=g) * 0.5).cuda()
    b = torch.randn(c0, generator=g)
    b[0], b[1] = 50.0, -50.0
    b = b.cuda()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    buf = torch.full((n * c0 + 1, ho * wo), 7.0, dtype=dt, device="cuda")
    _lib.check(_lib.load_library().yta_mbv2_stem(_p(x), n, h, w, _p(wt), _p(b), c0, int(half),
                                                 _p(buf), None))
    torch.cuda.synchronize()
    ref = F.relu6(F.conv2d(x.float(), wt, b, stride=2, padding=1))
    y = buf[:n * c0].view(n, c0, ho, wo)
    err, scale = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    print(shape, dt, "error / scale", err / scale)
    assert (ref == 6).any() and (y == 6).any() and (y == 0).any()
    assert err <= _bar(half) * scale
    assert (buf[n * c0] == 7.0).all()


# ---- yta_osnet_pointwise, relu = 2
def _pointwise(x, wk, bias, res, relu, half):
    n, k, p = x.shape
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
    return buf[:n * cout].view(n, cout, p), buf[n * cout]


@pytest.mark.parametrize("half", [False, True])
def test_pointwise_relu6(half):
    """relu = 2 clamps to [0, 6]; relu = 1 is still ReLU and 0 still linear (ragged: K = 33,
    cout = 89, P = 45, with a residual)."""
    n, k, cout, p = 2, 33, 89, 45
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(33 + 89 + 45)
    x = torch.randn((n, k, p), generator=g).to(dt).cuda()
    w = (torch.randn((cout, k), generator=g) * 0.6).cuda()
    bias = (1.0 + torch.randn(cout, generator=g)).cuda()
    res = torch.randn((n, cout, p), generator=g).to(dt).cuda()
    lin = torch.einsum("ok,nkp->nop", w, x.float()) + bias[None, :, None] + res.float()
    assert (lin > 6).any() and (lin < 0).any()
    wk = w.t().contiguous()
    for relu, ref in ((2, lin.clamp(0, 6)), (1, lin.relu()), (0, lin)):
        y, guard = _pointwise(x, wk, bias, res, relu, half)
        err, scale = (y.float() - ref).abs().max().item(), ref.abs().max().item()
        print("relu", relu, dt, "error / scale", err / scale)
        assert err <= _bar(half) * scale
        assert (guard == 7.0).all()
        if relu == 2:
            assert (y == 6).any() and (y == 0).any() and y.max().item() == 6.0
        if relu == 1:
            assert y.max().item() > 6.0 and (y == 0).any()


# ---- the network
SHAPES = (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32)),
          ("features_odd", (2, 3, 70, 38)))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "mobilenetv2_x0_25.npz"))
    sd = {k[4:]: g[k] for k in g.files if k.startswith("sd__")}
    rng = np.random.default_rng(int(g["input_seed"]))
    cases = {}
    for key, shape in SHAPES:
        cases[key] = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda(),
                      g[key])
    return sd, cases


def _golden_net(sd, **kw):
    return MobileNetV2ReID("mobilenetv2_x1_0", sd, device="cuda:0", width_mult=0.25, **kw)


def _rel(y, ref):
    return np.abs(y.float().cpu().numpy() - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("key", [k for k, _ in SHAPES])
def test_network_matches_reference_f32(golden, key, fused):
    sd, cases = golden
    x, ref = cases[key]
    net = _golden_net(sd, fused=fused)
    assert net.hip and net.fused == fused
    y = net(x)
    assert y.dtype == torch.float32 and y.shape == ref.shape
    err = _rel(y, ref)
    print(key, "fused" if fused else "unfused", "f32 error / scale", err)
    assert err <= 1e-4
    assert torch.equal(y, net(x))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("key", [k for k, _ in SHAPES])
def test_network_matches_reference_f16(golden, key, fused):
    """No fixed number for float16: the HIP forward may err against the golden at most twice
    what the same folded graph on PyTorch's float16 operators (hip=False, on the device) errs
    against it, with a floor of 2e-2, the project's float16 bar."""
    sd, cases = golden
    x, ref = cases[key]
    y = _golden_net(sd, fused=fused, half=True)(x.half())
    assert y.dtype == torch.float16
    e_hip = _rel(y, ref)
    e_torch = _rel(_golden_net(sd, hip=False, half=True)(x.half()), ref)
    print(key, "fused" if fused else "unfused", "f16 error / scale: hip", e_hip, "torch graph",
          e_torch)
    assert e_hip <= max(2 * e_torch, 2e-2)


def _randomise_bn(sd, seed):
    """The golden's BatchNorm recipe on a state_dict: the upper clamp becomes active."""
    rng = np.random.default_rng(seed)
    for k in [k for k in sd if k.endswith(".running_var")]:
        base, c = k[:-len("running_var")], sd[k].shape[0]
        sd[base + "running_mean"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[k] = rng.uniform(0.75, 1.25, c).astype(np.float32)
        sd[base + "weight"] = rng.uniform(1.5, 2.5, c).astype(np.float32)
        sd[base + "bias"] = (rng.standard_normal(c) * 0.3).astype(np.float32)
    return sd


@pytest.mark.parametrize("name,dim", [("mobilenetv2_x1_0", 1280), ("mobilenetv2_x1_4", 1792)])
def test_hip_forward_matches_torch_graph_full_width(name, dim):
    """The real channel counts (x1_4: 44, 22, 33, 89, 134, ...) without their weights: the HIP
    forward, fused and unfused, against the same folded graph on PyTorch's kernels."""
    sd = _randomise_bn(random_state_dict(name, 3), 4)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 256, 128))
                         .astype(np.float32)).cuda()
    t = MobileNetV2ReID(name, sd, device="cuda:0", hip=False, count_clamped=True)
    b = t(x)
    print(name, "ConvBlocks reaching 6:", t.clamped, "of 36; feature max", b.max().item())
    assert t.clamped >= 1 and b.shape == (2, dim) and b.abs().max().item() > 0
    for fused in (True, False):
        a = MobileNetV2ReID(name, sd, device="cuda:0", fused=fused)(x)
        err = (a - b).abs().max().item() / b.abs().max().item()
        print(name, "fused" if fused else "unfused", "hip vs torch graph, error / scale", err)
        assert a.shape == (2, dim)
        assert err <= 1e-5


def test_weight_file_and_create_tracker(tmp_path):
    """A reference-format mobilenetv2_x1_4_dukemtmcreid.pt ({'state_dict': ...}, 'module.'
    prefixes, classifier.* present) loads through ReIDDetectMultiBackend; get_features =
    network(crops) / global norm; create_tracker builds the producer from the path for the three
    trackers the reference's own tests run with this file, with 1792-d features."""
    from yolo_tracking_amd import create_tracker, get_tracker_config
    from yolo_tracking_amd.synth import make_frames
    sd = _randomise_bn(random_state_dict("mobilenetv2_x1_4", 5), 6)
    ck = {"module." + k: torch.from_numpy(v) for k, v in sd.items()}
    ck["module.classifier.weight"] = torch.zeros(702, 1792)
    ck["module.classifier.bias"] = torch.zeros(702)
    w = tmp_path / "mobilenetv2_x1_4_dukemtmcreid.pt"
    torch.save({"state_dict": ck}, w)
    reid = ReIDDetectMultiBackend(w, device=0, fp16=False)
    assert reid.model.name == "mobilenetv2_x1_4" and reid.model.feature_dim == 1792
    assert reid.model.hip and reid.model.fused
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    boxes = np.array([[10, 20, 110, 300], [300, 50, 380, 250], [500, 100, 639, 479]], np.float64)
    f = reid.get_features(boxes, img)
    raw = MobileNetV2ReID("mobilenetv2_x1_4", sd, device="cuda:0")(
        reid.preprocess(boxes, img)).cpu().numpy()
    assert f.shape == (3, 1792) and np.abs(raw).max() > 0
    np.testing.assert_allclose(f, raw / np.linalg.norm(raw), rtol=1e-5, atol=1e-7)
    img = rng.integers(0, 256, (640, 640, 3), dtype=np.uint8)
    frames = make_frames(24, 3, 5, canvas=600.0)
    for kind in ("botsort", "deepocsort", "strongsort"):
        t = create_tracker(kind, get_tracker_config(kind), w, "0", False, False)
        assert isinstance(t.model, ReIDDetectMultiBackend), kind
        assert t.model.model.name == "mobilenetv2_x1_4"
        rows = 0
        for dets, _ in frames:
            r = np.asarray(t.update(dets, img))
            assert r.size == 0 or (r.ndim == 2 and r.shape[1] == 8), kind
            rows += len(r) if r.size else 0
        print(kind, "rows over three frames:", rows)
    with pytest.raises(FileNotFoundError):
        ReIDDetectMultiBackend(tmp_path / "mobilenetv2_x1_0_msmt17.pt", device=0)
    with pytest.raises(NotImplementedError, match="osnet_ain_x1_0"):
        ReIDDetectMultiBackend(tmp_path / "resnet50_msmt17.pt", device=0)
