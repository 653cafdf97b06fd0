"""GPU: the instance-norm kernels of csrc/osnet.hip (yta_osnet_instnorm, yta_osnet_instnorm_maxpool,
yta_osnet_stem_linear) against PyTorch's float32 operators on the same device inputs, and the
OSNet-IBN / OSNet-AIN networks built on them against the reference's modules
(tests/golden/osnet_ain_x0_25.npz, osnet_ibn_x0_25.npz), against the same folded graph on
PyTorch's kernels, and through ReIDDetectMultiBackend / create_tracker from a weight file.

Bars: the kernel bars of test_gpu_osnet.py (1e-5 of the output scale in float32, 2e-3 in float16:
one rounding to float16, 2^-11, of a float32 result); the networks within 1e-4 (float32) and 2e-2
(float16) of the feature scale, DESIGN §9.1."""
import ctypes
import os

import numpy as np
import pytest
import torch

from yolo_tracking_amd import _lib
from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
from yolo_tracking_amd.appearance.osnet import OSNetReID, random_state_dict

pytestmark = pytest.mark.gpu
F = torch.nn.functional
OVER = (1, 2, 130, 70)   # 9100 pixels: over the resident bound, the looping path / the fallback


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _affine(c, g):
    """gamma in +-[0.75, 1.25], every second entry negative; beta of either sign."""
    gamma = torch.rand(c, generator=g) * 0.5 + 0.75
    gamma[::2] *= -1
    return gamma.cuda(), (torch.randn(c, generator=g) * 0.3).cuda()


def _instnorm(x, gamma, beta, res, relu, half):
    """yta_osnet_instnorm into a buffer with one extra plane of 7.0 -> (N, C, H, W) view, guard."""
    n, c, h, w = x.shape
    buf = torch.full((n * c + 1, h * w), 7.0, dtype=x.dtype, device="cuda")
    _lib.check(_lib.load_library().yta_osnet_instnorm(
        _p(x), _p(res), _p(gamma), _p(beta), n, c, h * w, int(relu), int(half), _p(buf), None))
    torch.cuda.synchronize()
    return buf[:n * c].view(n, c, h, w), buf[n * c]


def test_resident_bound():
    bound = _lib.load_library().yta_osnet_instnorm_resident()
    assert 8192 <= bound < OVER[2] * OVER[3]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 1, 2), (3, 7, 5, 3), (2, 4, 33, 17), (1, 3, 64, 32),
                                   (1, 2, 128, 64), OVER])
def test_instnorm_kernel(shape, with_res, relu, half):
    n, c, h, w = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(shape) + 2 * with_res + relu)
    x = (torch.randn(shape, generator=g) * 2 + 0.5).to(dt).cuda()
    res = torch.randn(shape, generator=g).to(dt).cuda() if with_res else None
    gamma, beta = _affine(c, g)
    y, guard = _instnorm(x, gamma, beta, res, relu, half)
    ref = F.instance_norm(x.float(), weight=gamma, bias=beta, eps=1e-5)
    if with_res:
        ref = ref + res.float()
    if relu:
        ref = ref.relu()
    err, scale = (y.float() - ref).abs().max().item(), ref.abs().max().item()
    print(shape, "res" if with_res else "", "relu" if relu else "", dt, "error / scale", err / scale)
    assert err <= (2e-3 if half else 1e-5) * scale
    assert (guard == 7.0).all()                     # the plane past N * C stays untouched
    y2, _ = _instnorm(x, gamma, beta, res, relu, half)
    assert torch.equal(y, y2)                       # fixed-order sums: bit-identical
    # A constant plane: x_hat = 0, so the output is exactly beta (+ res).  Checked against that and
    # not against the float32 operator, whose rounding of the plane's mean is multiplied by
    # 1 / sqrt(eps) = 316 where the variance is zero.
    x[0, 0] = 3.25
    y, _ = _instnorm(x, gamma, beta, res, relu, half)
    const = beta[0] + res[0, 0].float() if with_res else beta[0].expand(h, w)
    if relu:
        const = const.relu()
    assert torch.equal(y[0, 0], const.to(dt))
    assert torch.equal(y[1:], y2[1:]) and torch.equal(y[0, 1:], y2[0, 1:])


def test_instnorm_offset_plane():
    """1000 + N(0, 1): the plane a one-pass E[x^2] - mean^2 variance fails on.  No fixed tolerance:
    against the float64 instance norm of the same float32 inputs the kernel may err at most twice
    as much as F.instance_norm in float32 on the device (a different summation order, nothing
    more), with a floor of 1e-5 of the output scale.
    Measured on the MI355X: kernel 3.8e-7, F.instance_norm 0.49, scale 4.96."""
    g = torch.Generator().manual_seed(1000)
    x = (1000 + torch.randn((1, 1, 128, 64), generator=g)).cuda()
    gamma = torch.tensor([-1.2], device="cuda")
    beta = torch.tensor([0.1], device="cuda")
    xd = x.double()
    mean, var = xd.mean(dim=(2, 3), keepdim=True), xd.var(dim=(2, 3), unbiased=False, keepdim=True)
    ref = (xd - mean) / (var + 1e-5).sqrt() * gamma.double() + beta.double()
    y, _ = _instnorm(x, gamma, beta, None, False, False)
    t = F.instance_norm(x, weight=gamma, bias=beta, eps=1e-5)
    e_k, e_t = (y.double() - ref).abs().max().item(), (t.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print("offset plane: kernel", e_k, "F.instance_norm float32", e_t, "scale", scale)
    assert e_k <= max(2 * e_t, 1e-5 * scale)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", [(1, 3, 128, 64), (2, 5, 33, 17), (1, 2, 2, 1), OVER])
def test_instnorm_maxpool_kernel(shape, half):
    n, c, h, w = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=g) * 2 - 0.5).to(dt).cuda()
    gamma, beta = _affine(c, g)
    lib = _lib.load_library()
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    buf = torch.full((n * c + 1, ho * wo), 7.0, dtype=dt, device="cuda")
    work = torch.empty_like(x) if h * w > lib.yta_osnet_instnorm_resident() else None
    _lib.check(lib.yta_osnet_instnorm_maxpool(_p(x), _p(gamma), _p(beta), n, c, h, w, int(half),
                                              _p(work), _p(buf), None))
    torch.cuda.synchronize()
    ref = F.max_pool2d(F.relu(F.instance_norm(x.float(), weight=gamma, bias=beta, eps=1e-5)),
                       3, stride=2, padding=1)
    y = buf[:n * c].view(n, c, ho, wo).float()
    err, scale = (y - ref).abs().max().item(), ref.abs().max().item()
    print(shape, dt, "error / scale", err / scale)
    assert err <= (2e-3 if half else 1e-5) * scale
    assert (buf[n * c] == 7.0).all()


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", [(2, 256, 128, 16), (1, 37, 29, 64)])
def test_stem_linear_kernel(shape, half):
    """The stem convolution without the clamp (an instance norm follows): negative outputs
    survive.  float16: one rounding (2^-11) of the float32 sums."""
    n, h, w, c0 = shape
    dt = torch.float16 if half else torch.float32
    g = torch.Generator().manual_seed(h + w)
    x = torch.randn((n, 3, h, w), generator=g).to(dt).cuda()
    wt = (torch.randn((c0, 3, 7, 7), generator=g) * 0.1).cuda()
    b = torch.randn(c0, generator=g).cuda()
    y = torch.empty((n, c0, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=dt, device="cuda")
    _lib.check(_lib.load_library().yta_osnet_stem_linear(
        _p(x), n, h, w, _p(wt), _p(b), c0, int(half), _p(y), None))
    torch.cuda.synchronize()
    ref = F.conv2d(x.float(), wt, b, stride=2, padding=3)
    assert (ref < 0).any()
    assert (y.float() - ref).abs().max().item() <= (2e-3 if half else 1e-5) * ref.abs().max().item()


# ---- the networks
@pytest.fixture(scope="module", params=["osnet_ain_x0_25", "osnet_ibn_x0_25"])
def golden(request, golden_dir):
    g = np.load(os.path.join(golden_dir, request.param + ".npz"))
    sd = {k[4:]: g[k] for k in g.files if k.startswith("sd__")}
    rng = np.random.default_rng(int(g["input_seed"]))
    cases = {}
    for key, shape in (("features", (4, 3, 256, 128)), ("features_small", (2, 3, 64, 32))):
        cases[key] = (torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda(),
                      g[key])
    return request.param, sd, cases


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("key", ["features", "features_small"])
def test_network_matches_reference(golden, key, half):
    name, sd, cases = golden
    x, ref = cases[key]
    y = OSNetReID(name, sd, device="cuda:0", half=half)(x.half() if half else x)
    assert y.dtype == (torch.float16 if half else torch.float32)
    err = np.abs(y.float().cpu().numpy() - ref).max() / np.abs(ref).max()
    print(name, key, "f16" if half else "f32", "error / scale", err)
    assert err <= (2e-2 if half else 1e-4)


@pytest.mark.parametrize("name", ["osnet_ain_x1_0", "osnet_ibn_x1_0"])
def test_hip_forward_matches_torch_graph_x1_0(name):
    """The x1_0 channel counts (256 / 384 / 512) without an 8 MB fixture: the all-HIP forward
    against the same folded graph on PyTorch's kernels (hip=False), random weights with the
    instance-norm pairs randomised."""
    sd = random_state_dict(name, 3)
    rng = np.random.default_rng(4)
    for k in [k for k in sd if k.endswith(".IN.weight") or k == "conv1.bn.weight"]:
        c = sd[k].shape[0]
        gam = rng.uniform(0.75, 1.25, c)
        gam[::5] *= -1
        sd[k] = gam.astype(np.float32)
        sd[k[:-6] + "bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
    x = torch.from_numpy(rng.standard_normal((2, 3, 256, 128)).astype(np.float32)).cuda()
    a = OSNetReID(name, sd, device="cuda:0")(x)
    b = OSNetReID(name, sd, device="cuda:0", hip=False)(x)
    err = (a - b).abs().max().item() / b.abs().max().item()
    print(name, "hip vs torch graph, error / scale", err)
    assert a.shape == (2, 512) and b.abs().max().item() > 0
    assert err <= 1e-5


def test_weight_file_and_create_tracker(tmp_path):
    """A reference-format osnet_ain_x1_0 checkpoint ({'state_dict': ...}, 'module.' prefixes) loads
    through ReIDDetectMultiBackend; get_features = OSNet(crops) / global norm; create_tracker
    builds the producer from the path with no tracker change."""
    from yolo_tracking_amd import create_tracker, get_tracker_config
    from yolo_tracking_amd.synth import make_frames
    sd = random_state_dict("osnet_ain_x1_0", 5)
    w = tmp_path / "osnet_ain_x1_0_msmt17.pt"
    torch.save({"state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, w)
    reid = ReIDDetectMultiBackend(w, device=0, fp16=False)
    assert reid.model.name == "osnet_ain_x1_0"
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    boxes = np.array([[10, 20, 110, 300], [300, 50, 380, 250], [500, 100, 639, 479]], np.float64)
    f = reid.get_features(boxes, img)
    raw = OSNetReID("osnet_ain_x1_0", sd, device="cuda:0")(reid.preprocess(boxes, img)).cpu().numpy()
    np.testing.assert_allclose(f, raw / np.linalg.norm(raw), rtol=1e-5, atol=1e-7)
    t = create_tracker("botsort", get_tracker_config("botsort"), w, "0", False, False)
    assert isinstance(t.model, ReIDDetectMultiBackend) and t.model.model.kind == "ain"
    img = rng.integers(0, 256, (640, 640, 3), dtype=np.uint8)
    r = np.asarray(t.update(make_frames(24, 1, 5, canvas=600.0)[0][0], img))
    assert r.size == 0 or r.shape[1] == 8
    with pytest.raises(FileNotFoundError):
        ReIDDetectMultiBackend(tmp_path / "osnet_ain_x1_0_missing.pt", device=0)
    with pytest.raises(NotImplementedError, match="osnet_ain_x1_0"):
        ReIDDetectMultiBackend(tmp_path / "resnet50_msmt17.pt", device=0)
