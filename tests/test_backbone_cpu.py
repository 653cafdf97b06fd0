"""appearance/_backbone.py, the driver layer the ReID backbones share: BatchNorm folding against
PyTorch's own eval-mode modules, the k-major weight layout, and the chunked call of the base
class.  No GPU: the kernel and network tests of each family exercise Kernels."""
import numpy as np
import torch
import torch.nn.functional as F

from yolo_tracking_amd.appearance._backbone import (BN_EPS, ReIDBackbone, bn_affine, fold_bn,
                                                    kmajor, to_f64)

EPS = float(np.finfo(np.float64).eps)   # 2^-52, one ulp of 1.0; a rounding errs by at most EPS / 2
# The asserted bound on |folded - bn(layer(x))|, in ulps of the largest output (EPS max |ref|).
# The fold adds two roundings to what both sides do anyway: w' = fl(w s) on every weight, and the
# folded bias (fl(mean s), fl(beta - .), fl(cb s), fl(. + .): at most 3 on one term).  Those four
# half-ulp errors act on terms whose absolute sum A (see _bound) the inputs below keep under twice
# the largest output (asserted), so their worst case is 4 (EPS / 2) A <= 4 ulps.  Everything else
# (the layer's k products and sums, the BatchNorm's own handful of operations) is done by both
# sides in the same order, but on operands that differ by those roundings, so the two sides' errors
# do not cancel: they differ like two walks of the same length, by about as much as the fold's own
# roundings again, not by the worst case of _bound.  Twice 4 ulps: 8.  This is not a worst-case
# bound; _bound's (k + 8) EPS A is, and is asserted as well.
FEW_ULPS = 8


def _bn_stats(bn, g):
    """Non-trivial running statistics and affine pair."""
    c = bn.num_features
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 0.5)
        bn.running_var.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64) * 1.5)
        bn.weight.copy_(0.5 + torch.rand(c, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(c, generator=g, dtype=torch.float64) * 0.3)
    return bn.eval()


def _state(layer, bn):
    sd = {"c." + k: v for k, v in layer.state_dict().items()}
    sd.update({"b." + k: v for k, v in bn.state_dict().items() if k != "num_batches_tracked"})
    return to_f64(sd)


def _bound(k, x, layer, bn, apply):
    """(worst-case bound on |folded - bn(layer(x))|, A), from the inputs alone.

    With s = gamma / sqrt(var + eps) both sides evaluate, per output element,
        y = sum_{i < k} (s w_i) x_i + s cb - s mean + beta,
    whose terms have the absolute sum A = sum |s w_i x_i| + |s cb| + |s mean| + |beta| (computed
    below, maximised over the output; A >= max |y|).  Every rounding a term passes through
    changes the result by at most u A to first order, u = EPS / 2, so count the roundings on the
    longest path of each side:
      folded:     s itself (add, sqrt, divide: 3); the two roundings the fold adds, w' = fl(w s)
                  on the weights (1) and, on the bias side, fl(mean s), fl(beta - .), fl(cb s),
                  fl(. + .) of which a term passes through at most 3; the k products and k
                  additions of the layer, at most k + 1 per term.            3 + 1 + 3 + k + 1
      reference:  the same k + 1 in the layer; then - mean (1), times 1 / sqrt(var + eps) (1,
                  and 3 for that factor), times gamma (1), + beta (1).       k + 1 + 7
    The accumulations run in the same order on both sides but on differently rounded operands, so
    their errors do not cancel.  Sum: 2 (k + 8) u A = (k + 8) EPS A, of which the fold's own two
    roundings are 2 EPS A; fused multiply-adds or another summation order only round less.  A
    wrong epsilon, a dropped conv bias or a scale on the wrong axis is off by 1e-6 A or more."""
    sd = _state(layer, bn)
    s = sd["b.weight"] / (sd["b.running_var"] + bn.eps).sqrt()
    shape = (-1,) + (1,) * (sd["c.weight"].dim() - 1)
    a = apply(x.abs(), (sd["c.weight"] * s.reshape(shape)).abs(),
              (s * sd["c.bias"]).abs() + (s * sd["b.running_mean"]).abs() + sd["b.bias"].abs())
    return (k + 8) * EPS * a.max().item(), a.max().item()


def test_fold_bn_conv_with_bias_matches_batchnorm_of_conv():
    g = torch.Generator().manual_seed(0)
    conv = torch.nn.Conv2d(3, 4, 3, padding=1, bias=True).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64) * 0.4)
        conv.bias.copy_(torch.randn(4, generator=g, dtype=torch.float64))
    bn = _bn_stats(torch.nn.BatchNorm2d(4).double(), g)
    assert bn.eps == BN_EPS
    x = torch.randn((2, 3, 7, 5), generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = bn(conv(x))
    w, b = fold_bn(_state(conv, bn), "c", "b")
    assert w.dtype == b.dtype == torch.float64 and w.shape == conv.weight.shape and b.shape == (4,)
    got = F.conv2d(x, w, b, padding=1)
    err = (got - ref).abs().max().item()
    bound, a = _bound(27, x, conv, bn, lambda xa, wa, ba: F.conv2d(xa, wa, ba, padding=1))
    top = ref.abs().max().item()
    print(f"folded 3x3 conv + bias: max error {err:.3e} = {err / (EPS * top):.2f} ulps of the "
          f"largest output {top:.3f}; A = {a / top:.2f} of it; worst case "
          f"{bound / (EPS * top):.1f} ulps")
    assert a <= 2 * top                      # the inputs: little cancels at the largest output
    assert err <= FEW_ULPS * EPS * top
    assert err <= bound
    # the bias is part of the fold: without it the result is off by s * conv.bias
    sd = _state(conv, bn)
    del sd["c.bias"]
    _, b0 = fold_bn(sd, "c", "b")
    scale, shift = bn_affine(sd, "b")
    assert torch.equal(b0, shift) and torch.equal(b, shift + _state(conv, bn)["c.bias"] * scale)
    assert (b - b0).abs().min().item() > 1e3 * bound


def test_fold_bn_takes_a_linear_weight_as_it_takes_a_conv_weight():
    g = torch.Generator().manual_seed(1)
    lin = torch.nn.Linear(5, 4, bias=True).double()
    with torch.no_grad():
        lin.weight.copy_(torch.randn((4, 5), generator=g, dtype=torch.float64))
        lin.bias.copy_(torch.randn(4, generator=g, dtype=torch.float64))
    bn = _bn_stats(torch.nn.BatchNorm1d(4).double(), g)
    x = torch.randn((6, 5), generator=g, dtype=torch.float64)
    with torch.no_grad():
        ref = bn(lin(x))
    sd = _state(lin, bn)
    w, b = fold_bn(sd, "c", "b")
    assert w.shape == (4, 5)
    err = (F.linear(x, w, b) - ref).abs().max().item()
    bound, a = _bound(5, x, lin, bn, F.linear)
    top = ref.abs().max().item()
    print(f"folded linear + bias: max error {err:.3e} = {err / (EPS * top):.2f} ulps of the "
          f"largest output {top:.3f}; A = {a / top:.2f} of it; worst case "
          f"{bound / (EPS * top):.1f} ulps")
    assert a <= 2 * top
    assert err <= FEW_ULPS * EPS * top
    assert err <= bound
    # the same weight as a 1x1 convolution goes through the same function to the same numbers
    sd4 = dict(sd, **{"c.weight": sd["c.weight"].reshape(4, 5, 1, 1)})
    w4, b4 = fold_bn(sd4, "c", "b")
    assert w4.shape == (4, 5, 1, 1) and torch.equal(w4.reshape(4, 5), w) and torch.equal(b4, b)


def test_to_f64_drops_prefixes_and_takes_arrays():
    sd = to_f64({"a.weight": np.ones(2, np.float32), "classifier.weight": torch.ones(3),
                 "classifier_proj.weight": torch.ones(3)}, drop=("classifier.",))
    assert sorted(sd) == ["a.weight", "classifier_proj.weight"]
    assert all(v.dtype == torch.float64 for v in sd.values())
    assert sorted(to_f64({"classifier.weight": torch.ones(1)})) == ["classifier.weight"]


def test_kmajor_layout():
    """[groups][K][cout_g] float32 from (groups * cout_g, K, 1, 1): element (g, k, o) is the
    weight of output channel g * cout_g + o at input channel k."""
    G, cg, K = 2, 3, 5
    w = torch.arange(G * cg * K, dtype=torch.float64).reshape(G * cg, K, 1, 1)
    km = kmajor(w, "cpu", groups=G)
    assert km.dtype == torch.float32 and km.shape == (G, K, cg) and km.is_contiguous()
    for g_ in range(G):
        for k in range(K):
            for o in range(cg):
                assert km[g_, k, o].item() == w[g_ * cg + o, k, 0, 0].item()
    one = kmajor(w.reshape(G * cg, K), "cpu")
    assert one.shape == (1, K, G * cg) and torch.equal(one[0], w.reshape(G * cg, K).t().float())


class _Stub(ReIDBackbone):
    def __init__(self, chunk):
        self._setup("cpu", False, True, chunk)
        self.calls = []

    def _forward(self, crops):
        self.calls.append((crops.shape[0], torch.is_grad_enabled()))
        return crops.flatten(1)[:, :2] + 1.0


def test_chunked_call_slices_in_order():
    net = _Stub(chunk=2)
    assert net.chunk == 2 and not net.hip and net.K is None and net.dtype == torch.float32
    x = torch.arange(5 * 3 * 2 * 2, dtype=torch.float32).reshape(5, 3, 2, 2).requires_grad_()
    y = net(x)
    assert net.calls == [(2, False), (2, False), (1, False)]       # slice lengths, under no_grad
    assert torch.equal(y, x.detach().reshape(5, -1)[:, :2] + 1.0)  # concatenated in crop order
    net.calls.clear()
    y = net(x[:2])
    assert net.calls == [(2, False)] and y.shape == (2, 2)         # n <= chunk: exactly one call
    net.calls.clear()
    y = net(x[:0])                                                 # no crops: one call, as before
    assert net.calls == [(0, False)] and y.shape == (0, 2)
