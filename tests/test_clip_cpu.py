"""CPU: the CLIP-ReID graph (appearance/clip.py: patch embedding, tokens, twelve pre-norm blocks
with QuickGELU, the last block on token 0 alone, the necks folded into ln_post and proj) against
the reference's VisionTransformer and necks in eval mode (tests/golden/clip_small.npz: net "a"
width 128 / 2 heads / 129 tokens, net "b" width 64 / 16 tokens, weights regenerated from the
stored seeds), float32 on PyTorch's CPU operators, and one block against the reference's
ResidualAttentionBlock.  Bar per net: max(1e-5, 4 x the reference's own float32-versus-float64
deviation stored with it) of the feature scale (the project's CPU rule)."""
import re

import numpy as np
import pytest
import torch

import clip_golden
from yolo_tracking_amd.appearance import clip as C
from yolo_tracking_amd.appearance import mlfn, mobilenetv2, osnet

KEYS = list(clip_golden.NETS)


@pytest.mark.parametrize("key", KEYS)
def test_graph_matches_reference_module(key):
    sd, x, ref, dev = clip_golden.load()[1][key]
    width, (gh, gw), od, crops = clip_golden.NETS[key]
    net = C.ClipReID("clip", sd, device="cpu")
    assert not net.hip and net.name == "clip" and net.feature_dim == width + od
    assert (net.width, net.tokens, net.output_dim, net.layers) == (width, gh * gw + 1, od, 12)
    y = net(torch.from_numpy(x)).numpy()
    assert y.dtype == np.float32 and y.shape == ref.shape == (crops, width + od)
    err, scale = np.abs(y - ref).max(), np.abs(ref).max()
    bar = max(1e-5, 4 * dev)
    print(key, "error / scale", err / scale, "bar", bar, "reference float32 vs float64", dev)
    assert err <= bar * scale
    y64 = C.ClipReID("clip", sd, device="cpu", hip=False, double=True)(torch.from_numpy(x))
    assert y64.dtype == torch.float64
    assert np.abs(y64.numpy() - ref).max() <= bar * scale


def test_block_matches_reference_block():
    bsd, x, y_ref = clip_golden.load()[2]
    blk = C.ClipBlock(bsd, 64, device="cpu")
    assert not blk.hip
    y = blk(torch.from_numpy(x)).numpy()
    assert y.shape == y_ref.shape == (2, 9, 64)
    err = np.abs(y - y_ref).max() / np.abs(y_ref).max()
    print("block error / scale", err)
    assert err <= 1e-5


def test_checksum_guard(monkeypatch):
    """A drifted generator is reported as such, not as a wrong network."""
    clip_golden.load()
    real = C.random_state_dict

    def drifted(*a, **k):
        sd = real(*a, **k)
        sd["image_encoder.proj"] = sd["image_encoder.proj"] * np.float32(1.001)
        return sd
    monkeypatch.setattr(C, "random_state_dict", drifted)
    monkeypatch.setattr(clip_golden, "_cache", {})
    with pytest.raises(AssertionError, match="random_state_dict drifted"):
        clip_golden.load()


def test_fixture_is_small_and_has_no_network_weights():
    g = clip_golden.load()[0]
    assert not any("__sd__" in k and not k.startswith("blk__") for k in g.files)
    assert sum(g[k].size for k in g.files if g[k].dtype.kind == "f") < 100_000
    assert all(float(g[k + "__f64dev"]) <= 1e-5 for k in KEYS)   # the GPU test's 1e-4 presumes it


def test_random_state_dict_has_the_recorded_keys_and_shapes():
    g = clip_golden.load()[0]
    recorded = {str(k): tuple(int(v) for v in d if v)
                for k, d in zip(g["shapes__keys"], g["shapes__dims"])}
    assert len(recorded) == 5 + 12 * 12 + 3 + 8
    for k in ("image_encoder.conv1.weight", "image_encoder.class_embedding",
              "image_encoder.positional_embedding", "image_encoder.ln_pre.bias",
              "image_encoder.transformer.resblocks.11.attn.in_proj_weight",
              "image_encoder.transformer.resblocks.0.mlp.c_proj.bias", "image_encoder.proj",
              "bottleneck.running_var", "bottleneck_proj.weight"):
        assert k in recorded, k
    assert recorded["image_encoder.positional_embedding"] == (129, 768)
    assert recorded["image_encoder.proj"] == (768, 512)
    rnd = C.random_state_dict(1)
    assert {k: v.shape for k, v in rnd.items()} == recorded
    assert all(v.dtype == np.float32 for v in rnd.values())
    assert not any(k.startswith("classifier") for k in rnd)
    a, b = C.random_state_dict(2, 64, 15, 16), C.random_state_dict(2, 64, 15, 16)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["image_encoder.proj"],
                              C.random_state_dict(3, 64, 15, 16)["image_encoder.proj"])
    w = a["image_encoder.transformer.resblocks.0.attn.in_proj_weight"]
    assert w[:128].std() > 1.3 * w[128:].std()            # the q and k rows times 1.5
    assert 0.75 <= a["bottleneck.running_var"].min() and a["image_encoder.ln_pre.weight"].max() \
        <= 1.25


def test_variants_and_model_names(tmp_path):
    assert C.VARIANTS == {"clip": (768, 12, 512)}
    clips = ("clip_market1501.pt", "clip_duke.pt", "clip_veri.pt", "clip_vehicleid.pt")
    assert C.model_name("clip_market1501.pt") == "clip"
    assert C.model_name("weights/clip_duke.pt") == "clip"
    assert C.model_name(tmp_path / "clip_veri.pt") == "clip"
    for other in ("osnet_x0_25_msmt17.pt", "osnet_ain_x1_0_msmt17.pt", "osnet_ibn_x1_0_msmt17.pt",
                  "mobilenetv2_x1_4_dukemtmcreid.pt", "mlfn_msmt17.pt", "resnet50_msmt17.pt",
                  "hacnn_market1501.pt", "lmbn_n_cuhk03_d.pt"):
        assert C.model_name(other) is None, other
    assert C.model_name("clips/osnet_x0_25_msmt17.pt") is None       # the directory does not count
    assert osnet.model_name("clips/osnet_x0_25_msmt17.pt") == "osnet_x0_25"
    for name in clips:
        assert osnet.model_name(name) is None and mobilenetv2.model_name(name) is None
        assert mlfn.model_name(name) is None


def test_backend_dispatch_errors(tmp_path):
    """The name dispatch runs before any device work: a missing CLIP file is a
    FileNotFoundError, ResNet still NotImplementedError with every rebuilt network named; a file
    of another family in a directory called clips/ is looked for as that family."""
    from yolo_tracking_amd.appearance import ReIDDetectMultiBackend
    with pytest.raises(FileNotFoundError, match="clip"):
        ReIDDetectMultiBackend(tmp_path / "clip_market1501.pt", device=0)
    with pytest.raises(NotImplementedError, match="clip") as e:
        ReIDDetectMultiBackend(tmp_path / "resnet50_msmt17.pt", device=0)
    text = str(e.value)
    assert all(n in text for n in ("osnet_x0_25", "osnet_ibn_x1_0", "osnet_ain_x1_0",
                                   "mobilenetv2_x1_0", "mobilenetv2_x1_4", "mlfn", "clip"))
    (tmp_path / "clips").mkdir()
    with pytest.raises(FileNotFoundError, match="osnet_x0_25"):
        ReIDDetectMultiBackend(tmp_path / "clips" / "osnet_x0_25_msmt17.pt", device=0)


def test_unsupported_checkpoints_are_value_errors():
    with pytest.raises(ValueError, match="width 96"):
        C.ClipReID("clip", C.random_state_dict(1, 96, 15, 16), device="cpu")
    with pytest.raises(ValueError, match="11 transformer layers"):
        C.ClipReID("clip", C.random_state_dict(1, 64, 15, 16, layers=11), device="cpu")
    sd = C.random_state_dict(1, 64, 15, 16)
    p14 = dict(sd)
    p14["image_encoder.conv1.weight"] = np.zeros((64, 3, 14, 14), np.float32)
    with pytest.raises(ValueError, match="patch size 14"):
        C.ClipReID("clip", p14, device="cpu")
    net = C.ClipReID("clip", sd, device="cpu")
    assert net(torch.zeros(1, 3, 48, 80)).shape == (1, 80)
    with pytest.raises(ValueError, match="129 tokens.*16 rows.*another resolution"):
        net(torch.zeros(1, 3, 256, 128))
    with pytest.raises(ValueError, match="40 x 80"):
        net(torch.zeros(1, 3, 40, 80))
    sie = dict(sd)
    sie["cv_embed"] = np.zeros((6, 64), np.float32)
    with pytest.raises(ValueError, match="cv_embed"):
        C.ClipReID("clip", sie, device="cpu")
    rn50 = {"image_encoder.layer1.0.conv1.weight": np.zeros((64, 64, 1, 1), np.float32),
            "image_encoder.attnpool.positional_embedding": np.zeros((129, 2048), np.float32)}
    with pytest.raises(ValueError, match="RN50"):
        C.ClipReID("clip", rn50, device="cpu")
    with pytest.raises(KeyError):
        C.ClipReID("clip_rn50", sd, device="cpu")
    with pytest.raises(ValueError, match="float64"):
        C.ClipReID("clip", sd, device="cpu", half=True, double=True)


def test_checkpoint_extras_are_ignored():
    """classifier.weight and classifier_proj.weight of a real checkpoint do not matter."""
    sd, x, ref, dev = clip_golden.load()[1]["b"]
    more = dict(sd)
    more["classifier.weight"] = np.ones((751, 64), np.float32)
    more["classifier_proj.weight"] = np.ones((751, 16), np.float32)
    a = C.ClipReID("clip", sd, device="cpu")(torch.from_numpy(x))
    assert torch.equal(a, C.ClipReID("clip", more, device="cpu")(torch.from_numpy(x)))
    one = C.ClipReID("clip", sd, device="cpu", chunk=1)(torch.from_numpy(x))   # crop by crop
    assert one.shape == a.shape and (one - a).abs().max().item() <= 1e-5 * a.abs().max().item()


def test_library_exports_the_clip_entries():
    from yolo_tracking_amd import _lib
    names = ("yta_clip_linear", "yta_clip_layernorm", "yta_clip_patches", "yta_clip_tokens",
             "yta_clip_attention")
    lib = _lib.load_library()
    header = open(_lib.__file__.replace("yolo_tracking_amd/_lib.py",
                                        "include/yolo_tracking_amd.h")).read()
    for n in names:
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None
        assert re.search(r"\bint %s\(" % n, header), n
