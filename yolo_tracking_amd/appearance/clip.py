"""CLIP-ReID ViT-B/16 feature extractor for the MI355X ReID producer.

Reference: boxmot/appearance/backbones/clip/make_model.py build_transformer (:96-122, eval mode,
MODEL.NAME 'ViT-B-16', STRIDE_SIZE [16, 16], TEST.NECK_FEAT 'after', no SIE embedding) around
clip/clip/model.py VisionTransformer (:204-262): a 16 x 16 stride-16 patch convolution without
bias, the class embedding as token 0, the positional embedding, ln_pre, twelve
ResidualAttentionBlocks (x += out_proj(MHA(ln_1(x))); x += c_proj(QuickGELU(c_fc(ln_2(x))))),
then c = ln_post(token 0), p = c @ proj and cat(bottleneck(c), bottleneck_proj(p)): width +
output_dim = 1280 values.  As the other backbones this is an inference graph, not a module tree.
Parameters come from a checkpoint in the reference's key layout (image_encoder.conv1.weight,
image_encoder.transformer.resblocks.3.attn.in_proj_weight, image_encoder.proj,
bottleneck.running_var, ...), so the reference's .pt files load unchanged; classifier.weight and
classifier_proj.weight are ignored.  Sizes are read from the state dict as model.py:424-453 reads
them.  The two eval-mode BatchNorm1d necks are folded on the host in float64: bottleneck into a
second affine of ln_post (the first 768 features are one layer norm of token 0), bottleneck_proj
into proj's columns and a bias.  Only token 0 of the last block is used (model.py:252-262 with
make_model.py:108-109), so its ln_1 and k | v projections run on all tokens and everything else
of it on row 0 of each sample.  Parity with the reference module is pinned by
tests/golden/clip_small.npz.

On a GPU every layer runs in HIP (csrc/clip.hip): yta_clip_patches, yta_clip_linear (the patch
embedding, the four projections of a block with bias, QuickGELU and the residual in the epilogue,
the final projection), yta_clip_tokens, yta_clip_layernorm, yta_clip_attention.  Weights are held
as the checkpoint stores them ([out][in], the layout yta_clip_linear takes) in the storage type;
biases and layer-norm parameters stay float32.  `hip=False` runs the same folded graph on
PyTorch's operators: what a CPU device gets, and the measurement baseline; `double=True` (only
with hip=False) evaluates it in float64, the tests' yardstick.
"""
import re
from pathlib import Path

import numpy as np

from ._backbone import ReIDBackbone, bn_affine

# name -> (width, layers, output_dim): ViT-B/16 (make_model.py:42-44)
VARIANTS = {"clip": (768, 12, 512)}
PATCH = 16
HEAD_DIM = 64
LAYERS = 12          # model.py:252-253 hard-codes resblocks[:11] and resblocks[11]
LN_EPS = 1e-5        # nn.LayerNorm's default
MAX_TOKENS = 256     # yta_clip_attention keeps a head's K and V in LDS
# crops per forward pass.  A crop's activations at 129 tokens of width 768: tokens, a normed copy
# and the attention output (3 x 0.4 MB in float32), q | k | v (1.2 MB) and the MLP hidden
# (1.6 MB), 4 MB in all: 256 crops bound the workspace at 1 GB in float32 (0.5 GB in float16) and
# give the GEMMs 33024 rows, 258 row tiles of 128 for the 256 CUs (measured at 256 crops, DESIGN
# 9.4: 64.5 ms per forward in float32 against 74.1 ms in chunks of 64, 22.6 against 27.2 ms in
# float16).
CHUNK = 256

_BLOCK_KEYS = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias",
               "attn.out_proj.weight", "attn.out_proj.bias", "ln_2.weight", "ln_2.bias",
               "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")


def model_name(weights):
    """'clip' where it occurs in the weight file's name (reid_model_factory.get_model_name tests
    model.name, not the path)."""
    s = Path(str(weights)).name
    for name in VARIANTS:
        if name in s:
            return name
    return None


def _draw_block(rng, sd, key, width):
    """One ResidualAttentionBlock's parameters under `key`, in _BLOCK_KEYS' order."""
    def ln(k):
        sd[k + ".weight"] = rng.uniform(0.75, 1.25, width).astype(np.float32)
        sd[k + ".bias"] = rng.normal(0, 0.1, width).astype(np.float32)

    def linear(k, fout, fin):
        sd[k + ".weight"] = rng.normal(0, fin ** -0.5, (fout, fin)).astype(np.float32)
        sd[k + ".bias"] = rng.normal(0, 0.1, fout).astype(np.float32)

    ln(key + "ln_1")
    w = rng.normal(0, width ** -0.5, (3 * width, width))
    w[:2 * width] *= 1.5
    sd[key + "attn.in_proj_weight"] = w.astype(np.float32)
    sd[key + "attn.in_proj_bias"] = rng.normal(0, 0.1, 3 * width).astype(np.float32)
    linear(key + "attn.out_proj", width, width)
    ln(key + "ln_2")
    linear(key + "mlp.c_fc", 4 * width, width)
    linear(key + "mlp.c_proj", width, 4 * width)


def random_block_state_dict(seed, width):
    """One ResidualAttentionBlock's state_dict (keys without a prefix), drawn as
    random_state_dict draws a block's."""
    sd = {}
    _draw_block(np.random.default_rng(seed), sd, "", width)
    return sd


def random_state_dict(seed=0, width=768, grid=128, output_dim=512, layers=12):
    """A state_dict in the checkpoint's key layout, without the classifiers, all float32.

    Drawn from np.random.default_rng(seed) in this order: image_encoder.conv1.weight
    N(0, 1/768); class_embedding, positional_embedding N(0, 0.5^2); ln_pre weight, bias; per
    block transformer.resblocks.{i}: ln_1 weight, bias; attn.in_proj_weight N(0, 1/width) with
    the q and k rows times 1.5; attn.in_proj_bias; attn.out_proj weight, bias; ln_2 weight, bias;
    mlp.c_fc weight, bias; mlp.c_proj weight, bias; then ln_post weight, bias; proj
    N(0, 1/width); bottleneck and bottleneck_proj: running_mean N(0, 0.1^2), running_var
    U[0.75, 1.25], weight U[0.75, 1.25], bias N(0, 0.1^2) in this order.  Every layer-norm weight
    is U[0.75, 1.25] and bias N(0, 0.1^2); every Linear weight N(0, 1/fan_in) and bias
    N(0, 0.1^2).  With this recipe the softmax is neither uniform nor one-hot (mean maximal
    probability 0.14-0.56 per layer)."""
    rng = np.random.default_rng(seed)
    sd = {}
    e = "image_encoder."
    sd[e + "conv1.weight"] = rng.normal(0, 768 ** -0.5, (width, 3, PATCH, PATCH)) \
        .astype(np.float32)
    sd[e + "class_embedding"] = rng.normal(0, 0.5, width).astype(np.float32)
    sd[e + "positional_embedding"] = rng.normal(0, 0.5, (grid + 1, width)).astype(np.float32)
    sd[e + "ln_pre.weight"] = rng.uniform(0.75, 1.25, width).astype(np.float32)
    sd[e + "ln_pre.bias"] = rng.normal(0, 0.1, width).astype(np.float32)
    for i in range(layers):
        _draw_block(rng, sd, f"{e}transformer.resblocks.{i}.", width)
    sd[e + "ln_post.weight"] = rng.uniform(0.75, 1.25, width).astype(np.float32)
    sd[e + "ln_post.bias"] = rng.normal(0, 0.1, width).astype(np.float32)
    sd[e + "proj"] = rng.normal(0, width ** -0.5, (width, output_dim)).astype(np.float32)
    for key, c in (("bottleneck", width), ("bottleneck_proj", output_dim)):
        sd[key + ".running_mean"] = rng.normal(0, 0.1, c).astype(np.float32)
        sd[key + ".running_var"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
        sd[key + ".weight"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
        sd[key + ".bias"] = rng.normal(0, 0.1, c).astype(np.float32)
    return sd


def _tensor(torch, v):
    return v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))


# csrc/clip.hip's entry points on row-major matrices, through the shared Kernels `K`.  Operands
# are addresses (a tensor's data_ptr() plus a byte offset) with row strides in elements.
def _linear(K, x, xs, m, k, w, ws, bias, nout, y, ys, act=0, res=None, rs=0):
    K.call("yta_clip_linear", x, xs, w, ws, bias, res, rs, m, k, nout, act, K.half, y, ys)


def _layernorm(K, x, xs, m, c, gamma, beta, y, ys):
    K.call("yta_clip_layernorm", x, xs, m, c, gamma.data_ptr(), beta.data_ptr(), LN_EPS, K.half, y,
           ys)


def _attention_hip(K, qkv, n, L, width, lq, y):
    K.call("yta_clip_attention", qkv.data_ptr(), n, L, width, HEAD_DIM, lq, K.half, y.data_ptr())


class _BlockParams:
    """One ResidualAttentionBlock's parameters from a state_dict whose keys start with `prefix`:
    .T in the graph's dtype for PyTorch's operators, .H for the kernels (weights in the storage
    type, biases and layer-norm parameters float32)."""

    def __init__(self, torch, sd, prefix, width, device, dtype, hip):
        shapes = {"ln_1.weight": (width,), "ln_1.bias": (width,),
                  "attn.in_proj_weight": (3 * width, width), "attn.in_proj_bias": (3 * width,),
                  "attn.out_proj.weight": (width, width), "attn.out_proj.bias": (width,),
                  "ln_2.weight": (width,), "ln_2.bias": (width,),
                  "mlp.c_fc.weight": (4 * width, width), "mlp.c_fc.bias": (4 * width,),
                  "mlp.c_proj.weight": (width, 4 * width), "mlp.c_proj.bias": (width,)}
        self.T = self.H = None
        out = {}
        for k in _BLOCK_KEYS:
            if prefix + k not in sd:
                raise ValueError(f"the state_dict has no {prefix + k}")
            v = _tensor(torch, sd[prefix + k])
            if tuple(v.shape) != shapes[k]:
                raise ValueError(f"{prefix + k} is {tuple(v.shape)}, expected {shapes[k]}")
            matrix = hip and v.dim() == 2
            out[k] = v.to(device, dtype if (matrix or not hip) else torch.float32).contiguous()
        if hip:
            self.H = out
        else:
            self.T = out


def _attention_torch(torch, q, k, v):
    """softmax(q k^T / 8) v per head on (n, rows, width) tensors; the softmax in float32 where the
    storage is float16."""
    n, lq, w = q.shape
    heads = w // HEAD_DIM

    def split(t):
        return t.reshape(n, t.shape[1], heads, HEAD_DIM).transpose(1, 2)
    s = (split(q) * 0.125) @ split(k).transpose(-1, -2)
    s = s.float() if s.dtype == torch.float16 else s
    s = s - s.max(dim=-1, keepdim=True).values
    p = s.exp()
    p = (p / p.sum(dim=-1, keepdim=True)).to(q.dtype)
    return (p @ split(v)).transpose(1, 2).reshape(n, lq, w)


def _quick_gelu(torch, x):
    return x * torch.sigmoid(1.702 * x)


def _block_torch(torch, b, x, last=False, attention=_attention_torch, act=_quick_gelu):
    """x (n, L, width) -> the block's result, (n, 1, width) (token 0) where last."""
    F = torch.nn.functional
    T = b.T
    w = x.shape[-1]
    h = F.layer_norm(x, (w,), T["ln_1.weight"], T["ln_1.bias"], LN_EPS)
    wi, bi = T["attn.in_proj_weight"], T["attn.in_proj_bias"]
    if last:
        q = F.linear(h[:, :1], wi[:w], bi[:w])
        k, v = F.linear(h, wi[w:], bi[w:]).chunk(2, dim=-1)
        x = x[:, :1]
    else:
        q, k, v = F.linear(h, wi, bi).chunk(3, dim=-1)
    a = attention(torch, q, k, v)
    x = x + F.linear(a, T["attn.out_proj.weight"], T["attn.out_proj.bias"])
    h = F.layer_norm(x, (w,), T["ln_2.weight"], T["ln_2.bias"], LN_EPS)
    m = act(torch, F.linear(h, T["mlp.c_fc.weight"], T["mlp.c_fc.bias"]))
    return x + F.linear(m, T["mlp.c_proj.weight"], T["mlp.c_proj.bias"])


def _block_hip(K, b, x, n, L, w, last=False):
    """x contiguous (n, L, w), updated in place -> x, or a new (n, w) (token 0) where last."""
    H, es = b.H, K.es
    m = n * L
    h = K.empty(m, w)
    _layernorm(K, x.data_ptr(), w, m, w, H["ln_1.weight"], H["ln_1.bias"], h.data_ptr(), w)
    qkv = K.empty(n, L, 3 * w)
    wi, bi = H["attn.in_proj_weight"].data_ptr(), H["attn.in_proj_bias"].data_ptr()
    wo, bo = H["attn.out_proj.weight"].data_ptr(), H["attn.out_proj.bias"].data_ptr()
    wf, bf = H["mlp.c_fc.weight"].data_ptr(), H["mlp.c_fc.bias"].data_ptr()
    wp, bp = H["mlp.c_proj.weight"].data_ptr(), H["mlp.c_proj.bias"].data_ptr()
    if last:
        # k | v of every token into their columns; q of token 0 of each sample into its row
        _linear(K, h.data_ptr(), w, m, w, wi + es * w * w, w, bi + 4 * w, 2 * w,
                qkv.data_ptr() + es * w, 3 * w)
        _linear(K, h.data_ptr(), L * w, n, w, wi, w, bi, w, qkv.data_ptr(), L * 3 * w)
        rows, lq, xs = n, 1, L * w
        y = K.empty(n, w)
    else:
        _linear(K, h.data_ptr(), w, m, w, wi, w, bi, 3 * w, qkv.data_ptr(), 3 * w)
        rows, lq, xs = m, L, w
        y = x
    a = K.empty(rows, w)
    _attention_hip(K, qkv, n, L, w, lq, a)
    _linear(K, a.data_ptr(), w, rows, w, wo, w, bo, w, y.data_ptr(), w, res=x.data_ptr(), rs=xs)
    h = h if not last else K.empty(rows, w)
    _layernorm(K, y.data_ptr(), w, rows, w, H["ln_2.weight"], H["ln_2.bias"], h.data_ptr(), w)
    hid = K.empty(rows, 4 * w)
    _linear(K, h.data_ptr(), w, rows, w, wf, w, bf, 4 * w, hid.data_ptr(), 4 * w, act=1)
    _linear(K, hid.data_ptr(), 4 * w, rows, 4 * w, wp, 4 * w, bp, w, y.data_ptr(), w,
            res=y.data_ptr(), rs=w)
    return y


class ClipBlock(ReIDBackbone):
    """One ResidualAttentionBlock (model.py:169-190) from a state_dict in the module's keys:
    x (N, L, width) -> (N, L, width).  (The reference module takes (L, N, width).)  ClipReID is
    twelve of these between the token kernel and the neck; the block fixture runs one alone."""

    def __init__(self, state_dict, width, device="cuda:0", half=False, hip=True, double=False):
        self._setup(device, half, hip, double=double)
        torch = self.torch
        self.width = int(width)
        if self.width % HEAD_DIM:
            raise ValueError(f"width {self.width} is not a multiple of the head dimension 64")
        self.params = _BlockParams(torch, state_dict, "", self.width, self.device, self.dtype,
                                   self.hip)

    def __call__(self, x):
        torch = self.torch
        with torch.no_grad():
            x = x.to(self.device, self.dtype).contiguous()
            if not self.hip:
                return _block_torch(torch, self.params, x)
            n, L, w = x.shape
            return _block_hip(self.K, self.params, x.clone(), n, L, w)


class ClipReID(ReIDBackbone):
    """Eval-mode CLIP-ReID feature extractor: crops (N, 3, H, W) -> (N, width + output_dim) in the
    crops' dtype (float32 or float16), on the crops' device.  Width, output_dim, the token count
    and the layer count come from the state_dict; `name` stands for the sizes of the freshly
    initialised network (state_dict=None)."""

    def __init__(self, name="clip", state_dict=None, device="cuda:0", half=False, chunk=CHUNK,
                 hip=True, double=False):
        if name not in VARIANTS:
            raise KeyError(f"unknown CLIP-ReID variant {name!r}")
        self._setup(device, half, hip, chunk, double=double)
        self.name = name
        if state_dict is None:
            w0, l0, o0 = VARIANTS[name]
            state_dict = random_state_dict(0, w0, 128, o0, l0)
        self._build({re.sub(r"^image_encoder\.", "", k): v for k, v in state_dict.items()})

    def _build(self, sd):
        torch = self.torch
        if "conv1.weight" not in sd or "class_embedding" not in sd or "proj" not in sd:
            hint = " (an RN50 CLIP-ReID checkpoint: only the ViT-B-16 variant is rebuilt)" \
                if any(k.startswith(("layer1.", "attnpool.")) for k in sd) else ""
            raise ValueError(f"{self.name}: the state_dict has no image_encoder.conv1.weight / "
                             f"class_embedding / proj{hint}")
        if "cv_embed" in sd:
            raise ValueError(f"{self.name}: the checkpoint has a cv_embed (SIE camera / view "
                             "embedding), which is not rebuilt")
        conv1 = _tensor(torch, sd["conv1.weight"])
        # model.py:424-453: the sizes a state dict implies
        width, patch = int(conv1.shape[0]), int(conv1.shape[-1])
        pos = _tensor(torch, sd["positional_embedding"])
        proj = _tensor(torch, sd["proj"])
        layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
        if conv1.dim() != 4 or tuple(conv1.shape[1:]) != (3, patch, patch) or patch != PATCH:
            raise ValueError(f"{self.name}: conv1.weight is {tuple(conv1.shape)}: patch size "
                             f"{patch}, only 16 x 16 patches of 3 channels are rebuilt")
        if width % HEAD_DIM:
            raise ValueError(f"{self.name}: width {width} is not a multiple of the head "
                             "dimension 64")
        if layers != LAYERS:
            raise ValueError(f"{self.name}: {layers} transformer layers, the reference's forward "
                             "takes exactly 12 (model.py:252-253)")
        if pos.dim() != 2 or pos.shape[1] != width or proj.dim() != 2 or proj.shape[0] != width:
            raise ValueError(f"{self.name}: positional_embedding {tuple(pos.shape)} / proj "
                             f"{tuple(proj.shape)} do not fit width {width}")
        self.width, self.layers = width, layers
        self.tokens = int(pos.shape[0])
        self.output_dim = int(proj.shape[1])
        self.feature_dim = width + self.output_dim
        if self.hip and self.tokens > MAX_TOKENS:
            raise ValueError(f"{self.name}: {self.tokens} tokens, the attention kernel holds at "
                             f"most {MAX_TOKENS}")

        def f64(k, shape):
            if k not in sd:
                raise ValueError(f"{self.name}: the state_dict has no {k}")
            v = _tensor(torch, sd[k]).to(torch.float64)
            if tuple(v.shape) != shape:
                raise ValueError(f"{self.name}: {k} is {tuple(v.shape)}, expected {shape}")
            return v

        # the necks, folded in float64: bottleneck into a second affine of ln_post,
        # bottleneck_proj into proj's columns and a bias
        def neck(key, c):
            return bn_affine({f"{key}.{p}": f64(f"{key}.{p}", (c,)) for p in
                              ("weight", "running_var", "bias", "running_mean")}, key)
        g, b = f64("ln_post.weight", (width,)), f64("ln_post.bias", (width,))
        s1, t1 = neck("bottleneck", width)
        s2, t2 = neck("bottleneck_proj", self.output_dim)
        small = {"cls": f64("class_embedding", (width,)), "pos": pos.to(torch.float64),
                 "pre_g": f64("ln_pre.weight", (width,)), "pre_b": f64("ln_pre.bias", (width,)),
                 "post_g": g, "post_b": b, "neck_g": g * s1, "neck_b": b * s1 + t1,
                 "proj_b": t2}
        big = {"conv1": conv1.reshape(width, 3 * PATCH * PATCH),
               "proj": (proj.to(torch.float64) * s2).t()}
        self.S = {k: v.to(self.device, torch.float32 if self.hip else self.dtype).contiguous()
                  for k, v in small.items()}
        self.W = {k: v.to(self.device, self.dtype).contiguous() for k, v in big.items()}
        self.blocks = [_BlockParams(torch, sd, f"transformer.resblocks.{i}.", width, self.device,
                                    self.dtype, self.hip) for i in range(layers)]

    def _grid(self, crops):
        n, c, h, w = crops.shape
        if c != 3 or h % PATCH or w % PATCH or (h // PATCH) * (w // PATCH) + 1 != self.tokens:
            raise ValueError(
                f"{self.name}: crops of {h} x {w} make {(h // PATCH) * (w // PATCH) + 1} tokens "
                f"of 16 x 16 patches, the checkpoint's positional embedding has {self.tokens} "
                "rows: it was trained at another resolution or patch stride")
        return n, (h // PATCH) * (w // PATCH)

    # the two pieces a sensitivity check replaces (tests/golden/make_clip_golden.py)
    _attention = staticmethod(_attention_torch)
    _act = staticmethod(_quick_gelu)

    def _forward_torch(self, crops):
        torch, S, W = self.torch, self.S, self.W
        F = torch.nn.functional
        n, g = self._grid(crops)
        w = self.width
        x = crops.to(self.device, self.dtype)
        gh, gw = x.shape[2] // PATCH, x.shape[3] // PATCH
        x = x.reshape(n, 3, gh, PATCH, gw, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(n, g, -1)
        x = F.linear(x, W["conv1"])
        x = torch.cat([S["cls"].expand(n, 1, w), x], dim=1) + S["pos"]
        x = F.layer_norm(x, (w,), S["pre_g"], S["pre_b"], LN_EPS)
        for i, b in enumerate(self.blocks):
            x = _block_torch(torch, b, x, i == self.layers - 1, self._attention, self._act)
        x = x[:, 0]
        c = F.layer_norm(x, (w,), S["post_g"], S["post_b"], LN_EPS)
        return torch.cat([F.layer_norm(x, (w,), S["neck_g"], S["neck_b"], LN_EPS),
                          F.linear(c, W["proj"], S["proj_b"])], dim=1)

    def _forward_hip(self, crops):
        K, S, W = self.K, self.S, self.W
        n, g = self._grid(crops)
        w, L, od = self.width, self.tokens, self.output_dim
        x = crops.to(self.device, self.dtype).contiguous()
        pat = K.empty(n * g, 3 * PATCH * PATCH)
        K.call("yta_clip_patches", x.data_ptr(), n, x.shape[2], x.shape[3], K.half, pat.data_ptr())
        emb = K.empty(n * g, w)
        _linear(K, pat.data_ptr(), 768, n * g, 768, W["conv1"].data_ptr(), 768, None, w,
                emb.data_ptr(), w)
        x = K.empty(n, L, w)
        K.call("yta_clip_tokens", emb.data_ptr(), w, S["cls"].data_ptr(), S["pos"].data_ptr(), n, g,
               w, S["pre_g"].data_ptr(), S["pre_b"].data_ptr(), LN_EPS, K.half, x.data_ptr())
        for i, b in enumerate(self.blocks):
            x = _block_hip(K, b, x, n, L, w, i == self.layers - 1)
        out = K.empty(n, w + od)
        _layernorm(K, x.data_ptr(), w, n, w, S["neck_g"], S["neck_b"], out.data_ptr(), w + od)
        c = K.empty(n, w)
        _layernorm(K, x.data_ptr(), w, n, w, S["post_g"], S["post_b"], c.data_ptr(), w)
        _linear(K, c.data_ptr(), w, n, w, W["proj"].data_ptr(), w, S["proj_b"].data_ptr(), od,
                out.data_ptr() + K.es * w, w + od)
        return out
