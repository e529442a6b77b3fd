"""Reference for "IP-Adapter from a picture": the fp32 Resampler (IP-Adapter Plus image projection), synthetic Resamplers and Plus adapters,
the vision encoder's penultimate hidden states and image embeddings, and the device that lets tests/ref_unet.py and tests/ref_tryon.py -- both
unmodified, both knowing only the plain ImageProjection -- run with Plus tokens.

The Resampler is tencent-ailab/IP-Adapter's, restated from memory of that package (it is not installed and was not checked against it), every
LayerNorm with eps 1e-5:

    lat = latents.expand(n)                        parameter [1, N, dim]
    x   = proj_in(x)                               Linear E -> dim, bias
    for i in range(depth):
        xn, ln = LN(norm1)(x), LN(norm2)(lat)
        q = to_q(ln); k, v = to_kv(cat([xn, ln], tokens)).chunk(2, -1)            no biases; T + N keys
        a = softmax_fp32((q s) (k s)^T) v per head, s = dim_head ** -0.25
        lat = to_out(a) + lat
        lat = W2(gelu_erf(W1(LN(lat)))) + lat                                     dim -> 4 dim -> dim, no biases
    tokens = LN(norm_out)(proj_out(lat))           Linear dim -> out_dim, bias
"""
import torch
import torch.nn.functional as F

from oracle import vision as V
from tests import ip_adapter_ref as R

EPS = 1e-5


def resampler_forward(sd, x, heads, round16=False, return_prenorm=False):
    """sd: original-layout keys (no prefix), x [n, T, E] float32 -> tokens [n, N, out_dim] (and proj_out's output before norm_out).
    round16: every Linear and LayerNorm output (and the attention's) is rounded to fp16, as a device implementation that stores fp16 between
    its kernels does -- what the GPU thresholds have to survive."""
    r = (lambda t: t.half().float()) if round16 else (lambda t: t)
    ln = lambda p, t: r(F.layer_norm(t, (t.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], EPS))
    n = x.shape[0]
    lat = sd["latents"].expand(n, -1, -1)
    N, dim = lat.shape[1], lat.shape[2]
    x = r(F.linear(x, sd["proj_in.weight"], sd["proj_in.bias"]))
    depth = 0
    while "layers.%d.0.to_q.weight" % depth in sd:
        depth += 1
    for i in range(depth):
        p = "layers.%d." % i
        xn, l2 = ln(p + "0.norm1", x), ln(p + "0.norm2", lat)
        q = r(F.linear(l2, sd[p + "0.to_q.weight"]))
        kv = r(F.linear(torch.cat([xn, l2], 1), sd[p + "0.to_kv.weight"]))
        k, v = kv.chunk(2, -1)
        inner = q.shape[-1]
        dh = inner // heads
        sp = lambda t: t.reshape(n, -1, heads, dh).transpose(1, 2)
        s = dh ** -0.25
        w = torch.softmax((sp(q) * s) @ (sp(k) * s).transpose(-1, -2), -1)
        a = r((w @ sp(v)).transpose(1, 2).reshape(n, N, inner))
        lat = r(F.linear(a, sd[p + "0.to_out.weight"]) + lat)
        h = r(F.gelu(F.linear(ln(p + "1.0", lat), sd[p + "1.1.weight"])))
        lat = r(F.linear(h, sd[p + "1.3.weight"]) + lat)
    pre = r(F.linear(lat, sd["proj_out.weight"], sd["proj_out.bias"]))
    tok = r(F.layer_norm(pre, (pre.shape[-1],), sd["norm_out.weight"], sd["norm_out.bias"], EPS))
    return (tok, pre) if return_prenorm else tok


def make_resampler(E, dim, heads, depth, N, out_dim, seed=0):
    """original-layout keys, fp16-representable float32, variance-preserving (weights randn / sqrt(fan_in), so activations stay of order 1
    through every layer), latents = randn / sqrt(dim).  The attention is as wide as the latents: inner = dim, dim_head = dim / heads."""
    g = torch.Generator().manual_seed(7300 + seed)
    rn = lambda *s: torch.randn(s, generator=g)
    h = lambda t: t.half().float()
    lin = lambda o, i: h(rn(o, i) / i ** 0.5)
    sd = {"latents": h(rn(1, N, dim) / dim ** 0.5), "proj_in.weight": lin(dim, E), "proj_in.bias": h(0.1 * rn(dim)),
          "proj_out.weight": lin(out_dim, dim), "proj_out.bias": h(0.1 * rn(out_dim)),
          "norm_out.weight": h(1.0 + 0.1 * rn(out_dim)), "norm_out.bias": h(0.1 * rn(out_dim))}
    inner = dim
    for i in range(depth):
        p = "layers.%d." % i
        for k in ("0.norm1", "0.norm2", "1.0"):
            sd[p + k + ".weight"], sd[p + k + ".bias"] = h(1.0 + 0.1 * rn(dim)), h(0.1 * rn(dim))
        sd[p + "0.to_q.weight"], sd[p + "0.to_kv.weight"], sd[p + "0.to_out.weight"] = lin(inner, dim), lin(2 * inner, dim), lin(dim, inner)
        sd[p + "1.1.weight"], sd[p + "1.3.weight"] = lin(4 * dim, dim), lin(dim, 4 * dim)
    return sd


def make_plus_adapter(cfg, E, dim, heads, depth, N, seed=0):
    """a Plus adapter under the library's keys: image_proj.<Resampler key> (out_dim = the UNet's cross-attention width) and the to_k_ip /
    to_v_ip weights of ip_adapter_ref.make_adapter"""
    rs = make_resampler(E, dim, heads, depth, N, cfg["cross_attention_dim"], seed)
    sd = {"image_proj." + k: v for k, v in rs.items()}
    sd.update({k: v for k, v in R.make_adapter(cfg, N, 64, seed).items() if R.PROC in k})
    return sd


def resampler_of(sd_plus):
    return {k[len("image_proj."):]: v for k, v in sd_plus.items() if k.startswith("image_proj.")}


def as_plain(sd_plus):
    """The identity-projection device.  ref_unet / ref_tryon compute tokens = LayerNorm(norm)(Linear(proj)(embeds)).reshape(n, N, D)
    (ip_adapter_ref.image_proj).  With proj = the identity of size N D and zero bias, and norm = the Resampler's norm_out, the "embeddings"
    prenorm.reshape(n, N D) -- the Resampler's output before norm_out -- give exactly the Plus tokens.  -> the plain-layout adapter dict"""
    N, D = sd_plus["image_proj.latents"].shape[1], sd_plus["image_proj.norm_out.weight"].numel()
    sd = {"image_proj.proj.weight": torch.eye(N * D), "image_proj.proj.bias": torch.zeros(N * D),
          "image_proj.norm.weight": sd_plus["image_proj.norm_out.weight"], "image_proj.norm.bias": sd_plus["image_proj.norm_out.bias"]}
    sd.update({k: v for k, v in sd_plus.items() if R.PROC in k})
    return sd


def plain_embeds(sd_plus, hidden, heads):
    """the "embeddings" to hand the references together with as_plain(sd_plus): [n, N D]"""
    _, pre = resampler_forward(resampler_of(sd_plus), hidden, heads, return_prenorm=True)
    return pre.reshape(pre.shape[0], -1)


def penultimate(sd, cfg, pixel_values):
    """hidden_states[-2] of the vision encoder: the oracle over the same state dict with one layer fewer -- exact, because the blocks are
    sequential pre-LN blocks and neither output has post_layernorm applied (with one layer: the pre_layrnorm output)"""
    return V.clip_vision_forward(sd, dict(cfg, layers=cfg["layers"] - 1), pixel_values)[0]


def image_embeds(sd, cfg, pixel_values):
    return F.linear(V.clip_vision_forward(sd, cfg, pixel_values)[1], sd["visual_projection.weight"])


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_pixels(picture, size):
    """the pre-processing the reference applies to the in-shop cloth (oracle.e2e_cases.clip_pixels, at any size): the WHOLE picture [B, 3, H, W]
    in [-1, 1] resized (bilinear, antialiased) to size x size, the processor's 8-bit truncation, CLIP mean / std, rounded to fp16"""
    img = F.interpolate((picture + 1) / 2, size=(size, size), mode="bilinear", antialias=True, align_corners=False).clamp(0, 1)
    img = torch.floor(img * 255.0) / 255.0
    return ((img - torch.tensor(CLIP_MEAN).view(1, 3, 1, 1)) / torch.tensor(CLIP_STD).view(1, 3, 1, 1)).half().float()


def pictures(B, H=96, W=72, seed=0):
    """smooth random pictures in [-1, 1] (fp16-representable): low-frequency noise, so that the 8-bit truncation of the pre-processing
    flips few levels between two implementations of the resize"""
    g = torch.Generator().manual_seed(3100 + seed)
    low = torch.rand((B, 3, H // 8, W // 8), generator=g) * 2 - 1
    return F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False).clamp(-1, 1).half().float()


def loop_ip(adapter, vision_sd, vision_cfg, picture, heads=None, scales=None):
    """the `ip=` of tests/ref_tryon.tryon_reference for a run with `ip_adapter_image=picture`: (adapter dict, embeds, negative embeds,
    scales).  A Plus adapter (library keys) goes through the identity-projection device with the negative passed explicitly -- the states
    of zero pixel_values, one sample, broadcast; a plain adapter gets image_embeds and None (zeros)."""
    px = clip_pixels(picture, vision_cfg["image_size"])
    scales = [1.0] * 16 if scales is None else scales
    if "image_proj.latents" not in adapter:
        return adapter, image_embeds(vision_sd, vision_cfg, px), None, scales
    cond = plain_embeds(adapter, penultimate(vision_sd, vision_cfg, px), heads)
    unc = plain_embeds(adapter, penultimate(vision_sd, vision_cfg, torch.zeros_like(px[:1])), heads)
    return as_plain(adapter), cond, unc.expand(cond.shape[0], -1).contiguous(), scales


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases of the module tests (tests/test_gpu_ip_image.py runs them, tests/test_cpu_ip_image.py shows that their thresholds are reachable)
# (n, T, E, dim, heads, depth, N, out_dim)
# ---------------------------------------------------------------------------------------------------------------------------------------
RESAMPLER_CASES = [
    (3, 17, 320, 128, 2, 2, 16, 128),          # 33 keys
    (1, 5, 64, 64, 1, 1, 5, 128),              # N and T no multiples of 4, 10 keys
    (2, 257, 320, 128, 2, 1, 64, 128),         # the N limit
    (2, 257, 1280, 1024, 16, 4, 16, 1024),     # released width: other igemm tile selections than tiny
    (2, 17, 320, 160, 2, 1, 16, 128),          # dim_head 80: the generic-head-dim attention, widths that are multiples of 32 but not of 64
    (2, 9, 72, 64, 1, 1, 8, 128),              # E a multiple of 8 only: proj_in leaves the igemm path
]
MODULE_PSNR, MODULE_REL_L2 = 50.0, 5e-3        # the project's module contract (test_vision_encoder_tiny_vs_transformers_golden_and_oracle)


def case_id(c):
    return "n%d_T%d_E%d_dim%d_h%d_d%d_N%d_out%d" % c


def case_input(c):
    """[n, T, E] fp16-representable, unit variance"""
    return torch.randn((c[0], c[1], c[2]), generator=torch.Generator().manual_seed(97 + c[1] + c[3])).half().float()


def unet_case(cfg, n, h, w, T=17, E=320):
    """inputs of the UNet forward tests: latents-side input x [n, 31, h, w], text context [n, 8, D], hidden states [n, T, E]"""
    g = torch.Generator().manual_seed(1000 + h)
    x = torch.randn((n, cfg["in_channels"], h, w), generator=g).half().float()
    ehs = torch.randn((n, 8, cfg["cross_attention_dim"]), generator=g).half().float()
    hidden = torch.randn((n, T, E), generator=g).half().float()
    return x, ehs, hidden
