"""Reference for the IP-Adapter image prompt (diffusers IPAdapterAttnProcessor2_0 with the plain ImageProjection): the yardstick
tests/test_cpu_ip_adapter.py and tests/test_gpu_ip_adapter.py compare the library with.  The projection, a synthetic adapter and diffusers' file
layout are here; the second, decoupled cross-attention term
    attn2_out = to_out(attention(q, k_text, v_text) + s_block * attention(q, to_k_ip(tokens), to_v_ip(tokens)))
is tests/ref_unet.py's (ip=), the image tokens of every sample group of the loop tests/ref_tryon.py's (ip=).

    sd_ip     the adapter under the library's keys (ladi_vton_amd.ip_adapter.load_state's output): image_proj.{proj,norm}.{weight,bias} and
              <block>.transformer_blocks.0.attn2.processor.to_{k,v}_ip.weight
    tokens    [n, N, cross_dim]: image_proj(sd_ip, embeds), or anything else (set_ip_tokens)
    scales    one float per transformer block in execution order (ref_unet.block_prefixes)
"""
import torch
import torch.nn.functional as F

from tests import ref_unet as RU

PROC = ".transformer_blocks.0.attn2.processor."


def image_proj(sd_ip, embeds):
    """ImageProjection: LayerNorm(Linear(embeds)) per token, eps 1e-5; embeds [n, E] -> [n, N, cross_dim]"""
    D = sd_ip["image_proj.norm.weight"].numel()
    t = F.linear(embeds, sd_ip["image_proj.proj.weight"], sd_ip["image_proj.proj.bias"]).reshape(embeds.shape[0], -1, D)
    return F.layer_norm(t, (D,), sd_ip["image_proj.norm.weight"], sd_ip["image_proj.norm.bias"], 1e-5)


def make_adapter(cfg, N=4, E=64, seed=0, k_scale=1.0, v_scale=0.5):
    """a random adapter under the library's keys (fp16-representable float32).  Tokens are LayerNorm outputs (unit variance), so the image
    keys and values have the standard deviations k_scale / v_scale per channel: logits of order k_scale |q| / 8 and an image term of order
    v_scale, chosen so that the term is visible in the forward (tests/test_cpu_ip_adapter.py checks the margins)."""
    g = torch.Generator().manual_seed(4200 + seed)
    D = cfg["cross_attention_dim"]
    r = lambda *s: torch.randn(s, generator=g)
    h = lambda t: t.half().float()
    sd = {"image_proj.proj.weight": h(r(N * D, E) / E ** 0.5), "image_proj.proj.bias": h(r(N * D) * 0.3),
          "image_proj.norm.weight": h(1.0 + 0.1 * r(D)), "image_proj.norm.bias": h(0.1 * r(D))}
    boc, L = cfg["block_out_channels"], cfg["layers_per_block"]
    for p in RU.block_prefixes(L):
        C = boc[RU.level_of(p, L)]
        sd[p + PROC + "to_k_ip.weight"] = h(r(C, D) * k_scale / D ** 0.5)
        sd[p + PROC + "to_v_ip.weight"] = h(r(C, D) * v_scale / D ** 0.5)
    return sd


def to_diffusers(sd_ip, layers_per_block=2, numbered=True):
    """the adapter in diffusers' nested {"image_proj", "ip_adapter"} layout, with numbered ("<2k+1>.to_k_ip.weight", attn_processors order:
    down, up, mid) or module-named keys -- written independently of ladi_vton_amd.ip_adapter.numbered_order"""
    L = layers_per_block
    order = (["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(L)] +
             ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(L + 1)] + ["mid_block.attentions.0"])
    proj = {k[len("image_proj."):]: v for k, v in sd_ip.items() if k.startswith("image_proj.")}
    ada = {}
    for k, v in sd_ip.items():
        if PROC in k:
            p, name = k.split(PROC)
            ada["%d.%s" % (2 * order.index(p) + 1, name) if numbered else k] = v
    return {"image_proj": proj, "ip_adapter": ada}
