"""Reference for token merging (tomesd's bipartite_soft_matching_random2d as include/ladi_native.h "Token merging" states it): the yardstick
of tests/test_cpu_tome.py and tests/test_gpu_tome.py.  Plain torch in float64 / float32, written from the contract, not from the kernels.

    partition   T = h w tokens, one dst per full 2 x 2 cell at in-cell offset o (0, or splitmix64(seed * 2^32 + cell) % 4), every other
                token src; both lists ascending
    match       rows L2-normalised (norm clamped at 1e-12); score[i] = max_j a_i . b_j, node[i] = the lowest j that reaches it
    select      r = min(int(T * ratio), Ns); the r src with the largest score, ties to the lower src, NaN as -inf
    merged seq  [unmerged src, ascending ; dst], row Nu + j = mean of dst j and the src merged into it (summed in ascending src order)
    unmerge     out[p] = y[out_row[p]]
    block       x = u(attn1(m(norm1 x))) + x  (merge_attn), x = u(attn2(m(norm2 x), ctx)) + x  (merge_crossattn),
                x = u(ff(m(norm3 x))) + x  (merge_mlp); one plan per block, from the output of proj_in
A plan is a dict: r, Nu, out_row [T], unm [Nu] (token positions), segs (Nd lists of token positions), merged [Ns] bool, node [Ns].
"""
import torch
import torch.nn.functional as F

from oracle import models as M
from tests import guidance_ref as G
from tests import strength_ref as SR

MASK64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def tables(h, w, sx=2, sy=2, use_rand=False, seed=0):
    """-> (src_pos, dst_pos): ascending lists of token positions"""
    hsy, wsx = h // sy, w // sx
    dst = set()
    for cy in range(hsy):
        for cx in range(wsx):
            o = splitmix64(((seed << 32) + cy * wsx + cx) & MASK64) % (sx * sy) if use_rand else 0
            dst.add((cy * sy + o // sx) * w + cx * sx + o % sx)
    return [p for p in range(h * w) if p not in dst], sorted(dst)


def merge_count(T, Ns, ratio):
    return min(int(T * ratio), Ns)


def level_of(prefix, L=2):
    """resolution level of a transformer block by its diffusers prefix: down_blocks.i -> i, mid -> 3, up_blocks.i -> 3 - i"""
    p = prefix.split(".")
    return 3 if p[0] == "mid_block" else int(p[1]) if p[0] == "down_blocks" else 3 - int(p[1])


def scores(metric, src_pos, dst_pos, dtype=torch.float64):
    """cosine scores [Ns, Nd] of a metric [T, C] in `dtype`"""
    m = metric.to(dtype)
    m = m / m.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return m[src_pos] @ m[dst_pos].T


def match(S):
    """-> (score [Ns], node [Ns]): the row maximum and the lowest column that reaches it"""
    sc = S.max(dim=1).values
    idx = torch.arange(S.shape[1]).expand_as(S)
    node = torch.where(S == sc[:, None], idx, torch.full_like(idx, S.shape[1])).min(dim=1).values
    return sc, node.clamp_max(S.shape[1] - 1)


def select(score, r):
    """-> bool [Ns]: the r src with the largest score; ties to the lower index, NaN as -inf"""
    key = torch.where(torch.isnan(score), torch.full_like(score, float("-inf")), score)
    order = torch.sort(key, descending=True, stable=True).indices
    merged = torch.zeros(score.shape[0], dtype=torch.bool)
    merged[order[:r]] = True
    return merged


def make_plan(merged, node, src_pos, dst_pos):
    T, Ns, Nd = len(src_pos) + len(dst_pos), len(src_pos), len(dst_pos)
    r = int(merged.sum())
    Nu = Ns - r
    out_row = torch.zeros(T, dtype=torch.long)
    unm, segs, k = [], [[] for _ in range(Nd)], 0
    for i in range(Ns):
        if bool(merged[i]):
            out_row[src_pos[i]] = Nu + int(node[i])
            segs[int(node[i])].append(src_pos[i])
        else:
            out_row[src_pos[i]] = k
            unm.append(src_pos[i])
            k += 1
    for j in range(Nd):
        out_row[dst_pos[j]] = Nu + j
    return dict(r=r, Nu=Nu, T=T, out_row=out_row, unm=unm, segs=segs, dst=list(dst_pos), merged=merged.clone(), node=torch.as_tensor(node).clone())


def plan(score, node, src_pos, dst_pos, r):
    return make_plan(select(score, r), node, src_pos, dst_pos)


def plan_of_metric(metric, src_pos, dst_pos, r, dtype=torch.float64):
    sc, node = match(scores(metric, src_pos, dst_pos, dtype))
    return plan(sc, node, src_pos, dst_pos, r)


def plan_from_out_row(out_row, src_pos, dst_pos):
    """the plan a device out_row [T] encodes (a forced plan); asserts that it is one"""
    out_row = torch.as_tensor(out_row).long()
    Ns, Nd = len(src_pos), len(dst_pos)
    Nu = int(out_row[dst_pos[0]])
    assert 0 <= Nu <= Ns and all(int(out_row[dst_pos[j]]) == Nu + j for j in range(Nd)), "dst rows of out_row"
    rows = out_row[src_pos]
    merged = rows >= Nu
    assert int((~merged).sum()) == Nu and torch.equal(rows[~merged], torch.arange(Nu)), "unmerged rows of out_row"
    assert int(rows.max()) < Nu + Nd
    return make_plan(merged, (rows - Nu).clamp_min(0), src_pos, dst_pos)


def merge(x, p, dtype=torch.float64):
    """x [T, C] -> [T - r, C]: the sums in ascending src order in `dtype`"""
    x = x.to(dtype)
    rows = [x[q] for q in p["unm"]]
    for j, seg in enumerate(p["segs"]):
        acc = x[p["dst"][j]].clone()
        for q in seg:
            acc = acc + x[q]
        rows.append(acc / (1 + len(seg)))
    return torch.stack(rows)


def unmerge(y, p):
    return y[p["out_row"]]


def plan_diff(a, b):
    """share of src tokens whose (merged?, partner) differ between two plans"""
    same = (a["merged"] == b["merged"]) & (~a["merged"] | (a["node"] == b["node"]))
    return 1.0 - float(same.float().mean())


# ------------------------------------------------------------------------------------------------------------------ the block and the UNet
def transformer2d(sd, p, x, ehs, heads, groups, tcfg=None, forced=None, record=None, metric="proj_in", ip=None):
    """oracle.models.transformer2d with token merging.  tcfg: the configuration dict or None; forced: a plan per sample (else the plan is
    computed here, in x's dtype); record(p, t0, plans): a hook.  metric: "proj_in" (the contract), or a mis-wiring "norm1" / "input" the
    wiring test measures against.  ip: None or (sd_ip, tokens [n, N, cross_dim], scales per block in execution order), the IP-Adapter image
    term of tests/ip_adapter_ref.py: scale * attention(q2, to_k_ip(tokens), to_v_ip(tokens)) added to the attn2 output before to_out, q2 from
    the merged rows when merge_crossattn is on; a block whose scale is 0 has no image term"""
    n, C, h, w = x.shape
    res = x
    g = M.group_norm(sd, p + ".norm", x, groups, 1e-6).permute(0, 2, 3, 1).reshape(n, h * w, C)
    t = M.linear(sd, p + ".proj_in", g)
    b = p + ".transformer_blocks.0"
    plans = None
    if tcfg is not None:
        sp, dp = tables(h, w, 2, 2, tcfg["use_rand"], tcfg["seed"])
        r = merge_count(h * w, len(sp), tcfg["ratio"]) if dp else 0
        if r > 0:
            if forced is not None:
                plans = forced
            else:
                met = {"proj_in": t, "norm1": M.layer_norm(sd, b + ".norm1", t), "input": g}[metric]
                plans = [plan_of_metric(met[s], sp, dp, r, x.dtype) for s in range(n)]
            if record is not None:
                record(p, t, plans)
    m = (lambda a: torch.stack([merge(a[s], plans[s], a.dtype) for s in range(n)]))
    u = (lambda y: torch.stack([unmerge(y[s], plans[s]) for s in range(n)]))
    on = lambda flag: plans is not None and tcfg[flag]

    a = M.layer_norm(sd, b + ".norm1", t)
    a = m(a) if on("merge_attn") else a
    o = M.linear(sd, b + ".attn1.to_out.0", M.attention(M.linear(sd, b + ".attn1.to_q", a), M.linear(sd, b + ".attn1.to_k", a),
                                                        M.linear(sd, b + ".attn1.to_v", a), heads))
    t = (u(o) if on("merge_attn") else o) + t
    a = M.layer_norm(sd, b + ".norm2", t)
    a = m(a) if on("merge_crossattn") else a
    q2 = M.linear(sd, b + ".attn2.to_q", a)
    o = M.attention(q2, M.linear(sd, b + ".attn2.to_k", ehs), M.linear(sd, b + ".attn2.to_v", ehs), heads)
    if ip is not None:
        sd_ip, tokens, scales = ip
        scale = float(scales[block_prefixes().index(p)])
        if scale != 0.0:
            proc = p + ".transformer_blocks.0.attn2.processor."
            o = o + scale * M.attention(q2, F.linear(tokens, sd_ip[proc + "to_k_ip.weight"]), F.linear(tokens, sd_ip[proc + "to_v_ip.weight"]), heads)
    o = M.linear(sd, b + ".attn2.to_out.0", o)
    t = (u(o) if on("merge_crossattn") else o) + t
    a = M.layer_norm(sd, b + ".norm3", t)
    a = m(a) if on("merge_mlp") else a
    uu, gg = M.linear(sd, b + ".ff.net.0.proj", a).chunk(2, dim=-1)
    o = M.linear(sd, b + ".ff.net.2", uu * F.gelu(gg))
    t = (u(o) if on("merge_mlp") else o) + t
    t = M.linear(sd, p + ".proj_out", t)
    return t.reshape(n, h, w, C).permute(0, 3, 1, 2) + res


def block_prefixes(L=2):
    return (["down_blocks.%d.attentions.%d" % (i, j) for i in range(3) for j in range(L)] + ["mid_block.attentions.0"] +
            ["up_blocks.%d.attentions.%d" % (i, j) for i in (1, 2, 3) for j in range(L + 1)])


def merged_prefixes(tcfg, L=2):
    """the blocks a configuration merges, in execution order (the order of the library's merged-block index)"""
    return [p for p in block_prefixes(L) if level_of(p, L) < tcfg["max_downsample"]]


def unet_forward(sd, cfg, sample, timestep, ehs, tcfg=None, forced=None, record=None, metric="proj_in", ip=None):
    """the whole forward (any latent size) with token merging in the blocks of the first max_downsample levels.  forced: dict prefix -> a
    plan per sample; ip: as transformer2d's"""
    boc, heads, L = cfg["block_out_channels"], cfg["num_heads"], cfg["layers_per_block"]
    G_, eps = cfg["norm_num_groups"], cfg["norm_eps"]
    n = sample.shape[0]

    def xf(p, x, hd):
        on = tcfg is not None and tcfg["ratio"] > 0 and level_of(p, L) < tcfg["max_downsample"]
        return transformer2d(sd, p, x, ehs, hd, G_, tcfg if on else None, forced.get(p) if forced else None, record, metric, ip)
    forward_upsample_size = any(s % 8 != 0 for s in sample.shape[-2:])
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1).expand(n)
    temb = M.timestep_embedding(t, boc[0])
    temb = M.linear(sd, "time_embedding.linear_2", F.silu(M.linear(sd, "time_embedding.linear_1", temb)))
    x = M.conv(sd, "conv_in", sample)
    skips = [x]
    for i in range(4):
        for j in range(L):
            x = M.resnet(sd, "down_blocks.%d.resnets.%d" % (i, j), x, temb, G_, eps)
            if i < 3:
                x = xf("down_blocks.%d.attentions.%d" % (i, j), x, heads[i])
            skips.append(x)
        if i < 3:
            x = M.conv(sd, "down_blocks.%d.downsamplers.0.conv" % i, x, stride=2, padding=1)
            skips.append(x)
    x = M.resnet(sd, "mid_block.resnets.0", x, temb, G_, eps)
    x = xf("mid_block.attentions.0", x, heads[3])
    x = M.resnet(sd, "mid_block.resnets.1", x, temb, G_, eps)
    for i in range(4):
        for j in range(L + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            x = M.resnet(sd, "up_blocks.%d.resnets.%d" % (i, j), x, temb, G_, eps)
            if i > 0:
                x = xf("up_blocks.%d.attentions.%d" % (i, j), x, heads[3 - i])
        if i < 3:
            if forward_upsample_size:
                x = F.interpolate(x, size=skips[-1].shape[2:], mode="nearest")
            else:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = M.conv(sd, "up_blocks.%d.upsamplers.0.conv" % i, x)
    assert not skips
    return M.conv(sd, "conv_out", F.silu(M.group_norm(sd, "conv_norm_out", x, G_, eps)))


def tryon_reference(unet_sd, unet_cfg, vae_sd, vae_cfg, emasc_sd, inp, num_inference_steps, scheduler, tcfg, forced_per_eval, guidance=7.5,
                    int_layers=(1, 2, 3, 4, 5)):
    """the try-on loop (oracle modules, the mirror scheduler, CFG, cloth_cond_rate 1) with token merging; forced_per_eval[i]: dict prefix ->
    a plan per sample of the [uncond ; cond] batch of evaluation i"""
    image, mask_image = inp["image"].clone(), inp["mask_image"].clone()
    pose_map, cloth = inp["pose_map"], inp["warped_cloth"]
    h, w = image.shape[2] // 8, image.shape[3] // 8
    sf = vae_cfg["scaling_factor"]
    sch = SR.make_mirror(scheduler)
    sch.set_timesteps(num_inference_steps)
    pe_c, pe_u = inp["prompt_embeds"], inp["negative_prompt_embeds"]
    mask_image[mask_image < 0.5] = 0
    mask_image[mask_image >= 0.5] = 1
    masked_image = image.float() * (mask_image < 0.5)
    pose = F.interpolate(pose_map, size=(pose_map.shape[2] // 8, pose_map.shape[3] // 8), mode="bilinear")
    mom, _ = M.vae_encode(vae_sd, vae_cfg, cloth)
    cloth_latents = sf * M.posterior_sample(mom, inp["noise_cloth"])
    latents = inp["noise_latents"] * sch.init_noise_sigma
    mask_lat = F.interpolate(mask_image, size=(h, w))
    mom, feats = M.vae_encode(vae_sd, vae_cfg, masked_image)
    masked_lat = sf * M.posterior_sample(mom, inp["noise_masked"])
    inter = None
    if emasc_sd is not None:
        inter = M.mask_features(M.emasc_forward(emasc_sd, [feats[i] for i in int_layers]), mask_image)
    static_c = torch.cat([mask_lat, masked_lat, pose, cloth_latents], dim=1)
    static_u = torch.cat([mask_lat, masked_lat, torch.zeros_like(pose), torch.zeros_like(cloth_latents)], dim=1)
    for i, t in enumerate(sch.timesteps):
        xs = sch.scale_model_input(latents, t)
        eps = unet_forward(unet_sd, unet_cfg, torch.cat([torch.cat([xs, static_u], dim=1), torch.cat([xs, static_c], dim=1)]), t,
                           torch.cat([pe_u, pe_c]), tcfg, forced_per_eval[i] if forced_per_eval is not None else None)
        eu, ec = eps.chunk(2)
        latents = sch.step(G.guided_eps(eu, ec, guidance), t, latents).prev_sample
    img = M.vae_decode(vae_sd, vae_cfg, latents / sf, list(inter) if inter is not None else None,
                       list(int_layers) if inter is not None else None)
    img = (img / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).float()
    return img, latents
