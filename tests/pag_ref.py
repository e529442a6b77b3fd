"""Reference for perturbed-attention guidance (diffusers PAGMixin with PAGIdentitySelfAttnProcessor2_0 / PAGCFGIdentitySelfAttnProcessor2_0):
the yardstick tests/test_cpu_pag.py and tests/test_gpu_pag.py compare the library with.  The layer names, the per-evaluation scale and the
combine are here; the identity self-attention (O = V for the samples >= pag_first in the selected blocks) is tests/ref_unet.py's (pag=), the
third sample group of the loop tests/ref_tryon.py's (pag=).

    layers      the selected blocks as a set of diffusers module prefixes ("mid_block.attentions.0", "down_blocks.1.attentions.0", ..),
                from layer_prefixes(names, layers_per_block) with the names `pag_applied_layers` takes
    pag_first   samples [pag_first, n) of a forward are perturbed; None or >= n: none
    e = u + g (c - u) + s (c - p)      CFG evaluation           e = c + s (c - p)      no CFG, or a cond-only evaluation of a guided run
    rescale acts on the three-term sum of CFG evaluations (guidance_ref.rescale_factor with the cond prediction)
"""
from tests import guidance_ref as G
from tests import ref_unet as RU


def layer_prefixes(names, layers_per_block=2):
    """`pag_applied_layers` names -> the set of module prefixes they select, written independently of pipeline.pag_layer_mask: a name
    "down.block_1.attentions_0" selects the prefixes that start with "down_blocks.1.attentions.0", "mid" the mid block"""
    if isinstance(names, str):
        names = [names]
    out = set()
    every = RU.block_prefixes(layers_per_block)
    for name in names:
        p = name.split(".")
        if name == "mid":
            sel = {"mid_block.attentions.0"}
        elif len(p) == 1:
            sel = {b for b in every if b.startswith(p[0] + "_blocks.")}
        elif len(p) == 2:
            sel = {b for b in every if b.startswith(p[0] + "_blocks." + p[1][len("block_"):] + ".attentions.")}
        else:
            sel = {b for b in every if b == p[0] + "_blocks." + p[1][len("block_"):] + ".attentions." + p[2][len("attentions_"):]}
        assert sel, name
        out |= sel
    return out


def mask_of(prefixes, layers_per_block=2):
    return sum(1 << i for i, b in enumerate(RU.block_prefixes(layers_per_block)) if b in prefixes)


def pag_plan(pag_scale, pag_adaptive_scale, timesteps):
    """PAGMixin._get_pag_scale per evaluation"""
    if pag_adaptive_scale == 0:
        return [float(pag_scale)] * len(timesteps)
    return [max(float(pag_scale) - float(pag_adaptive_scale) * (1000.0 - float(t)), 0.0) for t in timesteps]


def guided_eps(eu, ec, ep, g, s, phi=0.0):
    """the combine of one evaluation in the inputs' dtype.  eu None: no CFG or a cond-only evaluation; ep None (s == 0): no PAG.  The
    rescale (CFG evaluations only) takes its statistics of the three-term sum, in float64"""
    e = ec if eu is None else eu + g * (ec - eu)
    if ep is not None and s > 0.0:
        e = e + s * (ec - ep)
    if eu is not None and phi > 0.0:
        e = (e.double() * G.rescale_factor(e, ec, phi)).to(e.dtype)
    return e


def sched_reference(sch, eps_seq, cfg, gtab, ptab, phi, lat0):
    """guidance_ref.sched_reference with the PAG combine.  eps_seq [evals, 3B or 2B, 4, h, w]: [uncond ; cond ; perturbed] with cfg, else
    [cond ; perturbed]; rows an evaluation must not read may hold NaN"""
    B = lat0.shape[0]
    x = lat0.double()
    for i, t in enumerate(sch.timesteps):
        o = B if cfg else 0
        ec = eps_seq[i, o:o + B].double()
        eu = eps_seq[i, :B].double() if cfg and G.is_cfg(gtab[i]) else None
        ep = eps_seq[i, o + B:o + 2 * B].double() if ptab[i] > 0.0 else None
        x = sch.step(guided_eps(eu, ec, ep, gtab[i] if cfg else 1.0, ptab[i], phi), t, x).prev_sample
    return x
