"""Token merging (tomesd.apply_patch) for the native UNet: the configuration, checked on the host, and the block arithmetic the pipeline
needs before it launches anything.  The kernels are csrc/tome.hip, the contract include/ladi_native.h "Token merging"."""
import math

FIELDS = ("ratio", "max_downsample", "sx", "sy", "use_rand", "seed", "merge_attn", "merge_crossattn", "merge_mlp")
DEFAULTS = dict(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=False, seed=0, merge_attn=True, merge_crossattn=False, merge_mlp=False)


def config(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=False, seed=0, merge_attn=True, merge_crossattn=False, merge_mlp=False):
    """the checked configuration as a dict (the fields of ladi_tome_config).  Raises ValueError with the library's reasons: a ratio outside
    [0, 1) or not finite, sx or sy other than 2, max_downsample not in {1, 2}, all three merge flags off with ratio > 0."""
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not math.isfinite(ratio) or not 0.0 <= ratio < 1.0:
        raise ValueError("token merging: ratio has to be a finite number in [0, 1) but is %r" % (ratio,))
    for name, v in (("sx", sx), ("sy", sy)):
        if isinstance(v, bool) or v != 2:
            raise ValueError("token merging: %s has to be 2 (only 2 x 2 cells are supported) but is %r" % (name, v))
    if isinstance(max_downsample, bool) or max_downsample not in (1, 2):
        raise ValueError("token merging: max_downsample has to be 1 or 2 but is %r" % (max_downsample,))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
        raise ValueError("token merging: seed has to be an int in [0, 2^32) but is %r" % (seed,))
    if ratio > 0 and not (merge_attn or merge_crossattn or merge_mlp):
        raise ValueError("token merging: merge_attn, merge_crossattn and merge_mlp are all off with ratio > 0")
    return dict(ratio=float(ratio), max_downsample=int(max_downsample), sx=2, sy=2, use_rand=bool(use_rand), seed=int(seed),
                merge_attn=bool(merge_attn), merge_crossattn=bool(merge_crossattn), merge_mlp=bool(merge_mlp))


def merged_blocks(max_downsample, layers_per_block=2):
    """the transformer blocks the configuration merges, as indices in execution order (the numbering of the PAG layer mask): level 0 is
    down_blocks.0 and up_blocks.3, level 1 down_blocks.1 and up_blocks.2"""
    L = layers_per_block
    out = []
    for b in range(6 * L + 4):
        level = b // L if b < 3 * L else 3 if b == 3 * L else 2 - (b - 3 * L - 1) // (L + 1)
        if level < max_downsample:
            out.append(b)
    return out


def merged_mask(cfg, layers_per_block=2):
    """bit mask of merged_blocks for a configuration dict (None or ratio 0: nothing merges)"""
    if not cfg or not cfg["ratio"] > 0:
        return 0
    return sum(1 << b for b in merged_blocks(cfg["max_downsample"], layers_per_block))


def check_pag_layers(cfg, pag_mask, layers_per_block=2):
    """perturbed-attention guidance perturbs the self-attention map of whole blocks, which a merged block no longer has at full length:
    raises ValueError when an applied PAG layer is a block that merges tokens"""
    both = merged_mask(cfg, layers_per_block) & int(pag_mask)
    if both:
        raise ValueError("pag_scale > 0 with token merging: the PAG layers include transformer block(s) %s, which merge tokens; choose "
                         "pag_applied_layers outside the merged levels (the default \"mid\" is) or remove_token_merging()"
                         % [b for b in range(32) if both >> b & 1])
