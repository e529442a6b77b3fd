"""Reference for token merging (tomesd's bipartite_soft_matching_random2d as include/ladi_native.h "Token merging" states it): the yardstick
of tests/test_cpu_tome.py and tests/test_gpu_tome.py.  Plain torch in float64 / float32, written from the contract, not from the kernels.

    partition   T = h w tokens, one dst per full 2 x 2 cell at in-cell offset o (0, or splitmix64(seed * 2^32 + cell) % 4), every other
                token src; both lists ascending
    match       rows L2-normalised (norm clamped at 1e-12); score[i] = max_j a_i . b_j, node[i] = the lowest j that reaches it
    select      r = min(int(T * ratio), Ns); the r src with the largest score, ties to the lower src, NaN as -inf
    merged seq  [unmerged src, ascending ; dst], row Nu + j = mean of dst j and the src merged into it (summed in ascending src order)
    unmerge     out[p] = y[out_row[p]]
    block       x = u(attn1(m(norm1 x))) + x  (merge_attn), x = u(attn2(m(norm2 x), ctx)) + x  (merge_crossattn),
                x = u(ff(m(norm3 x))) + x  (merge_mlp); one plan per block, from the output of proj_in: tests/ref_unet.py transformer2d
A plan is a dict: r, Nu, out_row [T], unm [Nu] (token positions), segs (Nd lists of token positions), merged [Ns] bool, node [Ns].
"""
import torch

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
