"""The operator cases of tests/test_gpu_ip_adapter.py as CPU data: operands, the float64 reference and the derived per-element bound of
ladi_op_ip_attn_add (csrc/ip_adapter.hip), o <- fp16(o + scale * softmax(0.125 q k^T) v) per (sample, head).  tests/test_cpu_ip_adapter.py
checks the bound on the CPU: a float32 torch evaluation stays inside it, and it is at most a tenth of the image term's own magnitude, so a
kernel that adds nothing fails.  Every bound comes from the reference alone; u = U32 = 2^-24.

The kernel's arithmetic and what each step contributes (per query, per head; d = 64, N keys):
  logits   s_j = 0.125 fl(sum_c q_c k_jc): products of two fp16 values are exact in fp32, the sum is 8 chained FMAs per lane and a 3-step
           butterfly (at most 11 roundings on any path <= the d + 1 of tests/util.py single_query_ref_bound), the factor 0.125 is exact
  softmax  w_j = exp(s_j - m), m the maximum of the computed logits; the argument's roundings and the fast exponential's are
           single_query_ref_bound's D_j and ACT_EVAL; numerator and denominator are N-term fp32 sums in key order
  scale    W = scale / den (one rounding), out = fma(W, num_c, o_c) (one rounding): 4 u |scale| sum_j p_j |v_jc| on top of the (2 N + 6) u of the
           sums, and u |out| for the fused add before the one rounding to fp16 (check_elem's ulp16(ref))
      bound = |scale| (single_query_ref_bound's bound + 4 u sum_j p_j |v_jc|) + u |ref|
"""
import torch

from tests import util as U

# (n, T, heads, N, padding of ldq / ldo beyond heads * 64 in halves, scale, kind).  T in {1, 5, 48, 768}, heads in {5, 20}, n in {1, 3},
# N in {1, 4, 5, 16, 64} are each met; "hot": logits near 40, so the subtraction of the row maximum matters (as SQ_CASES[-1] of helpers_cases.py)
CASES = [
    (1, 1, 5, 1, 0, 1.0, "plain"),
    (3, 5, 5, 4, 8, 0.6, "plain"),
    (1, 48, 20, 5, 8, 1.0, "plain"),
    (3, 48, 5, 16, 0, -0.5, "plain"),
    (1, 768, 5, 4, 8, 1.0, "plain"),
    (1, 768, 20, 16, 0, 0.7, "plain"),
    (3, 5, 20, 64, 8, 1.0, "plain"),
    (1, 131, 5, 64, 0, 0.5, "plain"),
    (1, 48, 5, 16, 8, 1.0, "hot"),
]


def case_id(c):
    return "n%d_T%d_h%d_N%d_pad%d_s%g_%s" % c


def make_case(n, T, heads, N, pad, scale, kind, seed=0):
    """-> dict(q, kv, o: fp16 CPU tensors [n, T, C], [n, N, 2C], [n, T, C]; ref, bound, term: float64 [n, T, C])"""
    C = heads * 64
    g = torch.Generator().manual_seed(1000 * n + T + 7 * heads + 13 * N + seed)
    qs, ks = (5.0, 4.0) if kind == "hot" else (1.0, 1.0)
    q = (torch.randn((n, T, C), generator=g) * qs).half()
    kv = torch.randn((n, N, 2 * C), generator=g)
    kv[..., :C] *= ks
    kv[..., C:] *= 1.5
    kv = kv.half()
    o = torch.randn((n, T, C), generator=g).half()
    qh = q.double().view(n, T, heads, 64).permute(0, 2, 1, 3)                              # [n, heads, T, 64]
    kh = kv[..., :C].double().view(n, N, heads, 64).permute(0, 2, 1, 3).unsqueeze(2).expand(n, heads, T, N, 64)
    vh = kv[..., C:].double().view(n, N, heads, 64).permute(0, 2, 1, 3).unsqueeze(2).expand(n, heads, T, N, 64)
    att, b = U.single_query_ref_bound(qh, kh, vh, 0.125)                                   # [n, heads, T, 64]
    p = torch.softmax((kh @ qh.unsqueeze(-1)).squeeze(-1) * 0.125, -1)                    # [n, heads, T, N]
    pv = (p.unsqueeze(-2) @ vh.abs()).squeeze(-2)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(n, T, C)
    term = scale * back(att)
    ref = o.double() + term
    bound = abs(scale) * (back(b) + 4 * U.U32 * back(pv)) + U.U32 * ref.abs()
    return dict(q=q, kv=kv, o=o, ref=ref, bound=bound, term=term, max_logit=float((kh @ qh.unsqueeze(-1)).abs().max() * 0.125))


def torch_f32(case, scale, heads):
    """the same function in float32 torch arithmetic, rounded once to fp16: what the CPU test holds against the bound"""
    q, kv, o = case["q"].float(), case["kv"].float(), case["o"].float()
    n, T, C = q.shape
    N = kv.shape[1]
    qh = q.view(n, T, heads, 64).permute(0, 2, 1, 3)
    kh = kv[..., :C].view(n, N, heads, 64).permute(0, 2, 1, 3)
    vh = kv[..., C:].view(n, N, heads, 64).permute(0, 2, 1, 3)
    p = torch.softmax((qh @ kh.transpose(-1, -2)) * 0.125, -1)
    return (o + scale * (p @ vh).permute(0, 2, 1, 3).reshape(n, T, C)).half()
