"""The cases of tests/test_gpu_helpers.py as CPU data: operands, float64 references and derived bounds of the helper kernels and of the fp32
warping path (csrc/elementwise.hip, f32path.hip, attention.hip attn_single_query_kernel).

tests/test_gpu_helpers.py places the operands in poisoned device buffers and judges the kernels with check_elem; tests/test_cpu_helpers_ref.py
pins the references against independent implementations and checks that no bound is loose (limit < 2e-2 max |ref| for every case).
Every bound comes from the reference alone; u = U32 = 2^-24 throughout."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import util as U

U32, ACT_EVAL = U.U32, U.ACT_EVAL


def randn(shape, seed, scale=1.0, half=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    return t.half().float() if half else t


# -------------------------------------------------------------------------------------------------------------- single-query attention
# (d, heads, Nk, n, multiplier of q): the first four are the issue's list -- d = 80 / 128 / 40 run the `lane + 64 < d` half or leave lanes idle,
# Nk = 257 / 1 / 70 -- the fifth repeats the smallest with q scaled so that the largest logits sit near 40 (the maximum subtraction)
SQ_CASES = [(80, 16, 257, 2, 1.0), (128, 2, 5, 1, 1.0), (64, 2, 1, 2, 1.0), (40, 3, 70, 1, 1.0), (40, 3, 70, 1, 16.0)]


@functools.lru_cache(maxsize=None)
def single_query_case(d, heads, Nk, n, qmul):
    """q [n, heads d], kv [n, Nk, 2 heads d] (k | v interleaved per row, as the inversion adapter's fused projection leaves them), scale, and
    (ref, bound) [n, heads d]"""
    H = heads * d
    q = (randn((n, H), 900 + d, qmul)).half().float()
    kv = randn((n, Nk, 2 * H), 901 + d, half=True)
    scale = 1.0 / math.sqrt(d)
    qh = q.reshape(n, heads, d)
    kh = kv[..., :H].reshape(n, Nk, heads, d).permute(0, 2, 1, 3)
    vh = kv[..., H:].reshape(n, Nk, heads, d).permute(0, 2, 1, 3)
    ref, bound = U.single_query_ref_bound(qh, kh, vh, scale)
    return q, kv, scale, ref.reshape(n, H), bound.reshape(n, H)


# ------------------------------------------------------------------------------------------------------------------------ small_linear
# (x fp32, out fp32, act, pre_silu, residual, M, N, K).  Rows 0-2 are the UNet's time-embedding MLP (runtime_unet.cpp: fp32 -> fp32 with SiLU, plain,
# and pre-SiLU), rows 3-5 the inversion adapter (runtime_vae.cpp: fp16 -> fp16 plain, with a residual at ldr != N, GELU), row 6 the TPS regression
# (runtime_tps.cpp: fp16 -> fp32, tanh, N = 50: the last block has two waves with nn >= N); the rest cross the remaining dtypes, activations and
# pre_silu / residual combinations.  M runs 1 / 8 / 9 / 19 around MT = 8, K 8 (one lane busy) / 512 (one pass) / 520 / 1280 (tail pass).
SL_CASES = [
    (1, 1, "silu", 0, 0, 1, 50, 8),
    (1, 1, "none", 0, 0, 8, 4, 512),
    (1, 1, "none", 1, 0, 9, 101, 1280),
    (0, 0, "none", 0, 0, 19, 50, 520),
    (0, 0, "none", 0, 1, 9, 101, 512),
    (0, 0, "gelu", 0, 0, 8, 50, 1280),
    (0, 1, "tanh", 0, 0, 1, 50, 520),
    (1, 0, "relu", 0, 1, 19, 4, 8),
    (0, 1, "silu", 1, 1, 9, 50, 512),
    (1, 0, "gelu", 1, 0, 8, 101, 520),
    (0, 0, "tanh", 1, 1, 1, 4, 1280),
    (1, 1, "relu", 0, 0, 19, 101, 520),
]


def linear_ref_bound(x, w, b, act="none", pre_silu=False, res=None):
    """out = act(x' w^T + b) (+ res), x' = silu(x) when pre_silu; x [M, K], w [N, K], float64.  tests/util.py conv_ref_bound's 1 x 1 case:
    (K + 2) u (|w| |x'| + |b|) for the K-term fp32 sum in any order (with fp32 operands the products are fused into the sum, not rounded on
    their own), propagated through ACT_LIP / ACT_EVAL.  pre_silu: x' is itself evaluated in fp32, ACT_EVAL |x'| per element, which enters as
    the operand perturbation x_err.  The residual is added in fp32 AFTER the activation with no rounding in between: one rounding, u |ref|."""
    x, w = x.double(), w.double()
    M, K = x.shape
    N = w.shape[0]
    xe = None
    if pre_silu:
        x = F.silu(x)
        xe = (ACT_EVAL * x.abs()).t().reshape(1, K, M, 1)
    r, e = U.conv_ref_bound(x.t().reshape(1, K, M, 1), w.reshape(N, K, 1, 1), bias=b, act=act, padding=0, x_err=xe)
    r, e = r.reshape(N, M).t(), e.reshape(N, M).t()
    if res is not None:
        r = r + res.double()
        e = e + U32 * r.abs()
    return r, e


@functools.lru_cache(maxsize=None)
def small_linear_case(xf, of, act, pre, has_res, M, N, K):
    seed = 1000 + 7 * M + N + K
    x = randn((M, K), seed, half=not xf)
    w = randn((N, K), seed + 1, 1.0 / math.sqrt(K), half=True)
    b = randn((N,), seed + 2, half=True)
    res = randn((M, N), seed + 3, half=True) if has_res else None
    ref, bound = linear_ref_bound(x, w, b, act, bool(pre), res)
    return x, w, b, res, ref, bound


@functools.lru_cache(maxsize=None)
def linear_f32_case(K):
    M, N = 2, 50
    x, w, b = randn((M, K), 1100 + K), randn((N, K), 1101 + K, 1.0 / math.sqrt(K)), randn((N,), 1102 + K, 0.5)
    return (x, w, b) + linear_ref_bound(x, w, b, "tanh")


# ---------------------------------------------------------------------------------------------------------------------------- conv_f32
class ConvF32Case:
    """one row of the issue's table: fp32 (not fp16-rounded) operands, NHWC sources with their own row strides, weights [Q][tap][C0 + C1]"""

    def __init__(self, name, C0, C1, Q, k, stride, pad, N, H, W, act, bias, ld0, ld1, ldo, seed):
        self.name, self.C0, self.C1, self.Q, self.k, self.stride, self.pad, self.N, self.H, self.W = name, C0, C1, Q, k, stride, pad, N, H, W
        self.act, self.ld0, self.ld1, self.ldo = act, ld0, ld1, ldo
        C = C0 + C1
        x = randn((N, C, H, W), seed)
        wt = randn((Q, C, k, k), seed + 1, 1.0 / math.sqrt(k * k * C))
        self.bias = randn((Q,), seed + 2, 0.5) if bias else None
        ref, bound = U.conv_ref_bound(x, wt, bias=self.bias, act=act, stride=stride, padding=pad)
        self.Ho, self.Wo = ref.shape[2], ref.shape[3]
        self.P, self.K = N * self.Ho * self.Wo, k * k * C
        nhwc = x.permute(0, 2, 3, 1).reshape(-1, C)
        self.src0, self.src1 = nhwc[:, :C0].contiguous(), (nhwc[:, C0:].contiguous() if C1 else None)
        self.w = wt.permute(0, 2, 3, 1).reshape(Q, self.K).contiguous()
        self.ref = ref.permute(0, 2, 3, 1).reshape(self.P, Q)
        self.bound = bound.permute(0, 2, 3, 1).reshape(self.P, Q)


@functools.lru_cache(maxsize=None)
def conv_f32_cases():
    c = ConvF32Case
    return {
        # a: <1,4> form, Q = 3: the scalar store tail; ldo = 3 (dense) and ldo = 8 (padding columns stay untouched)
        "a3": c("a3", 24, 0, 3, 3, 1, 1, 1, 9, 7, "tanh", True, 32, 0, 3, 1200),
        "a8": c("a8", 24, 0, 3, 3, 1, 1, 1, 9, 7, "tanh", True, 32, 0, 8, 1200),
        # b: two sources in the K loop, P = 306: a partial second 256-pixel block
        "b": c("b", 8, 16, 64, 3, 1, 1, 2, 17, 9, "relu", True, 12, 16, 72, 1210),
        # c: <2,2> form (Q > 64), 4x4 stride-2 taps, partial channel tile, one 128-pixel tile spans the three samples
        "c": c("c", 8, 0, 72, 4, 2, 1, 3, 12, 8, "relu", True, 12, 0, 80, 1220),
        # d: 1x1, two channel tiles, no activation, no bias, dense output rows
        "d": c("d", 16, 0, 136, 1, 1, 0, 1, 13, 11, "none", False, 20, 0, 136, 1230),
        # f: SiLU
        "f": c("f", 8, 0, 8, 3, 1, 1, 1, 5, 5, "silu", True, 12, 0, 12, 1240),
    }


@functools.lru_cache(maxsize=None)
def conv_f32_corr_case():
    """e: the batched correlation launch of the TPS network: per sample b, out[b][p][q] = sum_c fb[b][p][c] fa[b][q][c] -- the weight operand
    is the other feature map (ldw = C, bs_w = hw C), Q = P = hw = 24, batch 2"""
    B, C, hw = 2, 16, 24
    fb, fa = randn((B, hw, C), 1250), randn((B, hw, C), 1251)
    ref, bound = U.gemm_batched_ref_bound(list(fb), list(fa), out_f32=True)
    return fb, fa, ref, bound


# --------------------------------------------------------------------------------------------------------------- fp32 / fp16 helpers
def l2norm_ref_bound(x):
    """y = x / sqrt(sum_c x^2 + 1e-6) over the last dimension.  The sum of C non-negative terms carries (C + 1) u RELATIVE (products and
    additions), the added 1e-6 one more u; the square root halves that and adds its own rounding, the reciprocal and the final product one each:
    ((C + 2) / 2 + 4) u |y| (one spare).  A zero row gives exactly zero."""
    x = x.double()
    C = x.shape[-1]
    ref = x / torch.sqrt((x * x).sum(-1, keepdim=True) + 1e-6)
    return ref, ((C + 2) / 2.0 + 4.0) * U32 * ref.abs()


def l2norm_input(C, seed, half):
    x = randn((5, C), seed, half=half)
    x[3] = 0.0
    return x


def upsample_ref_bound(x):
    """F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True) of x [n, C, H, W] in float64, and the bound of the kernel's fp32
    form top = v00 + (v01 - v00) fx, bot likewise, out = top + (bot - top) fy.
    Interpolation: on the way to any output lie four fp32 roundings -- difference, fused multiply-add, difference, fused multiply-add -- each
    of a value of magnitude at most 2 A, A = the largest |corner| the pixel reads (a difference of two corners; the sums stay within A; the
    roundings inside top / bot reach the output weighted by (1 - fy) / fy and are covered by the same four): 4 u 2 A.
    Coordinate: s = o (H - 1) / (Ho - 1) is one fp32 division, |ds| <= u s <= u (H - 1) (the product of two small integers is exact, s - floor(s)
    is exact).  The interpolant is continuous and piecewise linear, so the output moves by at most |dv/ds| |ds|, with |dv/ds| <= the largest
    difference of vertical neighbours Dy (a rounding across an integer lands on the adjacent segment, hence the maximum over the plane);
    the same for x: u ((H - 1) Dy + (W - 1) Dx)."""
    x = x.double()
    n, C, H, W = x.shape
    ref = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    A = F.max_pool2d(F.pad(x.abs(), (1, 1, 1, 1)), 3, stride=1)                  # 3 x 3 neighbourhood maximum >= the four corners' maximum
    A = F.interpolate(A, scale_factor=2, mode="nearest")
    Dy = float((x[:, :, 1:] - x[:, :, :-1]).abs().max()) if H > 1 else 0.0
    Dx = float((x[:, :, :, 1:] - x[:, :, :, :-1]).abs().max()) if W > 1 else 0.0
    return ref, 8 * U32 * A + U32 * ((H - 1) * Dy + (W - 1) * Dx)


# -------------------------------------------------------------------------------------------------------------------------- TPS grid
def tps_lattice(grid=5, rng=1.0):
    """control points (x, y) of the grid x grid lattice on [-rng, rng]^2, x fastest -- float64"""
    v = torch.linspace(-rng, rng, grid, dtype=torch.float64)
    yy, xx = torch.meshgrid(v, v, indexing="ij")
    return torch.stack([xx.reshape(-1), yy.reshape(-1)], 1)


def tps_phi(r2):
    return torch.where(r2 > 0, 0.5 * r2 * torch.log(r2.clamp_min(1e-300)), torch.zeros_like(r2))


def tps_inverse_kernel(ctrl):
    """inverse of the TPS kernel matrix [[phi(|c_i - c_j|^2), 1, c], [1, 0, 0], [c^T, 0, 0]] of the control points, float64"""
    ctrl = ctrl.double()
    n = ctrl.shape[0]
    d = ctrl[:, None, :] - ctrl[None, :, :]
    K = torch.zeros((n + 3, n + 3), dtype=torch.float64)
    K[:n, :n] = tps_phi((d * d).sum(-1))
    K[:n, n] = 1
    K[n, :n] = 1
    K[:n, n + 1:] = ctrl
    K[n + 1:, :n] = ctrl.t()
    return torch.inverse(K)


def tps_grid_ref_bound(coor, inv, ctrl, H, W):
    """grid[b][y][x] = [phi(p, c_0 .. c_{N-1}), 1, X, Y] . (inv . [coor_b; 0; 0; 0]), phi(r^2) = r^2 log(r^2) / 2 (0 at r = 0),
    p = (X, Y) = (2 x / (W - 1) - 1, 2 y / (H - 1) - 1) -- the formula in the kernel's comment, float64 -- and the bound of its fp32 form.
      map = inv[:, :N] coor: N-term sums, e_map = (N + 1) u |inv| |coor|
      X, Y:   a division and a subtraction of values up to 2: dX = 4 u; d = X - c_k one more rounding: dd = 6 u (|d| <= 2)
      r^2:    dr2 = 2 (|dx| + |dy|) dd + 2 dd^2 + 3 u r^2
      phi:    |dphi/dr2| = (|log r^2| + 1) / 2, evaluated no closer to zero than the perturbation itself can bring r^2, ACT_EVAL |phi| for the
              logarithm, two products: dphi = (|log max(r^2, 2 dd^2)| + 1) dr2 / 2 + (ACT_EVAL + 2 u) |phi|.  Where the pixel IS the control
              point in fp32 too (dx = dy = 0 exactly) both sides take the r2 == 0 branch and dphi = 0
      sum:    N + 3 terms, (N + 4) u over the absolute terms, plus each term's own perturbation."""
    coor, inv, ctrl = coor.double(), inv.double(), ctrl.double()
    B, N = coor.shape[0], ctrl.shape[0]
    mp = torch.einsum("rk,bkd->brd", inv[:, :N], coor)                           # [B, N + 3, 2]
    e_mp = (N + 1) * U32 * torch.einsum("rk,bkd->brd", inv[:, :N].abs(), coor.abs())
    xs = torch.arange(W, dtype=torch.float64) * 2 / (W - 1) - 1
    ys = torch.arange(H, dtype=torch.float64) * 2 / (H - 1) - 1
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    P = torch.stack([X.reshape(-1), Y.reshape(-1)], 1)                           # [HW, 2]
    d = P[:, None, :] - ctrl[None, :, :]
    r2 = (d * d).sum(-1)                                                         # [HW, N]
    phi = tps_phi(r2)
    dd, dX = 6 * U32, 4 * U32
    dr2 = 2 * d.abs().sum(-1) * dd + 2 * dd * dd + 3 * U32 * r2
    dphi = 0.5 * (torch.log(r2.clamp_min(2 * dd * dd)).abs() + 1) * dr2 + (ACT_EVAL + 2 * U32) * phi.abs()
    dphi = torch.where(r2 == 0, torch.zeros_like(dphi), dphi)
    rep = torch.cat([phi, torch.ones((H * W, 1), dtype=torch.float64), P], 1)    # [HW, N + 3]
    drep = torch.cat([dphi, torch.zeros((H * W, 1), dtype=torch.float64), torch.full((H * W, 2), dX, dtype=torch.float64)], 1)
    ref = torch.einsum("pr,brd->bpd", rep, mp)
    bound = ((N + 4) * U32 * torch.einsum("pr,brd->bpd", rep.abs(), mp.abs()) + torch.einsum("pr,brd->bpd", rep.abs(), e_mp)
             + torch.einsum("pr,brd->bpd", drep, mp.abs() + e_mp))
    return ref.reshape(B, H, W, 2), bound.reshape(B, H, W, 2)


# (N, H, W): the product's 25 points on an even and an odd image, one point, the limit of 32, and the 5 x 5 image whose every pixel is a
# control point (the r2 == 0 branch)
TPS_CASES = [(25, 16, 12), (1, 17, 19), (32, 17, 19), (25, 5, 5)]


@functools.lru_cache(maxsize=None)
def tps_case(N, H, W):
    """coor [2, N, 2], inv [(N + 3)^2], ctrl [N, 2] as fp32 tensors, and (ref, bound).  N = 25: the 5 x 5 lattice (range 0.9 as in the product;
    range 1 for the 5 x 5 image, where lattice and pixel centres coincide) with inv the float64 inverse of its kernel matrix; N = 1 (whose
    kernel matrix is singular) and N = 32: random control points and a random matrix in place of the inverse -- the kernel only multiplies by it."""
    if N == 25:
        ctrl = tps_lattice(5, 1.0 if (H, W) == (5, 5) else 0.9)
        inv = tps_inverse_kernel(ctrl)
    else:
        ctrl = randn((N, 2), 1300 + N, 0.5).double().clamp(-1, 1)
        inv = randn((N + 3, N + 3), 1301 + N, 1.0 / math.sqrt(N + 3)).double()
    coor = (ctrl[None] + randn((2, N, 2), 1302 + N, 0.1).double()).clamp(-1, 1)
    coor, inv, ctrl = coor.float(), inv.float(), ctrl.float()                    # what the device holds; the reference starts from these
    ref, bound = tps_grid_ref_bound(coor, inv, ctrl, H, W)
    return coor, inv, ctrl, ref, bound


# ------------------------------------------------------------------------------------------------------------------ text and vision
TEXT_T, TEXT_VSTAR = 77, 300


def text_meta_ids():
    """[6, 77] int32: vstar at 70 only; at 3 and 70; none; the maximum at 10 and again at 70; the maximum at 65 and 66 (two lanes of the second
    pass, adjacent); all ids negative (maximum -2 at 40 and 41)"""
    g = torch.Generator().manual_seed(1400)
    ids = torch.randint(1, 290, (6, TEXT_T), generator=g, dtype=torch.int32)
    ids[0, 70] = TEXT_VSTAR
    ids[1, 3] = TEXT_VSTAR
    ids[1, 70] = TEXT_VSTAR
    ids[3, 10] = 319
    ids[3, 70] = 319
    ids[4, 65] = 319
    ids[4, 66] = 319
    ids[5] = -ids[5] - 2
    ids[5, 40] = -2
    ids[5, 41] = -2
    return ids


def text_meta_ref(ids, vstar, use_words):
    """(first, eot) by a plain Python loop: the first position holding vstar (-1: none or use_words == 0); b T + the FIRST maximum"""
    B, T = ids.shape
    first, eot = [], []
    for b in range(B):
        row = [int(v) for v in ids[b]]
        f = next((t for t, v in enumerate(row) if v == vstar), -1)
        first.append(f if use_words else -1)
        best = max(row)
        eot.append(b * T + next(t for t, v in enumerate(row) if v == best))
    return torch.tensor(first, dtype=torch.int32), torch.tensor(eot, dtype=torch.int32)


def text_embed_ref(ids, first, nv, tok, pos, wemb):
    """[B, T, H] fp16: (token | spliced pseudo-word) + position embedding, the sum formed in fp32 and rounded once; ids clamped to the table"""
    B, T = ids.shape
    vocab = tok.shape[0]
    a = tok[ids.long().clamp(0, vocab - 1)].clone()                              # [B, T, H]
    if wemb is not None:
        for b in range(B):
            f = int(first[b])
            for t in range(T):
                if f >= 0 and f <= t < f + nv:
                    a[b, t] = wemb[b, t - f]
    return (a.float() + pos[None, :T].float()).half()


def patchify_ref(px, ps, KP):
    """[B, 1 + G^2, KP] fp16: row 0 zero, row 1 + gy G + gx = the patch in (c, ky, kx) order, columns >= 3 ps^2 zero"""
    B, _, S, _ = px.shape
    G = S // ps
    p = px.reshape(B, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B, G * G, 3 * ps * ps)
    out = torch.zeros((B, 1 + G * G, KP), dtype=torch.float16)
    out[:, 1:, :3 * ps * ps] = p.half()
    return out


# ------------------------------------------------------------------------------------------------------------------------- loop glue
TIMESTEPS = [0.0, 1.0, 500.5, 981.0, 999.0]


def timestep_freq(dim):
    half = dim // 2
    return torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)


def timestep_ref_bound(t, dim, expf_ulps):
    """[cos(t f_j) | sin(t f_j)], f_j = exp(-ln(10000) j / half), float64.  The kernel's f_j carries expf_ulps fp32 ulps of relative error (the
    fast exponential and the fp32 arithmetic of its argument), the product t f_j one rounding and one is spare: the argument is off by at most
    |t f_j| (expf_ulps + 2) u, and cos / sin are 1-Lipschitz; their own evaluation is granted 2 u absolute."""
    arg = torch.tensor(t, dtype=torch.float64)[:, None] * timestep_freq(dim)[None, :]
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    e = arg.abs() * (expf_ulps + 2) * U32 + 2 * U32
    return ref, torch.cat([e, e], 1)


def post_quant_ref_bound(lat, pq, inv_sf):
    """z = lat inv_sf, out_c = b_c + sum_j w_cj z_j (identity without pq): the product with inv_sf and the four multiply-adds are five fp32
    operations, each rounding a partial result no larger than |b_c| + sum_j |w_cj| |z_j|: 5 u of that."""
    z = lat.double() * float(torch.tensor(inv_sf, dtype=torch.float32))
    w = pq[:16].double().reshape(4, 4) if pq is not None else torch.eye(4, dtype=torch.float64)
    b = pq[16:].double() if pq is not None else torch.zeros(4, dtype=torch.float64)
    return z @ w.t() + b, 5 * U32 * (z.abs() @ w.abs().t() + b.abs())


def all_finite_halves():
    """every finite fp16 bit pattern (63 488 of them) and one more zero: [21 163, 3] fp16"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7C00) != 0x7C00]
    assert bits.numel() == 63488
    bits = torch.cat([bits, torch.zeros(1, dtype=torch.int32)])
    return bits.to(torch.int16).view(torch.float16).reshape(21163, 3)


def image_post_ref(x):
    """(fp32 image, uint8 image) as numpy computes them: clip(x / 2 + 0.5, 0, 1) in fp32, round-half-to-even of v * 255"""
    import numpy as np
    v = np.clip(x.numpy().astype(np.float32) * np.float32(0.5) + np.float32(0.5), 0, 1).astype(np.float32)
    return torch.from_numpy(v), torch.from_numpy(np.round(v * np.float32(255)).astype(np.uint8))


# ----------------------------------------------------------------------------------------------------------- every bounded case, by name
def bounded_cases(expf_ulps):
    """(name, ref, bound, out_f32, out dtype is fp16) of every case test_gpu_helpers.py judges with check_elem"""
    for c in SQ_CASES:
        _, _, _, ref, bound = single_query_case(*c)
        yield "single_query/d%d_h%d_k%d_n%d_q%g" % c, ref, bound, False
    for c in SL_CASES:
        *_, ref, bound = small_linear_case(*c)
        yield "small_linear/" + "_".join(str(v) for v in c), ref, bound, bool(c[1])
    for K in (768, 40):
        *_, ref, bound = linear_f32_case(K)
        yield "linear_f32/K%d" % K, ref, bound, True
    for name, c in conv_f32_cases().items():
        yield "conv_f32/" + name, c.ref, c.bound, True
    _, _, ref, bound = conv_f32_corr_case()
    yield "conv_f32/e", ref, bound, True
    for C in (8, 72, 512):
        yield ("l2norm_f32/C%d" % C,) + l2norm_ref_bound(l2norm_input(C, 1500 + C, False)) + (True,)
    for C in (8, 512, 520):
        yield ("l2norm/C%d" % C,) + l2norm_ref_bound(l2norm_input(C, 1510 + C, True)) + (False,)
    for shape in ((2, 8, 10, 6), (1, 8, 1, 1), (1, 8, 1, 4)):
        yield ("upsample_f32/%dx%d" % shape[2:],) + upsample_ref_bound(randn(shape, 1520 + shape[3])) + (True,)
    for c in TPS_CASES:
        *_, ref, bound = tps_case(*c)
        yield "tps_grid/N%d_%dx%d" % c, ref, bound, True
    for dim in (320, 1280):
        yield ("timestep/dim%d" % dim,) + timestep_ref_bound(TIMESTEPS, dim, expf_ulps) + (True,)
    lat, pq = randn((37, 4), 1530, 4.0), randn((20,), 1531, 0.5)
    yield ("post_quant/pq",) + post_quant_ref_bound(lat, pq, 1.0 / 0.18215) + (False,)
    yield ("post_quant/identity",) + post_quant_ref_bound(lat, None, 1.0 / 0.18215) + (False,)
