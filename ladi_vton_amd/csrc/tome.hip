// Token merging (ToMe for Stable Diffusion: tomesd's bipartite_soft_matching_random2d) for the transformer blocks of the UNet.
// Arithmetic (tests/tome_ref.py restates it): the T = h w tokens of a block are split into one dst token per full 2 x 2 cell and the src
// tokens (all others); every src is matched to the dst with the largest cosine similarity of the block's token input, the r src with the
// largest score are averaged into their dst, and a sub-layer runs over the Tm = T - r rows [unmerged src (ascending) ; dst].  Five kernels:
//   prep     one wave per panel row: gather a token row, L2-normalise it (fp32 sum of squares, norm clamped at 1e-12, so an all-zero row
//            stays zero and scores 0) and store it as fp16 into the src panel [n][NsP][C] or the dst panel [n][NdP][C]; rows beyond Ns / Nd
//            are written as zeros, so the match kernel loads whole tiles without a test (NsP % 128 == 0, NdP % 32 == 0)
//   match    score = max_j a_i . b_j and node = the lowest such j, for 128 src rows per workgroup.  v_mfma_f32_32x32x16_f16 with the DST
//            tile as the A operand and the SRC rows as the B operand: D[dst row][src column] has its column on the lane, so the running
//            (max, argmax) of a src row lives in the registers of the two lanes that own its column -- the 16 accumulator registers of a lane
//            are 16 dst rows in ascending order, a strict > keeps the lowest j, one cross-half exchange at the end.  The score matrix never
//            goes to memory.  The src fragments of a wave stay in registers for C <= 640 (C / 16 fragments of 4 VGPRs; C = 640: 160 VGPRs);
//            the dst tile (32 rows) is staged in LDS, rows padded by 16 bytes, and shared by the 4 waves
//   plan     one workgroup per sample: radix select (4 x 8 bits) of the r-th largest key -- the fp32 score as an order-preserving unsigned,
//            NaN as -inf, -0 as +0 -- then, in ascending src order, block scans that give every src its rank among the ties (ties across the
//            r-th place go to the lower src) and among the unmerged; per-dst counts, their exclusive scan, an unordered fill and a rank pass
//            (position of a src in its segment = number of smaller src in it), so the segments are in ascending src order whatever order the
//            integer LDS atomics ran in.  Writes out_row[T] and the plan buffer [seg_off (Nd + 1) | unm_pos (Nu) | seg_src (r) | scratch (r)]
//   merge    one wave per merged row, 16-byte accesses: an unmerged row is a copy; row Nu + j is (x[dst_j] + sum x[src]) / (1 + count) with
//            an fp32 accumulator, the sum in segment (ascending src) order: bit-reproducible
//   unmerge  out[p] = fp16(float(y[out_row[p]]) + float(res[p])): the residual of the sub-layer is added here, one rounding
// Bounds: every token position read from a table or a plan is tested against T (Tm for out_row) before it becomes an address; panel rows
// are addressed below NsP / NdP only; the plan kernel's LDS holds Nd <= 4096 counters (the launcher refuses more).
#include "common.h"
#include "kernels.h"
#include <cstdint>
#include <cmath>
#include <vector>

namespace {

constexpr int TOME_MATCH_ROWS = 128;   // src rows per workgroup of the match kernel: 4 waves x 32
constexpr int TOME_MAX_C = 960;        // prep holds a row in two 16-byte vectors per lane; the dst tile 32 x (C + 8) halves fits 64 KB of LDS
constexpr int TOME_MAX_ND = 4096;      // per-dst counters of the plan kernel in LDS
constexpr int TOME_PLAN_THREADS = 1024;

__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
    const h16x8 h = *reinterpret_cast<const h16x8*>(&u);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)h[i];
}

// ------------------------------------------------------------------------------------------------ prep
struct PrepArgs {
    const h16* x; int ld; long long sx;
    const int* src_pos; const int* dst_pos;
    int T, Ns, Nd, NsP, NdP, C;
    h16* A; h16* B;
};

__global__ __launch_bounds__(256) void tome_prep_kernel(PrepArgs a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), s = blockIdx.y;
    if (row >= a.NsP + a.NdP) return;
    const bool is_src = row < a.NsP;
    const int i = is_src ? row : row - a.NsP;
    h16* out = is_src ? a.A + ((long long)s * a.NsP + i) * a.C : a.B + ((long long)s * a.NdP + i) * a.C;
    const int cv = a.C >> 3;
    int pos = -1;
    if (i < (is_src ? a.Ns : a.Nd)) pos = is_src ? a.src_pos[i] : a.dst_pos[i];
    if ((unsigned)pos >= (unsigned)a.T) {                  // a padding row (or a position outside the block: never read)
        for (int v = lane; v < cv; v += 64) *reinterpret_cast<uint4*>(out + v * 8) = make_uint4(0, 0, 0, 0);
        return;
    }
    const h16* xr = a.x + (long long)s * a.sx + (long long)pos * a.ld;
    float f[2][8];
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int v = lane + 64 * k;
        if (v < cv) {
            unpack8(*reinterpret_cast<const uint4*>(xr + v * 8), f[k]);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = fmaf(f[k][e], f[k][e], ss);
        }
    }
    ss = wave_sum(ss);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int v = lane + 64 * k;
        if (v < cv) {
            h16x8 r;
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = (h16)(f[k][e] / nrm);
            *reinterpret_cast<uint4*>(out + v * 8) = *reinterpret_cast<const uint4*>(&r);
        }
    }
}

// ------------------------------------------------------------------------------------------------ match
// CB: C / 64 when the wave's src fragments stay in registers, 0: any C, the fragments are re-read (from L1 / L2) for every dst tile
template <int CB>
__global__ __launch_bounds__(256) void tome_match_kernel(const h16* __restrict__ A, const h16* __restrict__ B, int Ns, int Nd, int NsP, int NdP, int C,
                                                         float* __restrict__ score, int* __restrict__ node) {
    extern __shared__ __align__(16) h16 tome_tile[];            // [32][C + 8]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, s = blockIdx.y;
    const int r32 = lane & 31, hh = lane >> 5;
    const int ldt = C + 8, cv = C >> 3;
    const int row = blockIdx.x * TOME_MATCH_ROWS + wv * 32 + r32;           // < NsP: NsP is a multiple of TOME_MATCH_ROWS
    const h16* Ar = A + ((long long)s * NsP + row) * C + 8 * hh;
    const h16* Bs = B + (long long)s * NdP * C;
    constexpr int KS = CB ? CB * 4 : 1;
    h16x8 sf[KS];
    if constexpr (CB > 0) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) sf[ks] = *reinterpret_cast<const h16x8*>(Ar + 16 * ks);
    }
    float best = -INFINITY;
    int bj = 0;
    const h16* tr = tome_tile + r32 * ldt + 8 * hh;
    for (int jt = 0; jt < NdP; jt += 32) {
        __syncthreads();                                         // the previous tile has been consumed by every wave
        for (int v = tid; v < 32 * cv; v += 256) {
            const int rr = v / cv, cc = v - rr * cv;
            *reinterpret_cast<uint4*>(tome_tile + rr * ldt + cc * 8) = *reinterpret_cast<const uint4*>(Bs + (long long)(jt + rr) * C + cc * 8);
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        if constexpr (CB > 0) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const h16x8*>(tr + 16 * ks), sf[ks], acc, 0, 0, 0);
        } else {
            for (int ks = 0; ks < C / 16; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const h16x8*>(tr + 16 * ks),
                                                             *reinterpret_cast<const h16x8*>(Ar + 16 * ks), acc, 0, 0, 0);
        }
        // D[dst row][src column]: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5): ascending in e
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = jt + (e & 3) + 8 * (e >> 2) + 4 * hh;
            const float v = acc[e];
            if (j < Nd && v > best) { best = v; bj = j; }
        }
    }
    const float ob = __shfl_xor(best, 32);
    const int oj = __shfl_xor(bj, 32);
    if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    if (hh == 0 && row < Ns) {
        score[(long long)s * Ns + row] = best;
        node[(long long)s * Ns + row] = bj;
    }
}

// ------------------------------------------------------------------------------------------------ plan
struct PlanArgs {
    const float* score; const int* node;        // [n][Ns]
    const int* src_pos; const int* dst_pos;
    int T, Ns, Nd, r;
    int* out_row;                               // [n][T]
    int* plan; long long ps;                    // [n][ps]: seg_off (Nd + 1) | unm_pos (Ns - r) | seg_src (r) | scratch (r)
};

// the fp32 score as an unsigned that orders like it; NaN counts as -inf, -0 as +0
__device__ __forceinline__ unsigned tome_key(float v) {
    if (v != v) v = -INFINITY;
    if (v == 0.f) v = 0.f;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive scan of one flag per thread over the workgroup (lanes by ballot, waves through LDS); *total: the workgroup's count
__device__ __forceinline__ int block_scan_flag(bool flag, int* wtot, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                             // wtot of the previous scan has been read
    if (lane == 0) wtot[wv] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < nw; ++k) { const int t = wtot[k]; if (k < wv) base += t; tot += t; }
    *total = tot;
    return base + before;
}

__global__ __launch_bounds__(TOME_PLAN_THREADS) void tome_plan_kernel(PlanArgs a) {
    __shared__ int hist[256];
    __shared__ int cnt[TOME_MAX_ND];
    __shared__ int wtot[TOME_PLAN_THREADS / 64];
    __shared__ unsigned sel[2];                                  // prefix of the r-th largest key, how many of it are still wanted
    const int tid = threadIdx.x, nt = blockDim.x, s = blockIdx.x;
    const float* sc = a.score + (long long)s * a.Ns;
    const int* nd = a.node + (long long)s * a.Ns;
    int* orow = a.out_row + (long long)s * a.T;
    int* seg_off = a.plan + (long long)s * a.ps;
    const int Nu = a.Ns - a.r;
    int* unm = seg_off + a.Nd + 1;
    int* seg_src = unm + Nu;
    int* tmp = seg_src + a.r;
    for (int j = tid; j < a.Nd; j += nt) cnt[j] = 0;
    if (tid == 0) { sel[0] = 0u; sel[1] = (unsigned)a.r; }
    // ---- the r-th largest key, 8 bits at a time from the top
    unsigned mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += nt) hist[b] = 0;
        __syncthreads();
        const unsigned prefix = sel[0];
        for (int i = tid; i < a.Ns; i += nt) {
            const unsigned k = tome_key(sc[i]);
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned want = sel[1], cum = 0u;
            int b = 255;
            for (; b > 0; --b) {
                if (cum + (unsigned)hist[b] >= want) break;
                cum += (unsigned)hist[b];
            }
            sel[0] = prefix | ((unsigned)b << shift);
            sel[1] = want - cum;
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned kstar = sel[0];
    const int want = (int)sel[1];                                // ties at kstar that are merged: the `want` lowest src among them
    // ---- ascending src order: rank among the ties, then rank among the unmerged
    int eq_base = 0, u_base = 0;
    for (int i0 = 0; i0 < a.Ns; i0 += nt) {
        const int i = i0 + tid;
        const bool in = i < a.Ns;
        const unsigned k = in ? tome_key(sc[i]) : 0u;
        const bool eq = in && k == kstar;
        int tot;
        const int er = block_scan_flag(eq, wtot, &tot) + eq_base;
        eq_base += tot;
        const bool merged = in && (k > kstar || (eq && er < want));
        const int ur = block_scan_flag(in && !merged, wtot, &tot) + u_base;
        u_base += tot;
        if (in) {
            const int pos = a.src_pos[i];
            int j = nd[i];
            j = j < 0 ? 0 : j >= a.Nd ? a.Nd - 1 : j;            // the match kernel never writes one outside; a caller's table might
            if ((unsigned)pos < (unsigned)a.T) orow[pos] = merged ? Nu + j : ur;
            if (merged) atomicAdd(&cnt[j], 1);
            else if (ur < Nu) unm[ur] = pos;
        }
    }
    __syncthreads();
    // ---- exclusive scan of the per-dst counts (4 consecutive dst per thread), dst rows of out_row
    {
        const int j0 = tid * 4;
        int c4[4], sum = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { c4[e] = (j0 + e < a.Nd) ? cnt[j0 + e] : 0; sum += c4[e]; }
        const int lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
        int inc = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
        __syncthreads();
        if (lane == 63) wtot[wv] = inc;
        __syncthreads();
        int base = 0;
        for (int k = 0; k < nw && k < wv; ++k) base += wtot[k];
        int off = base + inc - sum;
        __syncthreads();                                         // every count has been read before it becomes a cursor
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (j0 + e < a.Nd) {
                seg_off[j0 + e] = off;
                cnt[j0 + e] = off;
                const int pos = a.dst_pos[j0 + e];
                if ((unsigned)pos < (unsigned)a.T) orow[pos] = Nu + j0 + e;
            }
            off += c4[e];
        }
        if (tid == 0) seg_off[a.Nd] = a.r;
    }
    __syncthreads();
    // ---- unordered fill, then the rank inside the segment
    for (int i = tid; i < a.Ns; i += nt) {
        const int pos = a.src_pos[i];
        if ((unsigned)pos >= (unsigned)a.T || orow[pos] < Nu) continue;
        int j = nd[i];
        j = j < 0 ? 0 : j >= a.Nd ? a.Nd - 1 : j;
        const int p = atomicAdd(&cnt[j], 1);
        if (p < a.r) tmp[p] = i;
    }
    __syncthreads();
    for (int i = tid; i < a.Ns; i += nt) {
        const int pos = a.src_pos[i];
        if ((unsigned)pos >= (unsigned)a.T || orow[pos] < Nu) continue;
        int j = nd[i];
        j = j < 0 ? 0 : j >= a.Nd ? a.Nd - 1 : j;
        const int b = seg_off[j], e = j + 1 < a.Nd ? seg_off[j + 1] : a.r;
        int rank = 0;
        for (int q = b; q < e; ++q) rank += tmp[q] < i;
        if (b + rank < a.r) seg_src[b + rank] = pos;
    }
}

// ------------------------------------------------------------------------------------------------ merge
struct MergeArgs {
    const h16* x; int ldx; long long sx;
    h16* y; int ldy; long long sy;
    const int* dst_pos; const int* plan; long long ps;
    int T, Ns, Nd, r, C;
};

__global__ __launch_bounds__(256) void tome_merge_kernel(MergeArgs a) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6), s = blockIdx.y;
    const int Nu = a.Ns - a.r, Tm = a.T - a.r;
    if (m >= Tm) return;
    const int* seg_off = a.plan + (long long)s * a.ps;
    const int* unm = seg_off + a.Nd + 1;
    const int* seg_src = unm + Nu;
    const h16* xs = a.x + (long long)s * a.sx;
    h16* yr = a.y + (long long)s * a.sy + (long long)m * a.ldy;
    const int cv = a.C >> 3;
    if (m < Nu) {
        const int pos = unm[m];
        if ((unsigned)pos >= (unsigned)a.T) return;
        for (int v = lane; v < cv; v += 64) *reinterpret_cast<uint4*>(yr + v * 8) = *reinterpret_cast<const uint4*>(xs + (long long)pos * a.ldx + v * 8);
        return;
    }
    const int j = m - Nu;
    const int dpos = a.dst_pos[j];
    if ((unsigned)dpos >= (unsigned)a.T) return;
    int b = seg_off[j], e = seg_off[j + 1];
    b = b < 0 ? 0 : b; e = e > a.r ? a.r : e;
    const float den = (float)(1 + (e > b ? e - b : 0));
    for (int v = lane; v < cv; v += 64) {
        float acc[8];
        unpack8(*reinterpret_cast<const uint4*>(xs + (long long)dpos * a.ldx + v * 8), acc);
        for (int q = b; q < e; ++q) {
            const int pos = seg_src[q];
            if ((unsigned)pos >= (unsigned)a.T) continue;
            float f[8];
            unpack8(*reinterpret_cast<const uint4*>(xs + (long long)pos * a.ldx + v * 8), f);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += f[k];
        }
        h16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (h16)(acc[k] / den);
        *reinterpret_cast<uint4*>(yr + v * 8) = *reinterpret_cast<const uint4*>(&o);
    }
}

// ------------------------------------------------------------------------------------------------ unmerge + residual
struct UnmergeArgs {
    const h16* y; int ldy; long long sy;
    const h16* res; int ldr; long long sr;
    h16* out; int ldo; long long so;
    const int* out_row;
    int T, Tm, cv; long long vecs;
};

__global__ __launch_bounds__(256) void tome_unmerge_add_kernel(UnmergeArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;       // (sample, token, channel vector)
    if (i >= a.vecs) return;
    const long long tok = i / a.cv;
    const int c = (int)(i - tok * a.cv) * 8;
    const int s = (int)(tok / a.T), p = (int)(tok - (long long)s * a.T);
    const int row = a.out_row[tok];
    if ((unsigned)row >= (unsigned)a.Tm) return;
    float yf[8], rf[8];
    unpack8(*reinterpret_cast<const uint4*>(a.y + (long long)s * a.sy + (long long)row * a.ldy + c), yf);
    unpack8(*reinterpret_cast<const uint4*>(a.res + (long long)s * a.sr + (long long)p * a.ldr + c), rf);
    h16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (h16)(yf[k] + rf[k]);
    *reinterpret_cast<uint4*>(a.out + (long long)s * a.so + (long long)p * a.ldo + c) = *reinterpret_cast<const uint4*>(&o);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned long long splitmix64(unsigned long long x) {
    unsigned long long z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host
int ladi_tome_tables_host(int h, int w, int sx, int sy, int use_rand, unsigned seed, int* src_pos, int* dst_pos, int cap) {
    if (h < 1 || w < 1 || sx != 2 || sy != 2 || (long long)h * w > 0x3fffffffLL) return -1;
    const int hsy = h / sy, wsx = w / sx, T = h * w, Nd = hsy * wsx;
    if (!src_pos && !dst_pos) return Nd;
    if (!src_pos || !dst_pos || cap < Nd || cap < T - Nd) return -1;
    std::vector<char> is_dst((size_t)T, 0);
    for (int cy = 0; cy < hsy; ++cy)
        for (int cx = 0; cx < wsx; ++cx) {
            const unsigned long long c = (unsigned long long)cy * wsx + cx;
            const int o = use_rand ? (int)(splitmix64(((unsigned long long)seed << 32) + c) % (unsigned long long)(sx * sy)) : 0;
            is_dst[(size_t)(cy * sy + o / sx) * w + cx * sx + o % sx] = 1;
        }
    int ns = 0, nd = 0;
    for (int p = 0; p < T; ++p) {
        if (is_dst[p]) dst_pos[nd++] = p;
        else src_pos[ns++] = p;
    }
    return Nd;
}

int ladi_tome_count_host(int T, int Ns, double ratio) {
    if (T < 1 || Ns < 0 || !(ratio >= 0.0) || !(ratio < 1.0)) return -1;
    const int r = (int)((double)T * ratio);
    return r < Ns ? r : Ns;
}

int ladi_tome_pad_src(int Ns) { return (Ns + TOME_MATCH_ROWS - 1) / TOME_MATCH_ROWS * TOME_MATCH_ROWS; }
int ladi_tome_pad_dst(int Nd) { return (Nd + 31) / 32 * 32; }
long long ladi_tome_plan_ints(int Ns, int Nd, int r) { return (long long)Nd + 1 + Ns + r; }

int ladi_launch_tome_prep(const h16* x, int ld, long long sx, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int C,
                          h16* A, h16* B, hipStream_t st) {
    if (!x || !src_pos || !dst_pos || !A || !B || n < 1 || n > 65535 || T < 1 || Ns < 1 || Nd < 1 || Ns + Nd != T) return -1;
    if (C < 64 || (C & 63) || C > TOME_MAX_C) return -2;
    if (ld < C || (ld & 7) || (sx & 7) || !al16(x) || !al16(A) || !al16(B)) return -3;
    PrepArgs a{x, ld, sx, src_pos, dst_pos, T, Ns, Nd, ladi_tome_pad_src(Ns), ladi_tome_pad_dst(Nd), C, A, B};
    hipLaunchKernelGGL(tome_prep_kernel, dim3((unsigned)((a.NsP + a.NdP + 3) / 4), (unsigned)n), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}

int ladi_launch_tome_match(const h16* A, const h16* B, int n, int Ns, int Nd, int C, float* score, int* node, hipStream_t st) {
    if (!A || !B || !score || !node || n < 1 || n > 65535 || Ns < 1 || Nd < 1) return -1;
    if (C < 64 || (C & 63) || C > TOME_MAX_C) return -2;
    if (!al16(A) || !al16(B)) return -3;
    const int NsP = ladi_tome_pad_src(Ns), NdP = ladi_tome_pad_dst(Nd);
    const dim3 grid((unsigned)(NsP / TOME_MATCH_ROWS), (unsigned)n);
    const size_t lds = (size_t)32 * (C + 8) * sizeof(h16);
    switch (C / 64) {
#define TOME_MATCH_CASE(CB) case CB: hipLaunchKernelGGL(tome_match_kernel<CB>, grid, dim3(256), lds, st, A, B, Ns, Nd, NsP, NdP, C, score, node); break;
        TOME_MATCH_CASE(1) TOME_MATCH_CASE(2) TOME_MATCH_CASE(4) TOME_MATCH_CASE(5) TOME_MATCH_CASE(10)
#undef TOME_MATCH_CASE
        default: hipLaunchKernelGGL(tome_match_kernel<0>, grid, dim3(256), lds, st, A, B, Ns, Nd, NsP, NdP, C, score, node); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -11;
}

int ladi_launch_tome_plan(const float* score, const int* node, const int* src_pos, const int* dst_pos, int n, int T, int Ns, int Nd, int r,
                          int* out_row, int* plan, hipStream_t st) {
    if (!score || !node || !src_pos || !dst_pos || !out_row || !plan || n < 1 || T < 1 || Ns < 1 || Nd < 1 || Ns + Nd != T) return -1;
    if (r < 1 || r > Ns) return -1;
    if (Nd > TOME_MAX_ND) return -4;
    PlanArgs a{score, node, src_pos, dst_pos, T, Ns, Nd, r, out_row, plan, ladi_tome_plan_ints(Ns, Nd, r)};
    hipLaunchKernelGGL(tome_plan_kernel, dim3((unsigned)n), dim3(TOME_PLAN_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}

int ladi_launch_tome_merge(const h16* x, int ldx, long long sx, const int* dst_pos, const int* plan, int n, int T, int Ns, int Nd, int r, int C,
                           h16* y, int ldy, long long sy, hipStream_t st) {
    if (!x || !dst_pos || !plan || !y || n < 1 || n > 65535 || T < 1 || Ns < 1 || Nd < 1 || Ns + Nd != T || r < 0 || r > Ns) return -1;
    if (C < 8 || (C & 7)) return -2;
    if (ldx < C || ldy < C || (ldx & 7) || (ldy & 7) || (sx & 7) || (sy & 7) || !al16(x) || !al16(y)) return -3;
    MergeArgs a{x, ldx, sx, y, ldy, sy, dst_pos, plan, ladi_tome_plan_ints(Ns, Nd, r), T, Ns, Nd, r, C};
    hipLaunchKernelGGL(tome_merge_kernel, dim3((unsigned)((T - r + 3) / 4), (unsigned)n), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}

int ladi_launch_tome_unmerge_add(const h16* y, int ldy, long long sy, const h16* res, int ldr, long long sr, const int* out_row, int n, int T,
                                 int Tm, int C, h16* out, int ldo, long long so, hipStream_t st) {
    if (!y || !res || !out_row || !out || n < 1 || T < 1 || Tm < 1 || Tm > T) return -1;
    if (C < 8 || (C & 7)) return -2;
    if (ldy < C || ldr < C || ldo < C || ((ldy | ldr | ldo) & 7) || ((sy | sr | so) & 7) || !al16(y) || !al16(res) || !al16(out)) return -3;
    UnmergeArgs a{y, ldy, sy, res, ldr, sr, out, ldo, so, out_row, T, Tm, C / 8, (long long)n * T * (C / 8)};
    if ((a.vecs + 255) / 256 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(tome_unmerge_add_kernel, dim3((unsigned)((a.vecs + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}
