// IP-Adapter image prompt (diffusers IPAdapterAttnProcessor2_0): the decoupled cross-attention over the N image tokens of a sample,
// accumulated in place into the attention output flash_attn64 has just written for the text tokens:
//   o[s, t, h*64 + d] = fp16(float(o[s, t, h*64 + d]) + scale * sum_j p[s,t,h,j] * v[s, j, h*64 + d])
//   p[s,t,h,:] = softmax_j(0.125 * <q[s,t,h,:], k[s,j,h,:]>),  j < N <= 64
// Many queries (up to 3 072 per sample) against 4 .. 16 keys: as a 64-key stage of flash_attn64 it would be 75 - 94 % padding, with the
// sum as one more pass over o.  Here a workgroup is (128 queries, one head, one sample): the head's K and V rows (N x 2 x 128 bytes, at
// most 16 KB) are staged in LDS once and every query is owned by 8 consecutive lanes, lane i holding dims [8 i, 8 i + 8) -- one 16-byte
// load of q, one 16-byte load and one 16-byte store of o per lane, the 8 lanes of a query covering one whole 128-byte line and a wave 8
// such lines (8 consecutive queries).  The logits are four v_dot2_f32_f16 per lane and key (products of two fp16 values are exact in fp32,
// the sums are fp32) plus a 3-step DPP sum over the 8 lanes; softmax with the row maximum subtracted and the P V sum are fp32 in registers;
// one rounding per output element.  No MFMA and no LDS traffic besides the K / V reads (two ds_read_b128 per key, the same address in all 8
// query groups of a wave: a broadcast).
// Bound: the launch moves 3 x n T C x 2 bytes (q read, o read, o written; K / V are N x 2C halves per sample and stay in L2) -- at n = 16,
// 64x48 latents, C = 320: 94 MB, 15.0 us at the 6.29 TB/s a streaming copy reaches on MI355X; 32x24 / C = 640: 47 MB, 7.5 us.  Measured
// (BASELINE.md "IP-Adapter image term"): 19.7 / 11.3 us at N = 4 (4.8 / 4.2 TB/s).  At N = 16 the kernel is bound by its vector arithmetic
// instead, 36.5 / 20.6 us: each of the 8 lanes of a query evaluates the whole softmax, about 28 instructions per key.
// Every address is derived from (t < T, j < N, h < heads, s < n): rows beyond T are never touched, columns beyond heads * 64 neither.
#include "common.h"
#include "kernels.h"
#include <cstdint>

namespace {

constexpr int IP_QPP = 32;       // queries per pass of a 256-thread workgroup (8 lanes each)
constexpr int IP_PASSES = 4;     // passes per workgroup: 128 queries share one staged K / V tile

struct IpArgs {
    const h16* q; const h16* k; const h16* v; h16* o;
    int ldq, ldk, ldv, ldo;
    long long sq, sk, sv, so;
    int T, N;
    float scale;
};

__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
    const h16x8 h = *reinterpret_cast<const h16x8*>(&u);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)h[i];
}

// sum over the 8 lanes of a query (lanes 8 g .. 8 g + 7) with data-parallel-primitive moves, no LDS traffic: lane ^ 1 and lane ^ 2 inside
// the quad, then the mirrored lane of the 8 (7 - i: the other quad, which holds its own quad's sum by then).  Every lane gets the same bits
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float sum8(float v) {
    v = dpp_add<0xB1>(v);      // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);      // quad_perm [2, 3, 0, 1]
    return dpp_add<0x141>(v);  // row_half_mirror
}

// 8 dims of <q, k>: products of two fp16 values are exact in fp32; v_dot2_f32_f16 adds two of them to the fp32 accumulator
__device__ __forceinline__ float dot8(const uint4& q, const uint4& k) {
    const h16x2* a = reinterpret_cast<const h16x2*>(&q);
    const h16x2* b = reinterpret_cast<const h16x2*>(&k);
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) d = __builtin_amdgcn_fdot2(a[i], b[i], d, false);
    return d;
}

// NMAX: the unrolled key count (4 / 8 / 16 / 32 / 64, the smallest that holds N), so that the logits stay in registers; FULL: N == NMAX,
// no per-key test
template <int NMAX, bool FULL>
__global__ __launch_bounds__(256) void ip_attn_add_kernel(IpArgs a) {
    __shared__ uint4 kv[NMAX * 16];                 // [j][0..7]: K row of this head (128 bytes), [j][8..15]: V row
    const int tid = threadIdx.x, h = blockIdx.y, s = blockIdx.z;
    const int N = FULL ? NMAX : a.N;
    const h16* kb = a.k + (long long)s * a.sk + h * 64;
    const h16* vb = a.v + (long long)s * a.sv + h * 64;
    for (int i = tid; i < N * 16; i += 256) {
        const int j = i >> 4, c = i & 15;
        const h16* src = c < 8 ? kb + (long long)j * a.ldk + c * 8 : vb + (long long)j * a.ldv + (c - 8) * 8;
        kv[i] = *reinterpret_cast<const uint4*>(src);
    }
    __syncthreads();
    const int sub = tid & 7;
    const h16* qb = a.q + (long long)s * a.sq + h * 64 + sub * 8;
    h16* ob = a.o + (long long)s * a.so + h * 64 + sub * 8;
#pragma unroll 1
    for (int pass = 0; pass < IP_PASSES; ++pass) {
        const int t = (blockIdx.x * IP_PASSES + pass) * IP_QPP + (tid >> 3);
        if (t >= a.T) break;                        // the 8 lanes of a query leave together; later passes hold later queries
        const uint4 q = *reinterpret_cast<const uint4*>(qb + (long long)t * a.ldq);
        const uint4 o_in = *reinterpret_cast<const uint4*>(ob + (long long)t * a.ldo);
        float l[NMAX];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (FULL || j < N) {
                l[j] = 0.125f * sum8(dot8(q, kv[j * 16 + sub]));
                m = fmaxf(m, l[j]);
            }
        }
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float den = 0.f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (FULL || j < N) {
                const float e = __expf(l[j] - m);
                den += e;
                float vf[8];
                unpack8(kv[j * 16 + 8 + sub], vf);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(e, vf[i], acc[i]);
            }
        }
        const float w = a.scale / den;              // den >= 1: the maximum's own term
        float of[8];
        unpack8(o_in, of);
        h16x8 r;
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = (h16)fmaf(w, acc[i], of[i]);
        *reinterpret_cast<uint4*>(ob + (long long)t * a.ldo) = *reinterpret_cast<const uint4*>(&r);
    }
}

// the A/B route's second half (kernels.h ladi_launch_ip_scaled_add): o = fp16(o + scale * x), one 16-byte vector per thread
__global__ __launch_bounds__(256) void ip_scaled_add_kernel(const h16* __restrict__ x, int ldx, h16* __restrict__ o, int ldo, long long rows, int cv,
                                                            float scale) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // (row, channel vector)
    if (i >= rows * cv) return;
    const long long row = i / cv;
    const int c = (int)(i - row * cv) * 8;
    float xf[8], of[8];
    unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c), xf);
    unpack8(*reinterpret_cast<const uint4*>(o + row * ldo + c), of);
    h16x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (h16)fmaf(scale, xf[k], of[k]);
    *reinterpret_cast<uint4*>(o + row * ldo + c) = *reinterpret_cast<const uint4*>(&r);
}

}  // namespace

int ladi_launch_ip_scaled_add(const h16* x, int ldx, h16* o, int ldo, long long rows, int C, float scale, hipStream_t st) {
    if (!x || !o || rows < 1 || C < 8 || (C & 7) || ldx < C || ldo < C || (ldx & 7) || (ldo & 7) || ((uintptr_t)x & 15) || ((uintptr_t)o & 15)) return -1;
    const long long vecs = rows * (C / 8);
    if ((vecs + 255) / 256 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(ip_scaled_add_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, x, ldx, o, ldo, rows, C / 8, scale);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}

int ladi_launch_ip_attn_add(const h16* q, int ldq, long long sq, const h16* k, int ldk, long long sk, const h16* v, int ldv, long long sv,
                            h16* o, int ldo, long long so, int n, int heads, int T, int N, float scale, hipStream_t st) {
    if (!q || !k || !v || !o || n < 1 || heads < 1 || T < 1 || N < 1 || N > 64) return -1;
    if ((ldq & 7) || (ldk & 7) || (ldv & 7) || (ldo & 3)) return -1;
    // 16-byte accesses to all four operands: o's rows too have to start on 16 bytes (flash_attn64 itself accepts ldo % 8 == 4)
    if ((ldo & 7) || (sq & 7) || (sk & 7) || (sv & 7) || (so & 7) || (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15)) return -1;
    if (ldq < heads * 64 || ldk < heads * 64 || ldv < heads * 64 || ldo < heads * 64) return -1;
    if (heads > 65535 || n > 65535) return -1;
    IpArgs a{q, k, v, o, ldq, ldk, ldv, ldo, sq, sk, sv, so, T, N, scale};
    const dim3 grid((unsigned)((T + IP_QPP * IP_PASSES - 1) / (IP_QPP * IP_PASSES)), (unsigned)heads, (unsigned)n);
    auto go = [&](auto full, auto part, int nmax) {
        if (N == nmax) hipLaunchKernelGGL(full, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(part, grid, dim3(256), 0, st, a);
    };
    if (N <= 4) go(ip_attn_add_kernel<4, true>, ip_attn_add_kernel<4, false>, 4);
    else if (N <= 8) go(ip_attn_add_kernel<8, true>, ip_attn_add_kernel<8, false>, 8);
    else if (N <= 16) go(ip_attn_add_kernel<16, true>, ip_attn_add_kernel<16, false>, 16);
    else if (N <= 32) go(ip_attn_add_kernel<32, true>, ip_attn_add_kernel<32, false>, 32);
    else go(ip_attn_add_kernel<64, true>, ip_attn_add_kernel<64, false>, 64);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}
