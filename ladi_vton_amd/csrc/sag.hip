// Self-attention guidance (diffusers StableDiffusionSAGPipeline, Hong et al. 2023): the two kernels the rest of the tree cannot express.
//
// sag_map: the column sums of a self-attention's softmax, which flash attention never materialises.  For one sample with H heads, T tokens
// and head dimension 64,
//   P_h = softmax(Q_h K_h^T / 8) over keys,   s[j] = (sum_h sum_i P_h[i, j]) / H,   m[j] = s[j] > 1
// Structure: plain VALU, two launches, no atomics.  Stage 1 runs one workgroup of four waves per (sample, head).  It walks query tiles of
// 64 rows: lane = query (its 64 pre-scaled fp32 dims in registers), wave = a quarter (16 keys) of every 64-key tile staged in LDS as fp32
// and read as broadcasts.  Pass 1 over all key tiles gives every wave its rows' running maximum and sum; the four are combined through LDS
// in wave order.  Pass 2 recomputes the logits, forms p = exp(l - max) / sum and reduces every key's column over the wave's 64 queries with
// the xor butterfly; lane 0 of the one wave that owns the key adds the tile's column sum to partial[sample][head][key] (the first query
// tile stores), so successive query tiles are added in tile order by the same thread.  Stage 2 sums the heads in index order, divides by H
// and thresholds.  Every sum has a fixed order, so two launches -- eager or replayed -- give the same bits.
// Why not MFMA: at the flagship shape (T = 48, 20 heads, 16 samples) both passes together are under 0.1 GFLOP spread over 320 workgroups;
// the launch is bound by its latency, not by arithmetic, and fp32 VALU keeps the logits at the precision the threshold wants.
//
// sag_degrade: steps 2-3 of the method fused, one thread per latent pixel.  x0 = (x - sqrt(1 - a) b) / sqrt(a) from the loop's fp32 latents
// and the base prediction's fp16 rows; where the nearest-upsampled mask is set, the 9 x 9 sigma-1 Gaussian of x0 with 4-pixel reflect
// padding (x0 of every tap recomputed from x and b: 81 taps, no staging); xd = sqrt(a) x0d + sqrt(1 - a) b, rounded to fp16 into channels
// 0..3 of the second forward's input rows.  sqrt(a), sqrt(1 - a) and the model-input scale come from a device table row picked by the
// device step counter.  The base rows' other channels are copied when the destination rows are other rows.
#include "common.h"
#include "kernels.h"
#include <cstdint>
#include <cmath>

namespace {

constexpr int SAG_QT = 64;     // queries per tile = lanes of a wave
constexpr int SAG_KT = 64;     // keys per LDS tile; wave w owns keys [16 w, 16 w + 16) of it

__global__ __launch_bounds__(256) void sag_colsum_kernel(const h16* __restrict__ q, int ldq, long long sq, const h16* __restrict__ k, int ldk,
                                                         long long sk, int T, int heads, float* __restrict__ partial) {
    __shared__ float Ks[SAG_KT][64];          // the key tile, fp32; every lane of a wave reads the same address (broadcast)
    __shared__ float red[2][4][SAG_QT];       // pass 1: (max, sum) of every wave's quarter, per query
    const int s = blockIdx.x / heads, hd = blockIdx.x - s * heads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const h16* qb = q + (long long)s * sq + hd * 64;
    const h16* kb = k + (long long)s * sk + hd * 64;
    float* pout = partial + ((size_t)s * heads + hd) * T;
    for (int q0 = 0; q0 < T; q0 += SAG_QT) {
        const int qi = q0 + lane;
        const bool qok = qi < T;
        float qv[64];
        {
            const h16* qp = qb + (long long)(qok ? qi : q0) * ldq;
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const h16x8 x = *reinterpret_cast<const h16x8*>(qp + v * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) qv[v * 8 + e] = (float)x[e] * 0.125f;       // 1 / sqrt(64): exact
            }
        }
        float mx = -INFINITY, sum = 0.f, inv = 0.f;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 1
            for (int k0 = 0; k0 < T; k0 += SAG_KT) {
                const int kn = T - k0 < SAG_KT ? T - k0 : SAG_KT;
                __syncthreads();                                     // the previous tile's readers are done with Ks
                // 64 keys x 64 dims: 512 vectors of 8 halves, two per thread
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int v = threadIdx.x + r * 256, kr = v >> 3, kc = (v & 7) * 8;
                    if (kr < kn) {
                        const h16x8 x = *reinterpret_cast<const h16x8*>(kb + (long long)(k0 + kr) * ldk + kc);
                        float4 lo = make_float4((float)x[0], (float)x[1], (float)x[2], (float)x[3]);
                        float4 hi = make_float4((float)x[4], (float)x[5], (float)x[6], (float)x[7]);
                        *reinterpret_cast<float4*>(&Ks[kr][kc]) = lo;
                        *reinterpret_cast<float4*>(&Ks[kr][kc + 4]) = hi;
                    }
                }
                __syncthreads();
                const int j0 = wave * 16, j1 = j0 + 16 < kn ? j0 + 16 : kn;
                for (int j = j0; j < j1; ++j) {
                    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
                    for (int d = 0; d < 64; d += 4) {
                        const float4 kv = *reinterpret_cast<const float4*>(&Ks[j][d]);
                        a0 = fmaf(qv[d], kv.x, a0); a1 = fmaf(qv[d + 1], kv.y, a1);
                        a2 = fmaf(qv[d + 2], kv.z, a2); a3 = fmaf(qv[d + 3], kv.w, a3);
                    }
                    const float l = (a0 + a1) + (a2 + a3);
                    if (pass == 0) {
                        if (l > mx) { sum *= expf(mx - l); mx = l; }         // first key: sum = 0 * exp(-inf) = 0
                        sum += expf(l - mx);
                    } else {
                        const float p = qok ? expf(l - mx) * inv : 0.f;
                        const float col = wave_sum(p);
                        if (lane == 0) {
                            float* dst = pout + k0 + j;
                            *dst = q0 == 0 ? col : *dst + col;
                        }
                    }
                }
            }
            if (pass == 0) {
                red[0][wave][lane] = mx; red[1][wave][lane] = sum;
                __syncthreads();
                // the four quarters in wave order; a wave that had no key (T < 49 in the only tile) holds (-inf, 0) and adds 0
                float M = red[0][0][lane];
#pragma unroll
                for (int w = 1; w < 4; ++w) M = fmaxf(M, red[0][w][lane]);
                float L = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) { const float sw = red[1][w][lane]; if (sw != 0.f) L += sw * expf(red[0][w][lane] - M); }
                mx = M; inv = 1.f / L;
            }
        }
    }
}

__global__ __launch_bounds__(256) void sag_finish_kernel(const float* __restrict__ partial, int T, int heads, float* __restrict__ s_out,
                                                         unsigned char* __restrict__ m_out) {
    const int s = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= T) return;
    const float* p = partial + (size_t)s * heads * T + j;
    float acc = 0.f;
    for (int h = 0; h < heads; ++h) acc += p[(size_t)h * T];
    const float v = acc / (float)heads;
    s_out[(size_t)s * T + j] = v;
    m_out[(size_t)s * T + j] = v > 1.0f ? 1 : 0;
}

// the 1-D taps exp(-k^2 / 2), k = -4 .. 4, normalised to sum 1 in float64 on the host and held in fp32; the 2-D kernel is their outer product
struct SagTaps { float w[9]; };

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ __launch_bounds__(256) void sag_degrade_kernel(const float* __restrict__ latents, const h16* __restrict__ eps, int ld_eps,
                                                          const unsigned char* __restrict__ mask, int B, int h, int w, int hm, int wm,
                                                          const float* __restrict__ tab, const int* __restrict__ step_idx,
                                                          const h16* __restrict__ src_rows, h16* __restrict__ dst_rows, int ld_in,
                                                          int copy_end, const SagTaps taps) {
    const int hw = h * w;
    const int idx = blockIdx.x * 256 + threadIdx.x;      // (b, pixel)
    if (idx >= B * hw) return;
    const int b = idx / hw, p = idx - b * hw, y = p / w, x = p - y * w;
    const float* tr = tab + 4 * (size_t)(step_idx ? *step_idx : 0);
    const float sa = tr[0], s1 = tr[1], in_scale = tr[2];
    const float* wt = taps.w;
    const float* lb = latents + (size_t)b * hw * 4;
    const h16* eb = eps + (size_t)b * hw * ld_eps;
    auto x0_at = [&](int pp, float bb[4], float o[4]) {
        const float4 xv = *reinterpret_cast<const float4*>(lb + (size_t)pp * 4);
        const h16x4 ev = *reinterpret_cast<const h16x4*>(eb + (size_t)pp * ld_eps);
#pragma unroll
        for (int c = 0; c < 4; ++c) bb[c] = (float)ev[c];
        o[0] = (xv.x - s1 * bb[0]) / sa; o[1] = (xv.y - s1 * bb[1]) / sa;
        o[2] = (xv.z - s1 * bb[2]) / sa; o[3] = (xv.w - s1 * bb[3]) / sa;
    };
    float bc[4], x0[4];
    x0_at(p, bc, x0);
    // F.interpolate(mode="nearest"): source index = min(int(floor(dst * float(in) / float(out))), in - 1)
    const float sy = (float)hm / (float)h, sx = (float)wm / (float)w;
    int my = (int)floorf((float)y * sy), mxi = (int)floorf((float)x * sx);
    my = my < hm - 1 ? my : hm - 1; mxi = mxi < wm - 1 ? mxi : wm - 1;
    float xd[4];
    if (mask[(size_t)b * hm * wm + my * wm + mxi]) {
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ky = 0; ky < 9; ++ky) {
            const int yy = reflect_idx(y + ky - 4, h);
            float row[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kx = 0; kx < 9; ++kx) {
                const int xx = reflect_idx(x + kx - 4, w);
                float bt[4], t0[4];
                x0_at(yy * w + xx, bt, t0);
#pragma unroll
                for (int c = 0; c < 4; ++c) row[c] = fmaf(wt[kx], t0[c], row[c]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) g[c] = fmaf(wt[ky], row[c], g[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) xd[c] = sa * g[c] + s1 * bc[c];
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) xd[c] = sa * x0[c] + s1 * bc[c];
    }
    h16x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (h16)(xd[c] * in_scale);
    h16* drow = dst_rows + (size_t)idx * ld_in;
    *reinterpret_cast<h16x4*>(drow) = o;
    if (src_rows && src_rows != dst_rows) {
        const h16* srow = src_rows + (size_t)idx * ld_in;
        for (int c = 4; c < copy_end; c += 4) *reinterpret_cast<h16x4*>(drow + c) = *reinterpret_cast<const h16x4*>(srow + c);
    }
}

}  // namespace

long long ladi_sag_partial_floats(int n, int T, int heads) { return (long long)n * T * heads; }

int ladi_launch_sag_map(const h16* q, int ldq, long long sq, const h16* k, int ldk, long long sk, int n, int T, int heads, float* partial,
                        float* s_out, unsigned char* m_out, hipStream_t st) {
    if (!q || !k || !partial || !s_out || !m_out || n < 1 || T < 1 || heads < 1) return -1;
    if (ldq < heads * 64 || ldk < heads * 64 || (ldq & 7) || (ldk & 7) || (sq & 7) || (sk & 7) || ((uintptr_t)q & 15) || ((uintptr_t)k & 15)) return -3;
    if ((long long)n * heads > 0x7fffffffLL || n > 65535) return -1;
    hipLaunchKernelGGL(sag_colsum_kernel, dim3((unsigned)(n * heads)), dim3(256), 0, st, q, ldq, sq, k, ldk, sk, T, heads, partial);
    hipLaunchKernelGGL(sag_finish_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)n), dim3(256), 0, st, partial, T, heads, s_out, m_out);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}

int ladi_launch_sag_degrade(const float* latents, const h16* eps, int ld_eps, const unsigned char* mask, int B, int h, int w, int hm, int wm,
                            const float* tab, const int* step_idx, const h16* src_rows, h16* dst_rows, int ld_in, int copy_end, hipStream_t st) {
    if (!latents || !eps || !mask || !tab || !dst_rows || B < 1 || hm < 1 || wm < 1) return -1;
    if (h < 5 || w < 5) return -2;                       // 4-pixel reflect padding needs 5 pixels
    if (ld_eps < 4 || (ld_eps & 3) || ld_in < 4 || (ld_in & 3) || copy_end > ld_in || (copy_end & 3) || ((uintptr_t)latents & 15) ||
        ((uintptr_t)eps & 7) || ((uintptr_t)dst_rows & 7) || ((uintptr_t)src_rows & 7)) return -3;
    const long long total = (long long)B * h * w;
    if (total > 0x7fffffffLL - 256) return -1;
    SagTaps taps;
    double e[9], sum = 0.0;
    for (int i = 0; i < 9; ++i) { e[i] = std::exp(-0.5 * (double)((i - 4) * (i - 4))); sum += e[i]; }
    for (int i = 0; i < 9; ++i) taps.w[i] = (float)(e[i] / sum);
    hipLaunchKernelGGL(sag_degrade_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, latents, eps, ld_eps, mask, B, h, w, hm, wm,
                       tab, step_idx, src_rows, dst_rows, ld_in, copy_end, taps);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}
