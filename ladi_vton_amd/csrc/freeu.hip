// FreeU (diffusers UNet2DConditionModel.enable_freeu / apply_freeu): one launch per decoder site of up_blocks.0 / up_blocks.1, before the
// concatenation cat([hidden, skip]).
//   backbone  hidden[:, :C_h / 2] *= b                                      (one fp32 product, one rounding to fp16)
//   skip      fourier_filter(skip, threshold = 1, scale = s): fftn -> fftshift -> the centre 2x2 box times s -> ifftshift -> ifftn -> real
// The box holds the distinct frequencies u in {0, -1 mod H}, v in {0, -1 mod W}, so per (sample, channel) plane the filter is
//   F(u, v)  = sum_{y, x} x[y, x] e^{-2 pi i (u y / H + v x / W)}             at most four complex sums (F(0, 0) is real)
//   lp[y, x] = (1 / HW) Re sum_{(u, v) in box} F(u, v) e^{+2 pi i (u y / H + v x / W)}
//   out      = x + (s - 1) lp
// and needs no FFT.  NHWC: eight lanes hold the eight 16-byte channel vectors of a 64-channel chunk, the 32 lane groups of a workgroup
// stride over the pixels of one sample.  The sums are fp32 and reduced in a fixed order (three lane exchanges inside a wave, then the four
// waves through LDS): no atomics, two launches are bit-equal.  Any H, W >= 1: the plane is read twice from memory, never staged.
#include "common.h"
#include "kernels.h"
#include <algorithm>
#include <cstdint>

namespace {

constexpr int FREEU_NQ = 7;              // real sums per channel: F00 | Re, Im F(-1, 0) | Re, Im F(0, -1) | Re, Im F(-1, -1)
constexpr int FREEU_CH = 64;             // channels per workgroup
constexpr int FREEU_PG = 32;             // pixel groups per workgroup (256 threads / 8 channel vectors)

// e^{+2 pi i k / N}: (cos, sin), exact at the multiples of a quarter turn (N = 1, 2, 4)
__device__ __forceinline__ void twiddle(int k, float inv_n, float& c, float& s) { sincospif(2.f * (float)k * inv_n, &s, &c); }

__global__ __launch_bounds__(256) void freeu_kernel(h16* __restrict__ hidden, int ld_h, int half_v, float b, const h16* src, int ld_s, int C_s,
                                                    float sm1, h16* dst, int ld_d, int n, int H, int W, int chunks, int skip_blocks) {
    const int HW = H * W;
    if ((int)blockIdx.x >= skip_blocks) {
        // ---- backbone: channel vectors [0, half_v) of every pixel
        const size_t total = (size_t)n * HW * half_v;
        const size_t stride = (size_t)(gridDim.x - skip_blocks) * 256;
        for (size_t idx = (size_t)(blockIdx.x - skip_blocks) * 256 + threadIdx.x; idx < total; idx += stride) {
            const size_t p = idx / half_v;
            h16* q = hidden + p * ld_h + (idx - p * half_v) * 8;
            h16x8 v = *reinterpret_cast<const h16x8*>(q);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (h16)((float)v[e] * b);
            *reinterpret_cast<h16x8*>(q) = v;
        }
        return;
    }
    // ---- skip: sample blockIdx.x / chunks, channels [64 chunk, 64 chunk + 64)
    __shared__ float part[4][FREEU_NQ * FREEU_CH];
    __shared__ float red[FREEU_NQ * FREEU_CH];
    const int sample = blockIdx.x / chunks, chunk = blockIdx.x - sample * chunks;
    const int cv = threadIdx.x & 7, pg = threadIdx.x >> 3, wave = threadIdx.x >> 6;
    const int c0 = chunk * FREEU_CH + cv * 8;
    const bool active = c0 < C_s;
    const h16* sp = src + (size_t)sample * HW * ld_s + c0;
    h16* dp = dst + (size_t)sample * HW * ld_d + c0;
    const float inv_h = 1.f / (float)H, inv_w = 1.f / (float)W;
    float acc[FREEU_NQ][8];
#pragma unroll
    for (int q = 0; q < FREEU_NQ; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[q][e] = 0.f;
    if (active) {
        for (int p = pg; p < HW; p += FREEU_PG) {
            const int y = p / W, x = p - y * W;
            float cy, sy, cx, sx;
            twiddle(y, inv_h, cy, sy);
            twiddle(x, inv_w, cx, sx);
            const float cyx = cy * cx - sy * sx, syx = sy * cx + cy * sx;
            const h16x8 v = *reinterpret_cast<const h16x8*>(sp + (size_t)p * ld_s);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (float)v[e];
                acc[0][e] += f;
                acc[1][e] += f * cy;  acc[2][e] += f * sy;
                acc[3][e] += f * cx;  acc[4][e] += f * sx;
                acc[5][e] += f * cyx; acc[6][e] += f * syx;
            }
        }
    }
    // the eight pixel groups of a wave (lanes 8 apart), then the four waves: a fixed order
#pragma unroll
    for (int q = 0; q < FREEU_NQ; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = acc[q][e];
            a += __shfl_xor(a, 8); a += __shfl_xor(a, 16); a += __shfl_xor(a, 32);
            acc[q][e] = a;
        }
    if ((threadIdx.x & 63) < 8) {
#pragma unroll
        for (int q = 0; q < FREEU_NQ; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) part[wave][q * FREEU_CH + cv * 8 + e] = acc[q][e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FREEU_NQ * FREEU_CH; i += 256) red[i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
    __syncthreads();
    if (!active) return;
    // the frequency -1 of an axis of length 1 is the frequency 0 again: it is in the box once
    const float wy = H > 1 ? 1.f : 0.f, wx = W > 1 ? 1.f : 0.f, wyx = wy * wx;
    const float inv_hw = 1.f / (float)HW;
    float F[FREEU_NQ][8];
#pragma unroll
    for (int q = 0; q < FREEU_NQ; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) F[q][e] = red[q * FREEU_CH + cv * 8 + e];
    for (int p = pg; p < HW; p += FREEU_PG) {
        const int y = p / W, x = p - y * W;
        float cy, sy, cx, sx;
        twiddle(y, inv_h, cy, sy);
        twiddle(x, inv_w, cx, sx);
        const float cyx = cy * cx - sy * sx, syx = sy * cx + cy * sx;
        h16x8 v = *reinterpret_cast<const h16x8*>(sp + (size_t)p * ld_s);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            // Re[F(u, v) conj(t)] for the twiddle t = e^{+i ..} the sum was taken with
            float lp = F[0][e];
            lp += wy * (F[1][e] * cy + F[2][e] * sy);
            lp += wx * (F[3][e] * cx + F[4][e] * sx);
            lp += wyx * (F[5][e] * cyx + F[6][e] * syx);
            v[e] = (h16)((float)v[e] + sm1 * (lp * inv_hw));
        }
        *reinterpret_cast<h16x8*>(dp + (size_t)p * ld_d) = v;
    }
}

}  // namespace

int ladi_launch_freeu(h16* hidden, int ld_h, int C_h, float b, const h16* skip, int ld_s, int C_s, float s, h16* skip_out, int ld_d, int n,
                      int H, int W, hipStream_t st) {
    if ((!hidden && !skip) || n < 1 || H < 1 || W < 1) return -1;
    if ((size_t)n * H * W > 0x7fffffffULL / 8 || (size_t)H * W > 0x7fffffffULL / 64) return -1;
    if (hidden && (C_h < 16 || (C_h & 15))) return -2;
    if (skip && (C_s < 8 || (C_s & 7))) return -2;
    if (hidden && (ld_h < C_h || (ld_h & 7) || ((uintptr_t)hidden & 15))) return -3;
    if (skip && (!skip_out || ld_s < C_s || ld_d < C_s || (ld_s & 7) || (ld_d & 7) || ((uintptr_t)skip & 15) || ((uintptr_t)skip_out & 15))) return -3;
    const int chunks = skip ? (C_s + FREEU_CH - 1) / FREEU_CH : 0;
    const size_t skip_blocks = (size_t)n * chunks;
    const int half_v = hidden ? C_h / 16 : 0;
    const size_t back_blocks = std::min<size_t>(((size_t)n * H * W * half_v + 255) / 256, 2048);
    if (skip_blocks + back_blocks > 0x7fffffffULL) return -1;
    hipLaunchKernelGGL(freeu_kernel, dim3((unsigned)(skip_blocks + back_blocks)), dim3(256), 0, st, hidden, ld_h, half_v, b, skip, ld_s, C_s, s - 1.f,
                       skip_out, ld_d, n, H, W, chunks, (int)skip_blocks);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}
