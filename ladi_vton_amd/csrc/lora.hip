// LoRA merge onto a packed weight that already sits on the device (DESIGN.md "LoRA"):
//   W[row_map(o)][t][i] = fp16( float(base[row_map(o)][t][i]) + sum_a scale_a * ( sum_r up_a[o][r] * down_a[r][t][i] ) ),   i < cin
// base / W: fp16 in the igemm layout [rows of the whole weight][taps][cin_pad] (row pitch `pitch` halves); base is the pristine copy, W the
// live weight.  up_a fp32 [rows][r_a], down_a fp32 [r_a][taps][cin] (tap-major).  One launch serves one block of `rows` destination rows:
// row_map(o) = row0 + o, or the GEGLU interleave of load_geglu (source row j < half -> 64 (j / 32) + j % 32, half + j -> the same + 32).
//
// A workgroup of 256 threads owns 64 source rows x 64 columns of one tap (cin_pad is a multiple of 64, so a column tile never straddles two
// taps); a thread owns 2 rows x 8 columns: one 16-byte vector of each row.  Per adapter the rank is walked in chunks of 32: the up tile
// [64][32] and the down tile [32][64] are staged through LDS, the inner sum runs over ascending r as an fp32 fmaf chain in registers, then
// delta = fmaf(scale_a, inner_a, delta) in call order, one add onto the base, one rounding.  Nothing depends on the launch geometry or on
// timing: two launches with the same operands are bit-equal.  A delta of exactly zero keeps the base's bits (zero adapters -- the restore
// path --, scale 0), so a restore is a copy whatever the base holds.  Columns [cin, cin_pad) of a tap and rows outside the block are never
// written.  The results that are not finite after rounding are counted into *nonfinite (one atomicAdd per workgroup that saw any).
#include "common.h"
#include "kernels.h"
#include <cstdint>

namespace {

constexpr int TM = 64, TN = 64, RK = 32;

__device__ __forceinline__ int lora_row(int o, int row0, int geglu_half) {
    if (!geglu_half) return row0 + o;
    const int j = o < geglu_half ? o : o - geglu_half;
    return row0 + 64 * (j >> 5) + (j & 31) + (o < geglu_half ? 0 : 32);
}

__global__ __launch_bounds__(256) void lora_merge_kernel(LoraMergeArgs a) {
    __shared__ float up_s[TM][RK + 1];          // + 1: the 8 rows a wave reads at one r fall on 8 banks
    __shared__ __attribute__((aligned(16))) float dn_s[RK][TN];
    __shared__ unsigned bad_s;
    const int tid = threadIdx.x;
    const int tx = tid & 7, ty = tid >> 3;      // 8 column vectors x 32 row pairs
    const int col0 = blockIdx.x * TN;           // column of the packed row: tap * cin_pad + channel
    const int tap = col0 / a.cin_pad, ch0 = col0 - tap * a.cin_pad;
    const int o0 = blockIdx.y * TM;
    if (ch0 >= a.cin) return;                   // a tile of padding columns only (uniform over the workgroup)
    if (tid == 0) bad_s = 0;
    __syncthreads();

    float delta[2][8];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) delta[m][j] = 0.f;

    for (int ad = 0; ad < a.n_adapters; ++ad) {
        const float* __restrict__ up = a.up[ad];
        const float* __restrict__ dn = a.down[ad];
        const int rank = a.rank[ad];
        const long long dn_pitch = (long long)a.taps * a.cin;
        float inner[2][8];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 8; ++j) inner[m][j] = 0.f;
        for (int r0 = 0; r0 < rank; r0 += RK) {
            const int rc = min(RK, rank - r0);
            __syncthreads();                    // the previous chunk's readers are done
#pragma unroll
            for (int k = 0; k < TM * RK / 256; ++k) {
                const int e = tid + k * 256, row = e >> 5, rr = e & 31;
                const int o = o0 + row;
                up_s[row][rr] = (o < a.rows && rr < rc) ? up[(long long)o * rank + r0 + rr] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < RK * TN / 256; ++k) {
                const int e = tid + k * 256, rr = e >> 6, c = e & 63;
                const int ch = ch0 + c;
                dn_s[rr][c] = (rr < rc && ch < a.cin) ? dn[(long long)(r0 + rr) * dn_pitch + (long long)tap * a.cin + ch] : 0.f;
            }
            __syncthreads();
            for (int rr = 0; rr < rc; ++rr) {
                const float u0 = up_s[ty][rr], u1 = up_s[ty + 32][rr];
                const f32x4 d0 = *reinterpret_cast<const f32x4*>(&dn_s[rr][tx * 8]);
                const f32x4 d1 = *reinterpret_cast<const f32x4*>(&dn_s[rr][tx * 8 + 4]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    inner[0][j] = fmaf(u0, d0[j], inner[0][j]);
                    inner[0][j + 4] = fmaf(u0, d1[j], inner[0][j + 4]);
                    inner[1][j] = fmaf(u1, d0[j], inner[1][j]);
                    inner[1][j + 4] = fmaf(u1, d1[j], inner[1][j + 4]);
                }
            }
        }
        const float sc = a.scale[ad];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 8; ++j) delta[m][j] = fmaf(sc, inner[m][j], delta[m][j]);
    }

    unsigned bad = 0;
    const int ch = ch0 + tx * 8;                // first channel of this thread's vector
    if (ch < a.cin) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int o = o0 + ty + 32 * m;
            if (o >= a.rows) continue;
            const long long off = (long long)lora_row(o, a.row0, a.geglu_half) * a.pitch + col0 + tx * 8;
            const h16x8 b = *reinterpret_cast<const h16x8*>(a.base + off);
            h16x8 w = b;
            if (ch + 8 > a.cin) w = *reinterpret_cast<const h16x8*>(a.W + off);     // the vector reaches into the padding: those halves keep W's bits
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (ch + j >= a.cin) continue;
                const float d = delta[m][j];
                h16 v = b[j];
                if (d != 0.f) {
                    v = (h16)((float)b[j] + d);
                    const float f = (float)v;
                    if (!(fabsf(f) <= 65504.f)) ++bad;
                }
                w[j] = v;
            }
            *reinterpret_cast<h16x8*>(a.W + off) = w;
        }
    }
    if (a.nonfinite) {
        if (bad) atomicAdd(&bad_s, bad);
        __syncthreads();
        if (tid == 0 && bad_s) atomicAdd(a.nonfinite, bad_s);
    }
}

}  // namespace

int ladi_launch_lora_merge(const LoraMergeArgs& a, hipStream_t st) {
    if (!a.base || !a.W || a.base == a.W) return -1;
    if (a.rows < 1 || a.row0 < 0 || a.cin < 1 || a.taps < 1 || a.cin_pad < a.cin || (a.cin_pad & 63)) return -2;
    if (a.pitch < (long long)a.taps * a.cin_pad || (a.pitch & 7) || ((uintptr_t)a.base & 15) || ((uintptr_t)a.W & 15)) return -3;
    if (a.geglu_half && (a.geglu_half < 32 || (a.geglu_half & 31) || a.rows != 2 * a.geglu_half || (a.row0 & 63))) return -4;
    if (a.n_adapters < 0 || a.n_adapters > LORA_MAX_ADAPTERS) return -5;
    for (int i = 0; i < a.n_adapters; ++i) {
        if (!a.up[i] || !a.down[i] || a.rank[i] < 1 || a.rank[i] > LORA_MAX_RANK) return -6;
        if (((uintptr_t)a.up[i] & 3) || ((uintptr_t)a.down[i] & 3)) return -6;
    }
    const long long cols = (long long)a.taps * a.cin_pad;
    const long long gy = ((long long)a.rows + TM - 1) / TM;
    if (cols / TN > 0x7fffffffLL || gy > 65535) return -7;
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)(cols / TN), (unsigned)gy), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}
