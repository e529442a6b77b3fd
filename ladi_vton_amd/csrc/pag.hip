// Perturbed-attention guidance (diffusers PAGMixin, PAGIdentitySelfAttnProcessor2_0 / PAGCFGIdentitySelfAttnProcessor2_0): in a selected
// transformer block the self-attention map of a perturbed sample is the identity, so the attention output is the value projection itself,
//   O[row, 0:C] = V[row, 0:C]
// with V the last third of the fused QKV projection (row stride 3C) and O the buffer attn1.to_out reads.  One 16-byte vector per thread;
// a pure copy, so two launches are bit-equal.
#include "common.h"
#include "kernels.h"
#include <cstdint>

namespace {

__global__ __launch_bounds__(256) void pag_identity_kernel(const h16* __restrict__ v, int ldv, h16* __restrict__ o, int ldo, long long rows,
                                                           int cv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;      // (row, channel vector)
    if (i >= rows * cv) return;
    const long long row = i / cv;
    const int c = (int)(i - row * cv) * 8;
    *reinterpret_cast<uint4*>(o + row * ldo + c) = *reinterpret_cast<const uint4*>(v + row * ldv + c);
}

}  // namespace

int ladi_launch_pag_identity(const h16* v, int ldv, h16* o, int ldo, long long rows, int C, hipStream_t st) {
    if (!v || !o || rows < 1) return -1;
    if (C < 8 || (C & 7)) return -2;
    if (ldv < C || ldo < C || (ldv & 7) || (ldo & 7) || ((uintptr_t)v & 15) || ((uintptr_t)o & 15)) return -3;
    const long long vecs = rows * (C / 8);
    if ((vecs + 255) / 256 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(pag_identity_kernel, dim3((unsigned)((vecs + 255) / 256)), dim3(256), 0, st, v, ldv, o, ldo, rows, C / 8);
    return hipGetLastError() == hipSuccess ? 0 : -11;
}
