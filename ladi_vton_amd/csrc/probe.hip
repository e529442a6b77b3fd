// fp16 range probe: largest finite |x| and the number of inf / NaN elements of an NHWC fp16 view, accumulated into one slot
// {uint32 absmax_bits; uint32 nonfinite} with device atomics (runtime.h Probe).  The kernel only reads: a pure HBM stream, so it runs
// 16-byte loads (8 halves per lane, 1 KiB per wave instruction) with four of them in flight per lane, at full occupancy (no LDS beyond
// the words of the cross-wave reduction, a handful of VGPRs), on a grid-stride grid of at most 2 workgroups of 1024 per CU: the same 32
// waves per CU as small workgroups would give, but a quarter of the workgroups, and every workgroup ends in atomics on the SAME two
// words, which the L2 serialises, so the fewer workgroups the shorter that tail.  That is reasoning, not a committed measurement:
// tools/range_probe_ab.py times this kernel on the largest tensor of the 64 x 48 forward.
// The value is never computed on: each half is widened to fp32 (exact) and compared, so the result is the exact maximum.
#include "kernels.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kUnroll = 4;
constexpr int kBlocksPerCU = 2;

struct Acc { float m; unsigned cnt; };

__device__ __forceinline__ void take(Acc& a, h16 x) {
    const float v = fabsf((float)x);
    const bool fin = v <= 65504.f;            // false for inf and NaN
    a.m = fin ? fmaxf(a.m, v) : a.m;
    a.cnt += fin ? 0u : 1u;
}
__device__ __forceinline__ void take8(Acc& a, const h16x8& v) {
#pragma unroll
    for (int e = 0; e < 8; ++e) take(a, v[e]);
}

// VEC: C % 8 == 0, ld % 8 == 0, p 16-byte aligned -> work items are 8-half vectors of the C valid lanes of each row (cv = C / 8 per row);
// else one half per work item.  dense (ld == C): the view is one contiguous run, no row / column split.
template <bool VEC>
__device__ __forceinline__ long long item_offset(long long i, int per_row, int ld, bool dense) {
    if (dense) return VEC ? i * 8 : i;
    const long long r = i / per_row;
    const int col = (int)(i - r * per_row);
    return r * ld + (VEC ? col * 8 : col);
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void absmax_probe_kernel(const h16* __restrict__ p, long long items, int per_row, int ld, int dense,
                                                                 unsigned* __restrict__ amax_bits, unsigned* __restrict__ nonfinite,
                                                                 unsigned* __restrict__ seq, unsigned* __restrict__ first_rank) {
    Acc a{0.f, 0u};
    const long long stride = (long long)gridDim.x * kThreads;
    long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    // whole batches: kUnroll independent loads issued before the first use (no per-load condition inside the batch)
    for (; i + (kUnroll - 1) * stride < items; i += kUnroll * stride) {
        if constexpr (VEC) {
            h16x8 v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) v[u] = *reinterpret_cast<const h16x8*>(p + item_offset<true>(i + u * stride, per_row, ld, dense));
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) take8(a, v[u]);
        } else {
            h16 v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) v[u] = p[item_offset<false>(i + u * stride, per_row, ld, dense)];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) take(a, v[u]);
        }
    }
    for (; i < items; i += stride) {
        if constexpr (VEC) take8(a, *reinterpret_cast<const h16x8*>(p + item_offset<true>(i, per_row, ld, dense)));
        else take(a, p[item_offset<false>(i, per_row, ld, dense)]);
    }
    // wave, then across the waves of the workgroup through LDS; one atomic pair per workgroup
    a.m = wave_max(a.m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a.cnt += __shfl_xor(a.cnt, o);
    __shared__ float s_m[kThreads / LADI_WAVE];
    __shared__ unsigned s_c[kThreads / LADI_WAVE];
    const int wave = threadIdx.x / LADI_WAVE, lane = threadIdx.x % LADI_WAVE;
    if (lane == 0) { s_m[wave] = a.m; s_c[wave] = a.cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = s_m[0]; unsigned c = s_c[0];
#pragma unroll
        for (int w = 1; w < kThreads / LADI_WAVE; ++w) { m = fmaxf(m, s_m[w]); c += s_c[w]; }
        atomicMax(amax_bits, __float_as_uint(m));     // m >= 0: the bit pattern of a non-negative float orders like the value
        if (c > 0) {                                  // (adding zero would change nothing)
            const unsigned before = atomicAdd(nonfinite, c);
            // the one workgroup that takes the count from zero also takes the next rank of the probe's "went non-finite" sequence: ranks
            // order the slots by the time their first inf / NaN was seen (launches of one stream run in order)
            if (first_rank && before == 0) *first_rank = atomicAdd(seq, 1u) + 1u;
        }
    }
}

int cu_count() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int& n = cus[dev & 63];
    if (n <= 0 && (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)) n = 256;
    return n;
}

}  // namespace

int ladi_launch_absmax_probe(const h16* p, long long rows, int C, int ld, unsigned* absmax_bits, unsigned* nonfinite, hipStream_t st,
                             unsigned* seq, unsigned* first_rank) {
    if (!p || !absmax_bits || !nonfinite || rows < 0 || C < 1 || ld < C || (!seq != !first_rank)) return -1;
    if (rows == 0) return 0;
    const bool vec = (C % 8 == 0) && (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0);
    const int per_row = vec ? C / 8 : C;
    const long long items = rows * per_row;
    const long long want = (items + (long long)kThreads * kUnroll - 1) / ((long long)kThreads * kUnroll);
    const long long cap = (long long)cu_count() * kBlocksPerCU;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : want > cap ? cap : want);
    const int dense = ld == C ? 1 : 0;
    if (vec) hipLaunchKernelGGL(absmax_probe_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, p, items, per_row, ld, dense, absmax_bits, nonfinite, seq, first_rank);
    else hipLaunchKernelGGL(absmax_probe_kernel<false>, dim3(blocks), dim3(kThreads), 0, st, p, items, per_row, ld, dense, absmax_bits, nonfinite, seq, first_rank);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
