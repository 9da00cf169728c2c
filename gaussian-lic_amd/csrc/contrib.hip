// contrib.hip — per-Gaussian contribution statistics from the lists of a completed forward (gslic_contribution_accumulate; no reference
// counterpart: the blend weight w = alpha T of a (pixel, Gaussian) pair only exists inside the blend loop).
//
// contribution_kernel: ONE WORKGROUP OF FOUR WAVES PER 16x16 TILE, thread i owns element i of the tile-major per-pixel arrays (tile_pix_x /
//   tile_pix_y: wave = 8x8 quadrant), i.e. it reads its n_contrib from pix_final[tile * 256 + i] with one coalesced load.  The tile's list is
//   walked front to back in batches of 64 entries (one record per lane of wave 0, parked in LDS, read back at a wave-uniform address); the
//   walk ends at the tile's largest n_contrib, a wave's at its quadrant's.  A pixel REPLAYS the forward's strict arithmetic (absolute pixel
//   coordinates, the products of the power rounded one by one, expf_core, min(0.99, opacity exp(power)), T (1 - alpha)) for the entries in
//   front of its n_contrib and skips power > 0 / alpha < 1/255 as the forward did: between two skipped entries nothing of the forward's
//   state is needed, and the stop at T < 1e-4 is what n_contrib records.  There is no fast-math variant (header: gslic_hip.h).
//   Per entry the wave reduces {sum w, max w, #(w >= w_min)} over its 64 pixels (butterfly: a fixed order), lane j keeps entry j's three values
//   in registers; entries no pixel of the wave blends cost the replay only.  Per batch the four waves' partials meet in LDS and wave 0 adds
//   them in wave order, so a tile's partial sum is one float formed in a fixed order; it is converted ONCE to 32.32 fixed point
//   (round to nearest) and leaves as one 64-bit integer atomic — at most one global atomic per statistic per (tile, entry), none for an entry
//   the tile does not blend.  Integer max / add / saturating add commute: the accumulators do not depend on the order in which tiles finish.
// contribution_error_kernel (gslic_contribution_accumulate_error): the same body (contrib_body.inc, CONTRIB_ERR = 1) which also reduces w e(p),
//   e = the caller's per-pixel error image clamped to [0, 4], into a fourth accumulator by the same route.
// contribution_free_space_kernel (gslic_contribution_accumulate_free_space): the same body (CONTRIB_FREE = 1) which also reduces w over the pixels
//   with a measured near bound, and over those of them the entry lies in front of (z_g < near_bound[p]), into two more accumulators by that route.
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

__device__ __forceinline__ float wave_sum_butterfly(float v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);   // (a + b == b + a: every lane ends with the same bits)
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// n_pix[g] = min(2^32 - 1, n_pix[g] + c): below 2^31 a plain add cannot wrap (one launch adds less than 2^31 in total: the host checks
// 256 T < 2^31, and launches on one set of accumulators are ordered by their stream), above it a compare-and-swap loop saturates.  Both are
// the same function of the multiset of addends, whatever their order.
__device__ __forceinline__ void saturating_add_u32(uint32_t* p, uint32_t c)
{
    uint32_t cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur < 0x80000000u) { atomicAdd(p, c); return; }
    while (true) {
        const uint32_t want = cur > 0xffffffffu - c ? 0xffffffffu : cur + c;
        if (want == cur) return;
        const uint32_t seen = atomicCAS(p, cur, want);
        if (seen == cur) return;
        cur = seen;
    }
}

// e(p) of gslic_contribution_accumulate_error: err[p] clamped to [0, 4]; a negative value or a NaN reads as 0, +inf as 4
__device__ __forceinline__ float error_value(float e)
{
    return __builtin_amdgcn_fmed3f(e == e ? e : 0.0f, 0.0f, 4.0f);
}

__global__ __launch_bounds__(256) void contribution_kernel(ContribArgs a)
{
#define CONTRIB_ERR 0
#define CONTRIB_FREE 0
#include "contrib_body.inc"
#undef CONTRIB_FREE
#undef CONTRIB_ERR
}

__global__ __launch_bounds__(256) void contribution_error_kernel(ContribArgs a, const float* __restrict__ err, unsigned long long* __restrict__ err_sum)
{
#define CONTRIB_ERR 1
#define CONTRIB_FREE 0
#include "contrib_body.inc"
#undef CONTRIB_FREE
#undef CONTRIB_ERR
}

__global__ __launch_bounds__(256) void contribution_free_space_kernel(ContribArgs a, const float* __restrict__ near_bound,
                                                                      unsigned long long* __restrict__ free_sum, unsigned long long* __restrict__ meas_sum)
{
#define CONTRIB_ERR 0
#define CONTRIB_FREE 1
#include "contrib_body.inc"
#undef CONTRIB_FREE
#undef CONTRIB_ERR
}

int launch_contribution(const ContribArgs& a, hipStream_t s, const float* err, unsigned long long* err_sum, const float* near_bound,
                        unsigned long long* free_sum, unsigned long long* meas_sum)
{
    if (a.T <= 0) return GSLIC_OK;
    if ((uint64_t)a.T * GS_TILE_PIX >= 0x80000000ull) return set_error(GSLIC_ERR_INVALID_ARG, "contribution: %d tiles are more than one launch counts", a.T);
    if (free_sum) hipLaunchKernelGGL(contribution_free_space_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a, near_bound, free_sum, meas_sum);
    else if (err_sum) hipLaunchKernelGGL(contribution_error_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a, err, err_sum);
    else hipLaunchKernelGGL(contribution_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a);
    GS_HIP(hipGetLastError());
    return GSLIC_OK;
}

}  // namespace gslic
