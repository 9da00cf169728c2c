// preprocess_bwd_gstat.hip — the gradient-statistics variants of the fused per-Gaussian backward (preprocess_bwd_gstat_kernel,
// preprocess_bwd_defer_xyz_gstat_kernel) and the stand-alone gradient_stats_kernel, with their launchers.  A translation unit of its own: with
// these kernels in preprocess_bwd.hip's module the compiler scheduled one of the existing instantiations differently, and those stay instruction
// for instruction what they were (tools/kernel_disasm_diff.py).  Both units include the same device code, preprocess_bwd_device.inc.
#include "gslic_common.h"
#include "kernels.h"
#include <stdlib.h>

namespace gslic {

// This unit's copies of the two SH tables need names of their own (one external symbol cannot be defined twice).  They stay externally visible: a
// table the compiler can see through (static) is folded into the chain, which then contracts differently — and the statistics variants must round
// exactly as the kernels they copy do (tests/test_gradstats_gpu.py holds parameters and moments to the plain step's bits).
#define b_SH_C2 b_SH_C2_gstat
#define b_SH_C3 b_SH_C3_gstat
#include "preprocess_bwd_device.inc"

// gslic_rasterize_backward_adam_stats / _depth_adam_stats: the two fused-Adam kernels above with the statistics rule applied to every visible row
// right behind the gather, from the sums the thread holds (GSTAT).  Kernels of their own: the instantiations above stay what they were.
template <bool LDS_SH, int BS>
__global__ __launch_bounds__(BS) GS_PBWD_OCC void preprocess_bwd_gstat_kernel(PreprocessBwdArgs a, GradStatArgs gs)
{
    constexpr bool CAM = false;
    constexpr bool DEFER_XYZ = false;
    constexpr bool GSTAT = true;
#include "preprocess_bwd_body.inc"
}
template <bool LDS_SH, int BS>
__global__ __launch_bounds__(BS) GS_PBWD_OCC void preprocess_bwd_defer_xyz_gstat_kernel(PreprocessBwdArgs a, GradStatArgs gs)
{
    constexpr bool CAM = false;
    constexpr bool DEFER_XYZ = true;
    constexpr bool GSTAT = true;
#include "preprocess_bwd_body.inc"
}
// The same rule for a host that holds dL_dmean2D [P,3] and radii (gslic_gradient_stats_accumulate): one thread per row of [row_begin, row_end).
__global__ __launch_bounds__(256) void gradient_stats_kernel(int row_begin, int row_end, const float* __restrict__ dL_dmean2D,
                                                             const int32_t* __restrict__ radii, GradStatArgs gs)
{
    const int idx = row_begin + (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= row_end) return;
    const int32_t r = radii[idx];
    if (r <= 0) return;
    grad_stat_update(gs, idx, dL_dmean2D[3 * (size_t)idx], dL_dmean2D[3 * (size_t)idx + 1], r);
}

// the chain kernel of launch_preprocess_bwd when statistics are asked for: lds_sh / defer as that function chose them
int launch_preprocess_bwd_gstat(const PreprocessBwdArgs& a, const GradStatArgs& gs, bool lds_sh, bool defer, hipStream_t s)
{
    const int nrows = a.row_end - a.row_begin;
    if (lds_sh) {
        if (defer) GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_defer_xyz_gstat_kernel<true, 64>), dim3(div_up(nrows, 64)), dim3(64), 0, s, a, gs);
        else GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_gstat_kernel<true, 64>), dim3(div_up(nrows, 64)), dim3(64), 0, s, a, gs);
    } else {
        if (defer) GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_defer_xyz_gstat_kernel<false, 256>), dim3(div_up(nrows, 256)), dim3(256), 0, s, a, gs);
        else GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_gstat_kernel<false, 256>), dim3(div_up(nrows, 256)), dim3(256), 0, s, a, gs);
    }
    return GSLIC_OK;
}

int launch_gradient_stats(int row_begin, int row_end, const float* dL_dmean2D, const int32_t* radii, const GradStatArgs& gs, hipStream_t s)
{
    const int nrows = row_end - row_begin;
    if (nrows <= 0) return GSLIC_OK;
    GS_LAUNCH(K_PREPROCESS_BWD, gradient_stats_kernel, dim3(div_up(nrows, 256)), dim3(256), 0, s, row_begin, row_end, dL_dmean2D, radii, gs);
    return GSLIC_OK;
}

}  // namespace gslic
