// preprocess_bwd_cam_adam.hip — the camera gradient together with the fused Adam update (gslic_rasterize_backward_camera_adam /
// _depth_camera_adam): the depth variant's chain kernel (CAM and DEFER_XYZ), the tail kernel behind it, and the reduction of the partial rows that
// honours the forward's overflow word, with their launchers.  A translation unit of its own, as preprocess_bwd_gstat.hip is and for its reason: the
// instantiations of preprocess_bwd.hip stay instruction for instruction what they were (tools/kernel_disasm_diff.py).  The colour-only variant
// needs no chain kernel here: preprocess_bwd_kernel<.., CAM = true> reads a.adam at run time.
#include "gslic_common.h"
#include "kernels.h"
#include <stdlib.h>

namespace gslic {

// (the tables' names and their visibility: the note in preprocess_bwd_gstat.hip — the chain must contract as preprocess_bwd.hip's does)
#define b_SH_C2 b_SH_C2_cam_adam
#define b_SH_C3 b_SH_C3_cam_adam
#include "preprocess_bwd_device.inc"

// preprocess_bwd_kernel<.., CAM = true> with xyz's Adam update deferred, as preprocess_bwd_defer_xyz_kernel defers it: the 27 camera sums are
// formed in bwd_rest from the parameters as they were, every group but xyz is updated by the sinks, xyz's chain gradient goes to dL_dmean3D.
template <bool LDS_SH, int BS>
__global__ __launch_bounds__(BS) GS_PBWD_OCC void preprocess_bwd_cam_defer_xyz_kernel(PreprocessBwdArgs a)
{
    constexpr bool CAM = true;
    constexpr bool DEFER_XYZ = true;
    constexpr bool GSTAT = false;
    constexpr GradStatArgs gs{};   // (never read: every use sits under if constexpr (GSTAT))
#include "preprocess_bwd_body.inc"
}

// depth_mean3d_cam_kernel (preprocess_bwd.hip) with xyz's Adam update: the same gather, the same dL_dmean3D update and the same four products in
// slots 27..30 of the wave's partial row through the same xor-shuffle tree — and then adam_scalar on xyz from the complete gradient
// (depth_mean3d_row<true>).  The means are read through the Adam descriptor's own pointer (A.p[0] is means3D: api.hip checks it) and BEFORE the
// row's update: the sums are those of the parameters as they were.  No thread reads another thread's row.
__global__ __launch_bounds__(256) void depth_mean3d_cam_adam_kernel(int row_begin, int row_end, const int32_t* __restrict__ radii,
                                                                    const uint32_t* __restrict__ gauss_start, const uint32_t* __restrict__ tiles_touched,
                                                                    const uint8_t* __restrict__ dead, const float* __restrict__ partials_z,
                                                                    const float* __restrict__ V, const uint32_t* __restrict__ status,
                                                                    float* __restrict__ dL_dmean3D, float* __restrict__ cam_partials, AdamFusedArgs A)
{
#pragma clang fp contract(off)   // the four products are rounded on their own, as depth_mean3d_cam_kernel rounds them
    if (status[2] != 0u) return;   // capacity overflow in the forward: no row is written, cam_reduce_depth_kernel sums none, no Adam
    const int idx = row_begin + (int)(blockIdx.x * 256u + threadIdx.x);
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (idx < row_end && radii[idx] > 0) {
        const float x = A.p[0][3 * idx], y = A.p[0][3 * idx + 1], z = A.p[0][3 * idx + 2];
        const float dz = depth_mean3d_row<true>(idx, gauss_start, tiles_touched, dead, partials_z, V, dL_dmean3D, A);
        c[0] = dz * x; c[1] = dz * y; c[2] = dz * z; c[3] = dz;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float v = c[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        c[k] = v;
    }
    if ((threadIdx.x & 63) == 0) {
        float* row = cam_partials + 32 * ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6));
#pragma unroll
        for (int k = 0; k < 4; k++) row[27 + k] = c[k];
    }
}

// cam_reduce_kernel (preprocess_bwd.hip) behind a forward that may have overflowed its capacity buffers: the same 27 sums in the same order; after
// an overflow no partial row was written, nothing is summed and the outputs keep the zeros of the launch's memset (as cam_reduce_depth_kernel).
__global__ __launch_bounds__(256) void cam_reduce_checked_kernel(size_t rows, const float* __restrict__ partials, const uint32_t* __restrict__ status,
                                                                 float* __restrict__ out)
{
    __shared__ float red[256];
    if (status[2] != 0u) return;
    const int k = blockIdx.x;
    float s = 0.f;
    for (size_t r = threadIdx.x; r < rows; r += 256) s += partials[32 * r + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int dst;   // as cam_reduce_kernel
        if (k < 12) dst = 4 * (k / 3) + (k % 3);
        else if (k < 24) { const int kk = k - 12; const int r = kk % 3; dst = 16 + 4 * (kk / 3) + (r == 2 ? 3 : r); }
        else dst = 32 + (k - 24);
        out[dst] = red[0];
    }
}

int launch_preprocess_bwd_cam_defer_xyz(const PreprocessBwdArgs& a, bool lds_sh, hipStream_t s)
{
    const int nrows = a.row_end - a.row_begin;
    if (lds_sh) GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_cam_defer_xyz_kernel<true, 64>), dim3(div_up(nrows, 64)), dim3(64), 0, s, a);
    else GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_cam_defer_xyz_kernel<false, 256>), dim3(div_up(nrows, 256)), dim3(256), 0, s, a);
    return GSLIC_OK;
}

int launch_depth_mean3d_cam_adam(const PreprocessBwdArgs& a, hipStream_t s)
{
    const int nrows = a.row_end - a.row_begin;
    GS_LAUNCH(K_PREPROCESS_BWD, depth_mean3d_cam_adam_kernel, dim3(div_up(nrows, 256)), dim3(256), 0, s, a.row_begin, a.row_end, a.radii, a.gauss_start,
              a.tiles_touched, a.dead, a.partials_z, a.view, a.status, a.dL_dmean3D, a.cam_partials, a.adam);
    return GSLIC_OK;
}

int launch_cam_reduce_checked(size_t rows, const PreprocessBwdArgs& a, hipStream_t s)
{
    GS_LAUNCH(K_PREPROCESS_BWD, cam_reduce_checked_kernel, dim3(27), dim3(256), 0, s, rows, (const float*)a.cam_partials, a.status, a.cam_out);
    return GSLIC_OK;
}

}  // namespace gslic
