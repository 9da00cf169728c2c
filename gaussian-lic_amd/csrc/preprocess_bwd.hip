// preprocess_bwd.hip — one fused per-Gaussian backward pass.
//
// preprocess_bwd_kernel replaces, in ONE launch and one read of each input,
//   * the nine atomicAdd targets of PerGaussianRenderCUDA (backward.cu:585-596): here a contiguous segmented
//     sum over the Gaussian's emission slots [offsets[g-1], offsets[g]) of the partials render_bwd wrote;
//   * computeCov2DCUDA (backward.cu:138-255);
//   * preprocessCUDA<3> bwd + computeColorFromSH bwd + computeCov3D bwd (backward.cu:27-136,257-377);
//   * the ten torch::zeros() of RasterizeGaussiansBackwardCUDA (rasterize_points.cu:192-201): every output row
//     is written here, zeros for invisible Gaussians, so callers may pass uninitialised memory.
// Sigma_3D is recomputed from scale/rotation instead of being stored by the forward (24 B/Gaussian saved).
#include "gslic_common.h"
#include "kernels.h"
#include <stdlib.h>

namespace gslic {

#include "preprocess_bwd_device.inc"

// rows of per-wave partials -> the 35 outputs, fixed summation order (bit-reproducible).  grid = 27 blocks, one per term.
__global__ __launch_bounds__(256) void cam_reduce_kernel(size_t rows, const float* __restrict__ partials, float* __restrict__ out)
{
    __shared__ float red[256];
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
        // term k -> element: view (k < 12): [4c + r], r = k % 3, c = k / 3; proj (12 <= k < 24): rows 0, 1, 3; campos (k >= 24)
        int dst;
        if (k < 12) dst = 4 * (k / 3) + (k % 3);
        else if (k < 24) { const int kk = k - 12; const int r = kk % 3; dst = 16 + 4 * (kk / 3) + (r == 2 ? 3 : r); }
        else dst = 32 + (k - 24);
        out[dst] = red[0];
    }
}

// Depth backward (gslic_rasterize_backward_depth), behind preprocess_bwd_kernel: dL/dz of every visible Gaussian = the sum of its instances' partials_z
// (render_bwd's tenth per-instance sum), gathered like the nine partials (ascending emission slot, dead instances skipped: exact zeros), then
//   dL_dmean3D += dL/dz (V[2], V[6], V[10])      (z = V[2] x + V[6] y + V[10] z + V[14]: row 2 of the view matrix, element [4c + r]).
// A kernel of its own so that the per-Gaussian chain above stays the colour-only kernel instruction for instruction — the chain's contraction
// choices move with any change to its code (the note above GS_PBWD_STRICT_CHAIN), and a zero depth gradient must leave dL_dmean3D as it is.  The
// depth's share of dL/dopacity needs nothing here: it is inside the opacity partials already (the blend backward's fourth channel).
// ADAM (gslic_rasterize_backward_depth_adam, behind preprocess_bwd_defer_xyz_kernel): dL_dmean3D holds the chain's xyz gradient, the sum is formed by
// the same code and then consumed by the masked Adam update of group 0 (adam_scalar, as gslic_adam_update_groups applies it to visible rows): 12 B
// per Gaussian read and 12 written more than the colour-only fused step, plus the dz gather.
template <bool ADAM>
__global__ __launch_bounds__(256) void depth_mean3d_kernel(int row_begin, int row_end, const int32_t* __restrict__ radii,
                                                           const uint32_t* __restrict__ gauss_start, const uint32_t* __restrict__ tiles_touched,
                                                           const uint8_t* __restrict__ dead, const float* __restrict__ partials_z,
                                                           const float* __restrict__ V, const uint32_t* __restrict__ status, float* __restrict__ dL_dmean3D,
                                                           AdamFusedArgs A)
{
    if (status[2] != 0u) return;   // capacity overflow in the forward: preprocess_bwd_kernel wrote nothing either
    const int idx = row_begin + (int)(blockIdx.x * 256u + threadIdx.x);
    if (idx >= row_end || radii[idx] <= 0) return;   // invisible: the chain wrote exact zeros and there is no instance
    depth_mean3d_row<ADAM>(idx, gauss_start, tiles_touched, dead, partials_z, V, dL_dmean3D, A);
}

// Camera variant (gslic_rasterize_backward_depth_camera, behind preprocess_bwd_kernel<.., CAM = true>).  The depth reaches the camera through the 2D
// quantities — already inside the nine sums the CAM chain consumed — and directly through z = V[2] x + V[6] y + V[10] z + V[14]:
//   dL_dviewmatrix[2, 6, 10, 14] += sum_i dL/dz_i (x_i, y_i, z_i, 1).
// Per Gaussian the same gather and the same dL_dmean3D update as above, plus the four products; invisible lanes and lanes behind the range add
// zeros (every lane of the wave takes part in the xor-shuffle tree, the one of the CAM body), and lane 0 writes the four sums into the free slots
// 27..30 of the wave's 32-float partial row.  Row of a Gaussian = (idx - row_begin) / 64 in both layouts of the chain kernel (one-wave blocks of
// 64; 256-thread blocks x 4 waves), so this 256-thread kernel addresses the chain's rows in either.  No atomics: cam_reduce_depth_kernel adds the rows.
__global__ __launch_bounds__(256) void depth_mean3d_cam_kernel(int row_begin, int row_end, const int32_t* __restrict__ radii,
                                                               const uint32_t* __restrict__ gauss_start, const uint32_t* __restrict__ tiles_touched,
                                                               const uint8_t* __restrict__ dead, const float* __restrict__ partials_z,
                                                               const float* __restrict__ V, const uint32_t* __restrict__ status, const float* __restrict__ means,
                                                               float* __restrict__ dL_dmean3D, float* __restrict__ cam_partials)
{
#pragma clang fp contract(off)   // the four products are rounded on their own: the sums below depend on nothing but their order
    if (status[2] != 0u) return;   // capacity overflow in the forward: no row is written, cam_reduce_depth_kernel sums none
    const int idx = row_begin + (int)(blockIdx.x * 256u + threadIdx.x);
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (idx < row_end && radii[idx] > 0) {
        AdamFusedArgs none;   // (never read: ADAM = false)
        none.on = 0;
        const float dz = depth_mean3d_row<false>(idx, gauss_start, tiles_touched, dead, partials_z, V, dL_dmean3D, none);
        c[0] = dz * means[3 * idx]; c[1] = dz * means[3 * idx + 1]; c[2] = dz * means[3 * idx + 2]; c[3] = dz;
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

// cam_reduce_kernel for the depth camera backward: the same 27 sums in the same order, and for the view terms k = 2, 5, 8, 11 (row 2 of the view
// matrix, columns 0..3) the sum of slot 27 + k / 3 over the same rows in the same order, added last.  After a forward capacity overflow no row was
// written: nothing is summed and the outputs keep the zeros of the launch's memset.
__global__ __launch_bounds__(256) void cam_reduce_depth_kernel(size_t rows, const float* __restrict__ partials, const uint32_t* __restrict__ status,
                                                               float* __restrict__ out)
{
    __shared__ float red[256], redz[256];
    if (status[2] != 0u) return;
    const int k = blockIdx.x;
    const bool direct = k < 12 && (k % 3) == 2;
    const int kz = 27 + k / 3;
    float s = 0.f, sz = 0.f;
    for (size_t r = threadIdx.x; r < rows; r += 256) {
        s += partials[32 * r + k];
        if (direct) sz += partials[32 * r + kz];
    }
    red[threadIdx.x] = s;
    redz[threadIdx.x] = sz;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) {
            red[threadIdx.x] += red[threadIdx.x + d];
            redz[threadIdx.x] += redz[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int dst;   // as cam_reduce_kernel
        if (k < 12) dst = 4 * (k / 3) + (k % 3);
        else if (k < 24) { const int kk = k - 12; const int r = kk % 3; dst = 16 + 4 * (kk / 3) + (r == 2 ? 3 : r); }
        else dst = 32 + (k - 24);
        out[dst] = direct ? red[0] + redz[0] : red[0];
    }
}

int launch_preprocess_bwd(const PreprocessBwdArgs& a, hipStream_t s, const GradStatArgs* gs)
{
    if (gs && (!a.adam.on || a.cam_partials))
        return set_error(GSLIC_ERR_INVALID_ARG, "gradient statistics: the fused Adam backward only, without the camera gradient");
    if (a.partials_z && (a.dL_drgb || !a.dL_dmean3D))
        return set_error(GSLIC_ERR_INVALID_ARG, "depth backward: no dL_drgb output, and dL_dmean3D is required");
    if (a.partials_z && a.cam_partials && a.row_begin != 0)
        return set_error(GSLIC_ERR_INVALID_ARG, "depth camera backward: no row range");
    if (a.cam_partials && a.adam.on && (a.row_begin != 0 || a.row_end != a.P))
        return set_error(GSLIC_ERR_INVALID_ARG, "camera backward with the fused Adam: no row range");
    const bool defer = a.partials_z && a.adam.on;   // depth + fused Adam: xyz is updated by depth_mean3d_kernel<true> once dL/dz is in
    const bool cam = a.cam_partials != nullptr;
    const int nrows = a.row_end - a.row_begin;
    if (nrows <= 0) return GSLIC_OK;
    if (cam) GS_HIP(hipMemsetAsync(a.cam_out, 0, 35 * sizeof(float), s));  // row 3 of the view matrix, row 2 of the projection: untouched terms
    if (a.M == 15 && a.shs && (a.dL_dsh || a.adam.on || a.dL_drgb)) {
        // one wave per workgroup: 64 Gaussians' SH rows (11.25 KiB) + small-group gradients in LDS, the phase barriers are wave-level,
        // and ten workgroups per CU sit in different phases (measured 0.72 ms against 0.75 at 128 and 0.88 at 256 threads)
        if (cam && defer) GS_TRY(launch_preprocess_bwd_cam_defer_xyz(a, true, s));
        else if (cam) GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_kernel<true, 64, true>), dim3(div_up(nrows, 64)), dim3(64), 0, s, a);
        else if (gs) GS_TRY(launch_preprocess_bwd_gstat(a, *gs, true, defer, s));
        else if (defer) GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_defer_xyz_kernel<true, 64>), dim3(div_up(nrows, 64)), dim3(64), 0, s, a);
        else GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_kernel<true, 64, false>), dim3(div_up(nrows, 64)), dim3(64), 0, s, a);
    } else {
        if (cam && defer) GS_TRY(launch_preprocess_bwd_cam_defer_xyz(a, false, s));
        else if (cam) GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_kernel<false, 256, true>), dim3(div_up(nrows, 256)), dim3(256), 0, s, a);
        else if (gs) GS_TRY(launch_preprocess_bwd_gstat(a, *gs, false, defer, s));
        else if (defer) GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_defer_xyz_kernel<false, 256>), dim3(div_up(nrows, 256)), dim3(256), 0, s, a);
        else GS_LAUNCH(K_PREPROCESS_BWD, (preprocess_bwd_kernel<false, 256, false>), dim3(div_up(nrows, 256)), dim3(256), 0, s, a);
    }
    if (defer && cam)
        GS_TRY(launch_depth_mean3d_cam_adam(a, s));   // the four direct view-matrix sums from the means as they were, then xyz's Adam
    else if (defer)
        GS_LAUNCH(K_PREPROCESS_BWD, depth_mean3d_kernel<true>, dim3(div_up(nrows, 256)), dim3(256), 0, s, a.row_begin, a.row_end, a.radii, a.gauss_start,
                  a.tiles_touched, a.dead, a.partials_z, a.view, a.status, a.dL_dmean3D, a.adam);
    else if (a.partials_z && cam)
        GS_LAUNCH(K_PREPROCESS_BWD, depth_mean3d_cam_kernel, dim3(div_up(nrows, 256)), dim3(256), 0, s, a.row_begin, a.row_end, a.radii, a.gauss_start,
                  a.tiles_touched, a.dead, a.partials_z, a.view, a.status, a.means, a.dL_dmean3D, a.cam_partials);
    else if (a.partials_z)
        GS_LAUNCH(K_PREPROCESS_BWD, depth_mean3d_kernel<false>, dim3(div_up(nrows, 256)), dim3(256), 0, s, a.row_begin, a.row_end, a.radii, a.gauss_start,
                  a.tiles_touched, a.dead, a.partials_z, a.view, a.status, a.dL_dmean3D, a.adam);
    if (cam) {
        const size_t rows = (a.M == 15 && a.shs && (a.dL_dsh || a.adam.on || a.dL_drgb)) ? (size_t)div_up(a.P, 64) : (size_t)div_up(a.P, 256) * 4;
        if (a.partials_z) GS_LAUNCH(K_PREPROCESS_BWD, cam_reduce_depth_kernel, dim3(27), dim3(256), 0, s, rows, (const float*)a.cam_partials, a.status, a.cam_out);
        else if (a.adam.on) GS_TRY(launch_cam_reduce_checked(rows, a, s));   // (the fused step runs behind capacity-mode forwards: the overflow word is honoured)
        else GS_LAUNCH(K_PREPROCESS_BWD, cam_reduce_kernel, dim3(27), dim3(256), 0, s, rows, (const float*)a.cam_partials, a.cam_out);
    }
    return GSLIC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The SH backward is linear in the clamp-masked colour gradient: dL_ddc = SH_C0 * dRGB, dL_dsh[k] = c_k(dir) * dRGB (backward.cu:27-136) with
// c_k depending only on the view direction normalize(p - campos).  So the N > 1 exchange does not have to all-reduce the 48 floats of
// dL_ddc / dL_dsh per Gaussian: every rank all-gathers the views' 3-float dRGB and rebuilds the summed rows here — per view the very
// products the backward forms (sh_dir / sh_coefs shared, multiply then add, no contraction), summed in view order.
// One wave per 64 Gaussians; the rows leave through LDS as contiguous runs (M == 15) like the backward's own dL_dsh rows.
static constexpr int SGR = 32;
template <bool ADAM>
__global__ __launch_bounds__(64) void sh_grad_from_rgb_kernel(ShGradFromRgbArgs a)
{
#pragma clang fp contract(off)
    // SGR = 32 Gaussians per one-wave workgroup: lanes 0..31 rebuild a row each, then all 64 lanes stream the block's moments.  With 64 rows
    // the staging buffer was 12 KB and the kernel ran at 12 waves per CU; it lives on its occupancy like preprocess_bwd (6 KB: 20 waves).
    __shared__ __attribute__((aligned(16))) float lds_rows[SGR * 48];
    const int t = threadIdx.x;
    const int row0 = blockIdx.x * SGR;
    const int idx = t < SGR ? row0 + t : a.P;   // (lanes 32..63 own no Gaussian)
    const int rows = (a.P - row0) < SGR ? (a.P - row0) : SGR;
    float acc[45], adc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 45; k++) acc[k] = 0.f;
    if (idx < a.P) {
        const float px = a.means3D[3 * (size_t)idx], py = a.means3D[3 * (size_t)idx + 1], pz = a.means3D[3 * (size_t)idx + 2];
        for (int v = 0; v < a.n_views; v++) {
            const float* g = a.rgb_all + (size_t)v * a.rgb_stride + (size_t)idx * 3;
            float d[3] = {g[0], g[1], g[2]};
            if (d[0] == 0.f && d[1] == 0.f && d[2] == 0.f) continue;   // invisible in this view (or all channels clamped): adds exact zeros
            float dc_v[3];
            if (a.input_is_ddc) {   // the view's dL_ddc = SH_C0 * dRGB was shipped (hosts that only have the reference's gradient tensors)
#pragma unroll
                for (int ch = 0; ch < 3; ch++) { dc_v[ch] = d[ch]; d[ch] = d[ch] * (1.0f / SHC0); }
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) dc_v[ch] = SHC0 * d[ch];
            }
            float dox, doy, doz, x, y, z, c[15];
            sh_dir(px, py, pz, a.campos_all + (size_t)v * a.campos_stride, dox, doy, doz, x, y, z);
            sh_coefs(a.D, x, y, z, c);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) adc[ch] = adc[ch] + dc_v[ch];
#pragma unroll
            for (int k = 0; k < 15; k++) {
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const float prod = c[k] * d[ch];
                    acc[3 * k + ch] = acc[3 * k + ch] + prod;
                }
            }
        }
    }
    // dc rows [32 x 3] then rest rows [32 x 45] through LDS: contiguous float runs instead of 48 strided 4-byte stores per thread
    if (t < SGR) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) lds_rows[3 * t + ch] = adc[ch];
#pragma unroll
        for (int k = 0; k < 45; k++) lds_rows[3 * SGR + 45 * t + k] = acc[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (a.dL_ddc)
        for (int i = t; i < rows * 3; i += 64) a.dL_ddc[(size_t)row0 * 3 + i] = lds_rows[i];
    if (a.dL_dsh) {
        if (a.M == 15) {
            for (int i = t; i < rows * 45; i += 64) a.dL_dsh[(size_t)row0 * 45 + i] = lds_rows[3 * SGR + i];
        } else if (a.M > 0 && idx < a.P) {   // generic row width (lanes 0..31): coefficients above 15 (and above the active degree) are zero
            for (int k = 0; k < 3 * a.M; k++) a.dL_dsh[(size_t)3 * a.M * idx + k] = k < 45 ? lds_rows[3 * SGR + 45 * t + k] : 0.f;
        }
    }
    if constexpr (ADAM) {
        // the masked Adam of optim_utils.h:102-137 on features_dc and features_rest straight from the rebuilt rows (adam_scalar: the one
        // definition every call site shares), on float4 columns of the block's contiguous regions like the fused backward's phase C
        __shared__ uint8_t lds_vis[64];
        uint8_t myvis = 0;
        if (idx < a.P) {
            if (a.vis_stride) {   // the views' masks of an all-gathered payload, OR-ed here (no MAX-reduce launch in front of the step)
                for (int v = 0; v < a.n_views; v++) myvis |= a.visible[(size_t)v * a.vis_stride + idx];
                myvis = myvis ? 1 : 0;
                if (a.vis_out) a.vis_out[idx] = myvis;
            } else {
                myvis = a.visible[idx] ? 1 : 0;
            }
        }
        lds_vis[t] = myvis;   // (entries 32..63: never read)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const AdamFusedArgs& A = a.adam;
        auto update = [&](int grp, int width, const float* rows_lds, size_t base) {
            // region of this block: rows * width floats at param + base.  The float4 path needs 16-byte alignment of the gradient rows, the
            // parameter and both moments: row0 is a multiple of 32, so that holds whenever the BASE pointers are 16-byte aligned — which a gradient
            // slab with P % 4 != 0 does not give the opacity / rotation runs: checked here (wave-uniform), scalar path otherwise
            const bool aligned16 = ((reinterpret_cast<uintptr_t>(rows_lds) | reinterpret_cast<uintptr_t>(A.p[grp] + base) |
                                     reinterpret_cast<uintptr_t>(A.m[grp] + base) | reinterpret_cast<uintptr_t>(A.v[grp] + base)) & 15) == 0;
            if (rows == SGR && aligned16) {
                const int nv = SGR * width / 4;
                const float4* s4 = reinterpret_cast<const float4*>(rows_lds);
                constexpr int U = 4;
                for (int i0 = t; i0 < nv; i0 += 64 * U) {
                    float4 g[U], p[U], m[U], v[U];
                    bool vis[U][4], any[U];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const int i = i0 + 64 * u;
                        any[u] = false;
                        if (i < nv) {
                            g[u] = s4[i];
                            const int e = 4 * i;
                            vis[u][0] = lds_vis[e / width]; vis[u][1] = lds_vis[(e + 1) / width];
                            vis[u][2] = lds_vis[(e + 2) / width]; vis[u][3] = lds_vis[(e + 3) / width];
                            any[u] = vis[u][0] | vis[u][1] | vis[u][2] | vis[u][3];
                        }
                        if (any[u]) {
                            p[u] = ld_stream(reinterpret_cast<const float4*>(A.p[grp] + base) + i);
                            m[u] = ld_stream(reinterpret_cast<const float4*>(A.m[grp] + base) + i);
                            v[u] = ld_stream(reinterpret_cast<const float4*>(A.v[grp] + base) + i);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (!any[u]) continue;
                        const int i = i0 + 64 * u;
                        if (vis[u][0]) adam_scalar(p[u].x, g[u].x, m[u].x, v[u].x, A.lr[grp], A.b1, A.b2, A.eps);
                        if (vis[u][1]) adam_scalar(p[u].y, g[u].y, m[u].y, v[u].y, A.lr[grp], A.b1, A.b2, A.eps);
                        if (vis[u][2]) adam_scalar(p[u].z, g[u].z, m[u].z, v[u].z, A.lr[grp], A.b1, A.b2, A.eps);
                        if (vis[u][3]) adam_scalar(p[u].w, g[u].w, m[u].w, v[u].w, A.lr[grp], A.b1, A.b2, A.eps);
                        st_stream(reinterpret_cast<float4*>(A.p[grp] + base) + i, p[u]);
                        st_stream(reinterpret_cast<float4*>(A.m[grp] + base) + i, m[u]);
                        st_stream(reinterpret_cast<float4*>(A.v[grp] + base) + i, v[u]);
                    }
                }
            } else {
                for (int i = t; i < rows * width; i += 64)
                    if (lds_vis[i / width]) adam_scalar(A.p[grp][base + i], rows_lds[i], A.m[grp][base + i], A.v[grp][base + i], A.lr[grp], A.b1, A.b2, A.eps);
            }
        };
        if (a.g_small[0]) {   // the four small groups from their all-reduced gradients (read in place from the slab): the whole optimiser step in this launch
            update(0, 3, a.g_small[0] + (size_t)row0 * 3, (size_t)row0 * 3);
            update(3, 1, a.g_small[1] + (size_t)row0, (size_t)row0);
            update(4, 3, a.g_small[2] + (size_t)row0 * 3, (size_t)row0 * 3);
            update(5, 4, a.g_small[3] + (size_t)row0 * 4, (size_t)row0 * 4);
        }
        update(1, 3, lds_rows, (size_t)row0 * 3);
        if (a.M == 15) {
            update(2, 45, lds_rows + 3 * SGR, (size_t)row0 * 45);
        } else if (a.M > 0 && idx < a.P && lds_vis[t]) {
            for (int k = 0; k < 3 * a.M; k++) {
                const size_t o = (size_t)3 * a.M * idx + k;
                adam_scalar(A.p[2][o], k < 45 ? lds_rows[3 * SGR + 45 * t + k] : 0.f, A.m[2][o], A.v[2][o], A.lr[2], A.b1, A.b2, A.eps);
            }
        }
    }
}

int launch_sh_grad_from_rgb(const ShGradFromRgbArgs& a, hipStream_t s)
{
    if (a.P <= 0) return GSLIC_OK;
    if (a.adam.on) GS_LAUNCH(K_SH_REBUILD, sh_grad_from_rgb_kernel<true>, dim3(div_up(a.P, SGR)), dim3(64), 0, s, a);
    else GS_LAUNCH(K_SH_REBUILD, sh_grad_from_rgb_kernel<false>, dim3(div_up(a.P, SGR)), dim3(64), 0, s, a);
    return GSLIC_OK;
}


}  // namespace gslic
