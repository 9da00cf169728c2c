/*
 * gslic_hip.h — C-ABI of libgslic_hip.so: the MI355X (gfx950) differentiable 3D-Gaussian-splatting
 * hot path of Gaussian-LIC (render forward / backward, sparse Adam, fused SSIM, simple-knn).
 *
 * Drop-in boundary.  The reference has no FFI; its seam is the L2 layer of six free functions on
 * torch::Tensor that only unwrap pointers (src/rasterizer/rasterize_points.h:25-96,
 * src/fused-ssim/ssim.h:7-26, src/simple-knn/spatial.h:14) and the raw-pointer L1 layer underneath
 * (src/rasterizer/cuda_rasterizer/rasterizer.h:29-98, adam.h:12-23, src/simple-knn/simple_knn.h:18).
 * Every entry point below names the L1/L2 function it replaces.  The LibTorch shim that re-exports the
 * reference's exact L2 signatures on top of this header lives in gaussian-lic_amd/shim/.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch / C++ types.
 *  - every `const float*` / `float*` / `int*` tensor argument is a DEVICE pointer (HBM), fp32 / int32,
 *    contiguous row-major, exactly the layouts of the reference (SURVEY.md §8b "Layouts").
 *  - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream, as the reference uses).
 *  - every function returns GSLIC_OK (0) or a negative gslic_status; nothing throws across the boundary.
 *    gslic_last_error() returns a thread-local, NUL-terminated description of the last failure.
 *  - the library never frees or owns caller memory; scratch is obtained through the caller's allocator
 *    callbacks in the same order as the reference (geom -> img -> binning -> sample), each at most once.
 *  - the four scratch buffers are opaque: their internal layout is private to this library (it is NOT
 *    the reference's GeometryState/ImageState/BinningState/SampleState layout) and the buffers written by
 *    gslic_rasterize_forward must be handed unchanged to gslic_rasterize_backward.
 */
#ifndef GSLIC_HIP_H_INCLUDED
#define GSLIC_HIP_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSLIC_ABI_VERSION 8

typedef enum gslic_status {
    GSLIC_OK = 0,
    GSLIC_ERR_INVALID_ARG = -1,  /* NULL where a pointer is required, negative sizes, bad degree ...       */
    GSLIC_ERR_UNSUPPORTED = -2,  /* colors_precomp / cov3D_precomp non-NULL (dead in the reference's host) */
    GSLIC_ERR_ALLOC = -3,        /* an allocator callback returned NULL for a non-zero request             */
    GSLIC_ERR_HIP = -4,          /* a HIP runtime call or kernel launch failed                            */
    GSLIC_ERR_PREFILTERED = -5   /* prefiltered=1 and a Gaussian was culled (reference: device __trap)    */
} gslic_status;

/* Replaces std::function<char*(size_t)> (cuda_rasterizer/rasterizer.h:30-33; built by resizeFunctional,
 * rasterize_points.cu:40-48).  Must return a device pointer to at least `bytes` bytes (any alignment:
 * the library re-aligns to 256 B and has already added the slack), valid until the matching backward. */
typedef char* (*gslic_alloc_fn)(void* ctx, size_t bytes);

/* Scalar arguments of CudaRasterizer::Rasterizer::forward/backward (rasterizer.h:29-98), i.e. the fields
 * of GaussianRasterizationSettings (src/rasterizer/rasterizer.h:27-73) that reach the kernels. */
typedef struct gslic_raster_params {
    int32_t P;              /* number of Gaussians (means3D.size(0))                                   */
    int32_t D;              /* active SH degree 0..3 (sh_degree_)                                      */
    int32_t M;              /* number of "rest" SH coefficients per Gaussian = sh.size(1) (15), 0 if sh empty */
    int32_t width;          /* image_width                                                            */
    int32_t height;         /* image_height                                                           */
    float tan_fovx, tan_fovy;
    float limx_neg, limx_pos, limy_neg, limy_pos; /* asymmetric Jacobian clamp (src/camera.h:63-66)    */
    float scale_modifier;   /* always 1 in the reference                                               */
    int32_t prefiltered;    /* bool                                                                    */
    int32_t debug;          /* bool: synchronise + check after every stage (CHECK_CUDA, auxiliary.h:173-180) */
    int32_t no_color;       /* bool: transmittance-only render (forward.cu:338,362,412,446,470)         */
    int32_t raw_params;     /* bool, 0 for the drop-in shim.  1: `opacities`, `scales`, `rotations` are the
                               RAW parameters (logit, log, unnormalised quaternion); sigmoid / exp / normalize of
                               renderer.cpp:57-63 + gaussian.cpp:147-175 run inside the kernels, and the backward returns
                               dL/d(raw) in dL_dopacity / dL_dscale / dL_drot (the chain LibTorch autograd would apply). */
    const uint32_t* tie_rank; /* NULL for the drop-in shim (ABI 7).  DEVICE uint32[P], optional: for a host that keeps the map's rows in a
                               PERMUTED order (trainer.GaussianModel(order="morton"): rows sorted along a space-filling curve so that what a
                               view sees is contiguous in memory), tie_rank[i] = index of row i in the ORIGINAL (insertion) order.  The
                               reference lists Gaussians of equal (tile, depth bits) by ascending index (stable 64-bit sort of the
                               index-ordered emission, rasterizer_impl.cu:395-424); with tie_rank set, equal depths are listed by ascending
                               tie_rank instead of by row index, so a permuted map renders and trains bit-identically to the unpermuted
                               one.  Read by the forward only. */
} gslic_raster_params;

/* ------------------------------------------------------------------------------------------------
 * gslic_rasterize_forward — replaces CudaRasterizer::Rasterizer::forward (rasterizer_impl.cu:312-474),
 * reached from RasterizeGaussiansCUDA (rasterize_points.cu:50-149).
 *
 *  background      [3]      accepted and ignored, like the reference (forward.cu:335,460-469)
 *  means3D         [P,3]    dc [P,1,3]    shs [P,M,3] (NULL when M==0)
 *  colors_precomp  must be NULL   cov3D_precomp must be NULL   (rasterizer.cpp:200-201 always passes empty)
 *  opacities       [P,1] post-sigmoid   scales [P,3] post-exp   rotations [P,4] post-normalise (r,x,y,z)
 *  viewmatrix, projmatrix   [16] device, element (row r, col c) at [4c+r] (src/camera.h:86,109,60)
 *  cam_pos         [3] device
 *  out_color       [3,H,W] (untouched when no_color)   out_final_T [H,W]   radii [P] int32
 *  num_rendered    host int: R = number of (Gaussian, tile) instances      } the two ints the reference
 *  num_buckets     host int: B = number of checkpoint buckets (0 if no_color) } returns (rasterizer_impl.cu:473)
 *
 * Allocator call order geom(P) -> img(N,T) -> binning(R) -> sample(B); sample is called only when
 * !no_color (rasterizer_impl.cu:355,359,401,437-447).  The host waits for the device twice (to learn R and
 * B), exactly where the reference blocks (rasterizer_impl.cu:398,442); the wait is a spin on a pinned-memory
 * mailbox a one-thread kernel writes (GSLIC_NO_MAILBOX=1: hipMemcpyAsync + hipStreamSynchronize instead).
 * P == 0 returns immediately with R = B = 0 and calls no allocator (rasterize_points.cu:110).
 */
int gslic_rasterize_forward(
    const gslic_raster_params* prm,
    gslic_alloc_fn geom_alloc, void* geom_ctx,
    gslic_alloc_fn binning_alloc, void* binning_ctx,
    gslic_alloc_fn img_alloc, void* img_ctx,
    gslic_alloc_fn sample_alloc, void* sample_ctx,
    const float* background,
    const float* means3D,
    const float* dc,
    const float* shs,
    const float* colors_precomp,
    const float* opacities,
    const float* scales,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* cam_pos,
    float* out_color,
    float* out_final_T,
    int32_t* radii,
    int32_t* num_rendered,
    int32_t* num_buckets,
    void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_rasterize_forward_capacity — the same forward with NO host round trip (the reference blocks the host twice to learn R and B,
 * rasterizer_impl.cu:398,442; gslic_rasterize_forward keeps that contract for the allocator callbacks).  The caller owns the four
 * scratch buffers and passes their sizes; geom / img must hold gslic_geom_bytes(P) / gslic_img_bytes(W, H), binning and sample are
 * CAPACITIES: the number of instances / checkpoint buckets they hold is derived from their size (gslic_binning_bytes /
 * gslic_sample_bytes are monotonic), every launch is sized for that capacity and stops at the real count, which stays on the device.
 * Nothing in the call allocates, synchronises or copies to the host, so a whole training step can be captured in a hipGraph.
 *
 *  capacity_R, capacity_B   host ints: the capacities in use.  Pass THEM as R and B to gslic_rasterize_backward* (the buffer
 *                           layout depends on them); the backward stops at the real counts on the device.
 *  status                   DEVICE uint32[8], updated by the last kernel of the call (zero the words once; they accumulate):
 *                           [0] = R, [1] = B (real counts of THIS forward), [2] = its bits — 1: the instances did not fit into `binning`,
 *                           2: the buckets did not fit into `sample`, 4: prefiltered violation, 8: a scan / sort look-back wait timed out
 *                           (device preempted), 16: more than 2^31 instances — [3] += 1 when none of 1 | 2 | 8 | 16 is set (forwards
 *                           that completed), [4] += 1 always (forwards issued), [5] |= 1 << (issue index mod 32) for a forward that
 *                           did not complete, [6] / [7] = the largest R / B seen (what to size a retry from).
 *  The timeout / overflow bits of a forward live in its own geometry buffer (ABI 7): capacity-mode forwards on different buffers may run
 *  concurrently on several streams of one device, and nothing is allocated by the first call.
 *  On overflow or timeout (bit 1, 2, 8 or 16) nothing is written out of bounds, out_color / out_final_T are unspecified, and a following
 *  gslic_rasterize_backward* on these buffers does NOTHING (no gradients, no Adam update): the host re-runs the step with larger
 *  buffers once it has seen the bits.  All other arguments as gslic_rasterize_forward; results are bit-identical to it.
 */
int gslic_rasterize_forward_capacity(
    const gslic_raster_params* prm,
    char* geom_buffer, size_t geom_bytes,
    char* binning_buffer, size_t binning_bytes,
    char* img_buffer, size_t img_bytes,
    char* sample_buffer, size_t sample_bytes,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos,
    float* out_color, float* out_final_T, int32_t* radii,
    int32_t* capacity_R, int32_t* capacity_B, uint32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_rasterize_backward — replaces CudaRasterizer::Rasterizer::backward (rasterizer_impl.cu:476-581),
 * reached from RasterizeGaussiansBackwardCUDA (rasterize_points.cu:151-246).
 *
 *  R, B                       the two ints gslic_rasterize_forward returned
 *  geom/binning/img/sample    the SAME memory the forward filled (rasterizer.cpp:83-98 keeps it alive)
 *  dL_dpix        [3,H,W]     gradient of the loss w.r.t. out_color
 *  outputs (each [P,*], EVERY row is written — rows of invisible Gaussians get exact zeros — so the caller
 *  may pass uninitialised memory; the reference instead requires ten zero-filled tensors,
 *  rasterize_points.cu:192-201):
 *    dL_dmean2D [P,3] (NDC-scaled, z = 0)   dL_dconic [P,2,2] (x,y,-,w slots; slot 2 = 0)   dL_dopacity [P,1]
 *    dL_dcolor [P,3]   dL_dmean3D [P,3]   dL_dcov3D [P,6]   dL_ddc [P,1,3]   dL_dsh [P,M,3]
 *    dL_dscale [P,3]   dL_drot [P,4]
 *  dL_dmean2D, dL_dconic, dL_dcolor and dL_dcov3D may be NULL (the host discards them); the others are required
 *  (dL_dsh may be NULL when M == 0).
 *  shs == NULL skips the whole SH backward like the reference's `if (shs)` (backward.cu:352): dL_ddc = 0.
 */
int gslic_rasterize_backward(
    const gslic_raster_params* prm,
    int32_t R, int32_t B,
    const float* background,
    const float* means3D,
    const float* dc,
    const float* shs,
    const float* colors_precomp,
    const float* scales,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* cam_pos,
    const int32_t* radii,
    char* geom_buffer,
    char* binning_buffer,
    char* img_buffer,
    char* sample_buffer,
    const float* dL_dpix,
    float* dL_dmean2D,
    float* dL_dconic,
    float* dL_dopacity,
    float* dL_dcolor,
    float* dL_dmean3D,
    float* dL_dcov3D,
    float* dL_ddc,
    float* dL_dsh,
    float* dL_dscale,
    float* dL_drot,
    float lambda_erank,
    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth rendering (LiDAR depth supervision; no reference counterpart).
 *
 * gslic_rasterize_forward_depth — gslic_rasterize_forward plus one output:
 *  out_depth      [H,W]     depth[y,x] = sum_i T_i alpha_i z_i over EXACTLY the contributors of the pixel's colour (same alpha,
 *                           transmittance, cut-offs and early stop; same arithmetic mode, gslic_set_math_mode), z_i = the Gaussian's
 *                           view-space depth p_view.z (the key the forward sorts on).  The background contributes 0 and the depth is
 *                           NOT normalised: divide by (1 - out_final_T) for the expected depth of the covered part.
 *  Colour, final_T, radii, R and B are bit-identical to gslic_rasterize_forward's.  The allocator callbacks are asked for more bytes:
 *  img + 4 per pixel (of the 16x16 tile grid), sample + 4 per bucket-pixel (1 KiB per checkpoint bucket), binning + 4 per instance,
 *  carved behind every other array (the colour-only layout is an exact prefix).  no_color = 1, or out_depth == NULL with P > 0, is
 *  GSLIC_ERR_INVALID_ARG; P == 0 returns at once and calls no allocator.
 *
 * gslic_rasterize_backward_depth — gslic_rasterize_backward plus one input:
 *  dL_ddepth      [H,W]     gradient of the loss w.r.t. out_depth
 *  The ten outputs are as gslic_rasterize_backward's, with the depth's share added: through alpha (dL_dmean2D, dL_dconic,
 *  dL_dopacity and everything behind them) and through z (dL_dmean3D += dL/dz * row 2 of the view matrix, added last — so
 *  dL_ddepth = 0 gives gslic_rasterize_backward's results bit for bit).  dL_dcolor stays the colour's.  The buffers must come from
 *  gslic_rasterize_forward_depth (else GSLIC_ERR_INVALID_ARG; the library remembers its last 64 forwards, and only for buffers it does
 *  not know the check costs one 4-byte device read, the call then waits for the stream).  gslic_rasterize_backward on a depth forward's buffers is valid and returns the colour-only gradients.
 *  no_color = 1, or dL_ddepth == NULL with P > 0, is GSLIC_ERR_INVALID_ARG; P == 0 returns at once.
 *
 * The single-GPU fast path has depth too: gslic_rasterize_forward_depth_capacity (capacity / graph mode), gslic_rasterize_backward_depth_adam
 * (fused Adam) and gslic_depth_l1_loss_forward_backward (the loss) below.
 * The camera-pose gradient has depth too: gslic_rasterize_backward_depth_camera (behind gslic_rasterize_backward_camera, below).
 * Not covered by depth (unchanged, colour only): the N-GPU colour exchange (gslic_rasterize_backward_rgb*) and the LibTorch drop-in shim.
 */
int gslic_rasterize_forward_depth(
    const gslic_raster_params* prm,
    gslic_alloc_fn geom_alloc, void* geom_ctx,
    gslic_alloc_fn binning_alloc, void* binning_ctx,
    gslic_alloc_fn img_alloc, void* img_ctx,
    gslic_alloc_fn sample_alloc, void* sample_ctx,
    const float* background,
    const float* means3D,
    const float* dc,
    const float* shs,
    const float* colors_precomp,
    const float* opacities,
    const float* scales,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* cam_pos,
    float* out_color,
    float* out_final_T,
    float* out_depth,
    int32_t* radii,
    int32_t* num_rendered,
    int32_t* num_buckets,
    void* stream);

int gslic_rasterize_backward_depth(
    const gslic_raster_params* prm,
    int32_t R, int32_t B,
    const float* background,
    const float* means3D,
    const float* dc,
    const float* shs,
    const float* colors_precomp,
    const float* scales,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* cam_pos,
    const int32_t* radii,
    char* geom_buffer,
    char* binning_buffer,
    char* img_buffer,
    char* sample_buffer,
    const float* dL_dpix,
    const float* dL_ddepth,
    float* dL_dmean2D,
    float* dL_dconic,
    float* dL_dopacity,
    float* dL_dcolor,
    float* dL_dmean3D,
    float* dL_dcov3D,
    float* dL_ddc,
    float* dL_dsh,
    float* dL_dscale,
    float* dL_drot,
    float lambda_erank,
    void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_rasterize_backward_adam — single-GPU fast path (no reference counterpart; SURVEY.md §8f row 2 taken one step further):
 * exactly gslic_rasterize_backward with raw_params = 1 followed by gslic_adam_update_groups(visible = radii > 0) over the six
 * parameter groups, but the Adam update is applied inside the per-Gaussian backward kernel while the gradients are still in
 * registers / LDS, so the 236 B/Gaussian of gradients are neither written nor re-read (and no second launch).  Results are
 * bit-identical to the two-call sequence.  The six gradient output pointers may be NULL (nothing is written) or non-NULL.
 * Group order everywhere: xyz, features_dc, features_rest, opacity, scaling, rotation (src/gaussian.cpp:399-418);
 * param[0] / [1] / [2] / [4] / [5] must be the tensors passed as means3D / dc / shs / scales / rotations.
 * Not usable when gradients must be exchanged between GPUs before the update.
 */
typedef struct gslic_adam_fused {
    float* param[6];
    float* exp_avg[6];
    float* exp_avg_sq[6];
    float lr[6];
    float b1, b2, eps;
    uint8_t* visible_out;   /* optional (ABI 7) DEVICE [P]: gslic_rasterize_backward_adam also writes 1 = radii > 0 per Gaussian — the `visible` mask
                               of renderer.cpp:85 that the host reads for its statistics — so that no compare kernel has to be launched for it;
                               ignored by the other entry points that take this descriptor */
} gslic_adam_fused;
int gslic_rasterize_backward_adam(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix,
    float* dL_dopacity, float* dL_dmean3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
    float lambda_erank, const gslic_adam_fused* adam, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth on the single-GPU fast path (no reference counterpart).
 *
 * gslic_rasterize_forward_depth_capacity — gslic_rasterize_forward_capacity plus out_depth [H,W] (as gslic_rasterize_forward_depth): no host
 *  round trip, results bit-identical to gslic_rasterize_forward_depth, the same status words and overflow behaviour (nothing is written out of
 *  bounds; a following backward, _depth_adam included, does nothing).  The buffers are sized with the depth carves: img >= gslic_img_bytes_depth,
 *  and the capacities R / B are derived from gslic_binning_bytes_depth / gslic_sample_bytes_depth (each monotonic; the colour-only size of the
 *  same count is an exact prefix).  The forward leaves a host-side note, so a depth backward on these buffers needs no device read (graph capture).
 *
 * gslic_rasterize_backward_depth_adam — gslic_rasterize_backward_adam plus dL_ddepth [H,W]: bit-identical to gslic_rasterize_backward_depth with
 *  raw_params = 1 followed by gslic_adam_update_groups(visible = radii > 0); fills adam->visible_out like the colour entry point.  The fused
 *  kernel updates every group but xyz and leaves xyz's chain gradient in dL_dmean3D, which is therefore REQUIRED here ([P,3], any contents: every
 *  row is written); a second kernel adds dL/dz * row 2 of the view matrix and updates xyz from the complete gradient (which dL_dmean3D then holds).
 *  The other gradient pointers may be NULL.  dL_ddepth == NULL, dL_dmean3D == NULL or adam == NULL (P > 0) is GSLIC_ERR_INVALID_ARG.
 */
int gslic_rasterize_forward_depth_capacity(
    const gslic_raster_params* prm,
    char* geom_buffer, size_t geom_bytes,
    char* binning_buffer, size_t binning_bytes,
    char* img_buffer, size_t img_bytes,
    char* sample_buffer, size_t sample_bytes,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos,
    float* out_color, float* out_final_T, float* out_depth, int32_t* radii,
    int32_t* capacity_R, int32_t* capacity_B, uint32_t* status, void* stream);
int gslic_rasterize_backward_depth_adam(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix, const float* dL_ddepth,
    float* dL_dopacity, float* dL_dmean3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
    float lambda_erank, const gslic_adam_fused* adam, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient densification statistics (no reference counterpart; additive exports, ABI 8).
 *
 * The signal 3DGS hosts densify by is the accumulated norm of the view-space positional gradient (xyz_gradient_accum / denom) and, for the
 * screen-size prune, max_radii2D.  On the fused-Adam backwards that gradient never leaves the per-Gaussian kernel; these entry points accumulate
 * it there, in the one thread that owns the row.
 *
 * gslic_grad_stats: three per-row accumulators, DEVICE arrays of P elements each, caller-owned, persistent over views, in STORAGE row order.
 * All three pointers are required.
 *
 * THE RULE.  For one backward, every row i of the call's row range with radii[i] > 0 is updated as follows.  mx, my are the two sums the
 * per-Gaussian backward forms over the row's instances — the very numbers gslic_rasterize_backward writes to dL_dmean2D[3i] and [3i + 1]; the
 * 0.5 W / 0.5 H factors are in them, as in 3DGS's viewspace_points.grad.
 *     n = sqrtf((mx * mx) + (my * my))          each operation one float32 operation rounded on its own (no contraction), the square root
 *                                               correctly rounded
 *     if n is finite:  grad_sum[i] = grad_sum[i] + n,  n_seen[i] += 1        (a non-finite n changes neither)
 *     max_radius[i] = max(max_radius[i], radii[i])                           (whether or not n is finite)
 * Rows with radii[i] <= 0 and rows outside the range are not touched.  When the forward's status word reports a capacity overflow
 * (status[2] != 0: the step is a no-op) nothing is touched.  One thread owns a row: plain loads and stores, no atomics, and the result is a
 * fixed function of the sequence of views.
 *
 * gslic_rasterize_backward_adam_stats / gslic_rasterize_backward_depth_adam_stats — gslic_rasterize_backward_adam / _depth_adam (same
 *  arguments, same checks, bit-identical parameters and moments) which also apply the rule.  Refused with GSLIC_ERR_INVALID_ARG before any
 *  device work: stats == NULL or one of its pointers NULL; one of the three arrays ([P] x 4 bytes) overlapping another, or overlapping a
 *  param / exp_avg / exp_avg_sq tensor of the Adam descriptor.
 * gslic_gradient_stats_accumulate — the rule on a dL_dmean2D [P,3] (elements 0 and 1 of a row are mx, my) and radii [P] the caller already has
 *  (gslic_rasterize_backward and its depth / camera variants write them), rows [row_begin, row_end) (row_end < 0: P): one launch, one thread per
 *  row, bit-identical to the fused route on the same gradient.  NULL pointers, overlapping arrays and a bad row range are refused.
 */
typedef struct gslic_grad_stats {
    float* grad_sum;       /* float32 [P] */
    uint32_t* n_seen;      /* uint32  [P] */
    int32_t* max_radius;   /* int32   [P] */
} gslic_grad_stats;
int gslic_rasterize_backward_adam_stats(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix,
    float* dL_dopacity, float* dL_dmean3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
    float lambda_erank, const gslic_adam_fused* adam, const gslic_grad_stats* stats, void* stream);
int gslic_rasterize_backward_depth_adam_stats(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix, const float* dL_ddepth,
    float* dL_dopacity, float* dL_dmean3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
    float lambda_erank, const gslic_adam_fused* adam, const gslic_grad_stats* stats, void* stream);
int gslic_gradient_stats_accumulate(
    int32_t P, const float* dL_dmean2D, const int32_t* radii, const gslic_grad_stats* stats, int32_t row_begin, int32_t row_end, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_rasterize_backward_rgb + gslic_sh_grad_from_rgb — the backward split for the N-GPU exchange (no reference counterpart: the
 * reference is single-GPU).  The SH backward (computeColorFromSH, backward.cu:27-136) is linear in the clamp-masked colour gradient
 * dRGB: dL_ddc = SH_C0 dRGB and dL_dsh[k] = c_k(dir) dRGB, with c_k a function of the view direction normalize(p - campos) only.
 * So a rank does not have to all-reduce the 48 floats of dL_ddc / dL_dsh per Gaussian (81 % of the gradient bytes): it ships dRGB
 * (12 bytes), all-gathers the other views' dRGB and camera centres, and rebuilds the SUMMED rows locally.  xGMI is point-to-point —
 * bytes on the links are what bounds the N > 1 step.
 *
 * gslic_rasterize_backward_rgb  = gslic_rasterize_backward that writes dL_drgb [P,3] (zeros for invisible Gaussians) instead of
 *                                 dL_ddc / dL_dsh; the gradients the host discards are not materialised.
 * gslic_sh_grad_from_rgb        dL_ddc [P,3], dL_dsh [P,M,3] = sum over v < n_views of view v's rows, from
 *                                 rgb_all [n_views][P][3] and campos_all [n_views][3] (device), in view order with the backward's own
 *                                 arithmetic (bit-identical to summing the per-view gslic_rasterize_backward outputs in that order).
 *                                 input_is_ddc = 1: rgb_all holds the views' dL_ddc instead (hosts that only see the reference's
 *                                 gradient tensors); dRGB is then recovered as dL_ddc * (1 / SH_C0), exact to 1 ulp.
 *                                 view_stride = 0: the dense layouts above.  view_stride > 0 (floats, >= 3 P): view v's colour gradients
 *                                 start at rgb_all + v * view_stride and its camera centre at campos_all + v * view_stride — one
 *                                 all-gather of a per-rank payload {dRGB [P,3], camera centre [3], ...} needs no unpacking
 *                                 (pass campos_all = rgb_all + 3 P).
 */
int gslic_rasterize_backward_rgb(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix,
    float* dL_dopacity, float* dL_dmean3D, float* dL_drgb, float* dL_dscale, float* dL_drot,
    float lambda_erank, void* stream);
/* gslic_rasterize_backward_rgb that also fills the rest of a rank's all-gather payload {dRGB [P,3], camera centre [3], visibility [P] bytes}:
 * vis_out[g] = radii[g] > 0 and campos_out[0..2] = cam_pos are written by the per-Gaussian kernel, so the host issues no compare / copy
 * launches between the backward and the collective.  Either may be NULL. */
int gslic_rasterize_backward_rgb_payload(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix,
    float* dL_dopacity, float* dL_dmean3D, float* dL_drgb, float* dL_dscale, float* dL_drot,
    float lambda_erank, uint8_t* vis_out, float* campos_out, void* stream);
/* gslic_rasterize_backward_rgb in row chunks: the per-Gaussian half of the backward for Gaussians [row_begin, row_end) only (row_begin a
 * multiple of 64; the gradient pointers are still indexed by the ABSOLUTE Gaussian index), the blend half (one pass over the whole image) unless
 * skip_blend.  A host that exchanges gradients calls it once per chunk — the first call with skip_blend = 0 — and puts chunk c on the wire
 * while chunk c + 1 is computed. */
int gslic_rasterize_backward_rgb_rows(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix,
    float* dL_dopacity, float* dL_dmean3D, float* dL_drgb, float* dL_dscale, float* dL_drot,
    float lambda_erank, int32_t row_begin, int32_t row_end, int32_t skip_blend, void* stream);
int gslic_sh_grad_from_rgb(
    int32_t P, int32_t D, int32_t M, int32_t n_views, const float* means3D, const float* campos_all /*[n_views,3]*/,
    const float* rgb_all /*[n_views,P,3]*/, int32_t input_is_ddc, float* dL_ddc, float* dL_dsh, int64_t view_stride, void* stream);
/* The same rebuild with the masked Adam update of features_dc / features_rest (groups 1 and 2 of `adam`; the other groups are ignored)
 * applied straight from the rebuilt rows: the 192 B/Gaussian of dL_ddc / dL_dsh are neither written nor re-read.  `visible` = the
 * exchanged (OR-ed) mask, one byte per Gaussian.  dL_ddc / dL_dsh may be NULL (not materialised) or non-NULL (also written).
 * Bit-identical to gslic_sh_grad_from_rgb followed by gslic_adam_update_groups on the two groups. */
int gslic_sh_grad_from_rgb_adam(
    int32_t P, int32_t D, int32_t M, int32_t n_views, const float* means3D, const float* campos_all, const float* rgb_all,
    int32_t input_is_ddc, const uint8_t* visible, const gslic_adam_fused* adam, float* dL_ddc, float* dL_dsh, int64_t view_stride, void* stream);
/* The whole optimiser step of an N > 1 rank in ONE launch, straight from what the exchange delivered: the views' visibility masks are OR-ed
 * here (view v's mask at vis_all + v * vis_stride bytes; vis_stride = 0: vis_all is one already OR-ed mask; the OR is also written to vis_out
 * when that is non-NULL), dL_ddc / dL_dsh are rebuilt from the views' colour gradients and consumed by the masked Adam of groups 1 and 2,
 * and — when the four summed (all-reduced) small gradients dL_dmean3D [P,3], dL_dopacity [P,1], dL_dscale [P,3], dL_drot [P,4] are given —
 * the masked Adam of groups 0, 3, 4, 5 reads them in place.  Bit-identical to gslic_sh_grad_from_rgb_adam + gslic_adam_update_groups on the
 * OR-ed mask.  (src/gaussian.cpp:697-707 is the step this replaces on every rank: set_visibility_and_N + SparseGaussianAdam::step.) */
int gslic_sh_grad_from_rgb_adam_all(
    int32_t P, int32_t D, int32_t M, int32_t n_views, const float* means3D, const float* campos_all, const float* rgb_all,
    int32_t input_is_ddc, const uint8_t* vis_all, int64_t vis_stride, uint8_t* vis_out, const gslic_adam_fused* adam,
    const float* dL_dmean3D, const float* dL_dopacity, const float* dL_dscale, const float* dL_drot, int64_t view_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_rasterize_backward_camera — gslic_rasterize_backward plus the gradient w.r.t. the CAMERA inputs (the "cam" of the
 * north-star; no reference counterpart: the reference's autograd node returns an undefined tensor for the raster settings,
 * src/rasterizer/rasterizer.cpp:171-182).  viewmatrix, projmatrix and cam_pos are treated as the three independent inputs they
 * are at this boundary; a host that derives them from a pose chains through its own (tiny) LibTorch graph:
 *   dL_dviewmatrix [16]  same element order as viewmatrix ([4c+r]); rows 0..2 carry gradient — through t = V [p,1] (cov2D Jacobian; EXACT
 *                        through the frustum clamp: a clamped t.x = lim t.z still moves with t.z, a term the reference's parameter
 *                        gradients drop, backward.cu:225-233, and this one keeps) and through the rotation part W of T = W J (:180-197)
 *   dL_dprojmatrix [16]  rows 0, 1, 3 — through p_hom = P [p,1] -> mean2D (backward.cu:339-350)
 *   dL_dcampos     [3]   through the SH view direction normalize(p - campos) (backward.cu:27-136)
 * All three are sums over the visible Gaussians, reduced in a fixed order (bit-reproducible).  Depth ordering, culling and the
 * tile assignment are piecewise constant in the camera and contribute nothing, as for every other input.  All device pointers.
 */
int gslic_rasterize_backward_camera(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix,
    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
    float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot, float lambda_erank,
    float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, void* stream);

/* gslic_rasterize_backward_depth_camera — gslic_rasterize_backward_depth plus the three camera gradients of gslic_rasterize_backward_camera, for a
 * loss on colour AND depth (buffers of gslic_rasterize_forward_depth).  The depth reaches the camera through the 2D quantities (its share is inside
 * dL_dmean2D / dL_dconic / dL_dopacity, so all three camera outputs carry it) and directly through the view-space depth
 * z = V[2] x + V[6] y + V[10] z + V[14]:  dL_dviewmatrix[2, 6, 10, 14] += sum_i dL/dz_i (x_i, y_i, z_i, 1), added last.  dL_dprojmatrix and dL_dcampos
 * get no direct term.  The ten per-Gaussian outputs are gslic_rasterize_backward_depth's; dL_ddepth = 0 gives gslic_rasterize_backward_camera's
 * results bit for bit.  View row 3 and projection row 2 are exact zeros; the sums are reduced in a fixed order (bit-reproducible).
 * A NULL camera output, dL_ddepth == NULL, no_color = 1, SH degree > 3 or buffers of a colour-only forward: GSLIC_ERR_INVALID_ARG before any
 * device work.  P == 0: the three camera outputs are zeroed.  After a capacity-mode forward that overflowed, the per-Gaussian outputs are
 * left untouched and the three camera outputs are zeros.
 */
int gslic_rasterize_backward_depth_camera(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix, const float* dL_ddepth,
    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
    float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot, float lambda_erank,
    float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, void* stream);

/* The joint map + pose iteration on the single-GPU fast path (no reference counterpart; additive exports, ABI 8).
 *
 * gslic_rasterize_backward_camera_adam — gslic_rasterize_backward_adam plus the three camera gradients, in the same launches: the per-Gaussian
 *  kernel forms the 27 camera sums from the parameters AS THEY WERE, then applies the Adam update while the gradients are still in registers / LDS.
 * gslic_rasterize_backward_depth_camera_adam — gslic_rasterize_backward_depth_adam plus the same three, for a loss on colour AND depth: the fused
 *  kernel updates every group but xyz and leaves xyz's chain gradient in dL_dmean3D (REQUIRED, [P,3], any contents: every row is written); a second
 *  kernel adds dL/dz * row 2 of the view matrix, forms the four direct view-matrix sums dL/dz_i (x_i, y_i, z_i, 1) from the means as they were and
 *  then updates xyz from the complete gradient.
 *
 * THE RULE.  Parameters, both moments and adam->visible_out are bit-identical to gslic_rasterize_backward_camera / _depth_camera with
 * raw_params = 1 followed by gslic_adam_update_groups(visible = radii > 0) over the six groups; the three camera outputs are bit-identical to that
 * call's (sums over the parameters before the update, reduced in the same fixed order: no atomics, every run gives the same bits).  dL_dmean2D
 * (optional, [P,3]) receives what gslic_rasterize_backward writes there — the input of gslic_gradient_stats_accumulate; the six parameter-gradient
 * pointers may be NULL (but dL_dmean3D of the depth entry) or receive the gradients.  After a capacity-mode forward that overflowed, nothing
 * per-Gaussian is touched (no gradient, no moment, no parameter, no visible_out) and the three camera outputs are zeros.  Nothing allocates,
 * synchronises or reads back: both calls can be captured in a graph.  P == 0: the three camera outputs are zeroed.
 * GSLIC_ERR_INVALID_ARG before any device work: a NULL camera output, adam == NULL, raw_params = 0, everything gslic_rasterize_backward_adam
 * (gslic_rasterize_backward_depth_adam) and gslic_rasterize_backward_camera (_depth_camera) refuse.  There is no row range and no statistics
 * descriptor on these entries: the camera gradient combines with neither (the shared implementation refuses both).
 */
int gslic_rasterize_backward_camera_adam(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix,
    float* dL_dopacity, float* dL_dmean3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
    float lambda_erank, const gslic_adam_fused* adam,
    float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, float* dL_dmean2D, void* stream);
int gslic_rasterize_backward_depth_camera_adam(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const float* background, const float* means3D, const float* dc, const float* shs, const float* colors_precomp,
    const float* scales, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* cam_pos, const int32_t* radii,
    char* geom_buffer, char* binning_buffer, char* img_buffer, char* sample_buffer, const float* dL_dpix, const float* dL_ddepth,
    float* dL_dopacity, float* dL_dmean3D, float* dL_ddc, float* dL_dsh, float* dL_dscale, float* dL_drot,
    float lambda_erank, const gslic_adam_fused* adam,
    float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, float* dL_dmean2D, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_adam_update — replaces ADAM::adamUpdate / adamUpdateCUDA (cuda_rasterizer/adam.cu:9-66), reached
 * from adamUpdate (rasterize_points.cu:248-273) <- SparseGaussianAdam::custom_step (optim_utils.h:102-137).
 * In place on param / exp_avg / exp_avg_sq, all [N,M]; rows with visible[g]==0 are left untouched.
 * No bias correction, p += -lr*m/(sqrt(v)+eps).  `visible` is one byte per Gaussian (torch bool).
 */
int gslic_adam_update(
    float* param, const float* param_grad, float* exp_avg, float* exp_avg_sq,
    const uint8_t* visible,
    float lr, float b1, float b2, float eps,
    uint32_t N, uint32_t M, void* stream);

/* One launch over several parameter groups (the six groups of gaussian.cpp:399-418) — same arithmetic as
 * n_groups calls of gslic_adam_update; exists to remove five launches and the per-group grad.clone()
 * (optim_utils.h:130).  `groups` is a HOST array. */
typedef struct gslic_adam_group {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    float lr; uint32_t M;
} gslic_adam_group;
int gslic_adam_update_groups(
    const gslic_adam_group* groups, int32_t n_groups,
    const uint8_t* visible, float b1, float b2, float eps, uint32_t N, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_fusedssim_forward / _backward — replace fusedssim / fusedssim_backward and their kernels
 * (src/fused-ssim/ssim.cu:186-441).  Images are [B,CH,H,W]; 11-tap separable Gaussian window, zero padding.
 * Forward writes ssim_map and, when the three dm_* pointers are non-NULL (train=true), the partial
 * derivative maps; all outputs are fully overwritten (no pre-zeroing needed).
 */
int gslic_fusedssim_forward(
    int32_t B, int32_t CH, int32_t H, int32_t W, float C1, float C2,
    const float* img1, const float* img2,
    float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
    void* stream);
int gslic_fusedssim_backward(
    int32_t B, int32_t CH, int32_t H, int32_t W, float C1, float C2,
    const float* img1, const float* img2, const float* dL_dmap,
    const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
    float* dL_dimg1, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_l1_ssim_loss_forward / _backward — SURVEY.md §8f row 2: the loss of optimize() (src/gaussian.cpp:685-691),
 *   loss = (1 - lambda) * mean|img - gt| + lambda * (1 - mean(ssim_map(img, gt))),
 * with l1_loss (loss_utils.h:30-33) folded into the fused-SSIM kernels.  Forward writes the three derivative maps (as
 * gslic_fusedssim_forward with train = 1) and terms[0] = mean|img - gt|, terms[1] = mean ssim (DEVICE floats, reduced in a fixed
 * order: bit-reproducible); `partials` is DEVICE scratch of gslic_loss_partials_count(B,CH,H,W) floats.  Backward writes
 * dL/dimg for dL/dloss = 1: (1-lambda)/N sign(img-gt) - lambda/N (conv(dm_dmu1) + 2 img conv(dm_dsigma1_sq) + gt conv(dm_dsigma12)).
 */
int64_t gslic_loss_partials_count(int32_t B, int32_t CH, int32_t H, int32_t W);
int gslic_l1_ssim_loss_forward(
    int32_t B, int32_t CH, int32_t H, int32_t W, float C1, float C2, const float* img, const float* gt,
    float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, float* partials, float* terms /*[2] device*/, void* stream);
int gslic_l1_ssim_loss_backward(
    int32_t B, int32_t CH, int32_t H, int32_t W, float lambda_dssim, const float* img, const float* gt,
    const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg, void* stream);
/* Both of them as TWO launches instead of three (ABI 7): the fixed-order reduction of the forward's partial sums into `terms` rides on the
 * first workgroup of the backward kernel.  Same bits in the maps, in terms and in dL_dimg as the two calls above. */
int gslic_l1_ssim_loss_forward_backward(
    int32_t B, int32_t CH, int32_t H, int32_t W, float C1, float C2, float lambda_dssim, const float* img, const float* gt,
    float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, float* partials, float* terms /*[2] device*/, float* dL_dimg, void* stream);

/* gslic_l1_ssim_loss_weighted_forward_backward — the same loss and its gradient under a per-pixel weight image (additive, ABI 8; one image,
 * the fused callers never batch).  weight [H,W] float DEVICE, shared by the CH channels; a mask is the 0/1 case.  The kernels read NaN and
 * negative weights as 0 and weights above 1 (+inf included) as 1.  With S = sum_p w_p:
 *   terms[0] = L1_w = sum_p w_p sum_c |img - gt| / (CH S),  terms[1] = SSIM_w = sum_p w_p sum_c ssim_c(p) / (CH S),  terms[2] = S,
 *   dL_dimg = c_l1 w_p sign(img - gt) + fusedssim_backward(dL_dmap = c_ssim w_p),  c_l1 = (1-lambda)/(CH S),  c_ssim = -lambda/(CH S)
 * (each coefficient one float division by the float product CH * S; bit for bit that chain on the entry points above, and with w == 1 the
 * bits of gslic_l1_ssim_loss_forward_backward).  The window statistics are taken over ALL pixels: a window that straddles masked pixels is not
 * re-normalised.  S == 0: terms 0, 0, 0 and dL_dimg all zeros.  THREE launches (forward, a one-workgroup reduction that leaves the coefficients
 * in `partials`, backward), fixed summation order (bit-reproducible), no allocation, no host synchronisation (graph-capturable).
 * `partials`: DEVICE scratch of gslic_l1_ssim_loss_weighted_partials_count(CH, H, W) floats. */
int64_t gslic_l1_ssim_loss_weighted_partials_count(int32_t CH, int32_t H, int32_t W);
int gslic_l1_ssim_loss_weighted_forward_backward(
    int32_t CH, int32_t H, int32_t W, float C1, float C2, float lambda_dssim, const float* img, const float* gt, const float* weight,
    float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, float* partials, float* terms /*[3] device*/, float* dL_dimg, void* stream);

/* gslic_depth_l1_loss_forward_backward — the masked depth L1 of LiDAR depth supervision and its gradient in TWO launches (no reference
 * counterpart): mask = gt_depth > 0, n = number of masked pixels, term[0] = L_d = sum_mask |depth - gt_depth| / max(n, 1) (DEVICE float, fixed-order
 * reduction: bit-reproducible; n is an exact integer count), dL_ddepth [H,W] = (lambda_depth / max(n, 1)) sign(depth - gt_depth) on the mask and 0 off
 * it (sign(0) = 0) — the gradient of lambda_depth * L_d, bit for bit what autograd forms for it.  depth, gt_depth [H,W] device; `partials` is DEVICE
 * scratch of gslic_depth_l1_loss_partials_count(H, W) floats.  No allocation, no host synchronisation (graph-capturable). */
int64_t gslic_depth_l1_loss_partials_count(int32_t H, int32_t W);
int gslic_depth_l1_loss_forward_backward(
    int32_t H, int32_t W, float lambda_depth, const float* depth, const float* gt_depth, float* partials, float* term /*[1] device*/,
    float* dL_ddepth, void* stream);

/* gslic_depth_loss_weighted_forward_backward — the depth loss under a per-pixel weight image and a Huber (smooth-L1) threshold, and its gradient,
 * in TWO launches (additive, ABI 8; no reference counterpart).  depth, gt_depth [H,W] float DEVICE; weight [H,W] float DEVICE or NULL (every
 * pixel weighs 1); delta = the smooth-L1 `beta` in the unit of depth, 0 = plain L1.  Every step below is ONE IEEE float32 operation rounded on its
 * own (no contraction; the divisions are true divisions):
 *   w_p  = weight == NULL ? 1 : (weight_p > 0 && weight_p < +inf ? weight_p : 0)          NaN, negative and +inf weights read as 0
 *   m_p  = gt_p > 0 && w_p > 0                        (a NaN fails: unmeasured; a pixel with w_p = 0 IS an unmeasured pixel, whatever depth_p holds)
 *   r_p  = depth_p - gt_p,  a_p = |r_p|
 *   delta == 0:  rho_p = a_p                                             rho'_p = r_p > 0 ? 1 : (r_p < 0 ? -1 : 0)
 *   delta  > 0:  a_p <  delta:       rho_p = ((0.5 * a_p) * a_p) / delta    rho'_p = r_p / delta
 *                otherwise:          rho_p = a_p - 0.5 * delta              rho'_p = +-1 (0 for r_p = 0 or NaN) as above
 *   S = sum over m_p of w_p,  T = sum over m_p of w_p * rho_p           (float32, in the fixed order below; weight == NULL adds rho_p itself)
 *   terms[0] = L_d = S > 0 ? T / S : 0,   terms[1] = S
 *   k = S > 0 ? lambda_depth / S : 0
 *   dL_ddepth_p = m_p ? (k * w_p) * rho'_p : 0       where rho'_p = +-1: +-(k * w_p), and +0 where it is 0; weight == NULL: k in place of k * w_p
 * The gradient of lambda_depth * L_d; its magnitude never exceeds the L1's.  UNLIKE the colour weight above there is NO clamp at 1: inverse-variance
 * weights are not bounded by 1, and the division by S makes the scale of the weights irrelevant — the difference is deliberate.
 * Order of the sums: workgroups of 2048 consecutive pixels; thread t of 256 adds its pixels t, t + 256, ... in that order, the 256 thread sums go
 * through a xor-shuffle tree (distances 32 ... 1) per 64 lanes and (r0 + r1) + (r2 + r3) over the four; the per-workgroup partials b are added
 * the same way (thread t takes b = t, t + 256, ...).  That is the order of gslic_depth_l1_loss_forward_backward: with weight == NULL or all ones
 * and delta == 0, S is a sum of ones (exact below 2^24 pixels) and terms[0] and dL_ddepth have the bits of that entry point.
 * No atomics, no allocation, no host synchronisation: graph-capturable and bit-reproducible.  `partials`: DEVICE scratch of
 * gslic_depth_loss_weighted_partials_count(H, W) floats.  GSLIC_ERR_INVALID_ARG before any device work, naming the argument, for H or W <= 0, a
 * NULL depth / gt_depth / partials / terms / dL_ddepth, a delta that is negative, NaN or +inf, a NaN lambda_depth, and a dL_ddepth or terms that
 * overlaps depth, gt_depth or weight. */
int64_t gslic_depth_loss_weighted_partials_count(int32_t H, int32_t W);
int gslic_depth_loss_weighted_forward_backward(
    int32_t H, int32_t W, float lambda_depth, float delta, const float* depth, const float* gt_depth, const float* weight /*or NULL*/,
    float* partials, float* terms /*[2] device*/, float* dL_ddepth, void* stream);

/* gslic_exposure_apply / gslic_exposure_backward — the per-view exposure model: a 3x4 affine colour transform E applied to the rendered image before
 * the loss, and its gradient (additive, ABI 8; the reference creates, optimises and never applies such a tensor: gaussian.cpp:287-291, renderer.cpp:25).
 * image, out, dL_dout, dL_dimage: planar [3,H,W] float DEVICE; E: 12 floats DEVICE, row-major [3,4] (E[c,k] at 4 c + k).  Every product and sum
 * below is ONE IEEE float32 operation rounded on its own, in the order the parentheses give (no contraction).  With x = (r, g, b) the pixel of `image`
 * and g_c the pixel of dL_dout in channel c:
 *   out_c       = ((E[c,0] * r + E[c,1] * g) + E[c,2] * b) + E[c,3]                                    gslic_exposure_apply
 *   dL_dimage_k = ((E[0,k] * g_0 + E[1,k] * g_1) + E[2,k] * g_2)                                        gslic_exposure_backward, k = 0..2
 *   dL_dE[c,k]  = sum over the pixels p of g_c(p) * x_k(p)  (k < 3),   dL_dE[c,3] = sum over p of g_c(p)     x is `image`, the model's INPUT
 * Order of the twelve sums, a function of H * W alone (not of the device's CU count, not of the pointers): workgroups of 2048 consecutive pixels;
 * thread t of 256 adds, onto +0, the products of its pixels 4 (t + 256 j) + e in the order j = 0, 1 and e = 0 .. 3 within j (pixels at or past
 * H * W add nothing); the 256 thread sums go through a xor-shuffle tree (distances 32 ... 1) per 64 lanes and (r0 + r1) + (r2 + r3) over the four
 * waves; workgroup b stores its twelve sums as row b of `partials`.  A second launch of ONE workgroup adds the rows: thread t takes the rows t,
 * t + 256, ... in that order, then the same tree.  No atomics: dL_dE has the same bits on every run and every device, whatever `partials` held
 * before.  `partials`: DEVICE scratch of gslic_exposure_partials_count(H, W) floats (12 per workgroup).  Each call reads and writes every pixel
 * once — 24 and 36 bytes per pixel — with 16-byte accesses (dword-aligned ones unless H * W % 4 == 0 and the images are 16-byte aligned; the one
 * group of four that crosses the end of the image pixel by pixel); apply is one launch, backward two; no allocation, no host synchronisation, no
 * read-back: capturable in a graph.
 *
 * adam (optional): the second launch also updates E in place — row *view of the [V,12] / [V] DEVICE arrays, *view read ON THE DEVICE so that a
 * captured graph can change views — by torch.optim.Adam's rule WITH bias correction (what the reference's torch::optim::Adam of exposure_ applies;
 * NOT the map's uncorrected sparse Adam), per element with g = dL_dE[c,k]:
 *   t = step_count[view] + 1, stored back;   b1 = 1 - beta1^t,  b2 = 1 - beta2^t      in DOUBLE from the integer t (beta as the float given)
 *   s = (float)(lr / b1),  q = (float)sqrt(b2)                                        in double, each rounded to float once
 *   m = beta1 * m + (1 - beta1) * g,   v = beta2 * v + ((1 - beta2) * g) * g,   p = p - (s * m) / (sqrtf(v) / q + eps)       float32, as written
 * A host that applies E of the row the update will change passes E = param + 12 * view to both calls (a POINTER, not a view index: the first
 * launch of the backward reads E before the second one updates it).  skip (optional): a DEVICE word, e.g. &status[2] of the capacity-mode forward
 * whose image this is — when one of its bits 1 | 2 | 8 | 16 is set (that forward did not complete, the step is a no-op) nothing is updated; dL_dE
 * is still written.
 * GSLIC_ERR_INVALID_ARG before any device work, naming the argument, for H or W <= 0, a NULL E / image / out (apply) or E / image / dL_dout /
 * dL_dimage / partials / dL_dE (backward), an `out` that overlaps image or E, a dL_dimage or dL_dE that overlaps E, image or dL_dout (or each
 * other), an Adam descriptor with a NULL param / m / v / step_count / view, and one whose lr, beta1, beta2 or eps is NaN or negative or whose
 * beta1 or beta2 is >= 1. */
typedef struct gslic_exposure_adam {
    float* param;              /* [V,12] */
    float* m;                  /* [V,12] exp_avg */
    float* v;                  /* [V,12] exp_avg_sq */
    int32_t* step_count;       /* [V] */
    const int32_t* view;       /* [1] the row to update */
    float lr, beta1, beta2, eps;
    const uint32_t* skip;      /* optional [1]: see above */
} gslic_exposure_adam;
int64_t gslic_exposure_partials_count(int32_t H, int32_t W);
int gslic_exposure_apply(int32_t H, int32_t W, const float* E /*[12] device*/, const float* image, float* out, void* stream);
int gslic_exposure_backward(
    int32_t H, int32_t W, const float* E /*[12] device*/, const float* image, const float* dL_dout, float* dL_dimage, float* partials,
    float* dL_dE /*[12] device*/, const gslic_exposure_adam* adam /*or NULL*/, void* stream);

/* gslic_keyframe_encode / gslic_keyframe_decode — the keyframe store: ground-truth images kept on the device as the 8-bit pixels the camera
 * delivered, decoded into the float32 target of a pyramid level (additive, ABI 8; the reference keeps every keyframe as a float32 CPU tensor and
 * uploads it at every step: gaussian.cpp:49, :80, :678).  Three rules, each reproducible bit for bit from numpy (tests/keyframe_ref.py):
 *
 * STORAGE.  color_slab: uint8 [capacity, H, W, 3] DEVICE, interleaved RGB (pixel (x, y) of slot s, channel c at ((s H + y) W + x) 3 + c: what a
 * camera driver or OpenCV delivers, up to the channel order).  mask_slab (optional): uint8 [capacity, H, W] DEVICE.
 *
 * DECODE at level l, 0 <= l <= GSLIC_KEYFRAME_MAX_LEVEL: W_l = W >> l, H_l = H >> l (either 0: GSLIC_ERR_INVALID_ARG); the remainder columns on the
 * right and the remainder rows at the bottom are dropped.  Output pixel (X, Y) of channel c:
 *   out[c, Y, X] = (float)S * c_l,   S = the INTEGER sum of the 4^l bytes of channel c in the block [X 2^l, (X+1) 2^l) x [Y 2^l, (Y+1) 2^l),
 *   c_l = (1.0f / 255.0f) * 2^(-2 l)          (the float32 quotient, scaled exactly)
 * S <= 255 * 256 is exact in float32, so the rule is ONE float32 multiply per value.  The mask decodes by the same rule into weight_out, float32
 * [H_l, W_l]: a per-pixel weight image as gslic_l1_ssim_loss_weighted_forward_backward takes it.  out: planar float32 [3, H_l, W_l].  The slot is
 * read from the DEVICE word *frame, so a captured graph changes targets without a host copy; a word outside [0, n_frames) makes the launch write
 * NOTHING (a host validates the index before it fills the word).  One launch writes colour and, with mask_slab != NULL, the weight.  A lane owns
 * four consecutive output pixels where W % (4 << l) == 0 (aligned 4- / 8- / 16-byte non-temporal loads of the slab, one 16-byte store per plane),
 * one pixel otherwise.  No atomics, no allocation, no read-back: capturable in a graph.
 *
 * ENCODE.  image: planar float32 [3, H, W] DEVICE -> slot `slot` of color_slab; mask: float32 [H, W] DEVICE -> slot `slot` of mask_slab (either
 * pair may be NULL, not both).  Per value x:
 *   x' = x > 0 ? (x < 1 ? x : 1) : 0          (NaN reads as 0, -0 as 0, +inf as 1)
 *   q  = (uint8) floorf((x' * 255.0f) + 0.5f)  the product rounded to float32 on its own (never contracted into the add), then the add, then floor
 * Round trip: with d(v) = (float)v * c_0 the decoded value of byte v, encode(d(v)) == v for all 256 values, and so does encode of the float32
 * quotient v / 255.0f (which differs from d(v) in the last bit for 126 of them): decode(encode(x)) == d(v) bit for bit for either x.
 *
 * CAMERA at level l (the host's part; Camera.at_level in camera.py): width W_l, height H_l, fx / 2^l, fy / 2^l, cx / 2^l, cy / 2^l — all four exact
 * in float32 — and the pose, znear and zfar unchanged.  The continuous image coordinate u = fx x / z + cx spans [0, W) in this library's convention
 * (P[0,2] = (2 cx - W) / W; the floor of gslic_lidar_zbuffer_add), so halving u is the whole change: a point's level-l pixel is
 * floor(pixel_0 / 2^l) exactly, and it is dropped exactly when that lands in a remainder column or row.
 *
 * GSLIC_ERR_INVALID_ARG before any device work, naming the argument: W or H <= 0, a level outside [0, GSLIC_KEYFRAME_MAX_LEVEL], W_l or H_l of 0,
 * a NULL color_slab / frame / out (decode), mask_slab != NULL with weight_out == NULL, n_frames < 0, an out / weight_out / color_slab / mask_slab
 * that is not 16-byte aligned, an image that is not 4-byte aligned; (encode) capacity <= 0, a slot outside [0, capacity), image and mask both
 * NULL, an image without color_slab or a mask without mask_slab. */
#define GSLIC_KEYFRAME_MAX_LEVEL 4
int gslic_keyframe_decode(
    int32_t W, int32_t H, int32_t level, const uint8_t* color_slab, const uint8_t* mask_slab /*or NULL*/, const int32_t* frame /*[1] device*/,
    int32_t n_frames, float* out /*[3,H_l,W_l]*/, float* weight_out /*[H_l,W_l], with mask_slab*/, void* stream);
int gslic_keyframe_encode(
    int32_t W, int32_t H, const float* image /*[3,H,W] or NULL*/, const float* mask /*[H,W] or NULL*/, uint8_t* color_slab, uint8_t* mask_slab,
    int32_t capacity, int32_t slot, void* stream);

/* gslic_keyframe_encode_depth / gslic_keyframe_decode_depth — the keyframe store's LiDAR depth: one range image per slot kept as 16-bit codes (and
 * an optional 8-bit confidence weight), decoded into the float32 depth target (and depth weight) of a pyramid level (additive, ABI 8).  Three rules,
 * each reproducible bit for bit from numpy (tests/keyframe_depth_ref.py):
 *
 * STORAGE.  depth_slab: uint16 [capacity, H, W] DEVICE.  Code 0 = not measured; code k >= 1 = depth k * step.  step: float32, a power of two 2^e
 * with -16 <= e <= 0, the caller's choice and fixed per store (2^-9 m: 1.95 mm resolution, 127.998 m range); anything else is
 * GSLIC_ERR_INVALID_ARG.  dweight_slab (optional): uint8 [capacity, H, W] DEVICE.
 *
 * ENCODE.  depth: float32 [H, W] DEVICE -> slot `slot` of depth_slab; weight: float32 [H, W] DEVICE or NULL -> slot `slot` of dweight_slab.
 *   d is measured iff d > 0 and d is finite            (NaN, -x, +-0 and +inf are not)
 *   t = d * (1 / step)                                  exact: 1 / step is a power of two
 *   k = floorf(t + 0.5f)
 *   code = k if 1 <= k <= 65535, else 0                 a depth below half a step and one beyond the range read as NOT MEASURED, never as a clamped depth
 * A weight x is quantised by the mask's rule of gslic_keyframe_encode: x' = x clamped to [0, 1] (NaN -> 0), (uint8) floorf((x' * 255.0f) + 0.5f),
 * the product rounded on its own.  With a dweight_slab and weight == NULL the slot's weights are all 255.
 *
 * DECODE at level l (levels, W_l, H_l, the block [X 2^l, (X+1) 2^l) x [Y 2^l, (Y+1) 2^l) and the dropped remainder columns and rows as for
 * gslic_keyframe_decode).  Every block pixel with code c != 0 has the key
 *   key = c                                 without a dweight_slab
 *   key = (c << 8) | (255 - wcode)          with one
 * and m = the UNSIGNED MINIMUM of the block's keys: the nearest return, and among pixels that share its code the one of the largest weight, so the
 * result does not depend on a pixel's position inside its block.
 *   depth_out[Y, X]   = (float)code(m) * step                             exact (16 bits times a power of two); code(m) = m, or m >> 8
 *   dweight_out[Y, X] = (float)(255 - (m & 255)) * (1.0f / 255.0f)        the mask's level-0 value d(v)
 * and both are 0 where the block holds no measured pixel.  The slot is read from the DEVICE word *frame as in gslic_keyframe_decode: a word outside
 * [0, n_frames) writes NOTHING.
 *
 * PROPERTIES.  decode_0(encode(D)) == the code-rounded D.  decode_l(encode(D)) == positive_min_pool(decode_0(encode(D)), l): the minimum of codes is
 * taken on integers, ahead of the one multiply, and k -> k * step is monotonic.  The level-l LiDAR range image of Camera.at_level(l) is the
 * positive-minimum pool of the level-0 image (a point's level-l pixel is floor(pixel_0 / 2^l)), and rounding to codes is monotonic, so decode_l of an
 * encoded level-0 range image equals the code-rounded range image of the level-l camera: ONE stored image serves every level.
 *
 * Both calls are one launch, shaped like the colour pair: where W % (4 << l) == 0 a lane of the decode owns four consecutive output pixels (per
 * source row 8 << l bytes of codes and 4 << l bytes of weights in aligned 4- / 8- / 16-byte non-temporal loads, four running minima, one 16-byte
 * store per plane), one pixel otherwise; the encode takes four pixels per lane where H W % 4 == 0 and the images are 16-byte aligned (one 8-byte
 * store of codes, one dword of weights), one otherwise.  No atomics, no allocation, no read-back: capturable in a graph.
 *
 * GSLIC_ERR_INVALID_ARG before any device work, naming the argument: W or H <= 0, a level outside [0, GSLIC_KEYFRAME_MAX_LEVEL], W_l or H_l of 0,
 * n_frames < 0, a step that is not such a power of two, a NULL depth_slab / frame / depth_out (decode), dweight_slab != NULL with dweight_out == NULL,
 * a depth_out / dweight_out / depth_slab / dweight_slab that is not 16-byte aligned; (encode) capacity <= 0, a slot outside [0, capacity), a NULL
 * depth or depth_slab, a weight without dweight_slab, a depth or weight that is not 4-byte aligned, a slab that is not 16-byte aligned. */
int gslic_keyframe_decode_depth(
    int32_t W, int32_t H, int32_t level, const uint16_t* depth_slab, const uint8_t* dweight_slab /*or NULL*/, const int32_t* frame /*[1] device*/,
    int32_t n_frames, float step, float* depth_out /*[H_l,W_l]*/, float* dweight_out /*[H_l,W_l], with dweight_slab*/, void* stream);
int gslic_keyframe_encode_depth(
    int32_t W, int32_t H, const float* depth /*[H,W]*/, const float* weight /*[H,W] or NULL*/, uint16_t* depth_slab, uint8_t* dweight_slab /*or NULL*/,
    int32_t capacity, int32_t slot, float step, void* stream);

/* gslic_pose_step / gslic_pose_load — a set of trainable keyframe poses on the device (additive, ABI 8; the reference optimises no pose:
 * rasterizer.cpp:171-182 drops the camera gradient).  Per view i the set holds view[i,16], proj[i,16] and campos[i,3] in exactly the layout and
 * meaning of the viewmatrix, projmatrix and cam_pos arguments of the rasteriser (element (r, c) at [4 c + r]; V = [R | t; 0 0 0 1] the world-to-camera
 * matrix, proj = Pm V, campos = -R^T t), the Adam moments m[i,6], v[i,6] and the step count steps[i]; once per set the pose-independent projection
 * Pm[16] (same layout).  gslic_pose_step is ONE launch of one wave on row *view, read ON THE DEVICE so that a captured graph can change views.
 * Every product and sum below is ONE IEEE float32 operation rounded on its own, in the order the parentheses give (no contraction; sums of
 * products run over k ascending, ((p0 + p1) + p2) + p3), except where DOUBLE is named.  One lane runs the whole rule: no sum depends on a
 * reduction order.  With Gv(r,c) = dL_dviewmatrix[4 c + r], Gp(r,c) = dL_dprojmatrix[4 c + r], gc = dL_dcampos:
 *
 * CHAIN (Camera.pose_gradient of camera.py, term by term), r = 0..2:
 *   G(r,c)  = Gv(r,c) + (((Pm(0,r) Gp(0,c) + Pm(1,r) Gp(1,c)) + Pm(2,r) Gp(2,c)) + Pm(3,r) Gp(3,c))                    c = 0..3
 *   GR(r,c) = G(r,c) - t_r gc_c   (c = 0..2),      Gt_r = G(r,3) - ((R(r,0) gc_0 + R(r,1) gc_1) + R(r,2) gc_2)
 *   M(r,c)  = (GR(r,0) R(c,0) + GR(r,1) R(c,1)) + GR(r,2) R(c,2)
 *   g = (Gt_0, Gt_1, Gt_2,  (M(2,1) - M(1,2)) + (t_1 Gt_2 - t_2 Gt_1),  (M(0,2) - M(2,0)) + (t_2 Gt_0 - t_0 Gt_2),  (M(1,0) - M(0,1)) + (t_0 Gt_1 - t_1 Gt_0))
 * g — dL/d(rho, phi) of the LEFT increment T_cw <- exp((rho, phi)^) T_cw — is ALWAYS written to grad_out[6].
 *
 * ADAM (torch.optim.Adam WITH bias correction, as gslic_exposure_backward states it), per coordinate k with lr_k = lr_trans (k < 3) or lr_rot:
 *   n = steps[view] + 1, stored back;   b1 = 1 - beta1^n,  b2 = 1 - beta2^n               in DOUBLE from the integer n (beta as the float given)
 *   s_k = (float)(lr_k / b1),  q = (float)sqrt(b2)                                        in double, each rounded to float once
 *   m = beta1 m + (1 - beta1) g,   v = beta2 v + ((1 - beta2) g) g,   delta_k = -((s_k m) / (sqrtf(v) / q + eps))
 *
 * RETRACTION T_cw <- exp(delta^) T_cw (se3_exp of camera.py), rho = delta[0..2], phi = delta[3..5] = (x, y, z):
 *   theta^2 = (x x + y y) + z z,  theta = sqrt(theta^2)                                  in DOUBLE from the float phi
 *   theta <  GSLIC_POSE_SERIES_THETA:  a = 1 - theta^2 / 6,  b = 1/2 - theta^2 / 24,  c = 1/6 - theta^2 / 120
 *   otherwise:                         a = sin(theta) / theta,  b = (1 - cos(theta)) / theta^2,  c = (theta - sin(theta)) / (theta^2 theta)
 *                                                                                        in DOUBLE, each rounded to float once
 *   K = phi^ = [0 -z y; z 0 -x; -y x 0],   K2 = [-(y y + z z)  x y  x z;  x y  -(x x + z z)  y z;  x z  y z  -(x x + y y)]
 *   Rm(r,c) = (I(r,c) + a K(r,c)) + b K2(r,c),   Vm(r,c) = (I(r,c) + b K(r,c)) + c K2(r,c),   Et_r = (Vm(r,0) rho_0 + Vm(r,1) rho_1) + Vm(r,2) rho_2
 *   R'(r,c) = (Rm(r,0) R(0,c) + Rm(r,1) R(1,c)) + Rm(r,2) R(2,c),   t'_r = ((Rm(r,0) t_0 + Rm(r,1) t_1) + Rm(r,2) t_2) + Et_r
 * RE-ORTHONORMALISATION (Gram-Schmidt on the rows of R' in the order 0, 1; row 2 is their cross product, so det R = +1 and thousands of steps
 * accumulate no drift):
 *   r0 = R'[0] / sqrtf((R'(0,0)^2 + R'(0,1)^2) + R'(0,2)^2)
 *   u  = R'[1] - d r0,  d = (r0_0 R'(1,0) + r0_1 R'(1,1)) + r0_2 R'(1,2);     r1 = u / sqrtf((u_0^2 + u_1^2) + u_2^2)
 *   r2 = (r0_1 r1_2 - r0_2 r1_1,  r0_2 r1_0 - r0_0 r1_2,  r0_0 r1_1 - r0_1 r1_0)
 * RECOMPOSITION with V = [r0; r1; r2 | t'; 0 0 0 1]:
 *   view[4 c + r] = V(r,c);   proj[4 c + r] = ((Pm(r,0) V(0,c) + Pm(r,1) V(1,c)) + Pm(r,2) V(2,c)) + Pm(r,3) V(3,c);
 *   campos_c = -((V(0,c) t'_0 + V(1,c) t'_1) + V(2,c) t'_2)
 * A row the host loaded and no step moved keeps the host's bits.
 *
 * NO-OPS.  skip (optional DEVICE word, the bits of gslic_exposure_adam.skip: one of 1 | 2 | 8 | 16 set): nothing but grad_out is written.  A
 * coordinate of g that is not finite: nothing but grad_out is written, steps is not advanced.  delta zero in all six coordinates (a zero gradient
 * on zero moments, or both rates 0), or a coordinate of delta that is not finite (eps = 0 on a zero second moment): m, v and steps are updated,
 * view / proj / campos are not rewritten.  *view outside [0, n_views): nothing at all is written.
 * No atomics, no allocation, no read-back: capturable in a graph.  All stores are vector stores.
 * GSLIC_ERR_INVALID_ARG before any device work, naming the argument: a NULL descriptor, member (skip excepted), gradient or grad_out;
 * n_views <= 0; a gradient array or grad_out that overlaps a state array (the [n_views, ...] extents), or grad_out one of the gradients; lr_trans,
 * lr_rot, beta1, beta2 or eps NaN or negative; beta1 or beta2 >= 1.
 *
 * gslic_pose_load copies row *view_word — 35 floats — of the three pose arrays into three caller-owned DEVICE buffers in one launch: how a
 * captured step reads "the pose of the view the word names".  A word outside [0, n_views) writes NOTHING.  GSLIC_ERR_INVALID_ARG for a NULL
 * pointer, n_views <= 0, or an output that overlaps an input or another output. */
#define GSLIC_POSE_SERIES_THETA 1e-4
typedef struct gslic_pose_adam {
    float* view_all;           /* [V,16] */
    float* proj_all;           /* [V,16] */
    float* campos_all;         /* [V,3]  */
    float* m;                  /* [V,6] exp_avg of (rho, phi) */
    float* v;                  /* [V,6] exp_avg_sq */
    int32_t* step_count;       /* [V] */
    const float* projection;   /* [16] Pm, shared by the views */
    const int32_t* view;       /* [1] the row to step */
    int32_t n_views;           /* V */
    float lr_trans, lr_rot, beta1, beta2, eps;
    const uint32_t* skip;      /* optional [1]: see above */
} gslic_pose_adam;
int gslic_pose_step(
    const gslic_pose_adam* d, const float* dL_dviewmatrix /*[16]*/, const float* dL_dprojmatrix /*[16]*/, const float* dL_dcampos /*[3]*/,
    float* grad_out /*[6]*/, void* stream);
int gslic_pose_load(
    const float* view_all, const float* proj_all, const float* campos_all, const int32_t* view_word /*[1] device*/, int32_t n_views,
    float* view_out /*[16]*/, float* proj_out /*[16]*/, float* campos_out /*[3]*/, void* stream);

/* gslic_pose_step_shared / gslic_pose_calibrate_rows — the calibration the views of a pose set SHARE (additive, ABI 8): a correction of the
 * camera-body extrinsic and of the camera clock offset.  A left increment T_cw <- exp(d^) T_cw acts in the camera frame, so the gradient g of
 * gslic_pose_step for the rendered view is, unchanged, the gradient of an extrinsic correction every view takes; with the camera-frame twist
 * xi_j = (v, w) of view j (m/s, rad/s; T_cw(t + dt) ~ exp((dt xi)^) T_cw(t)) the product xi_i . g is the gradient of a common time offset.  Per set,
 * beside the three pose arrays and Pm of gslic_pose_step: twist[V,6], the Adam moments sm[7], sv[7] and the step count ssteps[1] of
 * (rho_x, phi_x, tau), the accumulated extrinsic correction X[12] (ROWS of [R_x | t_x]: element (r, c) at [4 r + c]; the identity at the start) and
 * the accumulated time offset tau[1] in seconds.  The per-view moments of gslic_pose_adam are neither read nor written.
 * gslic_pose_step_shared is ONE launch of ONE workgroup.  Every product and sum below is ONE IEEE float32 operation rounded on its own, in the order
 * the parentheses give, except where DOUBLE is named.  One thread runs CHAIN and ADAM; then each thread runs the whole MOVE of the rows it takes,
 * alone: no sum depends on a reduction order, and no row's result depends on V.
 *
 * CHAIN: gslic_pose_step's CHAIN on row i = *view, term for term, gives g[0..5]; then with xi = twist[i]
 *   g_tau = ((((g_0 xi_0 + g_1 xi_1) + g_2 xi_2) + g_3 xi_3) + g_4 xi_4) + g_5 xi_5
 * (g, g_tau) is ALWAYS written to grad_out[7].
 *
 * ADAM: gslic_pose_step's ADAM on the seven coordinates k of (g, g_tau), on sm, sv, with lr_k = lr_trans (k < 3), lr_rot (3 <= k < 6), lr_time (k = 6):
 *   n = ssteps[0] + 1, stored back;   b1 = 1 - beta1^n,  b2 = 1 - beta2^n               in DOUBLE from the integer n (beta as the float given)
 *   s_k = (float)(lr_k / b1),  q = (float)sqrt(b2)                                        in double, each rounded to float once
 *   m = beta1 sm_k + (1 - beta1) g_k,   v = beta2 sv_k + ((1 - beta2) g_k) g_k,   delta_k = -((s_k m) / (sqrtf(v) / q + eps))
 * d_x = delta[0..5], d_tau = delta[6].
 *
 * MOVE, for EVERY row j in [0, V):   d_j[k] = d_x[k] + d_tau xi_j[k]   (k = 0..5; one product, one sum), then gslic_pose_step's RETRACTION with
 * delta = d_j, RE-ORTHONORMALISATION and RECOMPOSITION on row j — the same formulas, constants and GSLIC_POSE_SERIES_THETA.
 *   X   <- the same RETRACTION by d_x and RE-ORTHONORMALISATION on the 3x4 [R_x | t_x] alone (no recomposition)
 *   tau <- tau + d_tau
 *
 * NO-OPS, row by row those of gslic_pose_step.  skip set (its bits 1 | 2 | 8 | 16): nothing but grad_out is written.  A coordinate of g or g_tau
 * that is not finite: nothing but grad_out is written, ssteps is not advanced.  Otherwise sm, sv and ssteps are updated, and: a row whose d_j is zero
 * in all six coordinates keeps its bits; a row whose d_j has a coordinate that is not finite keeps its bits; X keeps its bits when d_x is zero in
 * all six coordinates or has a coordinate that is not finite; tau keeps its bits when d_tau is zero or not finite.  *view outside [0, n_views):
 * nothing at all is written.
 * No atomics, no allocation, no read-back: capturable in a graph.  All stores are vector stores.
 * GSLIC_ERR_INVALID_ARG before any device work, naming the argument: a NULL descriptor, member (skip excepted), gradient or grad_out;
 * n_views <= 0; a gradient array or grad_out that overlaps a state array, or grad_out one of the gradients; lr_trans, lr_rot, lr_time, beta1, beta2
 * or eps NaN or negative; beta1 or beta2 >= 1.
 *
 * gslic_pose_calibrate_rows brings freshly loaded rows to the calibration the older rows were moved to.  This is a DEFINITION, first order in tau:
 * for every row j in [first, first + count), one thread per row,
 *   A_R(r,c) = (X(r,0) R(0,c) + X(r,1) R(1,c)) + X(r,2) R(2,c),   A_t_r = ((X(r,0) t_0 + X(r,1) t_1) + X(r,2) t_2) + X(r,3)          A = X T
 *   d[k] = tau xi_j[k]                                                                                                              k = 0..5
 *   T <- RETRACTION of [A_R | A_t] by d, RE-ORTHONORMALISATION, RECOMPOSITION (always run: d = 0 is the exact identity exp)
 * A row whose d has a coordinate that is not finite keeps its bits; rows outside the range are not touched.  With lr_time = 0 the result is, up to
 * rounding, the pose a row loaded from the same camera before the steps was moved to (X is the ordered product of their exp(d_x^)).  With
 * lr_time != 0 it composes ONE exp(tau xi_j) where the older rows took a product of exp(d_x + d_tau xi_j): equal to first order in the increments.
 * Reads view_all / proj_all / campos_all, projection, twist, X and tau of the descriptor (the other members may be NULL).
 * GSLIC_ERR_INVALID_ARG: a NULL descriptor or one of those members; n_views <= 0; first or count negative, or first + count > n_views.  count = 0 is
 * a no-op. */
typedef struct gslic_pose_shared {
    float* view_all;           /* [V,16] */
    float* proj_all;           /* [V,16] */
    float* campos_all;         /* [V,3]  */
    const float* projection;   /* [16] Pm, shared by the views */
    const int32_t* view;       /* [1] the row whose gradient this is */
    int32_t n_views;           /* V */
    const float* twist;        /* [V,6] camera-frame twist (v, w) of each view */
    float* sm;                 /* [7] exp_avg of (rho_x, phi_x, tau) */
    float* sv;                 /* [7] exp_avg_sq */
    int32_t* ssteps;           /* [1] */
    float* X;                  /* [12] rows of [R_x | t_x] */
    float* tau;                /* [1] seconds */
    float lr_trans, lr_rot, lr_time, beta1, beta2, eps;
    const uint32_t* skip;      /* optional [1]: as gslic_pose_adam.skip */
} gslic_pose_shared;
int gslic_pose_step_shared(
    const gslic_pose_shared* d, const float* dL_dviewmatrix /*[16]*/, const float* dL_dprojmatrix /*[16]*/, const float* dL_dcampos /*[3]*/,
    float* grad_out /*[7]*/, void* stream);
int gslic_pose_calibrate_rows(const gslic_pose_shared* d, int32_t first, int32_t count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_knn_mean_dist2 — replaces SimpleKNN::knn (src/simple-knn/simple_knn.cu:185-221) behind distCUDA2
 * (src/simple-knn/spatial.cu:15-26): mean_dists[i] = mean of the 3 smallest squared distances from point i
 * to the other points (FLT_MAX stands in for a missing neighbour when P < 4, as in the reference).
 * Scratch comes from the caller's allocator (the reference cudaMalloc's internally, simple_knn.cu:187-216).
 */
int gslic_knn_mean_dist2(
    int32_t P, const float* points, float* mean_dists,
    gslic_alloc_fn scratch_alloc, void* scratch_ctx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_extend_select / gslic_extend_emit — SURVEY.md §8f row 1: the device-side replacement of the point selection inside
 * extend() (src/gaussian.cpp:536-603; CPU unordered_map<string,...> dedupe at :557-572) and of the construction of the new
 * Gaussians' parameter rows (:605-626).  The caller renders the latest camera with no_color = 1 first (final_T, :501-507).
 *
 *  select: points [n,3] world, depths_rsp [n] (sensor range, :534), R_cw [9] row-major and t_cw [3] (DEVICE), intrinsics,
 *          final_T [H,W].  A point survives iff it is the nearest (smallest camera z, lowest index on ties) of the points
 *          falling into its pixel, the pixel is inside the image, depths_rsp > 0 and 1 - final_T < 0.99.
 *          Returns *count (host; the call synchronises the stream once) and two device arrays inside the scratch buffer:
 *          keep_flags [n] (0/1) and keep_pos [n] (exclusive rank among survivors, ascending point index — the reference's
 *          order is unordered_map iteration order, i.e. unspecified).
 *  emit:   writes `count` rows at the given row pointers (= the model's tensors offset to row P): xyz = point,
 *          dc = (colour - 0.5)/C0, rest = 0 [M,3], opacity = inverse_sigmoid(0.1), scaling = log(scaling_scale*range/focal) x3,
 *          rotation = (1,0,0,0).  Growing the tensors (densificationPostfix, :426-497) stays with the host.
 */
int gslic_extend_select(
    int32_t n, const float* points, const float* depths_rsp, const float* R_cw, const float* t_cw,
    float fx, float fy, float cx, float cy, int32_t width, int32_t height, const float* final_T,
    gslic_alloc_fn scratch_alloc, void* scratch_ctx,
    uint32_t** keep_flags, uint32_t** keep_pos, int32_t* count, void* stream);
int gslic_extend_emit(
    int32_t n, const uint32_t* keep_flags, const uint32_t* keep_pos, const float* points, const float* colors,
    const float* depths_rsp, float scaling_scale, float focal, int32_t M,
    float* xyz, float* dc, float* rest, float* opacity, float* scaling, float* rotation, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_lidar_zbuffer_add / gslic_lidar_zbuffer_resolve / gslic_lidar_zbuffer_resolve_weighted — the per-pixel LiDAR range image on the device:
 * what gt_depth (depth supervision, the pose gradient under depth), depth_weight (the weighted depth loss) and near_bound
 * (gslic_contribution_accumulate_free_space) are made from.  The reference's host builds it on the CPU
 * (a device-to-host copy of every point and an unordered_map keyed by "x_y" strings, gaussian.cpp:554-572); a LibTorch host needs about twenty
 * elementwise launches and scatter_reduce_(amin).  Both calls work on a CALLER-OWNED z-buffer zbuf of width * height uint64 on the DEVICE, one
 * key per pixel (row-major, pixel (x, y) at y * width + x): the all-ones word = empty, otherwise (float bits of z) << 32 | point index.
 *
 *  add:     with clear != 0 the buffer is first set to all ones.  Then one thread per point i < n; the rule is EXACT — every step below is ONE
 *           IEEE float32 operation rounded on its own (no contraction, true divisions), left to right, so the same steps in any IEEE float32
 *           arithmetic give the same image bit for bit.  points [n,3] world, R_cw [9] row-major and t_cw [3] on the DEVICE:
 *
 *             c_k = p_0 * R_cw[3k] + p_1 * R_cw[3k+1] + p_2 * R_cw[3k+2] + t_cw[k]      (k = 0, 1, 2;  z = c_2)
 *             the point is dropped unless z > 0 and z < +inf                             (z <= 0, NaN and +inf are dropped)
 *             xf = floor((c_0 * fx) / z + cx);   yf = floor((c_1 * fy) / z + cy)
 *             the point is dropped unless 0 <= xf < width and 0 <= yf < height           (compared as floats; a NaN fails)
 *             zbuf[yf * width + xf] = min(zbuf[...], (uint64) bits(z) << 32 | (uint32) (index_base + i))       (one 64-bit integer atomic)
 *
 *           The bits of a positive float order like its value, so the smallest z wins a pixel and equal z goes to the lowest index, whatever
 *           order the points arrive in.  Calls with clear == 0 accumulate further sweeps (each with its own pose) into the same image;
 *           index_base keeps their indices apart.  n == 0 with clear != 0 is valid and leaves an empty image.
 *  resolve: per pixel, key = the minimum of zbuf over the (2 footprint + 1) x (2 footprint + 1) window around the pixel, clipped to the image
 *           (footprint in [0, 8]; 0 reads the pixel's own key): the nearest return inside the window, a CONSERVATIVE footprint of sparse
 *           returns (how wide to make it is the host's policy).  Outputs on the DEVICE, [height, width] row-major, each may be NULL, at
 *           least one must not be:
 *             depth_out float32   the float whose bits are key >> 32;                          0 where key is empty
 *             index_out int32     (int32) (uint32) key;                                        -1 where key is empty
 *             near_out  float32   d - (margin_abs + margin_rel * d) of that depth d — one product, one add, one subtraction, each rounded on
 *                                 its own; a bound <= 0 is written as it is;                   0 where key is empty
 *           n_measured_out: optional DEVICE uint32; the call zeroes it on the stream and every workgroup adds its number of non-empty
 *           resolved pixels with one integer atomic (exact, independent of order).  zbuf is only read.
 *  Neither call allocates, synchronises or reads anything back (graph-capturable); no float atomics.  Refused with GSLIC_ERR_INVALID_ARG before
 *  any device work, the message naming the argument: n < 0; width <= 0 or height <= 0; a NULL zbuf; NULL points, R_cw or t_cw with n > 0;
 *  index_base < 0 or index_base + n > 2^31 - 1; footprint outside [0, 8]; a margin that is negative or NaN; depth_out, index_out and near_out
 *  all NULL; an output (n_measured_out included) whose bytes overlap zbuf's.  With N > 1 GPUs every rank calls both with identical arguments.
 *
 *  resolve_weighted (gslic_lidar_zbuffer_resolve_weighted): resolve with two more optional images from the SAME launch — how far away the return a
 *           pixel was given fell, and a weight for the depth loss (depth_weight) that says so.  A footprint r > 0 fills most of a sparse image with
 *           depths borrowed from up to r sqrt(2) pixels away; resolve hands back only the winning point's index, so without this call a host
 *           would have to re-project every point to learn the distance.  Every argument of resolve keeps its meaning and the four outputs of
 *           resolve are written as resolve writes them.  Per pixel (x, y), also EXACT:
 *
 *             key = the minimum of zbuf over the clipped (2r+1) x (2r+1) window                       (as resolve)
 *             s2  = the smallest dx^2 + dy^2 over the cells (x+dx, y+dy) of that same clipped window whose OWN zbuf key equals key
 *                   (an integer in 0 .. 2 r^2; one such cell always exists when key is not empty.  Keys are normally unique per pixel; "smallest"
 *                   makes the rule total when a caller reused an index_base.  s2 = 0: the pixel itself was measured and its own return is the
 *                   nearest of its window.  s2 > 0 on a measured pixel: its own return was overruled by a nearer neighbour's)
 *             dist2_out  int32    s2;                                                                  -1 where key is empty
 *             weight_out float32  with d the depth of key, four steps, each ONE float32 operation rounded on its own, true divisions:
 *                                   a  = sigma_abs + sigma_rel * d          (one product, one add)
 *                                   rw = sigma_abs / a
 *                                   f  = 1.0f / (1.0f + falloff * (float) s2)
 *                                   w  = rw * f;                                                      0 where key is empty
 *
 *           So at s2 = 0, f is exactly 1 and w is the host's range weight sigma_abs / (sigma_abs + sigma_rel d) bit for bit (the Python host's
 *           trainer.range_weight); at footprint 0 the whole weight image is that range weight of the depth image; at falloff 0 it is at any
 *           footprint.  A product that overflows to +inf gives weight 0 (a = +inf makes rw = 0; 1 + inf makes f = 0), which the depth loss reads as
 *           unmeasured.  The falloff is rational, not an exponential, so that any IEEE float32 arithmetic reproduces it.  Which sigmas, falloff and
 *           footprint to use is the host's policy.  n_measured_out as in resolve.  Same promises: no allocation, synchronisation, read-back or float
 *           atomics; graph-capturable.  Refused with GSLIC_ERR_INVALID_ARG before any device work, the message naming the argument: everything
 *           resolve refuses, "all NULL" now meaning depth_out, index_out, near_out, weight_out and dist2_out; with a weight_out, a sigma_abs
 *           that is not > 0 or not finite, a sigma_rel or a falloff that is negative, NaN or infinite (without one the three are not looked at);
 *           weight_out or dist2_out overlapping zbuf.
 */
int gslic_lidar_zbuffer_add(
    int32_t n, const float* points /*[n,3]*/, const float* R_cw /*[9]*/, const float* t_cw /*[3]*/,
    float fx, float fy, float cx, float cy, int32_t width, int32_t height,
    uint64_t* zbuf /*[height*width]*/, int32_t clear, int32_t index_base, void* stream);
int gslic_lidar_zbuffer_resolve(
    int32_t width, int32_t height, const uint64_t* zbuf /*[height*width]*/, int32_t footprint, float margin_abs, float margin_rel,
    float* depth_out /*[H,W] or NULL*/, int32_t* index_out /*[H,W] or NULL*/, float* near_out /*[H,W] or NULL*/,
    uint32_t* n_measured_out /*[1] or NULL*/, void* stream);
int gslic_lidar_zbuffer_resolve_weighted(
    int32_t width, int32_t height, const uint64_t* zbuf /*[height*width]*/, int32_t footprint, float margin_abs, float margin_rel,
    float sigma_abs, float sigma_rel, float falloff,
    float* depth_out /*[H,W] or NULL*/, int32_t* index_out /*[H,W] or NULL*/, float* near_out /*[H,W] or NULL*/,
    uint32_t* n_measured_out /*[1] or NULL*/, float* weight_out /*[H,W] or NULL*/, int32_t* dist2_out /*[H,W] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_prune_select / gslic_gather_rows — removing rows from the map (no reference counterpart: its map only grows; a LibTorch host
 * would run 19 boolean-index launches with 19 temporaries: 6 groups x {parameter, exp_avg, exp_avg_sq} + tie_rank).
 *
 *  select: one thread per row, then the u32 scan.  The rule is defined on the RAW (pre-activation) parameters xyz [P,3], dc [P,3],
 *          opacity_raw [P], scaling_raw [P,3], rotation_raw [P,4] and involves no transcendental on the device, so the same comparisons on the
 *          same float32 thresholds reproduce it exactly:
 *
 *            bad[i]  = any of xyz[i,0..2], dc[i,0..2], opacity[i], scaling[i,0..2], rotation[i,0..3] is not finite   (only if drop_nonfinite)
 *            hit[i]  = (drop != NULL && drop[i]) || opacity[i] < opacity_raw_min || max_j scaling[i,j] > scaling_raw_max
 *            keep[i] = !bad[i] && ((protect != NULL && protect[i]) || !hit[i])
 *
 *          Both comparisons are strict: a row AT a threshold stays.  opacity_raw_min = -inf or scaling_raw_max = +inf disables a threshold.
 *          (max_j ... > t is evaluated as "some scaling[i,j] > t": a NaN component compares false.)  features_rest is NOT scanned for
 *          non-finite values (180 B per row at SH degree 3).  protect is for rows that are large by construction (a skybox); a non-finite
 *          row goes even when protected.  drop / protect: one byte per row, non-zero = set.
 *          Outputs: kept_index (DEVICE [P]) — its first *count entries are the old row indices of the kept rows, ascending (a stable
 *          compaction); *count (host) — the number of kept rows, reading it is the call's one stream synchronisation; *count_below (host) —
 *          the kept rows with old index < split_row (a host that keeps rows [0, split_row) sorted moves that bound to it; split_row <= 0
 *          gives 0, split_row >= P gives *count); new_tie (DEVICE, its first *count entries), written only when tie_rank and new_tie are
 *          both given — the kept rows' ORIGINAL indices (gslic_raster_params.tie_rank, a permutation of 0..P-1) re-ranked densely:
 *          a permutation of 0..*count-1 in the same relative order as the old tie_rank of the kept rows.  Dense ranks keep "row appended as
 *          number k gets tie k" collision-free after a prune.  Scratch (16 P bytes, 8 P without ties) comes from the caller's allocator and
 *          is dead when the call returns.
 *  gather: dst_a[k, :] = src_a[index[k], :] for k < n_rows and every array a of the HOST array `arrays`, in one launch per 32 arrays
 *          (the map's 19 arrays: one).  Rows are row_dwords 4-byte words wide (any width >= 1; an array of width 0 is skipped);
 *          index [n_rows] is on the DEVICE, every entry below the source's row count.  src and dst must not overlap — tested on
 *          the first n_rows rows of every src against every dst, and dst against dst, before any device work: GSLIC_ERR_INVALID_ARG.
 *          No atomics; rows of dst from n_rows on are not written.
 *  P == 0 / n_rows == 0 / n_arrays == 0 return at once (no allocator call); negative sizes and NULL required pointers: GSLIC_ERR_INVALID_ARG.
 */
int gslic_prune_select(
    int32_t P, const float* xyz, const float* dc, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw,
    float opacity_raw_min, float scaling_raw_max, int32_t drop_nonfinite,
    const uint8_t* drop /*[P] or NULL*/, const uint8_t* protect /*[P] or NULL*/,
    const uint32_t* tie_rank /*[P] or NULL*/, int32_t split_row,
    gslic_alloc_fn scratch_alloc, void* scratch_ctx,
    uint32_t* kept_index /*[P]*/, uint32_t* new_tie /*[P] or NULL*/, int32_t* count, int32_t* count_below, void* stream);

typedef struct gslic_row_array { const void* src; void* dst; uint32_t row_dwords; } gslic_row_array;   /* HOST array */
int gslic_gather_rows(const gslic_row_array* arrays, int32_t n_arrays, const uint32_t* index, int32_t n_rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_morton_order / gslic_permute_rows — putting the map's rows (back) into Morton order on the device (no reference counterpart: its rows
 * stay in insertion order; a LibTorch host would run about ten elementwise int64 kernels, torch.sort and 19 index + copy round trips).  The
 * step runs measurably faster on rows in Morton order; rendering and training do not depend on the row order as long as
 * gslic_raster_params.tie_rank holds every row's original index, so tie_rank is one of the arrays a host permutes.
 *
 *  order:  one thread per row, then the library's stable radix sort over the 30 key bits.  The key rule is EXACT — every step below is one IEEE
 *          float32 operation rounded on its own (no contraction, a true division, no reciprocal), so the same steps in any IEEE float32
 *          arithmetic give the same keys bit for bit.  xyz [P,3] and box [6] = (lo_0, lo_1, lo_2, hi_0, hi_1, hi_2) are on the DEVICE.  Per axis k:
 *
 *            e = hi_k - lo_k;            d = (e > 1e-30f) ? e : 1e-30f             (max(hi - lo, 1e-30f); a NaN extent, inf - inf, reads as 1e-30f)
 *            t = (xyz[i,k] - lo_k) / d
 *            c = (t > 0) ? ((t < 1) ? t : 1) : 0                                    (min(max(t, 0), 1); NaN reads as 0)
 *            u_k = (uint32) trunc(c * 1023.0f)                                      (0 .. 1023)
 *            spread(u): u = (u | u << 16) & 0x030000FF;  u = (u | u << 8) & 0x0300F00F;  u = (u | u << 4) & 0x030C30C3;  u = (u | u << 2) & 0x09249249
 *          key[i] = spread(u_0) | spread(u_1) << 1 | spread(u_2) << 2                (30 bits)
 *
 *          A row outside the box is clamped onto its faces; a row with a NaN coordinate gets 0 on that axis, +inf 1023, -inf 0; an axis with
 *          hi <= lo puts rows at or below lo on 0 and rows 1e-30 or more above it on 1023.  The box is the caller's: where to put the grid is policy (this
 *          repository's hosts take a robust box from a sample of the rows).
 *          Outputs (DEVICE): perm [P] — perm[s] is the old row that becomes row s: rows ascending by key, equal keys in their current storage
 *          order (the sort is stable), so an already sorted map gives the identity; keys_sorted [P] or NULL — key[perm[s]].  Both are written
 *          by the sort's last pass; exactly P entries each.  Scratch (12 P bytes plus the sort's histograms) comes from the caller's allocator
 *          in ONE call and is dead when the launches have run; no stream synchronisation, no host read-back, no atomics.
 *  permute: a[s, :] <- a[perm[s], :] for s < n_rows and every array a of the HOST array `arrays`, IN PLACE: src == dst names the array (an
 *          entry with src != dst is GSLIC_ERR_INVALID_ARG; an array of width 0 is skipped).  perm [n_rows] on the DEVICE must be a permutation of
 *          0 .. n_rows-1: that is the caller's responsibility and is not checked on the device (an entry >= n_rows reads outside the rows).  Two
 *          steps on the stream: gslic_gather_rows' launch into `staging` (DEVICE; array i's rows at byte offset 4 n_rows times the sum of the
 *          row_dwords before it; one launch per 32 arrays, the map's 19: one), then one device-to-device copy per array back.  Rows from n_rows on are not
 *          touched.  staging must hold the sum of row_dwords * 4 * n_rows bytes; gslic_permute_rows_staging_bytes returns that sum rounded as
 *          gslic_scratch_round_up does (what a caching allocator should be asked for; 0 for no arrays / no rows).  A staging buffer that is
 *          smaller than the sum, or whose staging_bytes overlap the first n_rows rows of any array, and arrays that overlap each other, are
 *          GSLIC_ERR_INVALID_ARG before any device work.
 *  P == 0 / n_rows == 0 / n_arrays == 0 return at once (no allocator call); negative sizes and NULL required pointers: GSLIC_ERR_INVALID_ARG.
 *  With N > 1 GPUs every rank calls both with identical arguments.
 */
int gslic_morton_order(
    int32_t P, const float* xyz /*[P,3]*/, const float* box /*[6]: lo xyz, hi xyz*/,
    gslic_alloc_fn scratch_alloc, void* scratch_ctx,
    uint32_t* perm /*[P]*/, uint32_t* keys_sorted /*[P] or NULL*/, void* stream);
int gslic_permute_rows(
    const gslic_row_array* arrays /*HOST; src == dst: the array itself*/, int32_t n_arrays,
    const uint32_t* perm /*[n_rows]*/, int32_t n_rows, void* staging, size_t staging_bytes, void* stream);
size_t gslic_permute_rows_staging_bytes(const gslic_row_array* arrays, int32_t n_arrays, int32_t n_rows);

/* ------------------------------------------------------------------------------------------------
 * gslic_contribution_accumulate — per-Gaussian contribution statistics of ONE view, from the buffers a completed forward filled (no
 * reference counterpart; the signal a mapper prunes by: did this Gaussian ever carry weight in a pixel).  One launch, a pass of its own: the
 * training step is not touched.  geom / binning / img: the buffers of gslic_rasterize_forward, _forward_depth or their _capacity variants
 * (the colour-only layout is a prefix of all of them) with the R and B that forward returned — in capacity mode the capacities, as for the
 * backward.  A no_color forward stores no n_contrib: GSLIC_ERR_INVALID_ARG.
 *
 *  The rule.  For every pixel p of the image, with its tile's list e_0, e_1, ... (front to back) and its stored n_contrib[p]:
 *      T = 1
 *      for k in [0, n_contrib[p]):   d = mean2D(e_k) - p;  power = -0.5 (A d.x d.x + C d.y d.y) - B d.x d.y
 *          if power > 0: continue;   alpha = min(0.99, opacity(e_k) exp(power));   if alpha < 1/255: continue
 *          w = alpha T;   the pair (p, e_k) CONTRIBUTES with weight w;   T = T (1 - alpha)
 *  i.e. exactly the pairs the forward blended into the pixel, with the weight it gave them.  The arithmetic is the strict forward's
 *  (absolute pixel coordinates, every product rounded on its own, hipcc's expf): on a strict forward's buffers w is the forward's value bit
 *  for bit.  There is NO fast-math variant: on the buffers of a fast-mode forward (gslic_set_math_mode(0)) the kernel still replays in the
 *  strict arithmetic and honours that forward's n_contrib; the two arithmetics differ by rounding, so a few pairs per million sit on the
 *  other side of alpha < 1/255 and are classified differently from what that forward did.
 *  Accumulators (DEVICE, caller-owned, persistent across calls, indexed by STORAGE row g; each may be NULL; zero them to start):
 *      max_w [P] uint32  the float bits of max(max_w[g], w) over the contributing pairs of g — an unsigned integer max on the bit pattern
 *                        (w >= 0, so the patterns order like the values): exact and independent of the order of the updates
 *      n_pix [P] uint32  += the number of contributing pairs of g with w >= w_min.  It SATURATES at 2^32 - 1 and never wraps:
 *                        n_pix[g] = min(2^32 - 1, true count) whatever the order of the updates
 *      sum_w [P] uint64  += sum of w over the contributing pairs of g, in fixed point with 32 fractional bits.  A tile's partial sum for an
 *                        entry is formed in float in a fixed order over the tile's 256 pixels, converted ONCE (round to nearest) and added with a
 *                        64-bit integer add.  A tile partial is at most 256 = 2^8, i.e. 2^40 in fixed point: more than 2^24 tile partials fit
 *                        into a row before the 64 bits overflow.  sum in float units = sum_w / 2^32.
 *  All three are deterministic from run to run and independent of the order in which tiles finish (integer max and adds commute), so the
 *  ranks of an N-GPU run reach identical decisions from identical views.  Calls that share accumulators must be ordered (one stream).
 *  Capacity mode: the launch is sized from the image, the lists end at the real counts on the device, and nothing is accumulated when the
 *  forward's status words say the lists did not fit (what the backward does).  No host synchronisation, no allocation.
 *  P == 0 or R == 0 returns at once; all three outputs NULL likewise.  Negative R / B, no_color, a NaN w_min and NULL buffers are reported
 *  before any device work (GSLIC_ERR_INVALID_ARG, gslic_last_error).
 */
int gslic_contribution_accumulate(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const char* geom_buffer, const char* binning_buffer, const char* img_buffer, float w_min,
    uint32_t* max_w /*[P] or NULL*/, uint32_t* n_pix /*[P] or NULL*/, uint64_t* sum_w /*[P] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_contribution_accumulate_error — the same launch over the same pairs as gslic_contribution_accumulate, which in addition weights the
 * replay with a per-pixel error image: err_sum[g] += sum of w e(p) over the contributing pairs (p, g).  This is the error-based densification
 * score of Bulo et al., "Revising Densification in Gaussian Splatting": it needs no backward (the fused step's dL/dmean2D never leaves
 * registers) and stays an integer like the other statistics.  Building the error image is the host's policy (an L1 or 1 - SSIM map).
 *
 *  err [H,W] float, row-major, DEVICE.  e(p) = err[p] clamped to [0, 4]: a negative value or a NaN reads as 0, +inf reads as 4 (L1 and
 *  1 - SSIM maps live in [0, 2]).
 *  err_sum [P] uint64, DEVICE, caller-owned and persistent like sum_w, 32.32 fixed point.  Each pixel forms the product w e(p) in float32,
 *  rounded on its own; a wave combines its 64 products with the wave butterfly (a fixed order); the four waves' partials are added in wave
 *  order; the tile partial is converted ONCE (round to nearest) and added with one 64-bit integer add per (tile, entry).  A tile partial is
 *  at most 256 * 4 = 1024 = 2^10, i.e. 2^42 in fixed point: 2^22 tile partials fit into a row before the 64 bits overflow.
 *  err_sum in float units = err_sum / 2^32.
 *  Deterministic from run to run and independent of the order in which tiles finish.  max_w / n_pix / sum_w (each may be NULL) come out
 *  bit-identical to gslic_contribution_accumulate's: the same operations in the same order.  An error image of all ones gives
 *  err_sum == sum_w bit for bit.
 *  Argument checks, the capacity-mode rule and the early returns are those of gslic_contribution_accumulate (all three of max_w / n_pix /
 *  sum_w NULL does NOT return early here: err_sum is still accumulated); in addition err == NULL or err_sum == NULL is
 *  GSLIC_ERR_INVALID_ARG, reported before any device work.
 */
int gslic_contribution_accumulate_error(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const char* geom_buffer, const char* binning_buffer, const char* img_buffer, float w_min,
    uint32_t* max_w /*[P] or NULL*/, uint32_t* n_pix /*[P] or NULL*/, uint64_t* sum_w /*[P] or NULL*/,
    const float* err /*[H,W]*/, uint64_t* err_sum /*[P]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_contribution_accumulate_free_space — the same launch over the same pairs as gslic_contribution_accumulate, which in addition tells a
 * mapper with a measured range per pixel (a LiDAR depth image) which Gaussians carry blend weight IN FRONT of the measured surface, i.e. in
 * known free space: the floaters the colour loss keeps alive.  A pass of its own like _error; the training step is not touched.  How the bound
 * image is made (margins, dilation of sparse returns, dynamic objects) and when to prune is the host's policy.
 *
 *  near_bound [H,W] float, row-major, DEVICE, in view-space depth units: the nearest depth at which the measurement still allows a surface in
 *  that pixel — typically d - (margin_abs + margin_rel d) where the LiDAR depth d > 0, and 0 elsewhere.
 *  Pixel p is MEASURED iff near_bound[p] > 0: NaN, 0 and negative values are not measured, +inf is.
 *  The pairs are exactly the contributing pairs of gslic_contribution_accumulate, with the same w from the same operations in the same order.
 *  z_g is the float32 view depth in the Gaussian's record (what the depth blend reads).
 *      meas_sum [P] uint64  += sum of w over the contributing pairs (p, g) whose pixel is measured
 *      free_sum [P] uint64  += sum of w over the contributing pairs (p, g) whose pixel is measured AND z_g < near_bound[p]
 *  The comparison is a strict float32 < with no arithmetic on either side, so torch or numpy reproduce it exactly.  Both are DEVICE,
 *  caller-owned and persistent like sum_w, in 32.32 fixed point, formed by the route of sum_w and err_sum: the per-pixel addend is w or +0; a
 *  wave combines its 64 addends with the wave butterfly (a fixed order); the four waves' partials are added in wave order; the tile partial is
 *  converted ONCE (round to nearest) and added with one 64-bit integer add per (tile, entry), skipped when the partial is 0.  A tile partial is at
 *  most 256 = 2^8, i.e. 2^40 in fixed point: 2^24 tile partials fit into a row.  Deterministic from run to run and independent of the order
 *  in which tiles finish.  free_sum[g] <= meas_sum[g] <= what sum_w[g] gains, per tile partial and hence in total.
 *  Consequences:  max_w / n_pix / sum_w (each may be NULL) come out bit-identical to gslic_contribution_accumulate's.  near_bound = +inf
 *  everywhere gives free_sum == meas_sum == sum_w bit for bit.  A near_bound image of 0 and +inf only gives free_sum == meas_sum == the err_sum
 *  of gslic_contribution_accumulate_error with the error image that is 1 where near_bound is +inf and 0 elsewhere, bit for bit.
 *  Argument checks, the capacity-mode rule (nothing is accumulated when the forward's status words say the lists did not fit) and the early
 *  returns are those of gslic_contribution_accumulate_error: all three of max_w / n_pix / sum_w NULL does NOT return early; near_bound, free_sum
 *  or meas_sum NULL is GSLIC_ERR_INVALID_ARG, reported before any device work.  The replay is in the strict arithmetic only.
 */
int gslic_contribution_accumulate_free_space(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const char* geom_buffer, const char* binning_buffer, const char* img_buffer, float w_min,
    uint32_t* max_w /*[P] or NULL*/, uint32_t* n_pix /*[P] or NULL*/, uint64_t* sum_w /*[P] or NULL*/,
    const float* near_bound /*[H,W]*/, uint64_t* free_sum /*[P]*/, uint64_t* meas_sum /*[P]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_geometry_images — per-PIXEL geometry of ONE view, from the buffers a completed forward filled (no reference counterpart): the
 * accumulated opacity, the opacity-normalised and the median depth, and which Gaussian owns the pixel — what evaluation, mesh / TSDF export,
 * occlusion tests of LiDAR points and 2-D masks turned into row masks need, none of which needs a gradient.  The same replay as
 * gslic_contribution_accumulate, which keeps the per-pixel results instead of reducing them per Gaussian.  One launch, a pass of its own: the
 * training step is not touched.  geom / binning / img, R and B: the contract of gslic_contribution_accumulate (colour or depth forwards, plain
 * or capacity; a no_color forward stores no n_contrib: GSLIC_ERR_INVALID_ARG).
 *
 *  The rule.  For every pixel p of the image, with its tile's list e_0, e_1, ... (front to back) and its stored n_contrib[p]:
 *      T = 1;  A = 0;  D = 0;  zmed = 0;  found = false;  top = -1;  wtop = 0
 *      for the CONTRIBUTING pairs (p, e_k), k < n_contrib[p]   (the rule of gslic_contribution_accumulate: skip power > 0 and alpha < 1/255):
 *          z = the float32 view depth in e_k's record (what the depth blend reads);   w = alpha T
 *          D = D + (z alpha) T                                    (the strict depth forward's operation order)
 *          A = A + w
 *          if w > wtop:  wtop = w;  top = storage row of e_k      (strict >: the frontmost wins a tie)
 *          T = T (1 - alpha)
 *          if !found and T < 0.5:  zmed = z;  found = true        (the entry whose blending takes T below one half)
 *      transmittance[p] = T;   opacity[p] = A;   depth_sum[p] = D;   depth_median[p] = zmed   (0: one half was never reached)
 *      depth_norm[p] = A >= a_min ? D / A : 0                     (ONE IEEE float32 division; a_min > 0)
 *      top_row[p] = top   (-1: no contributor);   top_weight[p] = wtop
 *  The arithmetic is the strict forward's (absolute pixel coordinates, every product rounded on its own, hipcc's expf): on a strict forward's
 *  buffers transmittance is that forward's final_T and depth_sum its depth image (gslic_rasterize_forward_depth), bit for bit, and the buffers
 *  of a colour-only and of a depth forward give the same seven images.  There is NO fast-math variant: on the buffers of a fast-mode forward
 *  (gslic_set_math_mode(0)) the kernel still replays in the strict arithmetic and honours that forward's n_contrib; the two arithmetics differ
 *  by rounding, so a few pairs per million sit on the other side of alpha < 1/255 and are classified differently from what that forward did.
 *  Outputs (DEVICE, each [H*W] row-major, each may be NULL): EVERY pixel of the image is written by the launch — no memset is needed — and a
 *  pixel no list reaches gets the initial values (1, 0, 0, 0, 0, -1, 0).  top_row indexes STORAGE rows, like the contribution statistics.
 *  Deterministic: a pixel's values depend on its own list only; no atomics, no cross-pixel arithmetic.
 *  Capacity mode: the launch is sized from the image, the lists end at the real counts on the device, and NOTHING is written when the
 *  forward's status words say the lists did not fit (what the backward does).  No host synchronisation, no allocation; capturable in a graph.
 *  All seven outputs NULL returns at once.  P == 0 or R == 0: no list exists, the forward's buffers are not read (they may be NULL) and the
 *  outputs given get the initial values.  Negative R / B, no_color, NULL buffers (P > 0 and R > 0) and — with a non-NULL depth_norm — an
 *  a_min that is NaN or not > 0 are reported before any device work (GSLIC_ERR_INVALID_ARG, gslic_last_error).
 */
int gslic_geometry_images(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const char* geom_buffer, const char* binning_buffer, const char* img_buffer, float a_min,
    float* transmittance, float* opacity, float* depth_sum, float* depth_norm, float* depth_median,
    int32_t* top_row, float* top_weight /*each [H*W] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_densify_select / gslic_densify_emit — clone / split densification on the device (no reference counterpart: its map grows from
 * LiDAR returns only; a LibTorch host would run 18 index + cat launches plus the rewrite of the split parents).  Which rows to grow
 * (`grow`, e.g. a threshold on err_sum) and when is the host's policy.
 *
 *  select: one thread per row, then the u32 scan.  The rule is defined on the RAW (pre-activation) parameters and uses comparisons only:
 *
 *            eligible[i] = grow[i] && !(protect != NULL && protect[i])
 *                          && every one of xyz[i,0..2], dc[i,0..2], opacity[i], scaling[i,0..2], rotation[i,0..3] is finite
 *                          && |rotation[i]|^2 > 0      (the FLOAT32 value ((q0 q0 + q1 q1) + q2 q2) + q3 q3, every product and sum rounded on its
 *                                                       own: the number the split divides by; a quaternion whose squares all underflow is not eligible)
 *            split[i]    = eligible[i] && (some scaling[i,j] > scaling_raw_split)       (strict: a row AT the threshold clones)
 *            clone[i]    = eligible[i] && !split[i]
 *
 *          scaling_raw_split is the float32 of log(split_scale), converted once on the host (NaN: GSLIC_ERR_INVALID_ARG; +inf: every row
 *          clones).  grow / protect: one byte per row, non-zero = set.  features_rest is not scanned.  Every eligible row adds exactly ONE row.
 *          Positions: let o_i be row i's ORIGINAL index (tie_rank[i], or i without tie_rank; a row whose tie_rank is outside 0..P-1 is
 *          not eligible).  rank_i is the rank of o_i among the eligible rows' original indices (flags scattered to the original index,
 *          scanned, gathered back — as gslic_prune_select ranks its dense ties).  The new row of parent i is storage row P + rank_i and
 *          its tie is P + rank_i: a Morton-ordered and an insertion-ordered model of the same map densify to the same map.
 *          Outputs: parent_index (DEVICE [P]) — its first *count entries, parent_index[rank] = storage row of the parent of new row
 *          P + rank; *count (host) — the eligible rows, reading it is the call's one stream synchronisation; *count_split (host) — how
 *          many of them split.  Scratch — ONE allocator call for about 8 P bytes (two uint32 [P] arrays) plus the u32 scan's temporaries (a few
 *          words per 1024 rows) plus 1 KB of counters and alignment slack; the exact size is what the callback is asked for — is dead when the
 *          call returns.
 *  emit:   param / exp_avg / exp_avg_sq: HOST arrays of the six DEVICE base pointers (xyz [.,3], features_dc [.,3], features_rest [.,3M],
 *          opacity [.,1], scaling [.,3], rotation [.,4]; features_rest may be NULL when M == 0), each with capacity >= P + count rows.
 *          tie_rank: DEVICE [>= P + count] or NULL.  Two launches on the stream: the wide one (the 3 + 3M + 1 copied dwords of every new row
 *          and the zeroed moments, cut along the destination, contiguous dwords per wave, no atomics; it reads only parent fields that no
 *          thread writes, plus the parents' scaling BEFORE the second launch rewrites it), then one thread per parent, which reads its
 *          parent's xyz / scaling / rotation once and writes both children.
 *          Clone:  the new row is a bit copy of the parent's six parameter rows, its 2 x (14 + 3M) moment values are zero; the parent is
 *                  untouched, moments included.
 *          Split (3DGS densify_and_split with N = 2, in place): child 0 replaces the parent's row, child 1 is the new row.  Both take dc,
 *                  features_rest, opacity and rotation as bit copies, scaling_child = scaling_raw - (float)log(1.6) (ONE float32
 *                  subtraction per component) and xyz_child_c = xyz + R(q / |q|) (exp(scaling_raw_parent) (.) z_c), R the rotation matrix
 *                  of the unit quaternion (r, x, y, z) = q / |q|; all moment values of both rows are zero.
 *          Noise:  z_c comes from a counter generator keyed by the ORIGINAL index o_i — identical on every rank and in both row orders:
 *                    fmix32(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16            (uint32)
 *                    word(n) = fmix32( fmix32(fmix32(seed) ^ o_i) + 0x9E3779B9 * (n + 1) ),   n = 4c .. 4c + 3 for child c
 *                    u_n     = (2 * (word(n) >> 9) + 1) * 2^-24                                (exact in float32, inside (0, 1))
 *                    z_c     = ( r0 cos(2 pi u_{4c+1}), r0 sin(2 pi u_{4c+1}), r2 cos(2 pi u_{4c+3}) ),
 *                              r0 = sqrt(-2 ln u_{4c}),  r2 = sqrt(-2 ln u_{4c+2})
 *          scaling_raw_split and tie_rank must be those given to select.  Rows >= P + count and every row that is not a parent are not written.
 *  P == 0 / count == 0 return at once (no allocator call); negative sizes, count > P and NULL required pointers: GSLIC_ERR_INVALID_ARG before
 *  any device work.  With N > 1 GPUs every rank calls both with identical arguments and seed.
 */
int gslic_densify_select(
    int32_t P, const float* xyz, const float* dc, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw,
    const uint8_t* grow /*[P]*/, const uint8_t* protect /*[P] or NULL*/, const uint32_t* tie_rank /*[P] or NULL*/, float scaling_raw_split,
    gslic_alloc_fn scratch_alloc, void* scratch_ctx,
    uint32_t* parent_index /*[P]*/, int32_t* count, int32_t* count_split, void* stream);
int gslic_densify_emit(
    int32_t P, int32_t count, const uint32_t* parent_index, int32_t M,
    float* const param[6], float* const exp_avg[6], float* const exp_avg_sq[6],
    uint32_t* tie_rank /*[>= P + count] or NULL*/, float scaling_raw_split, uint32_t seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gslic_covis_* — covisibility sets: which keyframes see which Gaussians (no reference counterpart: its optimize() draws 100 keyframes at
 * random, gaussian.cpp:644-662, and keeps no relation between keyframes and rows).  Signals only: which keyframe to give up, which window to
 * train and which rows to protect stay the host's policy.
 *
 * THE DATA AND ITS RULE.  bits: uint32 [capacity, Wd], row-major, DEVICE, caller-owned, in STORAGE row order, with Wd = ceil(F / 32) dwords
 * per row and F = n_frames in 1 .. GSLIC_COVIS_MAX_FRAMES.  Bit f of row r is bit (f & 31) of word r * Wd + (f >> 5), and means "frame f, when
 * it was last recorded, had radii[r] > 0".  Bits f >= F of a row's last word are never set by the library and are ignored by the queries.  The
 * state is per row and Wd dwords wide, so gslic_gather_rows / gslic_permute_rows and the zero segments of gslic_densify_emit's launch carry
 * it through every map edit as one more row array of run-time width.  16 bytes per row at F = 128.  Every call below sees rows [0, P) only.
 *
 * gslic_covis_record — one launch, one thread per row of [row_begin, row_end) (row_end < 0: P).  With f = *frame_word:
 *      seen(r) = radii[r] > 0          (radii given: int32 [P])
 *              = visible[r] != 0       (visible given: uint8 [P])
 *              = false                 (both NULL: the column is cleared — what a replaced keyframe slot needs)
 *      word r * Wd + (f >> 5)  <-  (word & ~(1 << (f & 31))) | (seen(r) << (f & 31))
 *  by one plain load and one plain store of that single word; the other words of the row are neither read nor written.  The call REPLACES
 *  and does not OR: recording a frame again overwrites its column, so the state is a function of each frame's last record, whatever the order.
 *  frame_word is a required DEVICE int32; a value outside [0, F) touches nothing.  skip is an optional DEVICE int32 [1]: nonzero touches
 *  nothing (a training step passes its forward's status word, status[2]: a step that did not fit its buffers records nothing).  No
 *  allocation, no read-back, no synchronisation, no atomics: the call can be captured in a graph, and a captured graph changes column through
 *  the word.  Refused with GSLIC_ERR_INVALID_ARG before any device work: P < 0, F outside 1 .. GSLIC_COVIS_MAX_FRAMES, bits or frame_word
 *  NULL, radii and visible both given, a row range outside 0 <= row_begin <= row_end <= P, bits ([P, Wd] x 4 bytes) overlapping radii,
 *  visible, frame_word or skip.  An empty range returns at once.
 *
 * The three queries read bits and zero their outputs themselves (a memset node on the stream in front of the launch); every count is an
 * unsigned integer sum, so the results are the same on every run whatever the order of the adds.  Rows are expected to be sparse in set bits:
 * a thread owns a row and walks its set bits; counters live in the workgroup's LDS and are added to the output by integer atomics once per
 * workgroup.  P == 0 gives zeros.
 * gslic_covis_pair_counts  — pair[f * F + g] = number of rows r < P with bit f AND bit g.  Symmetric; the diagonal is each frame's visible
 *      count.  F <= GSLIC_COVIS_MAX_PAIR_FRAMES (the upper triangle of 128 x 128 counters is 33 KB of LDS); a larger F is refused.
 * gslic_covis_frame_counts — out[g] = number of rows with bit f AND bit g, f = *frame_word (DEVICE int32): the window query around one
 *      keyframe, any F.  f outside [0, F) gives zeros.
 * gslic_covis_row_counts   — n_seen[r] = popcount(row r AND frame_mask), frame_mask uint32 [Wd] on the DEVICE or NULL = every frame.  With
 *      redundant given: redundant[f] = number of rows with bit f (of the row as stored, masked or not) and n_seen[r] >= 1 + min_others —
 *      "f sees the row and so do at least min_others others" when f is in the mask.  min_others >= 0.
 *  Refused before any device work: P < 0, F out of range, a NULL bits / output / frame_word, min_others < 0, an output overlapping bits, an
 *  input or another output.
 */
#define GSLIC_COVIS_MAX_FRAMES 1024
#define GSLIC_COVIS_MAX_PAIR_FRAMES 128
int gslic_covis_record(
    int32_t P, int32_t F, uint32_t* bits /*[P,Wd]*/, const int32_t* radii /*[P] or NULL*/, const uint8_t* visible /*[P] or NULL*/,
    const int32_t* frame_word /*[1] device*/, const int32_t* skip /*[1] device or NULL*/, int32_t row_begin, int32_t row_end, void* stream);
int gslic_covis_pair_counts(int32_t P, int32_t F, const uint32_t* bits, uint32_t* pair /*[F*F]*/, void* stream);
int gslic_covis_frame_counts(int32_t P, int32_t F, const uint32_t* bits, const int32_t* frame_word /*[1] device*/, uint32_t* out /*[F]*/, void* stream);
int gslic_covis_row_counts(
    int32_t P, int32_t F, const uint32_t* bits, const uint32_t* frame_mask /*[Wd] or NULL*/, int32_t* n_seen /*[P]*/, int32_t min_others,
    uint32_t* redundant /*[F] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Introspection / measurement (no reference counterpart; used by bench.py and the tests).
 */
int gslic_abi_version(void);
const char* gslic_last_error(void);

/* Arithmetic of the two blend kernels (process-wide; returns the previous mode).
 * 1 (default) = strict: the reference's operations in source order (forward.cu:424-445, backward.cu:538-581) — absolute pixel
 * coordinates, every product of the power rounded on its own (no contraction), exp() as hipcc lowers expf() (the same instruction
 * sequence, inlined without its two range checks), opacity * exp, (colour * alpha) * T.  Image / final_T / n_contrib are bit-identical
 * to the reference's kernels compiled by hipcc -ffp-contract=off for the same GPU, every blend / skip decision of the backward is the
 * reference's, gradients agree to fp32 summation order (tests/test_fullsize_reference_gpu.py).  This is what bench.py times.
 * 0 = fast (opt-in: GSLIC_FAST_MATH=1 in the environment, or this call): conic pre-scaled by log2(e), tile-relative coordinates,
 * alpha = v_exp_f32(p2 + log2 opacity), fused multiply-adds — within fp32 rounding of the reference, which flips the alpha < 1/255
 * and T < 1e-4 decisions of a few (pixel, Gaussian) pairs per million (counted in the same test). */
int gslic_set_math_mode(int32_t strict);

/* How the forward groups the (Gaussian, tile) instances by tile — the tile half of cub::DeviceRadixSort::SortPairs,
 * rasterizer_impl.cu:419-424; the lists are the reference's bit for bit on either path.  Returns the previous mode.
 * 0 = auto (default; GSLIC_BINNING=auto): block-aggregated atomics on the tiles' list cursors while the map's row order keeps consecutive
 *     Gaussians on neighbouring tiles (measured per forward: the global atomics the binning kernel needed per instance), the stable radix sort
 *     otherwise, above 36864 tiles (the block histogram's 144 KB of LDS) and on a device / driver that does not grant a kernel more than
 *     64 KB of dynamic LDS while the image has more than 14336 tiles;  1 = always the radix sort (GSLIC_BINNING=radix);  2 = atomics
 *     whenever the tile count allows (GSLIC_BINNING=atomic: a refused LDS grant is then an error, GSLIC_ERR_HIP, instead of a fallback).
 *     Any other value only reads the mode.  Process-wide: the mode is atomic, and setting it makes EVERY host thread forget what its last
 *     forwards measured (ABI 8; until ABI 7 only the calling thread's state was reset). */
int gslic_set_binning_mode(int32_t mode);

/* Which grouping the calling thread's LAST forward with at least one instance took (ABI 8): GSLIC_BINNING_PATH_NONE before any,
 * _RADIX (sort_hist / sort_scatter / finalize_ranges launches) or _ATOMIC (tile_hist / tile_scan / tile_bin launches).  sampled_atomics /
 * sampled_instances (either may be NULL): what the binning kernel's sampled workgroups reported for that forward — global atomics and
 * instances; `auto` keeps the atomic path while atomics <= 0.4 * instances.  Zero on the radix path and in capacity mode (nothing is read back). */
#define GSLIC_BINNING_PATH_NONE 0
#define GSLIC_BINNING_PATH_RADIX 1
#define GSLIC_BINNING_PATH_ATOMIC 2
int gslic_get_binning_path(uint32_t* sampled_atomics, uint32_t* sampled_instances);

/* The size a host allocator should round a scratch request of `bytes` up to (ABI 8; the allocator callbacks of this repository's hosts —
 * _lib.TensorAllocator, the LibTorch shim's resize callbacks — all call it): requests above 1 MB go to 32 MB granules, above 64 MB to
 * granules of min(half the largest power of two in the request, 256 MB).  A caching allocator then keeps serving the same block while R and B
 * drift from step to step, a GROWING map pays a hipMalloc once per ~1.3x of growth below 512 MB, and the over-allocation stays below 50 % up
 * to 512 MB and below 256 MB beyond (a 2.1 GB request becomes 2.25 GB, not 3). */
size_t gslic_scratch_round_up(size_t bytes);

/* Sizes the four scratch buffers would need, for hosts that prefer to pre-size (bytes incl. slack). */
size_t gslic_geom_bytes(int32_t P);
size_t gslic_img_bytes(int32_t width, int32_t height);
size_t gslic_binning_bytes(int32_t R, int32_t no_color);
size_t gslic_sample_bytes(int32_t B);
/* The same for the buffers of a depth forward (gslic_rasterize_forward_depth*): the colour layout plus 4 bytes per pixel of the tile grid / per
 * instance / per bucket-pixel behind it. */
size_t gslic_img_bytes_depth(int32_t width, int32_t height);
size_t gslic_binning_bytes_depth(int32_t R);
size_t gslic_sample_bytes_depth(int32_t B);

/* Per-kernel HIP-event timing.  While enabled, every kernel launch of this library is bracketed by a
 * hipEvent pair recorded on the launch stream; gslic_profile_collect synchronises the device and adds the
 * elapsed times to per-kernel totals.  Kernel ids are stable and named by gslic_profile_kernel_name. */
#define GSLIC_PROFILE_MAX_KERNELS 48
int gslic_profile_enable(int32_t on); /* 0 = off, 1 or -1 = every kernel, otherwise bit i selects kernel id i (ids < 31) */
int gslic_profile_reset(void);
int gslic_profile_collect(void);
int gslic_profile_num_kernels(void);
const char* gslic_profile_kernel_name(int32_t id);
int gslic_profile_get(int32_t id, double* total_ms, int64_t* launches);

/* Test-only view into the opaque scratch buffers: copies stage boundaries to DEVICE arrays the caller owns
 * (any pointer may be NULL).  Used by the parity tests to compare tiles_touched / point_list / ranges with
 * the oracle bit-for-bit; not part of the drop-in surface. */
int gslic_debug_export(
    const gslic_raster_params* prm, int32_t R, int32_t B,
    const char* geom_buffer, const char* binning_buffer, const char* img_buffer, const char* sample_buffer,
    uint32_t* tiles_touched /*[P]*/, float* means2D /*[P,2]*/, float* depths /*[P]*/,
    float* conic_opacity /*[P,4]*/, float* rgb /*[P,3]*/,
    uint64_t* sorted_keys /*[R]*/, uint32_t* point_list /*[R]*/, uint32_t* ranges /*[T,2]*/,
    uint32_t* n_contrib /*[H*W] row-major image order*/, uint32_t* max_contrib /*[T]*/,
    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSLIC_HIP_H_INCLUDED */
