// kernels.h — argument blocks and host-side launchers of the rasterizer kernels (internal to libgslic_hip.so).
#pragma once
#include "gslic_common.h"

namespace gslic {

struct PreprocessArgs {
    int P, D, M, W, H, gx, gy;
    float focal_x, focal_y;
    float limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier;
    int prefiltered, no_color, raw;
    const float *means, *scales, *rots, *opac, *dc, *shs, *view, *proj, *campos;
    int32_t* radii;
    float4* rec;
    uint32_t* tiles_touched;
    uint32_t* depth_keys;  // optional [P] depth bits, 0xffffffff when culled (round 5: the forward no longer sorts the Gaussians by depth; NULL)
    uint2* ranges;         // [gx*gy] zeroed here (rasterizer_impl.cu:426) to save a memset launch
    uint32_t* flags;
};
int launch_preprocess(const PreprocessArgs& a, hipStream_t s);

struct KeybuildArgs {
    int P, gx, gy;
    const float4* rec;
    const uint32_t* order;     // NULL (round 5): thread i emits Gaussian i; else [P] Gaussian ids in emission order
    const uint32_t* offsets;   // [P] inclusive scan of tiles_touched in emission order
    uint32_t* tile_keys;       // [R] out: tile id per emission slot
    uint32_t* gauss;           // [R] out: Gaussian id per emission slot
    uint32_t* depth;           // [R] out: depth bits per emission slot (sort key of the per-tile depth sort)
    uint32_t* gauss_start;     // [P] out: first emission slot of each visible Gaussian
    uint32_t cap;              // slots available in tile_keys / gauss (capacity mode; the exact R otherwise)
    uint32_t* status;          // device status words: [2] |= 1 when an instance did not fit (nothing is written past cap)
};
int launch_keybuild(const KeybuildArgs& a, hipStream_t s);
// R_dev != NULL: the real instance count is read on the device and R is the capacity the launch is sized for
// dead != NULL: also clears the per-slot dead flags of the backward (BinningState::dead)
int launch_finalize_ranges(uint32_t R, const uint32_t* R_dev, const uint32_t* sorted_tiles, uint2* ranges, uint8_t* dead, hipStream_t s);
int launch_bucket_scan(int T, const uint2* ranges, uint32_t* bucket_offsets, uint32_t* max_contrib /* zeroed */, hipStream_t s);  // scan.hip

struct RenderFwdArgs {
    int W, H, gx, gy, no_color;
    const uint2* ranges;
    const uint32_t* point_list;
    const float4* rec;
    const uint32_t* bucket_offsets;
    uint32_t* bucket_to_tile;
    float4* ckpt;
    uint64_t* hit;             // SampleState::hit (written by the strict variant only, which then sets status[GS_FLAG_HITBITS])
    float4* pix_final;
    uint32_t* max_contrib;
    float* out_color;
    float* out_final_T;
    uint32_t capB;             // checkpoint buckets available in bucket_to_tile / ckpt
    uint32_t* status;          // device status words: [2] |= 2 when the buckets did not fit; a non-zero [2] on entry aborts the kernel
    int tail4_from;            // set by launch_render_fwd: tiles from this index on are blended by FOUR waves (one quadrant each); >= gx * gy: none
    // depth forward (gslic_rasterize_forward_depth; all NULL otherwise): D = sum T alpha z over the colour's contributors
    float* out_depth;          // [H,W]
    float* ckpt_depth;         // [B*256] D at the start of each bucket, per pixel (SampleState::ckpt_depth)
    float* pix_depth;          // [T*256] tile-major final D (ImageState::pix_depth)
};
int launch_render_fwd(const RenderFwdArgs& a, hipStream_t s);

struct RenderBwdArgs {
    int W, H, gx, B;
    const uint2* ranges;
    const uint32_t* point_list;
    const uint32_t* inst_slot;
    const float4* rec;
    const uint32_t* bucket_offsets;
    const uint32_t* bucket_to_tile;
    const float4* ckpt;
    const uint64_t* hit;       // SampleState::hit (valid when status[GS_FLAG_HITBITS] != 0)
    const float4* pix_final;
    const uint32_t* max_contrib;
    const float* dL_dpix;
    float* partials;           // [9R] 36-byte rows, written for the instances of live buckets only
    uint8_t* dead;             // [R] set to 1 for the instances of dead buckets (zeroed by the forward)
    const uint32_t* status;    // device status words: a non-zero [2] (capacity overflow in the forward) aborts the kernel
    int T;                     // tiles: bucket_offsets[T - 1] is the real bucket count (B may be a capacity)
    int xcd_lg;                // log2 of the run of consecutive buckets one XCD takes (launch_render_bwd); < 0: bucket = blockIdx.x
    int skip_if_bits;          // pipeline kernel only: leave when the forward recorded decision masks (the row-scan kernel has done the work)
    // depth backward (gslic_rasterize_backward_depth; all NULL otherwise)
    const float* dL_ddepth;    // [H,W]
    const float* ckpt_depth;   // [B*256]
    const float* pix_depth;    // [T*256]
    float* partials_z;         // [R] dL/dz (view-space depth) per instance, written where `partials` is
};
int launch_render_bwd(const RenderBwdArgs& a, hipStream_t s);
int launch_render_bwd_scan(const RenderBwdArgs& b, unsigned grid, hipStream_t s);   // render_bwd_scan.hip: strict arithmetic, needs SampleState::hit

struct AdamFusedArgs {
    float *p[6], *m[6], *v[6];  // xyz, features_dc, features_rest, opacity, scaling, rotation
    float lr[6];
    float b1, b2, eps;
    int on;
};

struct PreprocessBwdArgs {
    int P, D, M, W, H, raw;
    int row_begin, row_end;   // Gaussians [row_begin, row_end) of the P are processed (the whole range by default; row_begin % 64 == 0): the N > 1
                              // exchange runs the per-Gaussian backward in chunks and ships a chunk while the next one is computed
    float focal_x, focal_y;
    float limx_neg, limx_pos, limy_neg, limy_pos, scale_modifier, lambda_erank;
    const float *means, *scales, *rots, *dc, *shs, *view, *proj, *campos;
    const int32_t* radii;
    const float4* rec;
    const uint32_t* tiles_touched;
    const uint32_t* gauss_start;
    const float* partials;
    const uint8_t* dead;
    float *dL_dmean2D, *dL_dconic, *dL_dopacity, *dL_dcolor, *dL_dmean3D, *dL_dcov3D, *dL_ddc, *dL_dsh, *dL_dscale, *dL_drot;
    float* dL_drgb;          // optional [P,3]: dL/d(SH colour) AFTER the clamp mask (backward.cu:41-44) — what the SH backward is linear in.
                             // When set it is written INSTEAD of dL_ddc (which must be NULL): the N > 1 exchange ships these 12 bytes per
                             // Gaussian and every rank rebuilds dL_ddc / dL_dsh of all views from them (launch_sh_grad_from_rgb)
    AdamFusedArgs adam;
    const uint32_t* status;  // device status words: a non-zero [2] (capacity overflow in the forward) aborts the kernel (no gradients, no Adam)
    uint8_t* vis_out;     // optional [P]: 1 = radii > 0 — the visibility byte of the N > 1 exchange's payload, written here instead of by a host compare + copy
    float* campos_out;    // optional [3]: a copy of campos next to it (the payload's camera centre)
    float* cam_partials;  // optional [ceil(P/64)][32]: per-wave sums of the 27 camera-gradient terms (NULL: not computed)
    float* cam_out;       // [35] = dL_dviewmatrix[16] | dL_dprojmatrix[16] | dL_dcampos[3]
    const float* partials_z;  // optional [R] (depth backward): dL/dz per instance, gathered like `partials`; dL_dmean3D += sum * (V[2], V[6], V[10])
};
// The three per-row accumulators of the gradient densification statistics (gslic_grad_stats, include/gslic_hip.h): storage row order, caller-owned.
struct GradStatArgs {
    float* grad_sum;       // [P] sum over views of |dL/dmean2D| (finite norms only)
    uint32_t* n_seen;      // [P] views that added a finite norm
    int32_t* max_radius;   // [P] largest screen radius seen
};
// gs != NULL (fused Adam only, no camera gradient): the *_gstat_kernel instantiations, which also apply the statistics rule to every visible row
int launch_preprocess_bwd(const PreprocessBwdArgs& a, hipStream_t s, const GradStatArgs* gs = nullptr);
int launch_preprocess_bwd_gstat(const PreprocessBwdArgs& a, const GradStatArgs& gs, bool lds_sh, bool defer, hipStream_t s);   // preprocess_bwd_gstat.hip
// preprocess_bwd_cam_adam.hip: what launch_preprocess_bwd adds for the camera gradient WITH the fused Adam (a.cam_partials and a.adam.on) — under depth
// the chain kernel (CAM and DEFER_XYZ; lds_sh as that function chose it) and the tail behind it, which forms the four direct view-matrix sums from
// the means as they were and then steps xyz; colour-only the reduction of the partial rows that honours the forward's overflow word
int launch_preprocess_bwd_cam_defer_xyz(const PreprocessBwdArgs& a, bool lds_sh, hipStream_t s);
int launch_depth_mean3d_cam_adam(const PreprocessBwdArgs& a, hipStream_t s);
int launch_cam_reduce_checked(size_t rows, const PreprocessBwdArgs& a, hipStream_t s);
// the same rule on a dL_dmean2D [P,3] the caller already has, rows [row_begin, row_end): one thread per row
int launch_gradient_stats(int row_begin, int row_end, const float* dL_dmean2D, const int32_t* radii, const GradStatArgs& gs, hipStream_t s);

// dL_ddc [P,3] and dL_dsh [P,M,3] summed over n_views views from the views' masked colour gradients (rgb_all [n_views][P][3], or the
// views' dL_ddc when input_is_ddc) and camera centres (campos_all [n_views][3]): the SH backward (backward.cu:27-136) is the outer
// product of a direction-only coefficient vector with that colour gradient.  View order 0..n_views-1, plain multiply-then-add.
struct ShGradFromRgbArgs {
    int P, D, M, n_views, input_is_ddc;
    size_t rgb_stride, campos_stride;   // floats between consecutive views in rgb_all / campos_all (3 P and 3 for the dense layouts)
    const float *means3D, *campos_all, *rgb_all;
    float *dL_ddc, *dL_dsh;     // outputs; both may be NULL when the Adam update below consumes the rows
    const uint8_t* visible;     // [P] the exchanged visibility mask: rows the Adam update applies to.  vis_stride > 0: the views' masks sit vis_stride
    size_t vis_stride;          // bytes apart (an all-gathered payload) and are OR-ed here; vis_out (optional [P]) receives the OR
    uint8_t* vis_out;
    const float* g_small[4];    // optional: the summed (all-reduced) dL_dxyz [P,3], dL_dopacity [P,1], dL_dscaling [P,3], dL_drotation [P,4]: when set, the
                                // masked Adam of groups 0, 3, 4, 5 runs here too — one launch for the whole optimiser step of an N > 1 rank
    AdamFusedArgs adam;         // on: groups 1 (features_dc) and 2 (features_rest) are updated in place from the rebuilt rows
};
int launch_sh_grad_from_rgb(const ShGradFromRgbArgs& a, hipStream_t s);

// row_ops.hip: the segmented row kernel behind gslic_gather_rows and the wide launch of gslic_densify_emit (segment semantics: its header).  A
// caller value-initialises the block, sets n_rows, adds its segments (the copies [0, n_copy) first, then the zero segments) and launches.
static constexpr int ROW_OPS_MAX_SEGMENTS = 32;      // segments per launch (the map has 19 row arrays)
struct RowOpsArgs {
    uint32_t* src[ROW_OPS_MAX_SEGMENTS];             // row 0 of the source (only a zero segment stores to it)
    uint32_t* dst[ROW_OPS_MAX_SEGMENTS];             // destination row 0
    uint32_t width[ROW_OPS_MAX_SEGMENTS];            // dwords per row (> 0)
    uint32_t rows_per_block[ROW_OPS_MAX_SEGMENTS];   // max(1, 4096 / width)
    uint32_t block_end[ROW_OPS_MAX_SEGMENTS];        // exclusive end of the segment's workgroups in the grid
    int n_copy, n_segments;
    uint32_t n_rows;                                 // destination rows of every segment = entries of index
    uint32_t src_rows;                               // an index >= src_rows is never used as an address: its destination row is left as it is
    const uint32_t* index;
    const float* scaling;                            // zero segments only: [src_rows, 3] raw scaling and the split threshold
    float split_above;
};
// appends a segment of rows `width` dwords wide (0: skipped) and cuts its share of the grid; false when the grid no longer fits 31 bits
bool row_ops_add(RowOpsArgs& a, const void* src, void* dst, uint32_t width);
int launch_row_ops(const RowOpsArgs& a, hipStream_t s);   // one launch, booked as gather_rows; nothing to do without segments

// prune.hip: the keep rule of gslic_prune_select on the raw parameters -> kept_index / new_tie / the two counts (one stream synchronisation), and
// the gather of gslic_gather_rows over row_ops (arguments validated by the caller; arrays of width 0 are skipped)
int prune_select(int P, const float* xyz, const float* dc, const float* opacity, const float* scaling, const float* rotation, float opacity_min,
                 float scaling_max, int drop_nonfinite, const uint8_t* drop, const uint8_t* protect, const uint32_t* tie_rank, int split_row,
                 gslic_alloc_fn alloc, void* ctx, uint32_t* kept_index, uint32_t* new_tie, int32_t* count, int32_t* count_below, hipStream_t s);
int gather_rows(const gslic_row_array* arrays, int n_arrays, const uint32_t* index, int n_rows, hipStream_t s);

// morton.hip: the key rule of gslic_morton_order and the stable argsort over its 30 bits -> perm / keys_sorted (no synchronisation), and the
// in-place row permutation of gslic_permute_rows: gather_rows into `staging` (array i at the running sum of the widths before it, times
// 4 n_rows bytes), then one device-to-device copy per array back (arguments validated by the caller)
int morton_order(int P, const float* xyz, const float* box, gslic_alloc_fn alloc, void* ctx, uint32_t* perm, uint32_t* keys_sorted, hipStream_t s);
size_t permute_rows_bytes(const gslic_row_array* arrays, int n_arrays, int n_rows);   // the sum of row_dwords * 4 * n_rows, not rounded
int permute_rows(const gslic_row_array* arrays, int n_arrays, const uint32_t* perm, int n_rows, void* staging, hipStream_t s);

// lidar_depth.hip: the LiDAR z-buffer of gslic_lidar_zbuffer_add (optional clear, then one 64-bit atomicMin per point) and its resolution into
// depth / index / near-bound images and the measured-pixel count by gslic_lidar_zbuffer_resolve (arguments validated by the caller)
int lidar_zbuffer_add(int n, const float* points, const float* Rcw, const float* tcw, float fx, float fy, float cx, float cy, int W, int H,
                      unsigned long long* zbuf, bool clear, int32_t index_base, hipStream_t s);
int lidar_zbuffer_resolve(int W, int H, const unsigned long long* zbuf, int footprint, float margin_abs, float margin_rel, float* depth_out,
                          int32_t* index_out, float* near_out, uint32_t* n_measured_out, hipStream_t s);
// ... and gslic_lidar_zbuffer_resolve_weighted: the same images plus the weight and dist2 images, in one launch of a kernel of its own
int lidar_zbuffer_resolve_weighted(int W, int H, const unsigned long long* zbuf, int footprint, float margin_abs, float margin_rel, float sigma_abs,
                                   float sigma_rel, float falloff, float* depth_out, int32_t* index_out, float* near_out, uint32_t* n_measured_out,
                                   float* weight_out, int32_t* dist2_out, hipStream_t s);

// contrib.hip: the per-Gaussian contribution statistics of gslic_contribution_accumulate from a completed forward's lists (one workgroup per tile;
// arguments validated by the caller; any of the three accumulators may be NULL)
struct ContribArgs {
    int W, H, gx, T, P;
    uint32_t R;                       // entries of the point list: the exact count, or the capacity the binning block was carved for
    const uint2* ranges;              // ImageState::ranges
    const uint32_t* point_list;       // BinningState::point_list()
    const float4* rec;                // GeomState::rec
    const float4* pix_final;          // ImageState::pix_final (.w = n_contrib bits, tile-major)
    const uint32_t* status;           // GeomState::flags: a non-zero [2] (capacity overflow) makes the kernel return
    float w_min;
    uint32_t* max_w;                  // [P] float bits
    uint32_t* n_pix;                  // [P]
    unsigned long long* sum_w;        // [P] 32.32 fixed point
};
// err_sum != NULL: the error-weighted variant of gslic_contribution_accumulate_error (err [H,W] row-major; err_sum [P] 32.32 fixed point)
// free_sum != NULL: the free-space variant of gslic_contribution_accumulate_free_space (near_bound [H,W] row-major; free_sum / meas_sum [P] 32.32)
int launch_contribution(const ContribArgs& a, hipStream_t s, const float* err = nullptr, unsigned long long* err_sum = nullptr,
                        const float* near_bound = nullptr, unsigned long long* free_sum = nullptr, unsigned long long* meas_sum = nullptr);

// contrib.hip: the per-pixel geometry images of gslic_geometry_images from a completed forward's lists (the same replay, one workgroup per tile, the
// per-pixel results kept instead of reduced per Gaussian; arguments validated by the caller; any of the seven images may be NULL)
struct GeometryArgs {
    int W, H, gx, T, P;
    uint32_t R;                       // as ContribArgs
    const uint2* ranges;
    const uint32_t* point_list;
    const float4* rec;
    const float4* pix_final;
    const uint32_t* status;
    float a_min;
    float* transmittance;             // each [H*W] row-major
    float* opacity;
    float* depth_sum;
    float* depth_norm;
    float* depth_median;
    int32_t* top_row;
    float* top_weight;
};
// lists = false (P == 0 or R == 0: no list exists, the forward's buffers are not read): every pixel gets the rule's initial values
int launch_geometry_images(const GeometryArgs& a, bool lists, hipStream_t s);

// densify.hip: the clone / split rule of gslic_densify_select on the raw parameters -> parent_index / the two counts (one stream synchronisation),
// and the new rows of gslic_densify_emit: the wide launch (copied fields, zeroed moments) and then one thread per parent (arguments validated by
// the caller)
int densify_select(int P, const float* xyz, const float* dc, const float* opacity, const float* scaling, const float* rotation, const uint8_t* grow,
                   const uint8_t* protect, const uint32_t* tie_rank, float split_above, gslic_alloc_fn alloc, void* ctx, uint32_t* parent_index,
                   int32_t* count, int32_t* count_split, hipStream_t s);
int densify_emit(int P, int count, const uint32_t* parent_index, int M, float* const param[6], float* const exp_avg[6], float* const exp_avg_sq[6],
                 uint32_t* tie_rank, float split_above, uint32_t seed, hipStream_t s);

// exposure.hip: the 3x4 affine exposure model of gslic_exposure_apply / gslic_exposure_backward (arguments validated by the caller).  The backward is
// two launches: dL_dimage and one row of twelve partial sums per workgroup, then one workgroup that adds the rows, writes dL_dE and — adam != NULL —
// applies the bias-corrected Adam update to the row *adam->view of the [V,12] arrays
int64_t exposure_partials_count(int H, int W);
int exposure_apply(int H, int W, const float* E, const float* image, float* out, hipStream_t s);
int exposure_backward(int H, int W, const float* E, const float* image, const float* dL_dout, float* dL_dimage, float* partials, float* dL_dE,
                      const gslic_exposure_adam* adam, hipStream_t s);

// keyframes.hip: the keyframe store's decode (one launch: colour and, with a mask slab, the weight; the slot index read from the device word
// `frame`, a word outside [0, n_frames) writes nothing) and encode (one launch per image given) of gslic_keyframe_decode / gslic_keyframe_encode
// (arguments validated by the caller; color_slot / mask_slot: the first byte of the slot written)
int keyframe_decode(int W, int H, int level, const uint8_t* color, const uint8_t* mask, const int32_t* frame, int n_frames, float* out, float* weight,
                    hipStream_t s);
int keyframe_encode(int W, int H, const float* image, const float* mask, uint8_t* color_slot, uint8_t* mask_slot, hipStream_t s);
// the depth slabs of gslic_keyframe_decode_depth / gslic_keyframe_encode_depth: one launch each (depth and, with a weight slab, the depth weight)
int keyframe_decode_depth(int W, int H, int level, const uint16_t* depth, const uint8_t* dweight, const int32_t* frame, int n_frames, float step,
                          float* depth_out, float* dweight_out, hipStream_t s);
int keyframe_encode_depth(int W, int H, const float* depth, const float* weight, uint16_t* depth_slot, uint8_t* dweight_slot, float step, hipStream_t s);

// pose.hip: the trainable pose set of gslic_pose_step / gslic_pose_load (arguments validated by the caller), one launch of one wave each: the
// se(3) chain, Adam, retraction, Gram-Schmidt and recomposition on row *d->view; the copy of row *view_word into three caller-owned buffers
int pose_step(const gslic_pose_adam* d, const float* dL_dviewmatrix, const float* dL_dprojmatrix, const float* dL_dcampos, float* grad_out, hipStream_t s);
int pose_load(const float* view_all, const float* proj_all, const float* campos_all, const int32_t* view_word, int n_views, float* view_out,
              float* proj_out, float* campos_out, hipStream_t s);

// pose_shared.hip: the calibration the views of a pose set share (arguments validated by the caller).  gslic_pose_step_shared: one launch of one
// workgroup — chain and Adam on seven coordinates by one thread, then one thread per row moves EVERY row, the accumulated correction X and tau;
// gslic_pose_calibrate_rows: one thread per row of [first, first + count), T <- exp((tau xi_j)^) (X T)
int pose_step_shared(const gslic_pose_shared* d, const float* dL_dviewmatrix, const float* dL_dprojmatrix, const float* dL_dcampos, float* grad_out,
                     hipStream_t s);
int pose_calibrate_rows(const gslic_pose_shared* d, int first, int count, hipStream_t s);

// covis.hip: covisibility bits uint32 [P, ceil(F / 32)] (arguments validated by the caller).  record: one thread per row of the range, one word
// loaded and stored; the three queries zero their outputs on the stream, then one launch each (LDS counters, integer atomics per workgroup)
int covis_record(int F, uint32_t* bits, const int32_t* radii, const uint8_t* visible, const int32_t* frame_word, const int32_t* skip, int row_begin,
                 int row_end, hipStream_t s);
int covis_pair_counts(int P, int F, const uint32_t* bits, uint32_t* pair, hipStream_t s);
int covis_frame_counts(int P, int F, const uint32_t* bits, const int32_t* frame_word, uint32_t* out, hipStream_t s);
int covis_row_counts(int P, int F, const uint32_t* bits, const uint32_t* frame_mask, int32_t* n_seen, int min_others, uint32_t* redundant, hipStream_t s);

}  // namespace gslic
