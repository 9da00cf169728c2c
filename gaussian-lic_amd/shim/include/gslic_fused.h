// gslic_fused.h — the fused training step for the reference's C++ host (header-only: LibTorch + include/gslic_hip.h).
//
// What optimize()'s loop body does per view (src/gaussian.cpp:674-716) —
//     render() -> l1_loss + fused_ssim -> loss.backward() -> set_visibility_and_N() -> SparseGaussianAdam::step()
// — as four C-ABI calls with no autograd graph, no LibTorch elementwise launch and no gradient tensor:
//     gslic_rasterize_forward (raw_params = 1: sigmoid / exp / normalize of gaussian.cpp:147-175 inside the kernels)
//     gslic_l1_ssim_loss_forward / _backward (loss_utils.h:30-33,130-193; the loss of gaussian.cpp:685-691)
//     gslic_rasterize_backward_adam (backward + the masked Adam of optim_utils.h:102-137 in the per-Gaussian kernel)
// The arithmetic equals the operator path's up to fp32 rounding (tests/test_fused_gpu.py); the C++ and the Python host
// (gaussian-lic_amd/trainer.py:training_step_fused) issue the same calls, so their parameters agree bit for bit
// (tests/test_shim_gpu.py::test_fused_cpp_host).  Single GPU: with N > 1 the gradients must exist for the exchange (gslic_dist.h).
//
//   gslic::FusedStep fs({xyz_, features_dc_, features_rest_, opacity_, scaling_, rotation_},
//                       {1.6e-4f, 2.5e-3f, 2.5e-3f / 20, 5e-2f, 5e-3f, 1e-3f}, sh_degree_);
//   for (view : keyframes) { auto terms = fs.step(cam, gt_image); }        // terms = device [mean |img - gt|, mean ssim]
//   float loss = fs.loss_value(terms);                                     // only when the host wants the number (one sync)
//
// LiDAR depth supervision (gt_depth [H,W], 0 = no measurement; loss += lambda_depth * masked mean |depth - gt_depth|):
//   auto terms = fs.step(cam, gt_image, gt_depth, lambda_depth);           // device [mean |img - gt|, mean ssim, L_d]
//   float loss = fs.loss_value(terms, lambda_depth);
// issues gslic_rasterize_forward_depth, the two loss calls, gslic_depth_l1_loss_forward_backward and gslic_rasterize_backward_depth_adam — the
// calls of the Python host's training_step_fused(gt_depth=, lambda_depth=), so the two agree bit for bit (tests/test_depth_fused_gpu.py).
// With a depth weight image [H,W] and / or a Huber threshold (fs.step(cam, gt, gt_depth, lambda_depth, weight, depth_weight, depth_huber)) the depth
// loss call is gslic_depth_loss_weighted_forward_backward, as training_step_fused(depth_weight=, depth_huber=)'s (tests/test_depth_weighted_gpu.py).
//
// Per-row statistics (ContributionStats, GradientStats, Covisibility) follow the map's rows the way the Python host's _RowStatistics do: each object lists its
// arrays ONCE (rows(): tensor, scalar type, row width in dwords, created only when asked for), and the four row changes — prune, extend, densify,
// resort — walk the lists of the objects they carry (the ContributionStats* argument when it holds anything, the attached GradientStats and
// Covisibility) with four
// operations: fit to capacity, gather, zero rows, append to the permute list.  A new array is a field, an entry in its list and its accumulate call.
#pragma once
#include <torch/torch.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <limits>
#include <optional>
#include <vector>

#include "gslic_stream.h"
#include "../../../include/gslic_hip.h"

namespace gslic {

// the fields of Camera that reach the rasterizer (src/camera.h:38-110, renderer.cpp:28-50)
struct FusedCamera {
    int image_width = 0, image_height = 0;
    float tanfovx = 0, tanfovy = 0, limx_neg = 0, limx_pos = 0, limy_neg = 0, limy_pos = 0;
    torch::Tensor world_view_transform, full_proj_transform, camera_center;  // device fp32 [4,4] (stored transposed, camera.h:86,109), [4,4], [3]
};

// One per-row array of a statistics object, as the row changes of FusedStep see it
struct StatRow {
    torch::Tensor* array;     // [capacity] (cols == 0) or [capacity, cols] on the map's device, indexed by storage row
    torch::ScalarType type;
    uint32_t width;           // row width in dwords: 1 or 2 for a 1-D array, cols of an int32 [capacity, cols] array
    bool lazy;                // exists only once an accumulate call asked for it; until then the row changes pass over it
    int64_t cols = 0;         // the trailing dimension of a 2-D array (0: the array is 1-D)
};

// Per-Gaussian contribution statistics accumulated over views (gslic_contribution_accumulate, include/gslic_hip.h) — the Python host's
// trainer.ContributionStats as plain data: device arrays indexed by storage row, created (zero) and grown to the map's capacity by
// FusedStep::accumulate_contribution, carried through the row changes of FusedStep when handed to them.  Rows behind size() are zero, so rows
// appended by extend() start at zero.  max_w.view(kFloat32) is the largest weight; sum in float units = sum_w / 2^32.
struct ContributionStats {
    torch::Tensor max_w;   // int32 [capacity]: uint32 float bits of the largest w = alpha T
    torch::Tensor n_pix;   // int32 [capacity]: uint32 count of (pixel, view) pairs with w >= w_min (saturating)
    torch::Tensor sum_w;   // int64 [capacity]: uint64 sum of w, 32.32 fixed point
    torch::Tensor err_sum; // int64 [capacity]: uint64 sum of w e(p), 32.32 fixed point — undefined until a view is accumulated with an error image
    torch::Tensor free_sum; // int64 [capacity]: uint64 sum of w over the measured pixels the row lies in front of (z_g < near_bound[p]), 32.32 fixed point
    torch::Tensor meas_sum; // int64 [capacity]: uint64 sum of w over the measured pixels (near_bound[p] > 0) — both undefined until accumulate_free_space
    int64_t views = 0;
    bool defined() const { return max_w.defined(); }   // an object no view was accumulated into is not carried
    std::vector<StatRow> rows()
    {
        return {{&max_w, torch::kInt32, 1u, false}, {&n_pix, torch::kInt32, 1u, false}, {&sum_w, torch::kInt64, 2u, false},
                {&err_sum, torch::kInt64, 2u, true}, {&free_sum, torch::kInt64, 2u, true}, {&meas_sum, torch::kInt64, 2u, true}};
    }
};

// The gradient densification statistics of 3DGS accumulated over views (gslic_grad_stats, include/gslic_hip.h) — the Python host's
// trainer.GradientStats as plain data: per storage row the sum of the norms of dL/dmean2D (xyz_gradient_accum), the number of views that added one
// (denom) and the largest screen radius (max_radii2D).  Handed to FusedStep::set_gradient_stats, every step() adds its view inside the backward
// kernel, and prune / extend / densify / resort carry the arrays with the rows (created zero-filled, grown to the map's capacity; rows behind
// size() are zero).  When to densify or reset, and with which thresholds, is the host's policy.
struct GradientStats {
    torch::Tensor grad_sum;     // float32 [capacity]
    torch::Tensor n_seen;       // int32 [capacity]: uint32 count
    torch::Tensor max_radius;   // int32 [capacity]
    bool defined() const { return grad_sum.defined(); }
    std::vector<StatRow> rows() { return {{&grad_sum, torch::kFloat32, 1u, false}, {&n_seen, torch::kInt32, 1u, false}, {&max_radius, torch::kInt32, 1u, false}}; }
    void reset() { if (defined()) { grad_sum.zero_(); n_seen.zero_(); max_radius.zero_(); } }
    gslic_grad_stats descriptor() { return {grad_sum.data_ptr<float>(), reinterpret_cast<uint32_t*>(n_seen.data_ptr<int32_t>()), max_radius.data_ptr<int32_t>()}; }   // what the backward takes
    // bool [P] for FusedStep::densify: n_seen >= max(min_seen, 1) and grad_sum >= float(grad_above) * float(n_seen) — comparisons and one float32
    // product, the Python host's grow_mask (3DGS's >= is kept; a NaN sum does not grow)
    torch::Tensor grow_mask(int64_t P, float grad_above, int64_t min_seen = 1) const
    {
        const torch::Tensor n = n_seen.narrow(0, 0, P).to(torch::kInt64).bitwise_and(0xffffffffLL);
        const torch::Tensor lim = torch::full({}, grad_above, grad_sum.options()) * n.to(torch::kFloat32);
        return n.ge(std::max<int64_t>(min_seen, 1)).logical_and(grad_sum.narrow(0, 0, P).ge(lim));
    }
    // bool [P] for FusedStep::prune(drop): max_radius > max_screen_radius (3DGS's screen-size prune)
    torch::Tensor big_mask(int64_t P, int32_t max_screen_radius) const { return max_radius.narrow(0, 0, P).gt(max_screen_radius); }
};

// Covisibility sets (gslic_covis_*, include/gslic_hip.h) — the Python host's trainer.Covisibility as plain data: one bit per (row, frame) in
// int32 [capacity, Wd] rows, Wd = ceil(n_frames / 32); bit f of a row says "frame f, when last recorded, had radii > 0 on this row".  Handed to
// FusedStep::set_covisibility, FusedStep::record_covisibility(frame) replaces the frame's column by the last step's radii > 0, and prune / extend /
// densify / resort carry the rows (gathered, zero for new rows and split parents, permuted: one more row array of run-time width).  The queries
// take the map's row count P (FusedStep::size()) and read nothing back; which keyframe to give up and which rows to protect is the host's policy.
struct Covisibility {
    int32_t n_frames;
    torch::Tensor bits;    // int32 [capacity, Wd]
    torch::Tensor word;    // int32 [1]: the frame word of the calls that name their frame by a host int
    explicit Covisibility(int32_t frames) : n_frames(frames)
    {
        TORCH_CHECK(frames >= 1 && frames <= GSLIC_COVIS_MAX_FRAMES, "Covisibility: n_frames = ", frames, " is outside 1 .. ", GSLIC_COVIS_MAX_FRAMES);
    }
    int64_t words() const { return (n_frames + 31) / 32; }
    bool defined() const { return bits.defined(); }
    std::vector<StatRow> rows() { return {{&bits, torch::kInt32, (uint32_t)words(), false, words()}}; }
    void reset() { if (defined()) bits.zero_(); }
    // column `frame` <- seen: radii (int32 [P]: seen where > 0) or a visibility mask (bool / uint8 [P]); an undefined tensor clears the column
    void record(int64_t P, int frame, const torch::Tensor& seen = torch::Tensor())
    {
        ready(P);
        const bool radii = seen.defined() && seen.scalar_type() == torch::kInt32;
        TORCH_CHECK(!seen.defined() || (seen.dim() == 1 && seen.size(0) == P && (radii || seen.scalar_type() == torch::kBool || seen.scalar_type() == torch::kByte)),
                    "Covisibility::record: seen must be radii (int32) or a visibility mask (bool / uint8) of ", P, " rows");
        if (P == 0) return;
        const torch::Tensor s = seen.defined() ? seen.contiguous() : seen;
        check(gslic_covis_record((int32_t)P, n_frames, u32(bits), radii ? s.data_ptr<int32_t>() : nullptr,
                                 s.defined() && !radii ? static_cast<const uint8_t*>(s.data_ptr()) : nullptr, frame_word(frame), nullptr, 0, -1,
                                 current_stream()), "gslic_covis_record");
    }
    void clear(int64_t P, int frame) { record(P, frame); }
    torch::Tensor pair_counts(int64_t P)   // int64 [F, F]
    {
        ready(P);
        torch::Tensor out = torch::zeros({n_frames, n_frames}, bits.options());
        if (P) check(gslic_covis_pair_counts((int32_t)P, n_frames, u32(bits), u32(out), current_stream()), "gslic_covis_pair_counts");
        return out.to(torch::kInt64);
    }
    torch::Tensor frame_counts(int64_t P, int frame)   // int64 [F]
    {
        ready(P);
        torch::Tensor out = torch::zeros({n_frames}, bits.options());
        if (P) check(gslic_covis_frame_counts((int32_t)P, n_frames, u32(bits), frame_word(frame), u32(out), current_stream()), "gslic_covis_frame_counts");
        return out.to(torch::kInt64);
    }
    // int32 [P]: how many of the frames of frame_mask (int32 [Wd] device words; undefined: every frame) see each row
    torch::Tensor seen_count(int64_t P, const torch::Tensor& frame_mask = torch::Tensor()) { return row_counts(P, frame_mask, 0, nullptr); }
    // int64 [F]: [f] = the rows f sees that at least 1 + min_others frames (of frame_mask) see
    torch::Tensor redundant(int64_t P, int min_others, const torch::Tensor& frame_mask = torch::Tensor())
    {
        torch::Tensor red;
        row_counts(P, frame_mask, min_others, &red);
        return red.to(torch::kInt64);
    }
    torch::Tensor rows_of(int64_t P, int frame)   // bool [P]
    {
        ready(P);
        TORCH_CHECK(frame >= 0 && frame < n_frames, "Covisibility: frame ", frame, " is outside [0, ", n_frames, ")");
        return bits.narrow(0, 0, P).select(1, frame >> 5).bitwise_right_shift(frame & 31).bitwise_and(1).to(torch::kBool);
    }
    torch::Tensor seen_by_fewer_than(int64_t P, int n, const torch::Tensor& frame_mask = torch::Tensor()) { return seen_count(P, frame_mask).lt(n); }   // bool [P]
    torch::Tensor overlap(int64_t P, int frame)   // float32 [F]: frame_counts / the frame's own count, 0 where it sees nothing
    {
        const torch::Tensor fc = frame_counts(P, frame).to(torch::kFloat32), own = fc[frame];
        return torch::where(own.gt(0), fc / own.clamp_min(1.0f), torch::zeros_like(fc));
    }

private:
    static void check(int rc, const char* what) { TORCH_CHECK(rc == GSLIC_OK, what, " failed (", rc, "): ", gslic_last_error()); }
    static uint32_t* u32(torch::Tensor& t) { return reinterpret_cast<uint32_t*>(t.data_ptr<int32_t>()); }
    void ready(int64_t P) const { TORCH_CHECK(defined() && bits.size(0) >= P, "Covisibility: not attached to a map of ", P, " rows (FusedStep::set_covisibility)"); }
    const int32_t* frame_word(int frame)
    {
        TORCH_CHECK(frame >= 0 && frame < n_frames, "Covisibility: frame ", frame, " is outside [0, ", n_frames, ")");
        if (!word.defined()) word = torch::zeros({1}, bits.options());
        word.fill_(frame);
        return word.data_ptr<int32_t>();
    }
    torch::Tensor row_counts(int64_t P, const torch::Tensor& frame_mask, int min_others, torch::Tensor* red)
    {
        ready(P);
        TORCH_CHECK(!frame_mask.defined() || (frame_mask.scalar_type() == torch::kInt32 && frame_mask.numel() == words() && frame_mask.is_contiguous()),
                    "Covisibility: frame_mask must be ", words(), " contiguous int32 words");
        torch::Tensor n_seen = torch::zeros({P}, bits.options());
        if (red) *red = torch::zeros({n_frames}, bits.options());
        if (P)
            check(gslic_covis_row_counts((int32_t)P, n_frames, u32(bits), frame_mask.defined() ? reinterpret_cast<const uint32_t*>(frame_mask.data_ptr<int32_t>()) : nullptr,
                                         n_seen.data_ptr<int32_t>(), min_others, red ? u32(*red) : nullptr, current_stream()), "gslic_covis_row_counts");
        return n_seen;
    }
};

// The per-pixel LiDAR range image of one camera, built by the library (gslic_lidar_zbuffer_add / _resolve, include/gslic_hip.h) — the Python host's
// trainer.LidarDepth: it owns the z-buffer of width * height 64-bit keys on `device`.  The reference's host builds the image on the CPU
// (gaussian.cpp:554-572).  resolve()'s depth is usable as it is as the gt_depth of FusedStep::step and pose_gradient, its near_bound as the near_bound of
// FusedStep::accumulate_free_space.  Every call runs on the current stream, allocates only its result tensors and reads nothing back.
struct LidarImages {
    torch::Tensor depth;        // float32 [H,W]: nearest return of the pixel's window, 0 = none
    torch::Tensor near_bound;   // float32 [H,W]: depth - (margin_abs + margin_rel * depth) where measured, 0 elsewhere (only with margins)
    torch::Tensor index;        // int32 [H,W]: the winning point, -1 = none (only when asked for)
    torch::Tensor n_measured;   // int32 scalar on the device: measured pixels (only when asked for)
    torch::Tensor weight;       // float32 [H,W]: range weight times 1 / (1 + falloff * dist2), 0 = none; a depth_weight as it is (only with weight)
    torch::Tensor dist2;        // int32 [H,W]: squared pixel distance to the return the pixel was given, -1 = none (only when asked for)
};
// The per-pixel geometry images of one view (gslic_geometry_images, include/gslic_hip.h) — what the Python host's trainer.geometry_images
// returns: FusedStep::geometry_images writes the tensors that are DEFINED, each [H,W] on the map's device (float32, top_row int32); make()
// allocates the ones asked for.  Tensors a caller keeps are reused by the next call of the same size: no allocation, capturable in a graph.
struct GeometryImages {
    torch::Tensor transmittance;   // the forward's final_T
    torch::Tensor opacity;         // A = sum of w = alpha T
    torch::Tensor depth_sum;       // D = sum of T alpha z (the depth the loss trains on)
    torch::Tensor depth_norm;      // D / A where A >= a_min, 0 elsewhere
    torch::Tensor depth_median;    // the view depth of the entry that takes T below one half, 0: never reached
    torch::Tensor top_row;         // int32: the STORAGE row of the largest w, -1: no contributor
    torch::Tensor top_weight;      // that w
    std::array<torch::Tensor*, 7> all() { return {&transmittance, &opacity, &depth_sum, &depth_norm, &depth_median, &top_row, &top_weight}; }
    // allocates (on demand: a tensor of the right size stays) the images whose flag is set, in the order of all()
    void make(int64_t H, int64_t W, torch::Device device, std::array<bool, 7> want = {false, true, false, true, true, true, false})
    {
        const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(device);
        const auto imgs = all();
        for (int i = 0; i < 7; i++) {
            torch::Tensor& t = *imgs[i];
            if (!want[i]) { t = torch::Tensor(); continue; }
            if (!t.defined() || t.size(0) != H || t.size(1) != W) t = torch::empty({H, W}, i == 5 ? f32.dtype(torch::kInt32) : f32);
        }
    }
};

// Trainable per-view exposure — the Python host's trainer.Exposure: one 3x4 affine colour transform per view (which views share a row is the
// host's policy), applied to the rendered image before the loss (gslic_exposure_apply / gslic_exposure_backward, include/gslic_hip.h).  The
// reference's host owns such a tensor with an Adam of its own (gaussian.cpp:287-291, :419-422, :708-711) and never applies it; n_views = 1 is
// that tensor.  params [V,3,4] starts at [I | 0]; m, v and steps [V] int32 are torch::optim::Adam's state (bias-corrected), grad [3,4] the last
// dL/dE.  Handed to FusedStep::set_exposure, step() updates the view's row inside the exposure backward's second launch.
struct Exposure {
    torch::Tensor params, m, v;   // float32 [V,3,4]
    torch::Tensor steps;          // int32 [V]
    torch::Tensor grad;           // float32 [3,4]
    torch::Tensor views;          // int32 [V] = 0 .. V-1: the device word that names view i is views[i]
    float lr, beta1, beta2, eps;
    Exposure(int64_t n_views, torch::Device device = torch::kCUDA, float lr_ = 0.01f, float beta1_ = 0.9f, float beta2_ = 0.999f, float eps_ = 1e-8f)
        : lr(lr_), beta1(beta1_), beta2(beta2_), eps(eps_)
    {
        TORCH_CHECK(n_views >= 1, "Exposure: n_views must be at least 1");
        const auto fo = torch::TensorOptions().dtype(torch::kFloat32).device(device);
        params = torch::eye(3, 4, fo).unsqueeze(0).repeat({n_views, 1, 1}).contiguous();
        m = torch::zeros_like(params); v = torch::zeros_like(params);
        steps = torch::zeros({n_views}, fo.dtype(torch::kInt32));
        grad = torch::zeros({3, 4}, fo);
        views = torch::arange(n_views, fo.dtype(torch::kInt32));
    }
    int64_t n_views() const { return params.size(0); }
    torch::Tensor matrix(int64_t view) const   // the [3,4] transform of a view: a view into params
    {
        TORCH_CHECK(view >= 0 && view < n_views(), "Exposure: view ", view, " is outside [0, ", n_views(), ")");
        return params[view];
    }
    gslic_exposure_adam descriptor(int64_t view) const
    {
        matrix(view);
        gslic_exposure_adam ad{};
        ad.param = params.data_ptr<float>(); ad.m = m.data_ptr<float>(); ad.v = v.data_ptr<float>(); ad.step_count = steps.data_ptr<int32_t>();
        ad.view = views.data_ptr<int32_t>() + view;
        ad.lr = lr; ad.beta1 = beta1; ad.beta2 = beta2; ad.eps = eps;
        return ad;
    }
};

// Trainable keyframe poses on the device — the Python host's trainer.PoseSet: per view the three arrays the rasteriser reads (view, proj [V,16],
// campos [V,3], the layout of FusedCamera's tensors), torch::optim::Adam's state on the six coordinates of a left se(3) increment (m, v [V,6],
// steps [V] int32, bias-corrected, one rate for the translation and one for the rotation) and the shared projection [16].  gslic_pose_step — one
// launch — chains the three camera gradients, steps the row and retracts the pose (the rule is written out in include/gslic_hip.h); grad [6] is
// the last gradient.  load() takes a camera's three arrays as they are; row_camera() hands the row back as views (no copy, no synchronisation).
// shared = true adds the calibration the views SHARE, as the Python host's PoseSet(shared=True): twist [V,6] (camera-frame (v, w) of each view),
// Adam's state sm, sv [7], ssteps [1] on (rho_x, phi_x, tau) with the rates lr_trans, lr_rot, lr_time, the accumulated extrinsic correction X [12]
// (rows of [R_x | t_x]), the accumulated time offset tau [1] and shared_grad [7].  gslic_pose_step_shared (shared_adam_step) steps the seven
// coordinates from one view's gradient and moves EVERY row; gslic_pose_calibrate_rows (calibrate_rows, load(..., calibrated = true)) brings a row
// loaded later to the calibration.  shared = false is the set as it is without.
struct PoseSet {
    torch::Tensor view, proj;     // float32 [V,16]
    torch::Tensor campos;         // float32 [V,3]
    torch::Tensor m, v;           // float32 [V,6]
    torch::Tensor steps;          // int32 [V]
    torch::Tensor projection;     // float32 [16]: Camera.projection_matrix, element (r, c) at [4 c + r]
    torch::Tensor grad;           // float32 [6]
    torch::Tensor views;          // int32 [V] = 0 .. V-1: the device word that names view i is views[i]
    torch::Tensor no_step;        // int32 [1] = 1: a skip word that is set (the chain alone)
    float lr_trans, lr_rot, beta1, beta2, eps;
    bool shared;                  // the tensors below are defined
    float lr_time;
    torch::Tensor twist;          // float32 [V,6]
    torch::Tensor sm, sv;         // float32 [7]
    torch::Tensor ssteps;         // int32 [1]
    torch::Tensor X;              // float32 [12]: rows of [R_x | t_x]
    torch::Tensor tau;            // float32 [1], seconds
    torch::Tensor shared_grad;    // float32 [7]
    // projection16: the pose-independent projection the views share, 16 floats in any float32 tensor (host or device)
    PoseSet(int64_t n_views, const torch::Tensor& projection16, torch::Device device = torch::kCUDA, float lr_rot_ = 1e-3f, float lr_trans_ = 1e-3f,
            float beta1_ = 0.9f, float beta2_ = 0.999f, float eps_ = 1e-8f, bool shared_ = false, float lr_time_ = 0.0f)
        : lr_trans(lr_trans_), lr_rot(lr_rot_), beta1(beta1_), beta2(beta2_), eps(eps_), shared(shared_), lr_time(lr_time_)
    {
        TORCH_CHECK(lr_time_ >= 0.0f, "PoseSet: lr_time must be >= 0");
        TORCH_CHECK(shared_ || lr_time_ == 0.0f, "PoseSet: lr_time given to a set built without shared");
        TORCH_CHECK(n_views >= 1, "PoseSet: n_views must be at least 1");
        TORCH_CHECK(projection16.numel() == 16 && projection16.scalar_type() == torch::kFloat32, "PoseSet: projection must be 16 float32 values");
        const auto fo = torch::TensorOptions().dtype(torch::kFloat32).device(device);
        view = torch::zeros({n_views, 16}, fo); proj = torch::zeros({n_views, 16}, fo); campos = torch::zeros({n_views, 3}, fo);
        m = torch::zeros({n_views, 6}, fo); v = torch::zeros({n_views, 6}, fo);
        steps = torch::zeros({n_views}, fo.dtype(torch::kInt32));
        projection = projection16.reshape({16}).to(device).contiguous().clone();
        grad = torch::zeros({6}, fo);
        views = torch::arange(n_views, fo.dtype(torch::kInt32));
        no_step = torch::ones({1}, fo.dtype(torch::kInt32));
        if (shared) {
            twist = torch::zeros({n_views, 6}, fo);
            sm = torch::zeros({7}, fo); sv = torch::zeros({7}, fo); ssteps = torch::zeros({1}, fo.dtype(torch::kInt32));
            X = torch::eye(3, 4, fo).reshape({12}).contiguous();
            tau = torch::zeros({1}, fo);
            shared_grad = torch::zeros({7}, fo);
        }
    }
    int64_t n_views() const { return view.size(0); }
    void need_shared(const char* who) const { TORCH_CHECK(shared, who, ": the pose set was built without shared"); }
    void set_twist(int64_t i, const torch::Tensor& xi)   // the camera-frame twist (v, w) of row i: six float32 values, host or device
    {
        need_shared("PoseSet::set_twist");
        index(i);
        TORCH_CHECK(xi.numel() == 6 && xi.scalar_type() == torch::kFloat32, "PoseSet: a twist is six float32 values");
        twist[i].copy_(xi.reshape({6}));
    }
    // load, then (twist defined) set_twist, then (calibrated) gslic_pose_calibrate_rows on the row: T <- exp((tau xi)^) (X T)
    void load(int64_t i, const FusedCamera& cam, const torch::Tensor& xi, bool calibrated = false)
    {
        need_shared("PoseSet::load");
        load(i, cam);
        if (xi.defined()) set_twist(i, xi);
        if (calibrated) calibrate_rows(i, 1);
    }
    void reset_shared_moments() { need_shared("PoseSet::reset_shared_moments"); sm.zero_(); sv.zero_(); ssteps.zero_(); shared_grad.zero_(); }   // X and tau stay
    torch::Tensor extrinsic() const { need_shared("PoseSet::extrinsic"); return X.to(torch::kCPU).reshape({3, 4}); }   // [R_x | t_x] on the host; synchronises
    float time_offset() const { need_shared("PoseSet::time_offset"); return tau.to(torch::kCPU).item<float>(); }         // seconds; synchronises
    gslic_pose_shared shared_descriptor(int64_t i, bool do_step = true) const
    {
        need_shared("PoseSet");
        index(i);
        gslic_pose_shared d{};
        d.view_all = view.data_ptr<float>(); d.proj_all = proj.data_ptr<float>(); d.campos_all = campos.data_ptr<float>();
        d.projection = projection.data_ptr<float>(); d.view = views.data_ptr<int32_t>() + i; d.n_views = (int32_t)n_views();
        d.twist = twist.data_ptr<float>(); d.sm = sm.data_ptr<float>(); d.sv = sv.data_ptr<float>(); d.ssteps = ssteps.data_ptr<int32_t>();
        d.X = X.data_ptr<float>(); d.tau = tau.data_ptr<float>();
        d.lr_trans = lr_trans; d.lr_rot = lr_rot; d.lr_time = lr_time; d.beta1 = beta1; d.beta2 = beta2; d.eps = eps;
        d.skip = do_step ? nullptr : reinterpret_cast<const uint32_t*>(no_step.data_ptr<int32_t>());
        return d;
    }
    // gslic_pose_step_shared on gradients the caller holds (camg as adam_step's), taken as row i's: shared_grad <- (g, xi_i . g); do_step: every row moves
    void shared_adam_step(int64_t i, const torch::Tensor& camg, bool do_step = true)
    {
        TORCH_CHECK(camg.numel() == 35 && camg.scalar_type() == torch::kFloat32 && camg.is_contiguous(), "PoseSet: camg must be 35 contiguous float32 values");
        const gslic_pose_shared d = shared_descriptor(i, do_step);
        const float* g = camg.data_ptr<float>();
        const int rc = gslic_pose_step_shared(&d, g, g + 16, g + 32, shared_grad.data_ptr<float>(), current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_pose_step_shared failed (", rc, "): ", gslic_last_error());
    }
    void calibrate_rows(int64_t first, int64_t count)   // gslic_pose_calibrate_rows on rows [first, first + count)
    {
        const gslic_pose_shared d = shared_descriptor(0);
        const int rc = gslic_pose_calibrate_rows(&d, (int32_t)first, (int32_t)count, current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_pose_calibrate_rows failed (", rc, "): ", gslic_last_error());
    }
    int64_t index(int64_t i) const
    {
        TORCH_CHECK(i >= 0 && i < n_views(), "PoseSet: view ", i, " is outside [0, ", n_views(), ")");
        return i;
    }
    void load(int64_t i, const FusedCamera& cam)   // bit copies of the camera's three arrays; zero moments and step count
    {
        index(i);
        view[i].copy_(cam.world_view_transform.reshape({16})); proj[i].copy_(cam.full_proj_transform.reshape({16})); campos[i].copy_(cam.camera_center.reshape({3}));
        m[i].zero_(); v[i].zero_(); steps[i].zero_();
    }
    // The row as the camera a render takes: device VIEWS into the set (no copy, no synchronisation) with the image size and scalars of
    // `intrinsics` — the Python host's pose(view), not its camera(view), which reads the row back into a host Camera.
    FusedCamera row_camera(int64_t i, const FusedCamera& intrinsics) const
    {
        index(i);
        FusedCamera cam = intrinsics;
        cam.world_view_transform = view[i].view({4, 4}); cam.full_proj_transform = proj[i].view({4, 4}); cam.camera_center = campos[i];
        return cam;
    }
    void reset_moments(int64_t i = -1)   // zero moments and step count: one view, or (i < 0) all of them and the last gradient
    {
        if (i < 0) { m.zero_(); v.zero_(); steps.zero_(); grad.zero_(); return; }
        index(i);
        m[i].zero_(); v[i].zero_(); steps[i].zero_();
    }
    // The set's state by value — what the Python host's state_dict / load_state_dict / clone carry: the rows, the moments, the step counts, the
    // scalars and (clone) the last gradient.  copy_from refuses a set of another size or another projection.
    void copy_from(const PoseSet& o)
    {
        TORCH_CHECK(o.n_views() == n_views(), "PoseSet: the state holds ", o.n_views(), " views, this object ", n_views());
        TORCH_CHECK(torch::equal(o.projection.to(projection.device()), projection), "PoseSet: the state was saved under another projection");
        view.copy_(o.view); proj.copy_(o.proj); campos.copy_(o.campos); m.copy_(o.m); v.copy_(o.v); steps.copy_(o.steps);
        lr_trans = o.lr_trans; lr_rot = o.lr_rot; beta1 = o.beta1; beta2 = o.beta2; eps = o.eps;
        TORCH_CHECK(o.shared == shared, "PoseSet: one of the two sets was built with shared, the other without");
        if (shared) {
            twist.copy_(o.twist); sm.copy_(o.sm); sv.copy_(o.sv); ssteps.copy_(o.ssteps); X.copy_(o.X); tau.copy_(o.tau);
            lr_time = o.lr_time;
        }
    }
    PoseSet clone() const
    {
        PoseSet other(n_views(), projection, projection.device(), lr_rot, lr_trans, beta1, beta2, eps, shared, lr_time);
        other.copy_from(*this);
        other.grad.copy_(grad);
        if (shared) other.shared_grad.copy_(shared_grad);
        return other;
    }
    gslic_pose_adam descriptor(int64_t i, bool do_step = true) const
    {
        index(i);
        gslic_pose_adam d{};
        d.view_all = view.data_ptr<float>(); d.proj_all = proj.data_ptr<float>(); d.campos_all = campos.data_ptr<float>();
        d.m = m.data_ptr<float>(); d.v = v.data_ptr<float>(); d.step_count = steps.data_ptr<int32_t>(); d.projection = projection.data_ptr<float>();
        d.view = views.data_ptr<int32_t>() + i; d.n_views = (int32_t)n_views();
        d.lr_trans = lr_trans; d.lr_rot = lr_rot; d.beta1 = beta1; d.beta2 = beta2; d.eps = eps;
        d.skip = do_step ? nullptr : reinterpret_cast<const uint32_t*>(no_step.data_ptr<int32_t>());
        return d;
    }
    // gslic_pose_step on gradients the caller holds: camg = dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3] in one device tensor of 35 floats
    void adam_step(int64_t i, const torch::Tensor& camg, bool do_step = true)
    {
        TORCH_CHECK(camg.numel() == 35 && camg.scalar_type() == torch::kFloat32 && camg.is_contiguous(), "PoseSet: camg must be 35 contiguous float32 values");
        const gslic_pose_adam d = descriptor(i, do_step);
        const float* g = camg.data_ptr<float>();
        const int rc = gslic_pose_step(&d, g, g + 16, g + 32, grad.data_ptr<float>(), current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_pose_step failed (", rc, "): ", gslic_last_error());
    }
    // gslic_pose_load: the row the device word names into three buffers (how a captured step reads its pose)
    void load_row(const torch::Tensor& view_word, torch::Tensor& view_out, torch::Tensor& proj_out, torch::Tensor& campos_out) const
    {
        const int rc = gslic_pose_load(view.data_ptr<float>(), proj.data_ptr<float>(), campos.data_ptr<float>(), view_word.data_ptr<int32_t>(),
                                       (int32_t)n_views(), view_out.data_ptr<float>(), proj_out.data_ptr<float>(), campos_out.data_ptr<float>(), current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_pose_load failed (", rc, "): ", gslic_last_error());
    }
};

// The keyframes' ground-truth images on the device as 8-bit pixels — the Python host's trainer.KeyframeStore (gslic_keyframe_encode /
// gslic_keyframe_decode; storage, decode and encode rules in include/gslic_hip.h).  color: uint8 [capacity,H,W,3] interleaved RGB; mask (masks =
// true): uint8 [capacity,H,W], decoded into the float32 weight image the weighted loss takes.  target() is usable as it is as the gt_image (and weight)
// of FusedStep::step.  The reference keeps every keyframe as a float32 CPU tensor and uploads it at every step (gaussian.cpp:49, :80, :678).
// depths = true: every slot also holds its LiDAR range image as 16-bit codes (depth: uint16 [capacity,H,W], 0 = not measured, k = depth k *
// depth_step, depth_step a power of two in [2^-16, 1]) and, depth_weights = true, an 8-bit confidence weight (dweight: uint8 [capacity,H,W]) —
// gslic_keyframe_encode_depth / gslic_keyframe_decode_depth.  depth_target() is usable as it is as the gt_depth (and depth_weight) of FusedStep::step.
struct KeyframeTarget {
    torch::Tensor image;    // float32 [3,H_l,W_l]
    torch::Tensor weight;   // float32 [H_l,W_l] (a store with masks), undefined otherwise
};
struct KeyframeDepthTarget {
    torch::Tensor depth;    // float32 [H_l,W_l], 0 = not measured
    torch::Tensor weight;   // float32 [H_l,W_l] (a store with depth weights), undefined otherwise
};
class KeyframeStore {
public:
    torch::Tensor color, mask;   // the slabs
    torch::Tensor depth, dweight;   // the depth slabs (depths / depth_weights), undefined otherwise
    KeyframeStore(int width, int height, int capacity, torch::Device device = torch::kCUDA, bool masks = false, bool depths = false,
                  float depth_step = 0.001953125f /*2^-9*/, bool depth_weights = false)
        : W_(width), H_(height), cap_(capacity), depth_step_(depth_step)
    {
        TORCH_CHECK(width >= 1 && height >= 1 && capacity >= 1, "KeyframeStore: width, height and capacity must all be at least 1");
        TORCH_CHECK(depths || !depth_weights, "KeyframeStore: depth_weights needs depths (the weight is the depth's)");
        int e = 0;
        TORCH_CHECK(!depths || (depth_step > 0.0f && depth_step <= 1.0f && std::frexp(depth_step, &e) == 0.5f && e >= -15),
                    "KeyframeStore: depth_step = ", depth_step, " must be a power of two in [2^-16, 1]");
        const auto u8 = torch::TensorOptions().dtype(torch::kByte).device(device);
        color = torch::zeros({capacity, height, width, 3}, u8);
        if (masks) mask = torch::zeros({capacity, height, width}, u8);
        if (depths) depth = torch::zeros({capacity, height, width}, u8.dtype(torch::kUInt16));
        if (depth_weights) dweight = torch::zeros({capacity, height, width}, u8);
        frames_ = torch::arange(capacity, u8.dtype(torch::kInt32));
        serial_.assign((size_t)capacity, 0);
    }
    int n() const { return n_; }
    int64_t nbytes() const
    {
        return color.numel() + (mask.defined() ? mask.numel() : 0) + (depth.defined() ? 2 * depth.numel() : 0) + (dweight.defined() ? dweight.numel() : 0);
    }
    bool has_depths() const { return depth.defined(); }
    bool has_depth_weights() const { return dweight.defined(); }
    float depth_step() const { return depth_step_; }
    int64_t serial(int slot) const { return serial_[(size_t)index(slot)]; }
    // encodes a float32 [3,H,W] image (and, on a store with masks, a float32 [H,W] mask; undefined: weight 1 everywhere) into the next slot
    // depth_image / depth_weight (a store with depths / depth weights): float32 [H,W], encoded into the slot's codes; a slot written without a
    // depth image holds "nothing measured"
    int add(const torch::Tensor& image, const torch::Tensor& mask_image = torch::Tensor(), const torch::Tensor& depth_image = torch::Tensor(),
            const torch::Tensor& depth_weight = torch::Tensor())
    {
        TORCH_CHECK(n_ < cap_, "KeyframeStore: all ", cap_, " slots are filled");
        check_depth(depth_image, depth_weight);
        write(n_, image, mask_image);
        write_depth(n_, depth_image, depth_weight);
        return n_++;
    }
    // copies a uint8 [H,W,3] image (bgr: the channels flipped, in LibTorch) and a uint8 [H,W] mask into the next slot
    int add_u8(const torch::Tensor& hwc, const torch::Tensor& mask_u8 = torch::Tensor(), bool bgr = false,
               const torch::Tensor& depth_image = torch::Tensor(), const torch::Tensor& depth_weight = torch::Tensor())
    {
        TORCH_CHECK(n_ < cap_, "KeyframeStore: all ", cap_, " slots are filled");
        check_depth(depth_image, depth_weight);
        write_u8(n_, hwc, mask_u8, bgr);
        write_depth(n_, depth_image, depth_weight);
        return n_++;
    }
    // replaces a filled slot by a float image (as add) and bumps the slot's serial number
    void put(int slot, const torch::Tensor& image, const torch::Tensor& mask_image = torch::Tensor(), const torch::Tensor& depth_image = torch::Tensor(),
             const torch::Tensor& depth_weight = torch::Tensor())
    {
        check_depth(depth_image, depth_weight);
        write(index(slot), image, mask_image);
        write_depth(slot, depth_image, depth_weight);
        serial_[(size_t)slot]++;
    }
    void put_u8(int slot, const torch::Tensor& hwc, const torch::Tensor& mask_u8 = torch::Tensor(), bool bgr = false,
                const torch::Tensor& depth_image = torch::Tensor(), const torch::Tensor& depth_weight = torch::Tensor())
    {
        check_depth(depth_image, depth_weight);
        write_u8(index(slot), hwc, mask_u8, bgr);
        write_depth(slot, depth_image, depth_weight);
        serial_[(size_t)slot]++;
    }
    // replaces only the depth (and depth weight) of a filled slot — LiDAR that arrives after the image — and bumps the slot's serial number
    void put_depth(int slot, const torch::Tensor& depth_image, const torch::Tensor& depth_weight = torch::Tensor())
    {
        TORCH_CHECK(depth.defined(), "KeyframeStore: put_depth on a store built without depths");
        TORCH_CHECK(depth_image.defined(), "KeyframeStore: put_depth without a depth image");
        write_depth(index(slot), depth_image, depth_weight);
        serial_[(size_t)slot]++;
    }
    // the float32 target of a slot at a pyramid level (one launch; the slot index is read from a device word the store keeps)
    KeyframeTarget target(int slot, int level = 0)
    {
        torch::NoGradGuard ng;
        index(slot);
        TORCH_CHECK(level >= 0 && level <= GSLIC_KEYFRAME_MAX_LEVEL && (W_ >> level) >= 1 && (H_ >> level) >= 1, "KeyframeStore: a ", W_, " x ", H_,
                    " image has no level ", level);
        const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(color.device());
        KeyframeTarget out;
        out.image = torch::empty({3, H_ >> level, W_ >> level}, f32);
        if (mask.defined()) out.weight = torch::empty({H_ >> level, W_ >> level}, f32);
        const int rc = gslic_keyframe_decode(W_, H_, level, color.data_ptr<uint8_t>(), mask.defined() ? mask.data_ptr<uint8_t>() : nullptr,
                                             frames_.data_ptr<int32_t>() + slot, n_, out.image.data_ptr<float>(),
                                             mask.defined() ? out.weight.data_ptr<float>() : nullptr, current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_keyframe_decode failed (", rc, "): ", gslic_last_error());
        return out;
    }
    // the float32 depth target (and depth weight) of a slot at a pyramid level: the nearest return of every block (one launch)
    KeyframeDepthTarget depth_target(int slot, int level = 0)
    {
        torch::NoGradGuard ng;
        index(slot);
        TORCH_CHECK(depth.defined(), "KeyframeStore: this store was built without depths");
        TORCH_CHECK(level >= 0 && level <= GSLIC_KEYFRAME_MAX_LEVEL && (W_ >> level) >= 1 && (H_ >> level) >= 1, "KeyframeStore: a ", W_, " x ", H_,
                    " image has no level ", level);
        const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(color.device());
        KeyframeDepthTarget out;
        out.depth = torch::empty({H_ >> level, W_ >> level}, f32);
        if (dweight.defined()) out.weight = torch::empty({H_ >> level, W_ >> level}, f32);
        const int rc = gslic_keyframe_decode_depth(W_, H_, level, static_cast<const uint16_t*>(depth.data_ptr()),
                                                   dweight.defined() ? dweight.data_ptr<uint8_t>() : nullptr, frames_.data_ptr<int32_t>() + slot, n_,
                                                   depth_step_, out.depth.data_ptr<float>(), dweight.defined() ? out.weight.data_ptr<float>() : nullptr,
                                                   current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_keyframe_decode_depth failed (", rc, "): ", gslic_last_error());
        return out;
    }

private:
    int index(int slot) const
    {
        TORCH_CHECK(slot >= 0 && slot < n_, "KeyframeStore: slot ", slot, " is outside [0, ", n_, ")");
        return slot;
    }
    void check_depth(const torch::Tensor& depth_image, const torch::Tensor& depth_weight) const
    {
        TORCH_CHECK(!depth_image.defined() || depth.defined(), "KeyframeStore: depth given to a store built without depths");
        TORCH_CHECK(!depth_weight.defined() || dweight.defined(), "KeyframeStore: depth_weight given to a store built without depth weights");
        TORCH_CHECK(!depth_weight.defined() || depth_image.defined(), "KeyframeStore: depth_weight given without depth");
    }
    void write_depth(int slot, const torch::Tensor& depth_image, const torch::Tensor& depth_weight)
    {
        torch::NoGradGuard ng;
        check_depth(depth_image, depth_weight);
        if (!depth.defined()) return;
        if (!depth_image.defined()) {   // nothing measured
            depth[slot].view(torch::kInt16).zero_();
            if (dweight.defined()) dweight[slot].fill_(255);
            return;
        }
        const torch::Tensor d = depth_image.detach().to(color.device(), torch::kFloat32).contiguous();
        TORCH_CHECK(d.dim() == 2 && d.size(0) == H_ && d.size(1) == W_, "KeyframeStore: the depth image must be [", H_, ", ", W_, "]");
        torch::Tensor w;
        if (depth_weight.defined()) {
            w = depth_weight.detach().to(color.device(), torch::kFloat32).contiguous();
            TORCH_CHECK(w.dim() == 2 && w.size(0) == H_ && w.size(1) == W_, "KeyframeStore: the depth weight must be [", H_, ", ", W_, "]");
        }
        const int rc = gslic_keyframe_encode_depth(W_, H_, d.data_ptr<float>(), w.defined() ? w.data_ptr<float>() : nullptr,
                                                   static_cast<uint16_t*>(depth.data_ptr()), dweight.defined() ? dweight.data_ptr<uint8_t>() : nullptr,
                                                   cap_, slot, depth_step_, current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_keyframe_encode_depth failed (", rc, "): ", gslic_last_error());
    }
    void write(int slot, const torch::Tensor& image, const torch::Tensor& mask_image)
    {
        torch::NoGradGuard ng;
        TORCH_CHECK(!mask_image.defined() || mask.defined(), "KeyframeStore: mask given to a store built without masks");
        const torch::Tensor img = image.detach().to(color.device(), torch::kFloat32).contiguous();
        TORCH_CHECK(img.dim() == 3 && img.size(0) == 3 && img.size(1) == H_ && img.size(2) == W_, "KeyframeStore: the image must be [3, ", H_, ", ", W_, "]");
        torch::Tensor m;
        if (mask_image.defined()) {
            m = mask_image.detach().to(color.device(), torch::kFloat32).contiguous();
            TORCH_CHECK(m.dim() == 2 && m.size(0) == H_ && m.size(1) == W_, "KeyframeStore: the mask must be [", H_, ", ", W_, "]");
        } else if (mask.defined()) {
            mask[slot].fill_(255);
        }
        const int rc = gslic_keyframe_encode(W_, H_, img.data_ptr<float>(), m.defined() ? m.data_ptr<float>() : nullptr, color.data_ptr<uint8_t>(),
                                             m.defined() ? mask.data_ptr<uint8_t>() : nullptr, cap_, slot, current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_keyframe_encode failed (", rc, "): ", gslic_last_error());
    }
    void write_u8(int slot, const torch::Tensor& hwc, const torch::Tensor& mask_u8, bool bgr)
    {
        torch::NoGradGuard ng;
        TORCH_CHECK(!mask_u8.defined() || mask.defined(), "KeyframeStore: mask given to a store built without masks");
        TORCH_CHECK(hwc.scalar_type() == torch::kByte && hwc.dim() == 3 && hwc.size(0) == H_ && hwc.size(1) == W_ && hwc.size(2) == 3,
                    "KeyframeStore: add_u8 takes a uint8 [", H_, ", ", W_, ", 3] tensor");
        color[slot].copy_(bgr ? hwc.flip({-1}) : hwc);
        if (!mask.defined()) return;
        if (mask_u8.defined()) {
            TORCH_CHECK(mask_u8.scalar_type() == torch::kByte && mask_u8.dim() == 2 && mask_u8.size(0) == H_ && mask_u8.size(1) == W_,
                        "KeyframeStore: the mask of add_u8 is a uint8 [", H_, ", ", W_, "] tensor");
            mask[slot].copy_(mask_u8);
        } else {
            mask[slot].fill_(255);
        }
    }
    int W_, H_, cap_, n_ = 0;
    float depth_step_;
    torch::Tensor frames_;            // int32 [capacity] = 0 .. capacity-1: the device word that names slot i is frames_[i]
    std::vector<int64_t> serial_;
};

class LidarDepth {
public:
    LidarDepth(int width, int height, torch::Device device = torch::kCUDA) : W_(width), H_(height)
    {
        TORCH_CHECK(width > 0 && height > 0, "LidarDepth: the image must not be empty");
        zbuf_ = torch::empty({(int64_t)height * width}, torch::TensorOptions().dtype(torch::kInt64).device(device));
    }
    // empties the image: the next add() clears the z-buffer inside its call
    void clear() { pending_clear_ = true; n_points_ = 0; }
    // One sweep: points_world [n,3] (device), the world-to-camera pose R_cw [3,3] row-major and t_cw [3] (float32, rounded from the host's pose as
    // Camera.project_depth rounds it) and the intrinsics.  The nearest return wins a pixel, equal depths go to the lowest index.  Returns the
    // sweep's index_base: its point i is index base + i in resolve()'s index image.  Several sweeps, each with its own pose, accumulate.
    int64_t add(const torch::Tensor& points_world, const torch::Tensor& R_cw, const torch::Tensor& t_cw, float fx, float fy, float cx, float cy)
    {
        torch::NoGradGuard ng;
        TORCH_CHECK(points_world.dim() == 2 && points_world.size(1) == 3 && points_world.device() == zbuf_.device(),
                    "LidarDepth::add: points_world must be [n, 3] on the image's device");
        TORCH_CHECK(R_cw.numel() == 9 && t_cw.numel() == 3, "LidarDepth::add: R_cw must hold 9 and t_cw 3 values");
        const torch::Tensor pts = points_world.detach().to(torch::kFloat32).contiguous();
        const torch::Tensor R = R_cw.detach().to(zbuf_.device(), torch::kFloat32).contiguous(), t = t_cw.detach().to(zbuf_.device(), torch::kFloat32).contiguous();
        const int64_t n = pts.size(0);
        TORCH_CHECK(n_points_ + n <= std::numeric_limits<int32_t>::max(), "LidarDepth::add: more than 2^31 - 1 points in one image");
        return add_raw((int32_t)n, n ? pts.data_ptr<float>() : nullptr, R.data_ptr<float>(), t.data_ptr<float>(), fx, fy, cx, cy);
    }
    // The images of what was added since the last clear().  footprint r in [0, 8]: every pixel takes the nearest return of its (2r+1) x (2r+1)
    // window clipped to the image (0: its own).  margins: when set, near_bound is written too.  weight = {sigma_abs, sigma_rel, falloff}: when
    // set, the weight image sigma_abs / (sigma_abs + sigma_rel d) * 1 / (1 + falloff * dist2) is written too (sigma_abs > 0, sigma_rel >= 0,
    // falloff >= 0, all finite); dist2: the squared pixel distance to the return each pixel was given.  Both come from the same single launch
    // (gslic_lidar_zbuffer_resolve_weighted); with neither, the call is gslic_lidar_zbuffer_resolve's.
    LidarImages resolve(int footprint = 0, std::optional<std::array<float, 2>> margins = std::nullopt, bool index = false, bool count = false,
                        std::optional<std::array<float, 3>> weight = std::nullopt, bool dist2 = false)
    {
        torch::NoGradGuard ng;
        if (weight) {
            const float inf = std::numeric_limits<float>::infinity();
            TORCH_CHECK((*weight)[0] > 0.0f && (*weight)[0] < inf && (*weight)[1] >= 0.0f && (*weight)[1] < inf,
                        "LidarDepth::resolve: sigma_abs must be > 0 and sigma_rel >= 0, both finite");
            TORCH_CHECK((*weight)[2] >= 0.0f && (*weight)[2] < inf, "LidarDepth::resolve: the falloff must be >= 0 and finite");
        }
        if (pending_clear_) add_raw(0, nullptr, nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f);
        const auto f32 = torch::TensorOptions().dtype(torch::kFloat32).device(zbuf_.device()), i32 = f32.dtype(torch::kInt32);
        LidarImages out;
        out.depth = torch::empty({H_, W_}, f32);
        if (margins) out.near_bound = torch::empty({H_, W_}, f32);
        if (index) out.index = torch::empty({H_, W_}, i32);
        if (count) out.n_measured = torch::empty({}, i32);
        if (weight || dist2) {
            if (weight) out.weight = torch::empty({H_, W_}, f32);
            if (dist2) out.dist2 = torch::empty({H_, W_}, i32);
            const int rc = gslic_lidar_zbuffer_resolve_weighted(
                W_, H_, reinterpret_cast<const uint64_t*>(zbuf_.data_ptr<int64_t>()), footprint, margins ? (*margins)[0] : 0.0f,
                margins ? (*margins)[1] : 0.0f, weight ? (*weight)[0] : 1.0f, weight ? (*weight)[1] : 0.0f, weight ? (*weight)[2] : 0.0f,
                out.depth.data_ptr<float>(), index ? out.index.data_ptr<int32_t>() : nullptr, margins ? out.near_bound.data_ptr<float>() : nullptr,
                count ? reinterpret_cast<uint32_t*>(out.n_measured.data_ptr<int32_t>()) : nullptr, weight ? out.weight.data_ptr<float>() : nullptr,
                dist2 ? out.dist2.data_ptr<int32_t>() : nullptr, current_stream());
            TORCH_CHECK(rc == GSLIC_OK, "gslic_lidar_zbuffer_resolve_weighted failed (", rc, "): ", gslic_last_error());
            return out;
        }
        const int rc = gslic_lidar_zbuffer_resolve(W_, H_, reinterpret_cast<const uint64_t*>(zbuf_.data_ptr<int64_t>()), footprint, margins ? (*margins)[0] : 0.0f,
                                                   margins ? (*margins)[1] : 0.0f, out.depth.data_ptr<float>(), index ? out.index.data_ptr<int32_t>() : nullptr,
                                                   margins ? out.near_bound.data_ptr<float>() : nullptr,
                                                   count ? reinterpret_cast<uint32_t*>(out.n_measured.data_ptr<int32_t>()) : nullptr, current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_lidar_zbuffer_resolve failed (", rc, "): ", gslic_last_error());
        return out;
    }
    int64_t points() const { return n_points_; }   // points added since the last clear: the next sweep's index_base

private:
    int64_t add_raw(int32_t n, const float* pts, const float* R, const float* t, float fx, float fy, float cx, float cy)
    {
        const int64_t base = n_points_;
        const int rc = gslic_lidar_zbuffer_add(n, pts, R, t, fx, fy, cx, cy, W_, H_, reinterpret_cast<uint64_t*>(zbuf_.data_ptr<int64_t>()), pending_clear_ ? 1 : 0,
                                               (int32_t)base, current_stream());
        TORCH_CHECK(rc == GSLIC_OK, "gslic_lidar_zbuffer_add failed (", rc, "): ", gslic_last_error());
        pending_clear_ = false;
        n_points_ = base + n;
        return base;
    }
    int W_, H_;
    torch::Tensor zbuf_;
    bool pending_clear_ = true;
    int64_t n_points_ = 0;
};

class FusedStep {
public:
    // params: the six raw leaf tensors in the group order of trainingSetup (gaussian.cpp:399-418); updated IN PLACE.
    FusedStep(std::array<torch::Tensor, 6> params, std::array<float, 6> lrs, int sh_degree, float lambda_dssim = 0.2f,
              float lambda_erank = 0.0f, float b1 = 0.9f, float b2 = 0.999f, float eps = 1e-15f)
        : prm_(std::move(params)), lrs_(lrs), deg_(sh_degree), lambda_dssim_(lambda_dssim), lambda_erank_(lambda_erank), b1_(b1), b2_(b2), eps_(eps)
    {
        for (int i = 0; i < 6; i++) {
            TORCH_CHECK(prm_[i].is_cuda() && prm_[i].scalar_type() == torch::kFloat32 && prm_[i].is_contiguous(),
                        "FusedStep: parameter group ", i, " must be a contiguous fp32 device tensor (it is updated in place)");
            m_[i] = torch::zeros_like(prm_[i].detach());   // SparseGaussianAdam creates its state as zeros on the first step (optim_utils.h:116-123)
            v_[i] = torch::zeros_like(prm_[i].detach());
        }
        auto bytes = torch::TensorOptions().dtype(torch::kByte).device(prm_[0].device());
        for (auto& s : scratch_) s = torch::empty({0}, bytes);
        bg_ = torch::zeros({3}, prm_[0].options().requires_grad(false));
    }

    // continue from a SparseGaussianAdam (exp_avg / exp_avg_sq of group i), e.g. when switching an existing map over
    void adopt_state(int group, torch::Tensor exp_avg, torch::Tensor exp_avg_sq)
    {
        TORCH_CHECK(exp_avg.sizes() == prm_[group].sizes() && exp_avg_sq.sizes() == prm_[group].sizes() && exp_avg.is_contiguous() &&
                    exp_avg_sq.is_contiguous(), "FusedStep::adopt_state: shape / layout mismatch");
        m_[group] = std::move(exp_avg);
        v_[group] = std::move(exp_avg_sq);
    }
    // after densificationPostfix (gaussian.cpp:444-487) replaced the tensors: new parameters, moments extended with zeros by the host
    void rebind(std::array<torch::Tensor, 6> params, std::array<torch::Tensor, 6> exp_avg, std::array<torch::Tensor, 6> exp_avg_sq)
    {
        prm_ = std::move(params); m_ = std::move(exp_avg); v_ = std::move(exp_avg_sq);
    }
    void set_lr(int group, float lr) { lrs_[group] = lr; }
    // From here on every step() adds its view to *stats (gslic_rasterize_backward_adam_stats / _depth_adam_stats: the same step, bit-identical
    // parameters and moments) and prune() / extend() / densify() / resort() carry its arrays with the rows, beside the contribution statistics:
    // gathered, zero for new rows and split parents, permuted.  The object must outlive the step or be taken off with nullptr.
    void set_gradient_stats(GradientStats* stats)
    {
        gstats_ = stats;
        if (gstats_) fit_rows(gstats_->rows());
    }
    // From here on prune() / extend() / densify() / resort() carry *cv's rows with the map's (created zero-filled, grown to the map's capacity), and
    // record_covisibility(frame) replaces column `frame` by radii > 0 of the last step()'s forward — trainer.Covisibility.record(frame, radii).  The
    // object must outlive the step or be taken off with nullptr.
    void set_covisibility(Covisibility* cv)
    {
        covis_ = cv;
        if (covis_) fit_rows(covis_->rows());
    }
    void record_covisibility(int frame)
    {
        TORCH_CHECK(covis_, "record_covisibility: no Covisibility is attached (set_covisibility)");
        TORCH_CHECK(radii_.defined() && radii_.size(0) == size(), "record_covisibility: no step has run on the rows as they are");
        fit_rows(covis_->rows());
        covis_->record(size(), frame, radii_);
    }
    // From here on step() and pose_gradient() take the loss of the exposure-compensated image: E = exposure->matrix(view) applied into a scratch
    // image (gslic_exposure_apply), the loss calls unchanged on that image, then gslic_exposure_backward, which hands the rasteriser's backward
    // E^T dL/dout and leaves dL/dE in exposure->grad; step() also updates the row by torch-style Adam in that call's second launch, pose_gradient()
    // updates nothing.  The calls of the Python host's training_step_fused(exposure=, view=).  The depth image is not touched.  The object must
    // outlive the step or be taken off with nullptr, which is the step as it always was.
    void set_exposure(Exposure* exposure, int view = 0)
    {
        if (exposure) exposure->matrix(view);
        exposure_ = exposure;
        exposure_view_ = view;
    }
    // A host that keeps the map's rows in a PERMUTED order (e.g. sorted along a space-filling curve so that what a view sees is contiguous in
    // memory) passes the rows' ORIGINAL indices (device int32 [P]): the forward then lists Gaussians of equal depth in the original order, as the
    // reference's stable sort does (gslic_raster_params.tie_rank), and the map renders / trains bit-identically to the unpermuted one.
    // Rows appended by extend() get their row index.
    void set_tie_rank(torch::Tensor original_index)
    {
        TORCH_CHECK(original_index.defined() && original_index.device() == prm_[0].device() && original_index.numel() == prm_[0].size(0),
                    "FusedStep::set_tie_rank: expected one index per Gaussian (", prm_[0].size(0), ") on the model's device; got ", original_index.numel(),
                    " on ", original_index.device());   // (its data pointer goes straight to the kernels)
        tie_ = original_index.to(torch::kInt32).contiguous();
        sorted_P_ = prm_[0].size(0);   // (the host sorted its rows: the re-sort rule counts the rows appended from here on)
    }
    // Puts ALL rows into Morton order on the device — the Python host's GaussianModel.resort / to_morton_order (gaussian-lic_amd/trainer.py), same
    // calls, same result: the robust box from a strided sample of at most 65 536 rows (LibTorch: one sort of the sample, no host read-back),
    // ONE gslic_morton_order (the exact key rule of include/gslic_hip.h and the stable sort) and ONE gslic_permute_rows over the 18 parameter and
    // moment arrays, the tie rank and the statistics' arrays, in place through one staging tensor: addresses do not change, param(i) stays valid.
    // Without a tie rank (rows in insertion order) one is created as arange(P) first: every row's original index is its present row.  The map
    // renders and trains exactly as before.  Returns the permutation applied (device int64 [P]; new row s = old row perm[s]): per-row state the
    // host keeps outside is re-aligned with index_select(0, perm).  stats: contribution statistics of this map, permuted with it.
    torch::Tensor resort(ContributionStats* stats = nullptr)
    {
        torch::NoGradGuard ng;
        const int64_t P = prm_[0].size(0);
        auto io = prm_[0].options().requires_grad(false).dtype(torch::kInt32);
        if (!tie_.defined()) tie_ = torch::arange(P, io);
        sorted_P_ = P;
        n_resorts_++;
        if (P == 0) return last_perm_ = torch::empty({0}, io.dtype(torch::kInt64));
        const torch::Tensor q = prm_[0].detach();
        const torch::Tensor srt = std::get<0>(torch::sort(q.slice(0, 0, P, std::max<int64_t>(1, P / 65536)), 0));
        const int64_t ns = srt.size(0);
        const int64_t i_lo = std::min<int64_t>(ns - 1, (int64_t)(0.001 * (double)ns)), i_hi = std::max<int64_t>(0, std::min<int64_t>(ns - 1, (int64_t)(0.999 * (double)ns)));
        const torch::Tensor box = torch::cat({srt[i_lo], srt[i_hi]}).contiguous();   // lo xyz, hi xyz: the 0.1 % / 99.9 % order statistics per axis
        torch::Tensor perm = torch::empty({P}, io), sort_scratch = torch::empty({0}, io.dtype(torch::kByte));
        check(gslic_morton_order((int32_t)P, f(prm_[0]), box.data_ptr<float>(), grow_cb, &sort_scratch, reinterpret_cast<uint32_t*>(perm.data_ptr<int32_t>()),
                                 nullptr, current_stream()),
              "gslic_morton_order");
        std::vector<gslic_row_array> rows;
        auto add = [&](const torch::Tensor& t, uint32_t w) { if (w) rows.push_back({t.data_ptr(), t.data_ptr(), w}); };
        for (int g = 0; g < 6; g++) {
            const uint32_t w = (uint32_t)(prm_[g].numel() / P);   // (0: features_rest at SH degree 0)
            add(prm_[g], w); add(m_[g], w); add(v_[g], w);
        }
        add(tie_, 1u);
        for (const auto& list : carried(stats)) permute_rows(list, rows);
        const size_t bytes = gslic_permute_rows_staging_bytes(rows.data(), (int32_t)rows.size(), (int32_t)P);
        torch::Tensor staging = torch::empty({(int64_t)bytes}, io.dtype(torch::kByte));
        check(gslic_permute_rows(rows.data(), (int32_t)rows.size(), reinterpret_cast<const uint32_t*>(perm.data_ptr<int32_t>()), (int32_t)P, staging.data_ptr(),
                                 bytes, current_stream()),
              "gslic_permute_rows");
        return last_perm_ = perm.to(torch::kInt64);
    }
    // The re-sort rule of the Python model (GaussianModel.resort_fraction): once the rows appended by extend() / densify() behind the sorted block
    // make up more than `fraction` of the map, the call that appended them re-sorts the whole map (resort()).  nullopt (the default): never — a
    // host that does not ask sees no change.  It applies to maps with a tie rank (set_tie_rank, or a first resort()); prune() moves the sorted
    // block's bound to the kept rows below it.  resorts() counts the re-sorts so far and last_resort() is the last permutation applied (device
    // int64 [P]; undefined before the first): a host with per-row state of its own compares the count around extend() / densify().
    void set_resort_fraction(std::optional<double> fraction) { resort_fraction_ = fraction; }
    int64_t resorts() const { return n_resorts_; }
    const torch::Tensor& last_resort() const { return last_perm_; }
    int64_t sorted_rows() const { return sorted_P_; }   // rows [0, sorted_rows()) are in Morton order (0: no sort so far)

    // extend() of gaussian.cpp:499-638 for one new LiDAR frame: transmittance-only render of `cam` (no_color, :501-507), device-side
    // selection of the points that land on not-yet-opaque pixels (nearest per pixel, gslic_extend_select), append of the new Gaussians'
    // rows (gslic_extend_emit) and of zero Adam moments.  Storage grows by capacity doubling, so an append is in place most of the time
    // instead of the reference's six torch::cat of every parameter and moment (densificationPostfix, :426-497).  After a call that
    // returned k > 0 the six parameter tensors are NEW views: fetch them with param(i).
    //   points, colors [n,3], depths_rsp [n]: device fp32; R_cw [3,3] row-major, t_cw [3] (any device); returns the number inserted.
    // stats: contribution statistics of this map — grown with it (the appended rows are zero) and permuted when the append triggers the re-sort rule
    // (set_resort_fraction).
    int64_t extend(const FusedCamera& cam, const torch::Tensor& points, const torch::Tensor& colors, const torch::Tensor& depths_rsp,
                   const torch::Tensor& R_cw, const torch::Tensor& t_cw, float fx, float fy, float cx, float cy, float scaling_scale = 1.0f,
                   ContributionStats* stats = nullptr)
    {
        torch::NoGradGuard ng;
        const int64_t P = prm_[0].size(0), n = points.size(0);
        const int W = cam.image_width, H = cam.image_height;
        auto fo = prm_[0].options().requires_grad(false);
        // render(no_color) through the operator entry point with LibTorch activations, exactly as renderer.cpp:57-63 feeds it
        const gslic_raster_params rp = raster_params(cam, false, true);
        torch::Tensor op = torch::sigmoid(prm_[3]).contiguous(), sc = torch::exp(prm_[4]).contiguous();
        torch::Tensor rot = torch::nn::functional::normalize(prm_[5]).contiguous();
        torch::Tensor final_T = torch::empty({H, W}, fo), color = torch::empty({3, H, W}, fo), radii = torch::empty({P}, fo.dtype(torch::kInt32));
        int32_t R = 0, B = 0;
        forward(rp, cam, f(op), f(sc), f(rot), color, final_T, nullptr, radii, R, B);
        torch::Tensor pts = points.to(fo).contiguous(), col = colors.to(fo).contiguous(), rsp = depths_rsp.to(fo).contiguous();
        torch::Tensor Rc = R_cw.to(fo).contiguous(), tc = t_cw.to(fo).contiguous();
        torch::Tensor sel_scratch = torch::empty({0}, fo.dtype(torch::kByte));
        uint32_t *flags = nullptr, *pos = nullptr;
        int32_t count = 0;
        check(gslic_extend_select((int32_t)n, f(pts), f(rsp), f(Rc), f(tc), fx, fy, cx, cy, W, H, f(final_T), grow_cb, &sel_scratch, &flags, &pos, &count,
                                  current_stream()),
              "gslic_extend_select");
        if (count == 0) return 0;
        reserve(P + count);
        const int64_t M = buf_[2].numel() ? buf_[2].size(1) : 0;
        auto row = [&](int g) { return buf_[g].numel() ? buf_[g].data_ptr<float>() + P * (buf_[g].numel() / buf_[g].size(0)) : nullptr; };
        check(gslic_extend_emit((int32_t)n, flags, pos, f(pts), f(col), f(rsp), scaling_scale, (fx + fy) / 2.0f, (int32_t)M, row(0), row(1), row(2), row(3),
                                row(4), row(5), current_stream()),
              "gslic_extend_emit");
        for (int g = 0; g < 6; g++) {   // new rows start with zero moments (gaussian.cpp:458-459)
            mbuf_[g].narrow(0, P, count).zero_();
            vbuf_[g].narrow(0, P, count).zero_();
        }
        if (tie_.defined()) tie_ = torch::cat({tie_, torch::arange(P, P + count, tie_.options())});
        bind(P + count);
        for (const auto& list : carried(stats)) zero_rows(list, P, count);   // appended rows have been seen by no view yet
        torch::cuda::synchronize();   // (the selection scratch is released on return)
        rows_appended(stats);
        return count;
    }
    // Removes rows from the map on the device — the Python host's GaussianModel.prune (gaussian-lic_amd/trainer.py), same calls, same result:
    // ONE gslic_prune_select (which rows stay) and ONE gslic_gather_rows over the 18 parameter and moment arrays, out of place into fresh storage
    // of the same capacity.  min_opacity in (0, 1) and max_scale > 0 are limits in the ACTIVATED domain (nullopt: no limit); each is converted
    // once, in double, to logit(min_opacity) / log(max_scale) and rounded to float — the two thresholds of the raw-domain rule of
    // include/gslic_hip.h: a row goes when raw opacity < logit(min_opacity), some raw scaling > log(max_scale) (both strict) or drop[row] is set,
    // unless protect[row] is set; a row with a non-finite xyz / features_dc / opacity / scaling / rotation goes always (drop_nonfinite).
    // drop / protect: undefined or bool / uint8 [P] on the map's device.  A tie rank (set_tie_rank) is replaced by the kept rows' dense ranks.
    // Returns the kept rows' OLD indices (device int64 [P'], ascending): per-row state the host keeps is re-aligned with index_select(0, kept).
    // After a call that removed rows the six parameter tensors are NEW views: fetch them with param(i).
    // stats: contribution statistics of this map (accumulate_contribution) — gathered with the map by the same kept index (row widths 1, 1, 2).
    torch::Tensor prune(std::optional<double> min_opacity, std::optional<double> max_scale, const torch::Tensor& drop = torch::Tensor(),
                        const torch::Tensor& protect = torch::Tensor(), bool drop_nonfinite = true, ContributionStats* stats = nullptr)
    {
        torch::NoGradGuard ng;
        const int64_t P = prm_[0].size(0);
        auto io = prm_[0].options().requires_grad(false).dtype(torch::kInt32);
        float lo = -std::numeric_limits<float>::infinity(), hi = std::numeric_limits<float>::infinity();
        if (min_opacity) {
            TORCH_CHECK(*min_opacity > 0.0 && *min_opacity < 1.0, "FusedStep::prune: min_opacity must lie in (0, 1)");
            lo = (float)std::log(*min_opacity / (1.0 - *min_opacity));
        }
        if (max_scale) {
            TORCH_CHECK(*max_scale > 0.0 && std::isfinite(*max_scale), "FusedStep::prune: max_scale must be a finite number > 0");
            hi = (float)std::log(*max_scale);
        }
        if (P == 0) return torch::empty({0}, io.dtype(torch::kInt64));
        const torch::Tensor dr = row_mask(drop, "FusedStep::prune: ", "drop", P), pr = row_mask(protect, "FusedStep::prune: ", "protect", P);
        torch::Tensor kept = torch::empty({P}, io), new_tie = tie_.defined() ? torch::empty({P}, io) : torch::Tensor();
        torch::Tensor sel_scratch = torch::empty({0}, io.dtype(torch::kByte));
        int32_t count = 0, below = 0;
        check(gslic_prune_select((int32_t)P, f(prm_[0]), f(prm_[1]), f(prm_[3]), f(prm_[4]), f(prm_[5]), lo, hi, drop_nonfinite ? 1 : 0, u8(dr), u8(pr),
                                 tie_.defined() ? reinterpret_cast<const uint32_t*>(tie_.data_ptr<int32_t>()) : nullptr, (int32_t)std::min(sorted_P_, P), grow_cb,
                                 &sel_scratch, reinterpret_cast<uint32_t*>(kept.data_ptr<int32_t>()),
                                 new_tie.defined() ? reinterpret_cast<uint32_t*>(new_tie.data_ptr<int32_t>()) : nullptr, &count, &below, current_stream()),
              "gslic_prune_select");
        if (count == P) return torch::arange(P, io.dtype(torch::kInt64));
        const int64_t cap = capacity();
        std::array<torch::Tensor, 6> nb, nm, nv;
        std::vector<gslic_row_array> rows;
        for (int g = 0; g < 6; g++) {
            std::vector<int64_t> shp = prm_[g].sizes().vec();
            shp[0] = cap;
            nb[g] = torch::empty(shp, prm_[g].options().requires_grad(false)); nm[g] = torch::empty(shp, m_[g].options()); nv[g] = torch::empty(shp, v_[g].options());
            const uint32_t w = (uint32_t)(prm_[g].numel() / P);
            if (w == 0) continue;   // features_rest at SH degree 0
            rows.push_back({prm_[g].data_ptr(), nb[g].data_ptr(), w});
            rows.push_back({m_[g].data_ptr(), nm[g].data_ptr(), w});
            rows.push_back({v_[g].data_ptr(), nv[g].data_ptr(), w});
        }
        check(gslic_gather_rows(rows.data(), (int32_t)rows.size(), reinterpret_cast<const uint32_t*>(kept.data_ptr<int32_t>()), count, current_stream()),
              "gslic_gather_rows");
        buf_ = nb; mbuf_ = nm; vbuf_ = nv;
        bind(count);
        sorted_P_ = below;   // the kept rows below the old bound of the sorted block
        for (const auto& list : carried(stats)) gather_rows(list, kept, P, count);   // the statistics follow their rows: the same gather, on the same kept index
        if (tie_.defined()) tie_ = new_tie.narrow(0, 0, count).clone();
        return kept.narrow(0, 0, count).to(torch::kInt64);
    }
    // Adds the contribution statistics of ONE view to `stats` — the Python host's ContributionStats.accumulate: a raw-parameter forward of its own
    // (it reuses the step's scratch; call it between steps) and one gslic_contribution_accumulate on its buffers.  w_min: a (pixel, Gaussian)
    // pair counts into n_pix when its weight w = alpha T reaches it.  The arrays are created zero-filled on first use and grown to capacity().
    // error: undefined, or the view's per-pixel error image, float [H,W] on the map's device (host policy, e.g. (image - gt).abs().mean(0)).  The
    // launch is then gslic_contribution_accumulate_error: the same three statistics bit for bit, and stats.err_sum += sum of w e(p) with
    // e = error clamped to [0, 4] (NaN and negative values read as 0) — the error-based densification score.  stats.err_sum is created at the
    // first such call.
    void accumulate_contribution(const FusedCamera& cam, ContributionStats& stats, float w_min, const torch::Tensor& error = torch::Tensor())
    {
        torch::NoGradGuard ng;
        const int64_t P = prm_[0].size(0);
        const int W = cam.image_width, H = cam.image_height;
        torch::Tensor err;
        if (error.defined()) {
            TORCH_CHECK(error.dim() == 2 && error.size(0) == H && error.size(1) == W && error.is_floating_point() && error.device() == prm_[0].device(),
                        "FusedStep::accumulate_contribution: error must be a float [", H, ", ", W, "] tensor on the map's device");
            err = error.detach().to(torch::kFloat32).contiguous();
        }
        if (err.defined()) fit_rows(stats.rows(), {&stats.err_sum}); else fit_rows(stats.rows());
        stats.views++;
        if (P == 0) return;
        int32_t R = 0, B = 0;
        const gslic_raster_params rp = statistics_forward(cam, R, B);
        if (err.defined()) {
            check(gslic_contribution_accumulate_error(&rp, R, B, cptr(scratch_[0]), cptr(scratch_[1]), cptr(scratch_[2]), w_min,
                                                      reinterpret_cast<uint32_t*>(stats.max_w.data_ptr<int32_t>()),
                                                      reinterpret_cast<uint32_t*>(stats.n_pix.data_ptr<int32_t>()),
                                                      reinterpret_cast<uint64_t*>(stats.sum_w.data_ptr<int64_t>()), err.data_ptr<float>(),
                                                      reinterpret_cast<uint64_t*>(stats.err_sum.data_ptr<int64_t>()), current_stream()),
                  "gslic_contribution_accumulate_error");
            return;
        }
        check(gslic_contribution_accumulate(&rp, R, B, cptr(scratch_[0]), cptr(scratch_[1]), cptr(scratch_[2]), w_min,
                                            reinterpret_cast<uint32_t*>(stats.max_w.data_ptr<int32_t>()), reinterpret_cast<uint32_t*>(stats.n_pix.data_ptr<int32_t>()),
                                            reinterpret_cast<uint64_t*>(stats.sum_w.data_ptr<int64_t>()), current_stream()),
              "gslic_contribution_accumulate");
    }
    // Adds ONE view with a near-bound image — the Python host's ContributionStats.accumulate(camera, free_space=near): the same forward, then one
    // gslic_contribution_accumulate_free_space.  near_bound: float [H,W] on the map's device in view-space depth units (a pixel is measured where
    // it is > 0; typically d - (margin_abs + margin_rel d) of a LiDAR depth image, 0 where nothing was measured).  The three base statistics come out
    // as accumulate_contribution's, bit for bit; stats.meas_sum += sum of w over the measured pixels, stats.free_sum += sum of w over the
    // measured pixels the Gaussian lies in front of (view depth < bound).  The two arrays are created at the first such call.
    void accumulate_free_space(const FusedCamera& cam, ContributionStats& stats, float w_min, const torch::Tensor& near_bound)
    {
        torch::NoGradGuard ng;
        const int64_t P = prm_[0].size(0);
        const int W = cam.image_width, H = cam.image_height;
        TORCH_CHECK(near_bound.defined() && near_bound.dim() == 2 && near_bound.size(0) == H && near_bound.size(1) == W && near_bound.is_floating_point() &&
                        near_bound.device() == prm_[0].device(),
                    "FusedStep::accumulate_free_space: near_bound must be a float [", H, ", ", W, "] tensor on the map's device");
        const torch::Tensor near = near_bound.detach().to(torch::kFloat32).contiguous();
        fit_rows(stats.rows(), {&stats.free_sum, &stats.meas_sum});
        stats.views++;
        if (P == 0) return;
        int32_t R = 0, B = 0;
        const gslic_raster_params rp = statistics_forward(cam, R, B);
        check(gslic_contribution_accumulate_free_space(&rp, R, B, cptr(scratch_[0]), cptr(scratch_[1]), cptr(scratch_[2]), w_min,
                                                       reinterpret_cast<uint32_t*>(stats.max_w.data_ptr<int32_t>()),
                                                       reinterpret_cast<uint32_t*>(stats.n_pix.data_ptr<int32_t>()),
                                                       reinterpret_cast<uint64_t*>(stats.sum_w.data_ptr<int64_t>()), near.data_ptr<float>(),
                                                       reinterpret_cast<uint64_t*>(stats.free_sum.data_ptr<int64_t>()),
                                                       reinterpret_cast<uint64_t*>(stats.meas_sum.data_ptr<int64_t>()), current_stream()),
              "gslic_contribution_accumulate_free_space");
    }
    // The per-pixel geometry images of ONE view — the Python host's trainer.geometry_images: the statistics passes' raw-parameter forward (it
    // reuses the step's scratch; call it between steps) and one gslic_geometry_images on its buffers.  The images written are the tensors of `out`
    // that are defined (float32 [H,W] on the map's device, top_row int32, contiguous); an `out` with none gets the default set (opacity,
    // depth_norm, depth_median, top_row) from GeometryImages::make.  a_min > 0 guards depth_norm's division.  The map and its moments are not touched.
    void geometry_images(const FusedCamera& cam, GeometryImages& out, float a_min = 0.05f)
    {
        torch::NoGradGuard ng;
        const int64_t P = prm_[0].size(0);
        const int W = cam.image_width, H = cam.image_height;
        auto imgs = out.all();
        if (std::none_of(imgs.begin(), imgs.end(), [](const torch::Tensor* t) { return t->defined(); })) out.make(H, W, prm_[0].device());
        void* ptr[7];
        for (int i = 0; i < 7; i++) {
            const torch::Tensor& t = *imgs[i];
            TORCH_CHECK(!t.defined() || (t.numel() == (int64_t)H * W && t.is_contiguous() && t.device() == prm_[0].device() &&
                                         t.scalar_type() == (i == 5 ? torch::kInt32 : torch::kFloat32)),
                        "FusedStep::geometry_images: image ", i, " must be a contiguous ", i == 5 ? "int32" : "float32", " [", H, ", ", W, "] tensor on the map's device");
            ptr[i] = t.defined() ? t.data_ptr() : nullptr;
        }
        TORCH_CHECK(!out.depth_norm.defined() || a_min > 0.0f, "FusedStep::geometry_images: a_min must be > 0 for depth_norm");
        int32_t R = 0, B = 0;
        const gslic_raster_params rp = P > 0 ? statistics_forward(cam, R, B) : raster_params(cam, true, false);
        check(gslic_geometry_images(&rp, R, B, P > 0 ? cptr(scratch_[0]) : nullptr, P > 0 ? cptr(scratch_[1]) : nullptr, P > 0 ? cptr(scratch_[2]) : nullptr,
                                    a_min, (float*)ptr[0], (float*)ptr[1], (float*)ptr[2], (float*)ptr[3], (float*)ptr[4], (int32_t*)ptr[5], (float*)ptr[6],
                                    current_stream()),
              "gslic_geometry_images");
    }
    // Clone / split densification on the device — the Python host's GaussianModel.densify (gaussian-lic_amd/trainer.py), same calls, same result:
    // ONE gslic_densify_select (which rows grow, and where their new rows go) and ONE gslic_densify_emit (the new rows of the 18 parameter and
    // moment arrays plus the tie rank; the split parents' rows rewritten in place).  grow / protect: bool / uint8 [P] on the map's device in STORAGE
    // row order (protect may be undefined).  split_scale > 0 is a limit in the ACTIVATED domain, converted once, in double, to log(split_scale) and
    // rounded to float (nullopt or +inf: every row clones); the rule, the placement of the new rows and the counter-based noise keyed by `seed` and
    // the row's ORIGINAL index are written out in include/gslic_hip.h.  Every rank of an N-GPU run calls it with identical arguments and seed.
    // Returns the parents (device int64 [k]): parents[j] is the storage row of the parent of new row P + j.  max_new: more eligible rows than
    // this throw before anything is changed.  After a call that returned k > 0 the six parameter tensors are NEW views: fetch them with param(i);
    // a tie rank (set_tie_rank) gains the ties P .. P + k - 1.  stats: contribution statistics of this map — zero for the new rows and for the
    // split parents' rows (child 0 has contributed to nothing yet), unchanged for clone parents.  n_split: how many parents split.
    torch::Tensor densify(const torch::Tensor& grow, std::optional<double> split_scale, const torch::Tensor& protect = torch::Tensor(), uint32_t seed = 0,
                          ContributionStats* stats = nullptr, int64_t* n_split = nullptr, std::optional<int64_t> max_new = std::nullopt)
    {
        torch::NoGradGuard ng;
        const int64_t P = prm_[0].size(0);
        auto io = prm_[0].options().requires_grad(false).dtype(torch::kInt32);
        float thr = std::numeric_limits<float>::infinity();
        if (split_scale) {
            TORCH_CHECK(*split_scale > 0.0, "FusedStep::densify: split_scale must be a number > 0");
            if (std::isfinite(*split_scale)) thr = (float)std::log(*split_scale);
        }
        if (n_split) *n_split = 0;
        TORCH_CHECK(grow.defined(), "FusedStep::densify: grow is required");
        const torch::Tensor gr = row_mask(grow, "FusedStep::densify: ", "grow", P), pr = row_mask(protect, "FusedStep::densify: ", "protect", P);
        if (P == 0) return torch::empty({0}, io.dtype(torch::kInt64));
        torch::Tensor parent = torch::empty({P}, io), sel_scratch = torch::empty({0}, io.dtype(torch::kByte));
        int32_t count = 0, splits = 0;
        check(gslic_densify_select((int32_t)P, f(prm_[0]), f(prm_[1]), f(prm_[3]), f(prm_[4]), f(prm_[5]), u8(gr), u8(pr),
                                   tie_.defined() ? reinterpret_cast<const uint32_t*>(tie_.data_ptr<int32_t>()) : nullptr, thr, grow_cb, &sel_scratch,
                                   reinterpret_cast<uint32_t*>(parent.data_ptr<int32_t>()), &count, &splits, current_stream()),
              "gslic_densify_select");
        TORCH_CHECK(!max_new || count <= *max_new, "FusedStep::densify: ", count, " rows would be added, max_new is ", *max_new);
        if (count == 0) return torch::empty({0}, io.dtype(torch::kInt64));
        const torch::Tensor parents = parent.narrow(0, 0, count).to(torch::kInt64);
        torch::Tensor split_rows;   // which parents split, from the scaling the emission has not yet rewritten (the rule's own comparison)
        if (!carried(stats).empty() && splits > 0) split_rows = parents.masked_select(prm_[4].detach().index_select(0, parents).gt(thr).any(1));
        reserve(P + count);
        if (tie_.defined()) {
            torch::Tensor nt = torch::empty({P + count}, tie_.options());
            nt.narrow(0, 0, P).copy_(tie_);
            tie_ = nt;
        }
        const int64_t M = buf_[2].numel() ? buf_[2].size(1) : 0;
        float *pp[6], *pm[6], *pv[6];
        for (int g = 0; g < 6; g++) {
            const bool on = buf_[g].numel() != 0;   // features_rest is [cap,0,3] at SH degree 0
            pp[g] = on ? buf_[g].data_ptr<float>() : nullptr; pm[g] = on ? mbuf_[g].data_ptr<float>() : nullptr; pv[g] = on ? vbuf_[g].data_ptr<float>() : nullptr;
        }
        check(gslic_densify_emit((int32_t)P, count, reinterpret_cast<const uint32_t*>(parent.data_ptr<int32_t>()), (int32_t)M, pp, pm, pv,
                                 tie_.defined() ? reinterpret_cast<uint32_t*>(tie_.data_ptr<int32_t>()) : nullptr, thr, seed, current_stream()),
              "gslic_densify_emit");
        bind(P + count);
        // new rows and child 0 of a split have contributed to nothing and been seen by no view yet; a clone's parent is the Gaussian it was
        for (const auto& list : carried(stats)) zero_rows(list, P, count, split_rows);
        if (n_split) *n_split = splits;
        rows_appended(stats);   // (parents are the rows BEFORE a re-sort, as the Python host returns them)
        return parents;
    }
    const torch::Tensor& param(int group) const { return prm_[group]; }
    const torch::Tensor& tie_rank() const { return tie_; }   // int32 [P] original index of every storage row; undefined: the rows are in their original order
    int64_t size() const { return prm_[0].size(0); }
    int64_t capacity() const { return buf_[0].defined() ? buf_[0].size(0) : prm_[0].size(0); }

    // One optimisation step on one view.  Returns the device tensor [mean |image - gt|, mean ssim]; nothing synchronises.
    torch::Tensor step(const FusedCamera& cam, const torch::Tensor& gt_image) { return step_body(cam, gt_image, nullptr, 0.0f, nullptr, DepthLossOptions{}); }

    // One optimisation step on one view with LiDAR depth supervision.  Returns the device tensor [mean |image - gt|, mean ssim, L_d]; nothing
    // synchronises.  An undefined gt_depth or lambda_depth == 0 is the colour-only step above (two terms).
    // weight (optional, fp32 [H,W]; a mask is the 0/1 case): the colour loss becomes the weighted one — gslic_l1_ssim_loss_weighted_forward_backward,
    // the calls of the Python host's training_step_fused(weight=...); terms[0:2] are the weighted means and weight_sum() the sum of the weights.  An
    // undefined weight is the unweighted step, the same calls as ever.
    // depth_weight (optional, fp32 [H,W]) and depth_huber (the smooth-L1 threshold, 0 = L1): the depth loss becomes the weighted one —
    // gslic_depth_loss_weighted_forward_backward, the call of the Python host's training_step_fused(depth_weight=, depth_huber=): NaN, negative and
    // +inf weights read as 0, NO clamp at 1; depth_weight_sum() is the sum of the weights over the measured pixels.  An undefined depth_weight with
    // depth_huber == 0 is the unweighted depth loss, the same calls as ever.  Either of them without a depth target is an error.
    torch::Tensor step(const FusedCamera& cam, const torch::Tensor& gt_image, const torch::Tensor& gt_depth, float lambda_depth,
                       const torch::Tensor& weight = torch::Tensor(), const torch::Tensor& depth_weight = torch::Tensor(), float depth_huber = 0.0f)
    {
        TORCH_CHECK(gt_depth.defined() || (!depth_weight.defined() && depth_huber == 0.0f), "depth_weight / depth_huber given without gt_depth");
        const DepthLossOptions dlo{depth_weight.defined() ? &depth_weight : nullptr, depth_huber};
        return step_body(cam, gt_image, gt_depth.defined() && lambda_depth != 0.0f ? &gt_depth : nullptr, lambda_depth, weight.defined() ? &weight : nullptr, dlo);
    }
    // S = the sum of the depth weights over the measured pixels of the last weighted / Huber depth loss: a device [1] view (undefined before the first)
    torch::Tensor depth_weight_sum() const { return dwterms_.defined() ? dwterms_.slice(0, 1, 2) : torch::Tensor(); }
    // S = the sum of the (clamped) weights of the last weighted step / pose gradient: a device [1] view (undefined before the first)
    torch::Tensor weight_sum() const { return wterms_.defined() ? wterms_.slice(0, 2, 3) : torch::Tensor(); }

    // Gradient of the training loss w.r.t. a LEFT se(3) increment of the camera pose, T_cw <- exp(xi^) T_cw, xi = (rho, phi) — the "cam" of the
    // north-star; the reference's autograd node returns nothing for its camera inputs (rasterizer.cpp:171-182).  Forward + loss kernels +
    // gslic_rasterize_backward_camera (the map is NOT updated), then the chain of gaussian-lic_amd/camera.py:Camera.pose_gradient:
    //   G = dL/dV + Proj^T dL/d(Proj V) (top three rows; Proj = (Proj V) V^-1),  G_R = G[:, :3] - t g_c^T,  G_t = G[:, 3] - R g_c,
    //   dL/drho = G_t,  dL/dphi = vee(M - M^T) + t x G_t,  M = G_R R^T.          Returns {d/drho[3], d/dphi[3]}; synchronises (35 floats to the host).
    std::array<double, 6> pose_gradient(const FusedCamera& cam, const torch::Tensor& gt_image) { return pose_gradient_body(cam, gt_image, nullptr, 0.0f, nullptr, nullptr, DepthLossOptions{}); }
    // The same gradient under LiDAR depth supervision: loss = (1 - lambda) L1 + lambda (1 - SSIM) + lambda_depth L_d.  gslic_rasterize_forward_depth, the
    // colour and depth loss calls of step(cam, gt_image, gt_depth, lambda_depth), gslic_rasterize_backward_depth_camera, the same chain — the calls
    // gaussian-lic_amd/trainer.py:pose_gradient(gt_depth=...) issues.  terms_out (optional): the device tensor [mean L1, mean SSIM, L_d].  An undefined
    // gt_depth or lambda_depth == 0 is the colour-only gradient above.  weight (optional, fp32 [H,W]): the weighted colour loss, as step()'s.
    // depth_weight / depth_huber: the weighted / Huber depth loss, as step()'s.
    std::array<double, 6> pose_gradient(const FusedCamera& cam, const torch::Tensor& gt_image, const torch::Tensor& gt_depth, float lambda_depth,
                                        torch::Tensor* terms_out = nullptr, const torch::Tensor& weight = torch::Tensor(),
                                        const torch::Tensor& depth_weight = torch::Tensor(), float depth_huber = 0.0f)
    {
        TORCH_CHECK(gt_depth.defined() || (!depth_weight.defined() && depth_huber == 0.0f), "depth_weight / depth_huber given without gt_depth");
        const torch::Tensor* w = weight.defined() ? &weight : nullptr;
        if (!gt_depth.defined() || lambda_depth == 0.0f) return w ? pose_gradient_body(cam, gt_image, nullptr, 0.0f, terms_out, w, DepthLossOptions{}) : pose_gradient(cam, gt_image);
        return pose_gradient_body(cam, gt_image, &gt_depth, lambda_depth, terms_out, w, DepthLossOptions{depth_weight.defined() ? &depth_weight : nullptr, depth_huber});
    }
    // The same gradient for row `view` of a PoseSet, with the chain on the DEVICE: the render is from the row (`cam` supplies the image size and the
    // scalars), gslic_pose_step runs one launch behind the camera backward and leaves dL/d(rho, phi) in poses->grad — returned, a device [6]
    // tensor; no synchronisation, no host copy.  do_step: the same launch also steps the row (Adam on the six coordinates, the retraction).  The
    // calls gaussian-lic_amd/trainer.py:pose_gradient(poses=, view=, do_step=) issues.  gt_depth / lambda_depth / weight / depth_weight /
    // depth_huber as above; with set_exposure, the exposure row that call named.
    // shared (a set built with shared): gslic_pose_step_shared in place of gslic_pose_step — returns poses->shared_grad [7]; do_step moves every row.
    torch::Tensor pose_gradient(const FusedCamera& cam, const torch::Tensor& gt_image, PoseSet* poses, int view, bool do_step,
                                const torch::Tensor& gt_depth = torch::Tensor(), float lambda_depth = 0.0f, torch::Tensor* terms_out = nullptr,
                                const torch::Tensor& weight = torch::Tensor(), const torch::Tensor& depth_weight = torch::Tensor(), float depth_huber = 0.0f,
                                bool shared = false)
    {
        TORCH_CHECK(poses != nullptr, "pose_gradient: poses is NULL");
        TORCH_CHECK(gt_depth.defined() || (!depth_weight.defined() && depth_huber == 0.0f), "depth_weight / depth_huber given without gt_depth");
        const FusedCamera row = poses->row_camera(view, cam);
        const torch::Tensor* w = weight.defined() ? &weight : nullptr;
        const bool depth = gt_depth.defined() && lambda_depth != 0.0f;
        torch::Tensor camg;
        pose_gradient_body(row, gt_image, depth ? &gt_depth : nullptr, depth ? lambda_depth : 0.0f, terms_out, w,
                           depth ? DepthLossOptions{depth_weight.defined() ? &depth_weight : nullptr, depth_huber} : DepthLossOptions{}, &camg);
        if (shared) {
            poses->shared_adam_step(view, camg, do_step);
            return poses->shared_grad;
        }
        poses->adam_step(view, camg, do_step);
        return poses->grad;
    }
    // One joint map + pose iteration on row `view` of a PoseSet: the render is from the row (`cam` supplies the image size and the scalars), the
    // map's masked Adam runs inside the backward that also returns the camera gradient (gslic_rasterize_backward_camera_adam / _depth_camera_adam: the
    // gradient of the map as it was before its update), and gslic_pose_step, one launch behind it, steps the row and leaves dL/d(rho, phi) in
    // poses->grad.  The calls gaussian-lic_amd/trainer.py:training_step_with_pose(poses=, view=, adam_in_backward=True) issues; returns the terms
    // tensor; no synchronisation, no host copy.  gt_depth / lambda_depth / weight / depth_weight / depth_huber as step()'s; with set_exposure the
    // exposure row that call named is applied and updated as step() does.  Not with attached gradient statistics (the camera backward accumulates none).
    // shared (a set built with shared): the pose launch is gslic_pose_step_shared — the view's gradient steps the shared extrinsic / time-offset
    // coordinates and every row moves (trainer.training_step_with_pose(shared=True, adam_in_backward=True)); the gradient is poses->shared_grad.
    torch::Tensor step_with_pose(const FusedCamera& cam, const torch::Tensor& gt_image, PoseSet* poses, int view,
                                 const torch::Tensor& gt_depth = torch::Tensor(), float lambda_depth = 0.0f, const torch::Tensor& weight = torch::Tensor(),
                                 const torch::Tensor& depth_weight = torch::Tensor(), float depth_huber = 0.0f, bool shared = false)
    {
        TORCH_CHECK(poses != nullptr, "step_with_pose: poses is NULL");
        TORCH_CHECK(!gstats_, "step_with_pose: gradient statistics are attached (the fused camera backward accumulates none)");
        TORCH_CHECK(gt_depth.defined() || (!depth_weight.defined() && depth_huber == 0.0f), "depth_weight / depth_huber given without gt_depth");
        const FusedCamera row = poses->row_camera(view, cam);
        const bool depth = gt_depth.defined() && lambda_depth != 0.0f;
        torch::Tensor camg;
        torch::Tensor terms = step_body(row, gt_image, depth ? &gt_depth : nullptr, depth ? lambda_depth : 0.0f, weight.defined() ? &weight : nullptr,
                                        depth ? DepthLossOptions{depth_weight.defined() ? &depth_weight : nullptr, depth_huber} : DepthLossOptions{}, &camg);
        if (shared) poses->shared_adam_step(view, camg, /*do_step=*/true);
        else poses->adam_step(view, camg, /*do_step=*/true);
        return terms;
    }
    // the chain alone, on host arrays in the element order of the kernels' inputs (float[16] with (r, c) at [4c + r])
    static std::array<double, 6> se3_pose_gradient(const float* view16, const float* fullproj16, const float* dview16, const float* dproj16, const float* dcampos3)
    {
        auto at = [](const float* m, int r, int c) { return (double)m[4 * c + r]; };
        double V[4][4], PV[4][4], Vi[4][4], Pj[4][4];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { V[r][c] = at(view16, r, c); PV[r][c] = at(fullproj16, r, c); }
        // V^-1 of a rigid [R | t; 0 0 0 1]: [R^T | -R^T t]
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) Vi[r][c] = V[c][r]; Vi[r][3] = -(V[0][r] * V[0][3] + V[1][r] * V[1][3] + V[2][r] * V[2][3]); }
        Vi[3][0] = Vi[3][1] = Vi[3][2] = 0.0; Vi[3][3] = 1.0;
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { Pj[r][c] = 0; for (int k = 0; k < 4; k++) Pj[r][c] += PV[r][k] * Vi[k][c]; }   // Proj = (Proj V) V^-1
        double G[3][4];
        for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) { G[r][c] = at(dview16, r, c); for (int k = 0; k < 4; k++) G[r][c] += Pj[k][r] * at(dproj16, k, c); }
        const double gc[3] = {dcampos3[0], dcampos3[1], dcampos3[2]}, t[3] = {V[0][3], V[1][3], V[2][3]};
        double GR[3][3], Gt[3], M[3][3];
        for (int j = 0; j < 3; j++) {
            for (int i = 0; i < 3; i++) GR[j][i] = G[j][i] - t[j] * gc[i];
            Gt[j] = G[j][3] - (V[j][0] * gc[0] + V[j][1] * gc[1] + V[j][2] * gc[2]);
        }
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { M[i][j] = 0; for (int k = 0; k < 3; k++) M[i][j] += GR[i][k] * V[j][k]; }   // G_R R^T
        return {Gt[0], Gt[1], Gt[2], M[2][1] - M[1][2] + (t[1] * Gt[2] - t[2] * Gt[1]), M[0][2] - M[2][0] + (t[2] * Gt[0] - t[0] * Gt[2]),
                M[1][0] - M[0][1] + (t[0] * Gt[1] - t[1] * Gt[0])};
    }

    float loss_value(const torch::Tensor& terms) const   // (1 - lambda) L1 + lambda (1 - SSIM), gaussian.cpp:685-691; synchronises
    {
        torch::Tensor t = terms.to(torch::kCPU);
        return (1.0f - lambda_dssim_) * t[0].item<float>() + lambda_dssim_ * (1.0f - t[1].item<float>());
    }
    float loss_value(const torch::Tensor& terms, float lambda_depth) const   // + lambda_depth L_d for the three terms of a depth step; synchronises
    {
        if (lambda_depth == 0.0f) return loss_value(terms);
        torch::Tensor t = terms.to(torch::kCPU);
        return (1.0f - lambda_dssim_) * t[0].item<float>() + lambda_dssim_ * (1.0f - t[1].item<float>()) + lambda_depth * t[2].item<float>();
    }
    const torch::Tensor& depth() const { return depth_; }                 // last depth render [H,W] (depth steps)
    const torch::Tensor& image() const { return image_; }                 // last render [3,H,W]
    torch::Tensor visible() const { return radii_ > 0; }                  // render_pkg's visibility filter (renderer.cpp:86)
    const torch::Tensor& exp_avg(int group) const { return m_[group]; }
    const torch::Tensor& exp_avg_sq(int group) const { return v_[group]; }

private:
    // what shapes the depth loss beyond its target: the per-pixel weight image (nullptr: none) and the Huber threshold (0: L1)
    struct DepthLossOptions {
        const torch::Tensor* weight = nullptr;
        float huber = 0.0f;
    };
    // the params of one view: raw = the six tensors are the RAW parameters (activated inside the kernels); no_color = transmittance only
    gslic_raster_params raster_params(const FusedCamera& cam, bool raw, bool no_color) const
    {
        gslic_raster_params rp{};
        rp.tie_rank = tie_.defined() ? reinterpret_cast<const uint32_t*>(tie_.data_ptr<int32_t>()) : nullptr;
        rp.P = (int32_t)prm_[0].size(0); rp.D = deg_; rp.M = prm_[2].numel() ? (int32_t)prm_[2].size(1) : 0;
        rp.width = cam.image_width; rp.height = cam.image_height;
        rp.tan_fovx = cam.tanfovx; rp.tan_fovy = cam.tanfovy;
        rp.limx_neg = cam.limx_neg; rp.limx_pos = cam.limx_pos; rp.limy_neg = cam.limy_neg; rp.limy_pos = cam.limy_pos;
        rp.scale_modifier = 1.0f; rp.raw_params = raw ? 1 : 0; rp.no_color = no_color ? 1 : 0;
        return rp;
    }
    // the step's persistent buffers: created on the first step and when the image size / the number of Gaussians changes
    void ensure_image_buffers(int H, int W)
    {
        if (image_.defined() && image_.size(1) == H && image_.size(2) == W) return;
        auto fo = prm_[0].options().requires_grad(false);
        image_ = torch::empty({3, H, W}, fo);
        final_T_ = torch::empty({H, W}, fo);
        for (auto& d : dm_) d = torch::empty({3, H, W}, fo);
        dL_dimage_ = torch::empty({3, H, W}, fo);
        partials_ = torch::empty({gslic_loss_partials_count(1, 3, H, W)}, fo);
    }
    void ensure_depth_buffers(int H, int W)
    {
        if (depth_.defined() && depth_.size(0) == H && depth_.size(1) == W) return;
        auto fo = prm_[0].options().requires_grad(false);
        depth_ = torch::empty({H, W}, fo);
        dL_ddepth_ = torch::empty({H, W}, fo);
        depth_partials_ = torch::empty({gslic_depth_l1_loss_partials_count(H, W)}, fo);
    }
    void ensure_rows(int64_t P)
    {
        if (!radii_.defined() || radii_.size(0) != P) radii_ = torch::empty({P}, prm_[0].options().requires_grad(false).dtype(torch::kInt32));
    }
    // The colour loss of a view, forward and backward: terms[0:2] and dL.  weight: the weighted loss (its three launches, then terms[0:2] <- the
    // weighted means; S stays in wterms_[2]: weight_sum()).  Otherwise the fused pair of launches — the reduction of the partial sums rides on the
    // backward kernel — or, two_calls, gslic_l1_ssim_loss_forward + _backward: the colour-only pose gradient, as it always ran.
    void colour_loss(int H, int W, const torch::Tensor& image, const torch::Tensor& gt_image, const torch::Tensor* weight, torch::Tensor (&dm)[3],
                     torch::Tensor& partials, torch::Tensor& terms, torch::Tensor& dL, bool two_calls = false)
    {
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;   // loss_utils.h:187-188
        float *d1 = dm[0].data_ptr<float>(), *d2 = dm[1].data_ptr<float>(), *d3 = dm[2].data_ptr<float>();
        if (weight) {
            TORCH_CHECK(weight->is_contiguous() && weight->scalar_type() == torch::kFloat32 && weight->dim() == 2 && weight->size(0) == H && weight->size(1) == W,
                        "weight must be contiguous fp32 [H,W]");
            auto fo = prm_[0].options().requires_grad(false);
            const int64_t n = gslic_l1_ssim_loss_weighted_partials_count(3, H, W);
            if (!wpartials_.defined() || wpartials_.size(0) != n) wpartials_ = torch::empty({n}, fo);
            if (!wterms_.defined()) wterms_ = torch::zeros({3}, fo);
            check(gslic_l1_ssim_loss_weighted_forward_backward(3, H, W, C1, C2, lambda_dssim_, f(image), f(gt_image), f(*weight), d1, d2, d3,
                                                               wpartials_.data_ptr<float>(), wterms_.data_ptr<float>(), dL.data_ptr<float>(), current_stream()),
                  "gslic_l1_ssim_loss_weighted_forward_backward");
            terms.slice(0, 0, 2).copy_(wterms_.slice(0, 0, 2));
        } else if (two_calls) {
            check(gslic_l1_ssim_loss_forward(1, 3, H, W, C1, C2, f(image), f(gt_image), d1, d2, d3, partials.data_ptr<float>(), terms.data_ptr<float>(),
                                             current_stream()),
                  "gslic_l1_ssim_loss_forward");
            check(gslic_l1_ssim_loss_backward(1, 3, H, W, lambda_dssim_, f(image), f(gt_image), d1, d2, d3, dL.data_ptr<float>(), current_stream()),
                  "gslic_l1_ssim_loss_backward");
        } else {
            check(gslic_l1_ssim_loss_forward_backward(1, 3, H, W, C1, C2, lambda_dssim_, f(image), f(gt_image), d1, d2, d3, partials.data_ptr<float>(),
                                                      terms.data_ptr<float>(), dL.data_ptr<float>(), current_stream()),
                  "gslic_l1_ssim_loss_forward_backward");
        }
    }
    // the depth loss of a view, forward and backward: terms[2] and dLd.  With a weight image or a Huber threshold the weighted call (its two launches,
    // then terms[2] <- L_d; S stays in dwterms_[1]: depth_weight_sum()), otherwise the unweighted call as it always ran.
    void depth_loss(int H, int W, float lambda_depth, const torch::Tensor& depth, const torch::Tensor& gt_depth, torch::Tensor& partials, torch::Tensor& terms,
                    torch::Tensor& dLd, const DepthLossOptions& dlo)
    {
        if (dlo.weight || dlo.huber != 0.0f) {
            const torch::Tensor* w = dlo.weight;
            TORCH_CHECK(!w || (w->is_contiguous() && w->scalar_type() == torch::kFloat32 && w->dim() == 2 && w->size(0) == H && w->size(1) == W),
                        "depth_weight must be contiguous fp32 [H,W]");
            auto fo = prm_[0].options().requires_grad(false);
            const int64_t n = gslic_depth_loss_weighted_partials_count(H, W);
            if (!dwpartials_.defined() || dwpartials_.size(0) != n) dwpartials_ = torch::empty({n}, fo);
            if (!dwterms_.defined()) dwterms_ = torch::zeros({2}, fo);
            check(gslic_depth_loss_weighted_forward_backward(H, W, lambda_depth, dlo.huber, f(depth), f(gt_depth), w ? f(*w) : nullptr,
                                                             dwpartials_.data_ptr<float>(), dwterms_.data_ptr<float>(), dLd.data_ptr<float>(), current_stream()),
                  "gslic_depth_loss_weighted_forward_backward");
            terms.slice(0, 2, 3).copy_(dwterms_.slice(0, 0, 1));
            return;
        }
        check(gslic_depth_l1_loss_forward_backward(H, W, lambda_depth, f(depth), f(gt_depth), partials.data_ptr<float>(), terms.data_ptr<float>() + 2,
                                                   dLd.data_ptr<float>(), current_stream()),
              "gslic_depth_l1_loss_forward_backward");
    }
    // the exposure model around the colour loss: E of the attached view applied into ex_image_ (returned), and the backward that turns the loss's
    // dL/dout into dL (= E^T dL/dout) and exposure_->grad, with the row's Adam update when asked for
    const torch::Tensor& exposure_apply(int H, int W, const torch::Tensor& image)
    {
        if (!ex_image_.defined() || ex_image_.size(1) != H || ex_image_.size(2) != W) {
            auto fo = prm_[0].options().requires_grad(false);
            ex_image_ = torch::empty({3, H, W}, fo);
            ex_dL_ = torch::empty({3, H, W}, fo);
            ex_partials_ = torch::empty({gslic_exposure_partials_count(H, W)}, fo);
        }
        check(gslic_exposure_apply(H, W, f(exposure_->matrix(exposure_view_)), f(image), ex_image_.data_ptr<float>(), current_stream()), "gslic_exposure_apply");
        return ex_image_;
    }
    void exposure_backward(int H, int W, const torch::Tensor& image, const torch::Tensor& dL_dout, torch::Tensor& dL, bool adam)
    {
        const gslic_exposure_adam ad = exposure_->descriptor(exposure_view_);
        check(gslic_exposure_backward(H, W, f(exposure_->matrix(exposure_view_)), f(image), f(dL_dout), dL.data_ptr<float>(), ex_partials_.data_ptr<float>(),
                                      exposure_->grad.data_ptr<float>(), adam ? &ad : nullptr, current_stream()),
              "gslic_exposure_backward");
    }
    static void check_targets(const FusedCamera& cam, const torch::Tensor& gt_image, const torch::Tensor* gt_depth)
    {
        const int W = cam.image_width, H = cam.image_height;
        TORCH_CHECK(gt_image.is_contiguous() && gt_image.dim() == 3 && gt_image.size(1) == H && gt_image.size(2) == W, "gt_image must be contiguous [3,H,W]");
        TORCH_CHECK(!gt_depth || (gt_depth->is_contiguous() && gt_depth->scalar_type() == torch::kFloat32 && gt_depth->dim() == 2 &&
                                  gt_depth->size(0) == H && gt_depth->size(1) == W), "gt_depth must be contiguous fp32 [H,W]");
    }

    // The forward of a view: gslic_rasterize_forward, or gslic_rasterize_forward_depth when a depth image is asked for.  op / sc / rot: opacity, scaling
    // and rotation as rp.raw_params says (the raw parameters, or LibTorch's activations of them).  Fills scratch_[0..3] and the two counts.
    void forward(const gslic_raster_params& rp, const FusedCamera& cam, const float* op, const float* sc, const float* rot, torch::Tensor& image,
                 torch::Tensor& final_T, torch::Tensor* depth, torch::Tensor& radii, int32_t& R, int32_t& B)
    {
        const float *xyz = f(prm_[0]), *dc = f(prm_[1]), *rest = f(prm_[2]);
        const float *view = f(cam.world_view_transform), *proj = f(cam.full_proj_transform), *cpos = f(cam.camera_center);
        if (depth)
            check(gslic_rasterize_forward_depth(&rp, grow_cb, &scratch_[0], grow_cb, &scratch_[1], grow_cb, &scratch_[2], grow_cb, &scratch_[3], f(bg_), xyz,
                                                dc, rest, nullptr, op, sc, rot, nullptr, view, proj, cpos, image.data_ptr<float>(), final_T.data_ptr<float>(),
                                                depth->data_ptr<float>(), radii.data_ptr<int32_t>(), &R, &B, current_stream()),
                  "gslic_rasterize_forward_depth");
        else
            check(gslic_rasterize_forward(&rp, grow_cb, &scratch_[0], grow_cb, &scratch_[1], grow_cb, &scratch_[2], grow_cb, &scratch_[3], f(bg_), xyz, dc,
                                          rest, nullptr, op, sc, rot, nullptr, view, proj, cpos, image.data_ptr<float>(), final_T.data_ptr<float>(),
                                          radii.data_ptr<int32_t>(), &R, &B, current_stream()),
                  "gslic_rasterize_forward");
    }
// what all six backward entry points take first: the forward's parameters, inputs and buffers, and dL/dimage
#define GSLIC_FUSED_BACKWARD_INPUTS(radii, dL)                                                                                                                \
    &rp, R, B, f(bg_), f(prm_[0]), f(prm_[1]), f(prm_[2]), nullptr, f(prm_[4]), f(prm_[5]), nullptr, f(cam.world_view_transform),                              \
        f(cam.full_proj_transform), f(cam.camera_center), (radii).data_ptr<int32_t>(), cptr(scratch_[0]), cptr(scratch_[1]), cptr(scratch_[2]),              \
        cptr(scratch_[3]), f(dL)
    // The backward of a step with the masked Adam inside: one of the four *_adam* entry points, by whether the view is depth-supervised and whether
    // gradient statistics are attached (the same step, which also adds this view to them).  Reads the step's own buffers.
    void backward_adam(const gslic_raster_params& rp, const FusedCamera& cam, int32_t R, int32_t B, bool depth)
    {
        const gslic_adam_fused ad = adam_descriptor();
        float* xg = depth ? xyz_grad_.data_ptr<float>() : nullptr;
        if (gstats_) {
            fit_rows(gstats_->rows());
            const gslic_grad_stats gs = gstats_->descriptor();
            if (depth)
                check(gslic_rasterize_backward_depth_adam_stats(GSLIC_FUSED_BACKWARD_INPUTS(radii_, dL_dimage_), f(dL_ddepth_), nullptr, xg, nullptr, nullptr,
                                                                nullptr, nullptr, lambda_erank_, &ad, &gs, current_stream()),
                      "gslic_rasterize_backward_depth_adam_stats");
            else
                check(gslic_rasterize_backward_adam_stats(GSLIC_FUSED_BACKWARD_INPUTS(radii_, dL_dimage_), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                          lambda_erank_, &ad, &gs, current_stream()),
                      "gslic_rasterize_backward_adam_stats");
        } else if (depth) {
            check(gslic_rasterize_backward_depth_adam(GSLIC_FUSED_BACKWARD_INPUTS(radii_, dL_dimage_), f(dL_ddepth_), nullptr, xg, nullptr, nullptr, nullptr,
                                                      nullptr, lambda_erank_, &ad, current_stream()),
                  "gslic_rasterize_backward_depth_adam");
        } else {
            check(gslic_rasterize_backward_adam(GSLIC_FUSED_BACKWARD_INPUTS(radii_, dL_dimage_), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                lambda_erank_, &ad, current_stream()),
                  "gslic_rasterize_backward_adam");
        }
    }
    // The backward of a pose gradient: the six parameter gradients into g (group order) and the camera's 16 + 16 + 3 floats into cg; with a defined dLd
    // the depth entry point.  The map is not touched.
    void backward_camera(const gslic_raster_params& rp, const FusedCamera& cam, int32_t R, int32_t B, torch::Tensor& radii, const torch::Tensor& dL,
                         const torch::Tensor& dLd, std::array<torch::Tensor, 6>& g, float* cg)
    {
        auto w = [](torch::Tensor& t) { return t.numel() ? t.data_ptr<float>() : nullptr; };
        if (dLd.defined())
            check(gslic_rasterize_backward_depth_camera(GSLIC_FUSED_BACKWARD_INPUTS(radii, dL), f(dLd), nullptr, nullptr, w(g[3]), nullptr, w(g[0]), nullptr,
                                                        w(g[1]), w(g[2]), w(g[4]), w(g[5]), lambda_erank_, cg, cg + 16, cg + 32, current_stream()),
                  "gslic_rasterize_backward_depth_camera");
        else
            check(gslic_rasterize_backward_camera(GSLIC_FUSED_BACKWARD_INPUTS(radii, dL), nullptr, nullptr, w(g[3]), nullptr, w(g[0]), nullptr, w(g[1]), w(g[2]),
                                                  w(g[4]), w(g[5]), lambda_erank_, cg, cg + 16, cg + 32, current_stream()),
                  "gslic_rasterize_backward_camera");
    }
    // The backward of a joint map + pose step: the masked Adam inside AND the camera's 16 + 16 + 3 floats into cg (gslic_rasterize_backward_camera_adam /
    // _depth_camera_adam).  Reads the step's own buffers.
    void backward_camera_adam(const gslic_raster_params& rp, const FusedCamera& cam, int32_t R, int32_t B, bool depth, float* cg)
    {
        const gslic_adam_fused ad = adam_descriptor();
        if (depth)
            check(gslic_rasterize_backward_depth_camera_adam(GSLIC_FUSED_BACKWARD_INPUTS(radii_, dL_dimage_), f(dL_ddepth_), nullptr, xyz_grad_.data_ptr<float>(),
                                                             nullptr, nullptr, nullptr, nullptr, lambda_erank_, &ad, cg, cg + 16, cg + 32, nullptr, current_stream()),
                  "gslic_rasterize_backward_depth_camera_adam");
        else
            check(gslic_rasterize_backward_camera_adam(GSLIC_FUSED_BACKWARD_INPUTS(radii_, dL_dimage_), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       lambda_erank_, &ad, cg, cg + 16, cg + 32, nullptr, current_stream()),
                  "gslic_rasterize_backward_camera_adam");
    }
#undef GSLIC_FUSED_BACKWARD_INPUTS

    // the step: forward, loss, depth loss, backward.  gt_depth != nullptr: under depth supervision
    // camg_out (step_with_pose): the backward also returns the camera gradient, 35 floats that stay on the device
    torch::Tensor step_body(const FusedCamera& cam, const torch::Tensor& gt_image, const torch::Tensor* gt_depth, float lambda_depth,
                            const torch::Tensor* weight, const DepthLossOptions& dlo, torch::Tensor* camg_out = nullptr)
    {
        torch::NoGradGuard ng;
        const bool depth = gt_depth != nullptr;
        const int64_t P = prm_[0].size(0);
        const int W = cam.image_width, H = cam.image_height;
        check_targets(cam, gt_image, gt_depth);
        const gslic_raster_params rp = raster_params(cam, true, false);
        auto fo = prm_[0].options().requires_grad(false);
        ensure_image_buffers(H, W);
        if (depth) ensure_depth_buffers(H, W);
        ensure_rows(P);
        if (depth && (!xyz_grad_.defined() || xyz_grad_.size(0) != P)) xyz_grad_ = torch::empty({P, 3}, fo);   // (xyz's gradient is assembled there before its update)
        torch::Tensor terms = torch::empty({depth ? 3 : 2}, fo);
        int32_t R = 0, B = 0;
        forward(rp, cam, f(prm_[3]), f(prm_[4]), f(prm_[5]), image_, final_T_, depth ? &depth_ : nullptr, radii_, R, B);
        if (exposure_) {
            colour_loss(H, W, exposure_apply(H, W, image_), gt_image, weight, dm_, partials_, terms, ex_dL_);
            exposure_backward(H, W, image_, ex_dL_, dL_dimage_, /*adam=*/true);
        } else {
            colour_loss(H, W, image_, gt_image, weight, dm_, partials_, terms, dL_dimage_);
        }
        if (depth) depth_loss(H, W, lambda_depth, depth_, *gt_depth, depth_partials_, terms, dL_ddepth_, dlo);
        if (camg_out) {
            *camg_out = torch::empty({35}, fo);
            backward_camera_adam(rp, cam, R, B, depth, camg_out->data_ptr<float>());
        } else {
            backward_adam(rp, cam, R, B, depth);
        }
        return terms;
    }

    // the pose gradient: forward, loss, depth loss, camera backward, the chain on the host.  gt_depth != nullptr: under depth supervision.  (The
    // colour-only path runs the unweighted loss as gslic_l1_ssim_loss_forward + _backward, every other path as the fused pair: both as they were.)
    std::array<double, 6> pose_gradient_body(const FusedCamera& cam, const torch::Tensor& gt_image, const torch::Tensor* gt_depth, float lambda_depth,
                                             torch::Tensor* terms_out, const torch::Tensor* weight, const DepthLossOptions& dlo,
                                             torch::Tensor* camg_out = nullptr)   // camg_out: the 35 camera gradient floats stay on the device, no chain here
    {
        torch::NoGradGuard ng;
        const bool depth = gt_depth != nullptr;
        const int64_t P = prm_[0].size(0);
        const int W = cam.image_width, H = cam.image_height;
        if (depth) check_targets(cam, gt_image, gt_depth);
        const gslic_raster_params rp = raster_params(cam, true, false);
        auto fo = prm_[0].options().requires_grad(false);
        torch::Tensor image = torch::empty({3, H, W}, fo), final_T = torch::empty({H, W}, fo), dL = torch::empty({3, H, W}, fo), dm[3], zimg, dLd, dpartials;
        for (torch::Tensor& d : dm) d = torch::empty({3, H, W}, fo);
        if (depth) { zimg = torch::empty({H, W}, fo); dLd = torch::empty({H, W}, fo); dpartials = torch::empty({gslic_depth_l1_loss_partials_count(H, W)}, fo); }
        torch::Tensor radii = torch::empty({P}, fo.dtype(torch::kInt32));
        torch::Tensor partials = torch::empty({gslic_loss_partials_count(1, 3, H, W)}, fo), terms = torch::empty({depth ? 3 : 2}, fo), camg = torch::zeros({35}, fo);
        std::array<torch::Tensor, 6> g;
        for (int i = 0; i < 6; i++) g[i] = torch::empty_like(prm_[i], fo);
        int32_t R = 0, B = 0;
        forward(rp, cam, f(prm_[3]), f(prm_[4]), f(prm_[5]), image, final_T, depth ? &zimg : nullptr, radii, R, B);
        if (exposure_) {
            torch::Tensor dLo = torch::empty({3, H, W}, fo);
            colour_loss(H, W, exposure_apply(H, W, image), gt_image, weight, dm, partials, terms, dLo);   // (the fused pair, as the Python host's)
            exposure_backward(H, W, image, dLo, dL, /*adam=*/false);
        } else {
            colour_loss(H, W, image, gt_image, weight, dm, partials, terms, dL, /*two_calls=*/!depth && !camg_out);   // (the pose-set route: the fused pair, as the Python host's)
        }
        if (depth) depth_loss(H, W, lambda_depth, zimg, *gt_depth, dpartials, terms, dLd, dlo);
        backward_camera(rp, cam, R, B, radii, dL, dLd, g, camg.data_ptr<float>());
        if (terms_out) *terms_out = terms;
        if (camg_out) { *camg_out = camg; return {}; }
        torch::Tensor hc = camg.to(torch::kCPU), hv = cam.world_view_transform.to(torch::kCPU).contiguous(), hp = cam.full_proj_transform.to(torch::kCPU).contiguous();
        return se3_pose_gradient(hv.data_ptr<float>(), hp.data_ptr<float>(), hc.data_ptr<float>(), hc.data_ptr<float>() + 16, hc.data_ptr<float>() + 32);
    }

    // the raw-parameter forward the statistics passes replay (P > 0): fills scratch_[0..2], returns its parameters and the two counts
    gslic_raster_params statistics_forward(const FusedCamera& cam, int32_t& R, int32_t& B)
    {
        const gslic_raster_params rp = raster_params(cam, true, false);
        ensure_image_buffers(cam.image_height, cam.image_width);
        ensure_rows(prm_[0].size(0));
        forward(rp, cam, f(prm_[3]), f(prm_[4]), f(prm_[5]), image_, final_T_, nullptr, radii_, R, B);
        return rp;
    }
    // GaussianModel._rows_appended's rule: the appended tail has grown past resort_fraction of the map
    void rows_appended(ContributionStats* stats)
    {
        const int64_t P = prm_[0].size(0);
        if (tie_.defined() && resort_fraction_ && (double)(P - sorted_P_) > *resort_fraction_ * (double)P) resort(stats);
    }
    // ---- The statistics objects that follow the rows, and the four operations the row changes apply to their row lists: the counterpart of the Python
    // host's _RowStatistics.  The invariant all of them keep: in every statistics array the rows behind size() are zero — so zero-extending an array
    // to capacity(), or zeroing rows that were just appended, never changes what an existing row holds.
    // carried: the ContributionStats handed to the row change when it holds anything, and the attached GradientStats
    std::vector<std::vector<StatRow>> carried(ContributionStats* stats) const
    {
        std::vector<std::vector<StatRow>> lists;
        if (stats && stats->defined()) lists.push_back(stats->rows());
        if (gstats_) lists.push_back(gstats_->rows());
        if (covis_) lists.push_back(covis_->rows());
        return lists;
    }
    // fit to capacity: every array created zero-filled, or zero-extended, to capacity() rows; a lazy array that does not exist only when it is `wanted`
    void fit_rows(const std::vector<StatRow>& rows, std::initializer_list<const torch::Tensor*> wanted = {})
    {
        const int64_t cap = capacity();
        for (const StatRow& r : rows) {
            torch::Tensor& t = *r.array;
            if (t.defined() ? t.size(0) >= cap : (r.lazy && std::find(wanted.begin(), wanted.end(), r.array) == wanted.end())) continue;
            torch::Tensor n = torch::zeros(r.cols ? std::vector<int64_t>{cap, r.cols} : std::vector<int64_t>{cap}, prm_[0].options().requires_grad(false).dtype(r.type));
            if (t.defined()) n.narrow(0, 0, t.size(0)).copy_(t);
            t = n;
        }
    }
    // gather (prune): fresh zero arrays of capacity(), rows [0, count) <- the old rows kept[0 .. count) in ONE gslic_gather_rows; P = the rows before
    void gather_rows(const std::vector<StatRow>& rows, const torch::Tensor& kept, int64_t P, int32_t count)
    {
        std::vector<torch::Tensor> old;
        std::vector<gslic_row_array> list;
        for (const StatRow& r : rows) TORCH_CHECK(!r.array->defined() || r.array->size(0) >= P, "FusedStep::prune: the statistics hold fewer rows than the map");
        for (const StatRow& r : rows) {
            if (!r.array->defined()) continue;
            old.push_back(*r.array);   // (alive until the launch is issued)
            std::vector<int64_t> shape = old.back().sizes().vec();
            shape[0] = capacity();
            *r.array = torch::zeros(shape, old.back().options());
            list.push_back({old.back().data_ptr(), r.array->data_ptr(), r.width});
        }
        if (count > 0 && !list.empty())
            check(gslic_gather_rows(list.data(), (int32_t)list.size(), reinterpret_cast<const uint32_t*>(kept.data_ptr<int32_t>()), count, current_stream()),
                  "gslic_gather_rows (statistics)");
    }
    // appended / zero rows (extend, densify): rows [P, P + k) and, when given, the rows `also` (densify's split parents) start from zero
    void zero_rows(const std::vector<StatRow>& rows, int64_t P, int64_t k, const torch::Tensor& also = torch::Tensor())
    {
        fit_rows(rows);
        for (const StatRow& r : rows) {
            if (!r.array->defined()) continue;
            r.array->narrow(0, P, k).zero_();
            if (also.defined()) r.array->index_fill_(0, also, 0);
        }
    }
    // append to a permute list (resort): the arrays, in place
    void permute_rows(const std::vector<StatRow>& rows, std::vector<gslic_row_array>& list)
    {
        fit_rows(rows);
        for (const StatRow& r : rows)
            if (r.array->defined()) list.push_back({r.array->data_ptr(), r.array->data_ptr(), r.width});
    }
    // capacity storage: created by the first extend(); until then the tensors handed to the constructor are used in place
    void reserve(int64_t newP)
    {
        const int64_t P = prm_[0].size(0);
        if (buf_[0].defined() && newP <= buf_[0].size(0)) return;
        const int64_t cap = std::max<int64_t>(2 * capacity(), newP);
        for (int g = 0; g < 6; g++) {
            std::vector<int64_t> shp = prm_[g].sizes().vec();
            shp[0] = cap;
            torch::Tensor nb = torch::empty(shp, prm_[g].options().requires_grad(false)), nm = torch::zeros(shp, m_[g].options()), nv = torch::zeros(shp, v_[g].options());
            nb.narrow(0, 0, P).copy_(prm_[g].detach());
            nm.narrow(0, 0, P).copy_(m_[g]);
            nv.narrow(0, 0, P).copy_(v_[g]);
            buf_[g] = nb; mbuf_[g] = nm; vbuf_[g] = nv;
        }
        bind(P);
    }
    void bind(int64_t P)
    {
        for (int g = 0; g < 6; g++) { prm_[g] = buf_[g].narrow(0, 0, P); m_[g] = mbuf_[g].narrow(0, 0, P); v_[g] = vbuf_[g].narrow(0, 0, P); }
    }
    gslic_adam_fused adam_descriptor() const
    {
        gslic_adam_fused ad{};
        for (int i = 0; i < 6; i++) {
            const bool on = prm_[i].numel() != 0;   // features_rest is [P,0,3] at SH degree 0: an empty group is a no-op, as in the reference
            ad.param[i] = on ? prm_[i].data_ptr<float>() : nullptr;
            ad.exp_avg[i] = on ? m_[i].data_ptr<float>() : nullptr;
            ad.exp_avg_sq[i] = on ? v_[i].data_ptr<float>() : nullptr;
            ad.lr[i] = lrs_[i];
        }
        ad.b1 = b1_; ad.b2 = b2_; ad.eps = eps_;
        return ad;
    }
    static const float* f(const torch::Tensor& t) { return t.numel() ? t.data_ptr<float>() : nullptr; }
    static const uint8_t* u8(const torch::Tensor& t) { return t.defined() ? t.data_ptr<uint8_t>() : nullptr; }
    // a per-row mask argument of prune() / densify() as a contiguous uint8 tensor [P] on the parameters' device (undefined stays undefined)
    torch::Tensor row_mask(const torch::Tensor& t, const char* who, const char* what, int64_t P) const
    {
        if (!t.defined()) return torch::Tensor();
        TORCH_CHECK(t.dim() == 1 && t.size(0) == P && (t.scalar_type() == torch::kBool || t.scalar_type() == torch::kByte), who, what,
                    " must be a bool / uint8 tensor of ", P, " rows");
        return t.to(prm_[0].device()).to(torch::kByte).contiguous();
    }
    static char* cptr(torch::Tensor& t) { return t.numel() ? reinterpret_cast<char*>(t.data_ptr()) : nullptr; }
    static void check(int rc, const char* what) { TORCH_CHECK(rc == GSLIC_OK, what, " failed (", rc, "): ", gslic_last_error()); }
    // the role of resizeFunctional (rasterize_points.cu:40-48) for buffers that persist across steps: grow only, with headroom, so a
    // steady-state step allocates nothing
    static char* grow_cb(void* ctx, size_t n)
    {
        torch::Tensor& t = *static_cast<torch::Tensor*>(ctx);
        if ((size_t)t.numel() < n) t = torch::empty({(int64_t)(n + n / 8 + 256)}, t.options());
        return reinterpret_cast<char*>(t.data_ptr());
    }

    std::array<torch::Tensor, 6> prm_, m_, v_;
    std::array<torch::Tensor, 6> buf_, mbuf_, vbuf_;
    std::array<float, 6> lrs_;
    int deg_;
    float lambda_dssim_, lambda_erank_, b1_, b2_, eps_;
    torch::Tensor scratch_[4];   // geom, binning, img, sample — order of the C-ABI's allocator arguments
    torch::Tensor bg_, image_, final_T_, radii_, dm_[3], dL_dimage_, partials_, tie_;
    torch::Tensor depth_, dL_ddepth_, depth_partials_, xyz_grad_;   // depth steps
    torch::Tensor wpartials_, wterms_;                              // weighted loss: scratch and {L1_w, SSIM_w, S}
    torch::Tensor dwpartials_, dwterms_;                            // weighted / Huber depth loss: scratch and {L_d, S}
    std::optional<double> resort_fraction_;                         // the re-sort rule (off by default)
    int64_t sorted_P_ = 0, n_resorts_ = 0;                          // rows [0, sorted_P_) are in Morton order; resort() calls so far
    torch::Tensor last_perm_;                                       // the last resort()'s permutation
    GradientStats* gstats_ = nullptr;                               // set_gradient_stats: accumulated by step(), carried by the row changes
    Covisibility* covis_ = nullptr;                                 // set_covisibility: recorded by record_covisibility(), carried by the row changes
    Exposure* exposure_ = nullptr;                                  // set_exposure: applied and updated by step(), applied by pose_gradient()
    int exposure_view_ = 0;
    torch::Tensor ex_image_, ex_dL_, ex_partials_;                  // exposure: the compensated image, the loss's gradient w.r.t. it, the partial sums
};

}  // namespace gslic
