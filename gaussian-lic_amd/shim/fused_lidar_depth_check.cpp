// fused_lidar_depth_check.cpp — the LiDAR range image from C++ (gslic::LidarDepth of shim/include/gslic_fused.h) and its two consumers, so a test
// can hold the C++ host against the Python host (trainer.LidarDepth, training_step_fused(gt_depth=...), ContributionStats.accumulate(free_space=...)).
// Same file protocol as fused_depth_check.cpp:
//   fused_lidar_depth_check <dir> <P> <W> <H> <deg> <n> <footprint>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims), points.f32 [n,3] (world) and
// lidar.f32 = R_cw [9] row-major, t_cw [3], fx, fy, cx, cy, margin_abs, margin_rel, lambda_depth, w_min (20 floats).  The run: one sweep into a
// LidarDepth, resolved at <footprint> with the margins, index and count; ONE step(cam, gt, depth, lambda_depth); ONE accumulate_free_space(cam, near).
// Writes out_lidar_depth.f32, out_lidar_near.f32, out_lidar_index.i32 [H,W], out_lidar_count.i32 [1], the raw bytes of the 18 parameter and moment
// arrays (fused_check_io.h: dump_rows) and the five accumulators out_{max_w,n_pix}.i32, out_{sum_w,free_sum,meas_sum}.i64, printing
// "lidar measured <count> base <index_base>".  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 8, "usage: fused_lidar_depth_check <dir> <P> <W> <H> <deg> <n> <footprint>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]);
    const int64_t n = std::stoll(argv[6]);
    const int footprint = std::stoi(argv[7]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), points = load(d + "/points.f32", {n, 3});
    const torch::Tensor lidar = load(d + "/lidar.f32", {20}), lh = lidar.to(torch::kCPU);
    const float* s = lh.data_ptr<float>();
    const float margin_abs = s[16], margin_rel = s[17], lambda_depth = s[18], w_min = s[19];

    gslic::LidarDepth ld((int)W, (int)H);
    const int64_t base = ld.add(points, lidar.slice(0, 0, 9), lidar.slice(0, 9, 12), s[12], s[13], s[14], s[15]);
    const gslic::LidarImages im = ld.resolve(footprint, std::array<float, 2>{margin_abs, margin_rel}, true, true);
    save_raw(d + "/out_lidar_depth.f32", im.depth); save_raw(d + "/out_lidar_near.f32", im.near_bound);
    save_raw(d + "/out_lidar_index.i32", im.index); save_raw(d + "/out_lidar_count.i32", im.n_measured.reshape({1}));
    std::cout << "lidar measured " << im.n_measured.item<int>() << " base " << base << std::endl;

    gslic::FusedStep fs = make_step(in, deg);
    const torch::Tensor terms = fs.step(in.cam, gt, im.depth, lambda_depth);
    std::cout << "loss " << fs.loss_value(terms, lambda_depth) << std::endl;
    gslic::ContributionStats st;
    fs.accumulate_free_space(in.cam, st, w_min, im.near_bound);
    dump_rows(fs, d);
    save_raw(d + "/out_max_w.i32", st.max_w.narrow(0, 0, P)); save_raw(d + "/out_n_pix.i32", st.n_pix.narrow(0, 0, P));
    save_raw(d + "/out_sum_w.i64", st.sum_w.narrow(0, 0, P)); save_raw(d + "/out_free_sum.i64", st.free_sum.narrow(0, 0, P));
    save_raw(d + "/out_meas_sum.i64", st.meas_sum.narrow(0, 0, P));
    return 0;
}
