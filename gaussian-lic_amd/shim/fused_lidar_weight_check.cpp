// fused_lidar_weight_check.cpp — the weighted LiDAR range image from C++ (gslic::LidarDepth::resolve with `weight` and `dist2`,
// shim/include/gslic_fused.h) feeding the weighted depth step, so a test can hold the C++ host against the Python host
// (trainer.LidarDepth.resolve(weight=, dist2=), training_step_fused(gt_depth=, depth_weight=, depth_huber=)).  Same file protocol as
// fused_lidar_depth_check.cpp:
//   fused_lidar_weight_check <dir> <P> <W> <H> <deg> <n> <footprint>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims), points.f32 [n,3] (world) and
// lidar.f32 = R_cw [9] row-major, t_cw [3], fx, fy, cx, cy, sigma_abs, sigma_rel, falloff, lambda_depth, depth_huber (21 floats).  The run: one
// sweep into a LidarDepth, resolved at <footprint> with index, count, weight and dist2; ONE step(cam, gt, depth, lambda_depth, {}, weight, huber).
// Writes out_lidar_depth.f32, out_lidar_weight.f32, out_lidar_index.i32, out_lidar_dist2.i32 [H,W], out_lidar_count.i32 [1] and the raw bytes of
// the 18 parameter and moment arrays (fused_check_io.h: dump_rows), printing "lidar measured <count> base <index_base>".  LibTorch and
// libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 8, "usage: fused_lidar_weight_check <dir> <P> <W> <H> <deg> <n> <footprint>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]);
    const int64_t n = std::stoll(argv[6]);
    const int footprint = std::stoi(argv[7]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), points = load(d + "/points.f32", {n, 3});
    const torch::Tensor lidar = load(d + "/lidar.f32", {21}), lh = lidar.to(torch::kCPU);
    const float* s = lh.data_ptr<float>();
    const float sigma_abs = s[16], sigma_rel = s[17], falloff = s[18], lambda_depth = s[19], depth_huber = s[20];

    gslic::LidarDepth ld((int)W, (int)H);
    const int64_t base = ld.add(points, lidar.slice(0, 0, 9), lidar.slice(0, 9, 12), s[12], s[13], s[14], s[15]);
    const gslic::LidarImages im = ld.resolve(footprint, std::nullopt, true, true, std::array<float, 3>{sigma_abs, sigma_rel, falloff}, true);
    save_raw(d + "/out_lidar_depth.f32", im.depth); save_raw(d + "/out_lidar_weight.f32", im.weight);
    save_raw(d + "/out_lidar_index.i32", im.index); save_raw(d + "/out_lidar_dist2.i32", im.dist2);
    save_raw(d + "/out_lidar_count.i32", im.n_measured.reshape({1}));
    std::cout << "lidar measured " << im.n_measured.item<int>() << " base " << base << std::endl;

    gslic::FusedStep fs = make_step(in, deg);
    const torch::Tensor terms = fs.step(in.cam, gt, im.depth, lambda_depth, {}, im.weight, depth_huber);
    std::cout << "loss " << fs.loss_value(terms, lambda_depth) << std::endl;
    dump_rows(fs, d);
    return 0;
}
