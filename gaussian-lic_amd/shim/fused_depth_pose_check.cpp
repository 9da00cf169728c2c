// fused_depth_pose_check.cpp — the camera-pose gradient under LiDAR depth supervision driven from C++ (gslic::FusedStep::pose_gradient(cam, gt,
// gt_depth, lambda_depth) of shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host (trainer.pose_gradient with
// gt_depth / lambda_depth).  Same input files as fused_depth_check.cpp:
//   fused_depth_pose_check <dir> <P> <W> <H> <deg> <lambda_depth>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims) and gt_depth.f32 [H,W],
// prints "pose_gradient <d/drho x3> <d/dphi x3>" and "terms <mean L1> <mean SSIM> <L_d>"; the map is not touched.  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 7, "usage: fused_depth_pose_check <dir> <P> <W> <H> <deg> <lambda_depth>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]);
    const float lambda_depth = std::stof(argv[6]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), gt_depth = load(d + "/gt_depth.f32", {H, W});

    gslic::FusedStep fs = make_step(in, deg);
    torch::Tensor terms;
    const auto g = fs.pose_gradient(in.cam, gt, gt_depth, lambda_depth, &terms);
    std::cout.precision(9);
    std::cout << "pose_gradient " << g[0] << " " << g[1] << " " << g[2] << " " << g[3] << " " << g[4] << " " << g[5] << std::endl;
    torch::Tensor t = terms.to(torch::kCPU);
    std::cout << "terms " << t[0].item<float>() << " " << t[1].item<float>() << " " << t[2].item<float>() << std::endl;
    return 0;
}
