// fused_depth_pose_check.cpp — the camera-pose gradient under LiDAR depth supervision driven from C++ (gslic::FusedStep::pose_gradient(cam, gt,
// gt_depth, lambda_depth) of shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host (trainer.pose_gradient with
// gt_depth / lambda_depth).  Same input files as fused_depth_check.cpp:
//   fused_depth_pose_check <dir> <P> <W> <H> <deg> <lambda_depth>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims) and gt_depth.f32 [H,W],
// prints "pose_gradient <d/drho x3> <d/dphi x3>" and "terms <mean L1> <mean SSIM> <L_d>"; the map is not touched.  LibTorch and libgslic_hip.so only.
#include "gslic_fused.h"

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

static torch::Tensor load(const std::string& path, std::vector<int64_t> shape)
{
    int64_t n = 1;
    for (auto s : shape) n *= s;
    std::vector<float> buf(n);
    std::ifstream f(path, std::ios::binary);
    TORCH_CHECK(f.good(), "cannot open ", path);
    f.read(reinterpret_cast<char*>(buf.data()), n * sizeof(float));
    return torch::from_blob(buf.data(), shape, torch::kFloat32).clone().to(torch::kCUDA);
}

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 7, "usage: fused_depth_pose_check <dir> <P> <W> <H> <deg> <lambda_depth>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]);
    const float lambda_depth = std::stof(argv[6]);
    const int64_t M = deg > 0 ? 15 : 0;
    torch::Tensor xyz = load(d + "/xyz.f32", {P, 3}), scaling = load(d + "/scaling.f32", {P, 3}), rotation = load(d + "/rotation.f32", {P, 4});
    torch::Tensor opacity = load(d + "/opacity.f32", {P, 1}), dc = load(d + "/dc.f32", {P, 1, 3});
    torch::Tensor rest = M > 0 ? load(d + "/rest.f32", {P, M, 3}) : torch::zeros({P, 0, 3}, torch::kCUDA);
    gslic::FusedCamera cam;
    cam.image_width = (int)W; cam.image_height = (int)H;
    cam.world_view_transform = load(d + "/view.f32", {4, 4}); cam.full_proj_transform = load(d + "/proj.f32", {4, 4}); cam.camera_center = load(d + "/campos.f32", {3});
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), gt_depth = load(d + "/gt_depth.f32", {H, W});
    torch::Tensor sc = load(d + "/scalars.f32", {6}).to(torch::kCPU);
    const float* s = sc.data_ptr<float>();
    cam.tanfovx = s[0]; cam.tanfovy = s[1]; cam.limx_neg = s[2]; cam.limx_pos = s[3]; cam.limy_neg = s[4]; cam.limy_pos = s[5];

    gslic::FusedStep fs({xyz, dc, rest, opacity, scaling, rotation}, {1.6e-4f, 2.5e-3f, (float)(2.5e-3 / 20.0), 5e-2f, 5e-3f, 1e-3f}, deg);
    torch::Tensor terms;
    const auto g = fs.pose_gradient(cam, gt, gt_depth, lambda_depth, &terms);
    std::cout.precision(9);
    std::cout << "pose_gradient " << g[0] << " " << g[1] << " " << g[2] << " " << g[3] << " " << g[4] << " " << g[5] << std::endl;
    torch::Tensor t = terms.to(torch::kCPU);
    std::cout << "terms " << t[0].item<float>() << " " << t[1].item<float>() << " " << t[2].item<float>() << std::endl;
    return 0;
}
