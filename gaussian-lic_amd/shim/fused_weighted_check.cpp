// fused_weighted_check.cpp — the fused training step under a per-pixel weight image driven from C++ (gslic::FusedStep::step / pose_gradient with
// `weight`, shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host (trainer.training_step_fused / pose_gradient
// with weight=...).  Same file protocol as fused_check.cpp:
//   fused_weighted_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims), weight.f32 [H,W] and, for
// lambda_depth != 0, gt_depth.f32 [H,W]; prints "pose <6 numbers>" (the pose gradient of the initial map), then runs <iters> steps printing
// "iter <i> loss <loss> visible <n>", and writes <dir>/out_{image,xyz,scaling,rotation,opacity,dc,rest}.f32, out_terms.f32 (the last step's terms)
// and out_weight_sum.f32; then the one-node autograd loss (loss_utils::l1_ssim_loss with the weight, loss_utils_fused.h) on the last image:
// out_onenode.f32 (the loss) and out_onenode_grad.f32 (d(2 loss)/dimage).  LibTorch and libgslic_hip.so only.
#include "gslic_fused.h"
#include "loss_utils_fused.h"

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
static void save(const std::string& path, const torch::Tensor& t)
{
    torch::Tensor c = t.detach().to(torch::kCPU).contiguous();
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(c.data_ptr<float>()), c.numel() * sizeof(float));
}

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 8, "usage: fused_weighted_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float lambda_depth = std::stof(argv[7]);
    const int64_t M = deg > 0 ? 15 : 0;
    torch::Tensor xyz = load(d + "/xyz.f32", {P, 3}), scaling = load(d + "/scaling.f32", {P, 3}), rotation = load(d + "/rotation.f32", {P, 4});
    torch::Tensor opacity = load(d + "/opacity.f32", {P, 1}), dc = load(d + "/dc.f32", {P, 1, 3});
    torch::Tensor rest = M > 0 ? load(d + "/rest.f32", {P, M, 3}) : torch::zeros({P, 0, 3}, torch::kCUDA);
    gslic::FusedCamera cam;
    cam.image_width = (int)W; cam.image_height = (int)H;
    cam.world_view_transform = load(d + "/view.f32", {4, 4}); cam.full_proj_transform = load(d + "/proj.f32", {4, 4}); cam.camera_center = load(d + "/campos.f32", {3});
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), weight = load(d + "/weight.f32", {H, W}), gt_depth;
    if (lambda_depth != 0.0f) gt_depth = load(d + "/gt_depth.f32", {H, W});
    torch::Tensor sc = load(d + "/scalars.f32", {6}).to(torch::kCPU);
    const float* s = sc.data_ptr<float>();
    cam.tanfovx = s[0]; cam.tanfovy = s[1]; cam.limx_neg = s[2]; cam.limx_pos = s[3]; cam.limy_neg = s[4]; cam.limy_pos = s[5];

    // trainingSetup (gaussian.cpp:399-418) with config/fastlivo.yaml learning rates
    gslic::FusedStep fs({xyz, dc, rest, opacity, scaling, rotation}, {1.6e-4f, 2.5e-3f, (float)(2.5e-3 / 20.0), 5e-2f, 5e-3f, 1e-3f}, deg);
    torch::Tensor terms;
    const std::array<double, 6> g = fs.pose_gradient(cam, gt, gt_depth, lambda_depth, nullptr, weight);
    std::cout.precision(17);
    std::cout << "pose";
    for (double v : g) std::cout << " " << v;
    std::cout << std::endl;
    for (int it = 0; it < iters; it++) {
        terms = fs.step(cam, gt, gt_depth, lambda_depth, weight);
        std::cout << "iter " << it << " loss " << fs.loss_value(terms, lambda_depth) << " visible " << fs.visible().sum().item<int>() << std::endl;
    }
    save(d + "/out_image.f32", fs.image());
    if (terms.defined()) save(d + "/out_terms.f32", terms);
    save(d + "/out_weight_sum.f32", fs.weight_sum());
    {
        torch::Tensor x = fs.image().detach().clone().requires_grad_(true);
        torch::Tensor one = loss_utils::l1_ssim_loss(x, gt, 0.2, weight);
        (2.0 * one).backward();
        save(d + "/out_onenode.f32", one.reshape({1}));
        save(d + "/out_onenode_grad.f32", x.grad());
    }
    save(d + "/out_xyz.f32", xyz); save(d + "/out_scaling.f32", scaling); save(d + "/out_rotation.f32", rotation);
    save(d + "/out_opacity.f32", opacity); save(d + "/out_dc.f32", dc);
    if (M > 0) save(d + "/out_rest.f32", rest);
    return 0;
}
