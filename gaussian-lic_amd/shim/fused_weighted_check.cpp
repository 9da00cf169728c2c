// fused_weighted_check.cpp — the fused training step under a per-pixel weight image driven from C++ (gslic::FusedStep::step / pose_gradient with
// `weight`, shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host (trainer.training_step_fused / pose_gradient
// with weight=...).  Same file protocol as fused_check.cpp:
//   fused_weighted_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims), weight.f32 [H,W] and, for
// lambda_depth != 0, gt_depth.f32 [H,W]; prints "pose <6 numbers>" (the pose gradient of the initial map), then runs <iters> steps printing
// "iter <i> loss <loss> visible <n>", and writes <dir>/out_{image,xyz,scaling,rotation,opacity,dc,rest}.f32, out_terms.f32 (the last step's terms)
// and out_weight_sum.f32; then the one-node autograd loss (loss_utils::l1_ssim_loss with the weight, loss_utils_fused.h) on the last image:
// out_onenode.f32 (the loss) and out_onenode_grad.f32 (d(2 loss)/dimage).  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"
#include "loss_utils_fused.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 8, "usage: fused_weighted_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float lambda_depth = std::stof(argv[7]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera& cam = in.cam;
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), weight = load(d + "/weight.f32", {H, W}), gt_depth;
    if (lambda_depth != 0.0f) gt_depth = load(d + "/gt_depth.f32", {H, W});

    gslic::FusedStep fs = make_step(in, deg);
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
    dump_params(fs, d);
    return 0;
}
