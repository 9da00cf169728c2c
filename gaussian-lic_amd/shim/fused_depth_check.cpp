// fused_depth_check.cpp — the fused training step WITH LiDAR depth supervision driven from C++ (gslic::FusedStep::step(cam, gt, gt_depth,
// lambda_depth) of shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host (trainer.training_step_fused with
// gt_depth / lambda_depth).  Same file protocol as fused_check.cpp:
//   fused_depth_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims) and gt_depth.f32 [H,W],
// writes <dir>/out_{image,depth,xyz,scaling,rotation,opacity,dc,rest}.f32 and out_terms.f32 (the last step's three terms) after <iters> steps,
// printing "iter <i> loss <loss> visible <n>" per step.  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 8, "usage: fused_depth_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float lambda_depth = std::stof(argv[7]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), gt_depth = load(d + "/gt_depth.f32", {H, W});

    gslic::FusedStep fs = make_step(in, deg);
    torch::Tensor terms;
    for (int it = 0; it < iters; it++) {
        terms = fs.step(in.cam, gt, gt_depth, lambda_depth);
        std::cout << "iter " << it << " loss " << fs.loss_value(terms, lambda_depth) << " visible " << fs.visible().sum().item<int>() << std::endl;
    }
    save(d + "/out_image.f32", fs.image());
    if (fs.depth().defined()) save(d + "/out_depth.f32", fs.depth());
    if (terms.defined()) save(d + "/out_terms.f32", terms);
    dump_params(fs, d);
    return 0;
}
