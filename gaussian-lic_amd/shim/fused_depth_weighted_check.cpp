// fused_depth_weighted_check.cpp — the fused training step under a per-pixel depth weight image and a Huber threshold driven from C++
// (gslic::FusedStep::step / pose_gradient with `depth_weight` / `depth_huber`, shim/include/gslic_fused.h), so a test can hold the C++ host
// against the Python host (trainer.training_step_fused / pose_gradient with depth_weight= / depth_huber=).  Same file protocol as fused_check.cpp:
//   fused_depth_weighted_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth> <depth_huber> <use_weight>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims), gt_depth.f32 [H,W] and, for
// use_weight != 0, depth_weight.f32 [H,W]; prints "pose <6 numbers>" (the pose gradient of the initial map), then runs <iters> steps printing
// "iter <i> loss <loss> visible <n>", and writes the 19 row arrays (dump_rows), out_image.f32, out_terms.f32 (the last step's terms) and
// out_depth_weight_sum.f32.  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 10, "usage: fused_depth_weighted_check <dir> <P> <W> <H> <deg> <iters> <lambda_depth> <depth_huber> <use_weight>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float lambda_depth = std::stof(argv[7]), depth_huber = std::stof(argv[8]);
    const bool use_weight = std::stoi(argv[9]) != 0;
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera& cam = in.cam;
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), gt_depth = load(d + "/gt_depth.f32", {H, W}), depth_weight;
    if (use_weight) depth_weight = load(d + "/depth_weight.f32", {H, W});

    gslic::FusedStep fs = make_step(in, deg);
    torch::Tensor terms;
    const std::array<double, 6> g = fs.pose_gradient(cam, gt, gt_depth, lambda_depth, nullptr, torch::Tensor(), depth_weight, depth_huber);
    std::cout.precision(17);
    std::cout << "pose";
    for (double v : g) std::cout << " " << v;
    std::cout << std::endl;
    for (int it = 0; it < iters; it++) {
        terms = fs.step(cam, gt, gt_depth, lambda_depth, torch::Tensor(), depth_weight, depth_huber);
        std::cout << "iter " << it << " loss " << fs.loss_value(terms, lambda_depth) << " visible " << fs.visible().sum().item<int>() << std::endl;
    }
    save(d + "/out_image.f32", fs.image());
    if (terms.defined()) save(d + "/out_terms.f32", terms);
    if (fs.depth_weight_sum().defined()) save(d + "/out_depth_weight_sum.f32", fs.depth_weight_sum());
    dump_rows(fs, d);
    return 0;
}
