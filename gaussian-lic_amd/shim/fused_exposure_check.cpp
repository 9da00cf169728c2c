// fused_exposure_check.cpp — the fused training step under a trainable per-view exposure driven from C++ (gslic::Exposure and
// gslic::FusedStep::set_exposure, shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host
// (trainer.training_step_fused(exposure=, view=)).  Same file protocol as fused_check.cpp:
//   fused_exposure_check <dir> <P> <W> <H> <deg> <iters> <exposure_lr>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32, two cameras {view,proj,campos}.f32 / {view,proj,campos}2.f32 with scalars.f32 (tanfovx,
// tanfovy, 4 lims: both cameras), their targets gt.f32 / gt2.f32 and E.f32 [2,3,4], the exposures the run starts from; prints "pose <6 numbers>"
// (the pose gradient of the initial map under view 0's exposure, which updates nothing), then runs <iters> steps, step i on camera and exposure
// row i % 2, printing "iter <i> loss <loss> visible <n>", and writes the 19 row arrays (dump_rows), out_E.f32, out_E_m.f32, out_E_v.f32 [2,3,4],
// out_E_steps.i32 [2], out_E_grad.f32 [3,4] (the last step's dL/dE) and out_terms.f32 [iters,2].  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 8, "usage: fused_exposure_check <dir> <P> <W> <H> <deg> <iters> <exposure_lr>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float exposure_lr = std::stof(argv[7]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera cams[2] = {in.cam, read_camera(d, W, H, in.scalars.data(), "2")};
    const torch::Tensor gts[2] = {load(d + "/gt.f32", {3, H, W}), load(d + "/gt2.f32", {3, H, W})};

    gslic::FusedStep fs = make_step(in, deg);
    gslic::Exposure ex(2, torch::kCUDA, exposure_lr);
    ex.params.copy_(load(d + "/E.f32", {2, 3, 4}));
    fs.set_exposure(&ex, 0);
    const std::array<double, 6> g = fs.pose_gradient(cams[0], gts[0]);
    std::cout.precision(17);
    std::cout << "pose";
    for (double v : g) std::cout << " " << v;
    std::cout << std::endl;
    std::vector<torch::Tensor> all_terms;
    for (int it = 0; it < iters; it++) {
        fs.set_exposure(&ex, it % 2);
        const torch::Tensor terms = fs.step(cams[it % 2], gts[it % 2]);
        all_terms.push_back(terms);
        std::cout << "iter " << it << " loss " << fs.loss_value(terms) << " visible " << fs.visible().sum().item<int>() << std::endl;
    }
    dump_rows(fs, d);
    save_raw(d + "/out_E.f32", ex.params);
    save_raw(d + "/out_E_m.f32", ex.m);
    save_raw(d + "/out_E_v.f32", ex.v);
    save_raw(d + "/out_E_steps.i32", ex.steps);
    save_raw(d + "/out_E_grad.f32", ex.grad);
    if (!all_terms.empty()) save_raw(d + "/out_terms.f32", torch::stack(all_terms));
    return 0;
}
