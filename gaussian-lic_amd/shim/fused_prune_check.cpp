// fused_prune_check.cpp — pruning the map from C++ (gslic::FusedStep::prune of shim/include/gslic_fused.h) between fused training steps, so a
// test can hold the C++ host against the Python host (trainer.GaussianModel.prune).  Same file protocol as fused_check.cpp:
//   fused_prune_check <dir> <P> <W> <H> <deg> <iters> <min_opacity> <max_scale>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims) and, when present,
// tie_rank.f32 (the rows' original indices of a map stored in a permuted order), runs <iters> steps, prunes with the two limits (activated
// domain; <= 0 disables one), runs <iters> more steps and writes <dir>/out_kept.f32 (the kept rows' old indices, as floats: P < 2^24),
// out_{xyz,scaling,rotation,opacity,dc,rest}.f32 and out_m_xyz.f32 / out_v_xyz.f32 (Adam moments of the positions), printing
// "prune removed <n> size <P'>".  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 9, "usage: fused_prune_check <dir> <P> <W> <H> <deg> <iters> <min_opacity> <max_scale>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const double min_opacity = std::stod(argv[7]), max_scale = std::stod(argv[8]);
    TORCH_CHECK(P < (1 << 24), "out_kept.f32 holds row indices as floats");
    const Inputs in = read_inputs(d, P, W, H, deg);
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W});

    gslic::FusedStep fs = make_step(in, deg);
    probe_tie_rank(fs, d, P);
    for (int it = 0; it < iters; it++) fs.step(in.cam, gt);
    const torch::Tensor kept = fs.prune(min_opacity > 0.0 ? std::optional<double>(min_opacity) : std::nullopt,
                                        max_scale > 0.0 ? std::optional<double>(max_scale) : std::nullopt);
    std::cout << "prune removed " << (P - kept.size(0)) << " size " << fs.size() << std::endl;
    for (int it = 0; it < iters; it++) {
        torch::Tensor terms = fs.step(in.cam, gt);
        std::cout << "iter " << (iters + it) << " loss " << fs.loss_value(terms) << " visible " << fs.visible().sum().item<int>() << std::endl;
    }
    save(d + "/out_kept.f32", kept);
    dump_params(fs, d);
    save(d + "/out_m_xyz.f32", fs.exp_avg(0)); save(d + "/out_v_xyz.f32", fs.exp_avg_sq(0));
    return 0;
}
