// fused_gradient_stats_check.cpp — the gradient densification statistics from C++ (gslic::GradientStats and gslic::FusedStep::set_gradient_stats of
// shim/include/gslic_fused.h), accumulated by the fused steps and carried through densify, prune and resort, so a test can hold the C++ host
// against the Python host (trainer.GradientStats / trainer.GaussianModel).  Same file protocol as fused_densify_check.cpp:
//   fused_gradient_stats_check <dir> <P> <W> <H> <deg> <iters> <grad_above> <max_screen_radius> <split_scale> <seed>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims) and, when present,
// tie_rank.f32 (the rows' original indices of a map stored in a permuted order); with the statistics set it runs <iters> steps, densifies the rows
// of grow_mask(<grad_above>) (splitting above <split_scale>, activated domain), runs <iters> steps, prunes the rows of
// big_mask(<max_screen_radius>), runs <iters> steps, re-sorts the map and runs <iters> more; then writes the raw bytes of all 19 arrays —
// out_{xyz,dc,rest,opacity,scaling,rotation}.f32, out_m_<name>.f32, out_v_<name>.f32, out_tie.i32 — and of out_grad_sum.f32, out_n_seen.i32,
// out_max_radius.i32, printing "densify added <k> splits <s> pruned <n> size <P'>".  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 11, "usage: fused_gradient_stats_check <dir> <P> <W> <H> <deg> <iters> <grad_above> <max_screen_radius> <split_scale> <seed>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float grad_above = (float)std::stod(argv[7]);
    const int32_t max_screen_radius = (int32_t)std::stol(argv[8]);
    const double split_scale = std::stod(argv[9]);
    const uint32_t seed = (uint32_t)std::stoul(argv[10]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera& cam = in.cam;
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W});

    gslic::FusedStep fs = make_step(in, deg);
    probe_tie_rank(fs, d, P);
    gslic::GradientStats st;
    fs.set_gradient_stats(&st);
    for (int it = 0; it < iters; it++) fs.step(cam, gt);
    int64_t n_split = 0;
    const torch::Tensor parents = fs.densify(st.grow_mask(fs.size(), grad_above), split_scale > 0.0 ? std::optional<double>(split_scale) : std::nullopt,
                                             torch::Tensor(), seed, nullptr, &n_split);
    for (int it = 0; it < iters; it++) fs.step(cam, gt);
    const int64_t before = fs.size();
    fs.prune(std::nullopt, std::nullopt, st.big_mask(fs.size(), max_screen_radius));
    std::cout << "densify added " << parents.size(0) << " splits " << n_split << " pruned " << (before - fs.size()) << " size " << fs.size() << std::endl;
    for (int it = 0; it < iters; it++) fs.step(cam, gt);
    fs.resort();
    for (int it = 0; it < iters; it++) {
        torch::Tensor terms = fs.step(cam, gt);
        std::cout << "iter " << (3 * iters + it) << " loss " << fs.loss_value(terms) << std::endl;
    }
    dump_rows(fs, d);
    save_raw(d + "/out_grad_sum.f32", st.grad_sum.narrow(0, 0, fs.size()));
    save_raw(d + "/out_n_seen.i32", st.n_seen.narrow(0, 0, fs.size()));
    save_raw(d + "/out_max_radius.i32", st.max_radius.narrow(0, 0, fs.size()));
    return 0;
}
