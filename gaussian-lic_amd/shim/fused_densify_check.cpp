// fused_densify_check.cpp — densification from C++ (gslic::FusedStep::accumulate_contribution with an error image and gslic::FusedStep::densify
// of shim/include/gslic_fused.h) between fused training steps, so a test can hold the C++ host against the Python host
// (trainer.ContributionStats / trainer.GaussianModel.densify).  Same file protocol as fused_prune_check.cpp:
//   fused_densify_check <dir> <P> <W> <H> <deg> <iters> <w_min> <error_above_fixed> <split_scale> <seed>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt,err}.f32 (err: the [H,W] error image), scalars.f32 (tanfovx, tanfovy,
// 4 lims) and, when present, tie_rank.f32 (the rows' original indices of a map stored in a permuted order); runs <iters> steps, accumulates the
// view with the error image, grows the rows whose 32.32 fixed-point error sum exceeds <error_above_fixed> (an integer), splitting above
// <split_scale> (activated domain; <= 0: every row clones), runs <iters> more steps and writes the raw bytes of all 19 arrays —
// out_{xyz,dc,rest,opacity,scaling,rotation}.f32, out_m_<name>.f32, out_v_<name>.f32, out_tie.i32 (when there is a tie rank) — and of
// out_err_sum.i64 and out_parents.i64, printing "densify added <k> splits <s> size <P'>".  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 11, "usage: fused_densify_check <dir> <P> <W> <H> <deg> <iters> <w_min> <error_above_fixed> <split_scale> <seed>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float w_min = std::stof(argv[7]);
    const int64_t error_above = std::stoll(argv[8]);
    const double split_scale = std::stod(argv[9]);
    const uint32_t seed = (uint32_t)std::stoul(argv[10]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera& cam = in.cam;
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), err = load(d + "/err.f32", {H, W});

    gslic::FusedStep fs = make_step(in, deg);
    probe_tie_rank(fs, d, P);
    for (int it = 0; it < iters; it++) fs.step(cam, gt);
    gslic::ContributionStats st;
    fs.accumulate_contribution(cam, st, w_min, err);
    // the Python host's grow_mask(error_above): an integer comparison on the stored sums
    const torch::Tensor grow = st.err_sum.narrow(0, 0, P) > error_above;
    int64_t n_split = 0;
    const torch::Tensor parents = fs.densify(grow, split_scale > 0.0 ? std::optional<double>(split_scale) : std::nullopt, torch::Tensor(), seed, &st, &n_split);
    std::cout << "densify added " << parents.size(0) << " splits " << n_split << " size " << fs.size() << std::endl;
    for (int it = 0; it < iters; it++) {
        torch::Tensor terms = fs.step(cam, gt);
        std::cout << "iter " << (iters + it) << " loss " << fs.loss_value(terms) << std::endl;
    }
    dump_rows(fs, d);
    save_raw(d + "/out_err_sum.i64", st.err_sum.narrow(0, 0, fs.size()));
    save_raw(d + "/out_parents.i64", parents);
    return 0;
}
