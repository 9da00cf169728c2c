// fused_covis_check.cpp — covisibility sets from C++ (gslic::Covisibility and gslic::FusedStep::set_covisibility / record_covisibility of
// shim/include/gslic_fused.h), recorded behind fused steps and carried through densify, prune and resort, so a test can hold the C++ host against
// the Python host (trainer.Covisibility / trainer.GaussianModel).  The file protocol of fused_gradient_stats_check.cpp, with the frame count:
//   fused_covis_check <dir> <P> <W> <H> <deg> <iters> <grad_above> <max_screen_radius> <split_scale> <seed> <n_frames>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32, two cameras {view,proj,campos}{,2}.f32 with scalars.f32, gt.f32 and, when present,
// tie_rank.f32.  Step i (counted over the whole run) renders camera i % 2 and is recorded as frame (5 * i) % n_frames.  With gradient statistics
// and the covisibility set attached it runs <iters> steps, densifies the rows of grow_mask(<grad_above>), runs <iters> steps, prunes the rows of
// big_mask(<max_screen_radius>), runs <iters> steps, clears frame 0, re-sorts the map and runs <iters> more; then writes the 19 row arrays
// (dump_rows), out_covis_bits.i32 [P', Wd], out_covis_frame.i64 (frame_counts of the last recorded frame), out_covis_seen.i32, out_covis_red.i64
// (redundant(1)), out_covis_fewer.u8 (seen_by_fewer_than(2)), out_covis_overlap.f32 and, for n_frames <= 128, out_covis_pair.i64; prints
// "densify added <k> splits <s> pruned <n> size <P'>".  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 12, "usage: fused_covis_check <dir> <P> <W> <H> <deg> <iters> <grad_above> <max_screen_radius> <split_scale> <seed> <n_frames>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float grad_above = (float)std::stod(argv[7]);
    const int32_t max_screen_radius = (int32_t)std::stol(argv[8]);
    const double split_scale = std::stod(argv[9]);
    const uint32_t seed = (uint32_t)std::stoul(argv[10]);
    const int32_t n_frames = (int32_t)std::stol(argv[11]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera cams[2] = {in.cam, read_camera(d, W, H, in.scalars.data(), "2")};
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W});

    gslic::FusedStep fs = make_step(in, deg);
    probe_tie_rank(fs, d, P);
    gslic::GradientStats st;
    gslic::Covisibility cv(n_frames);
    fs.set_gradient_stats(&st);
    fs.set_covisibility(&cv);
    int step = 0, last = 0;
    auto steps = [&]() {
        for (int it = 0; it < iters; it++, step++) {
            fs.step(cams[step % 2], gt);
            last = (5 * step) % n_frames;
            fs.record_covisibility(last);
        }
    };
    steps();
    int64_t n_split = 0;
    const torch::Tensor parents = fs.densify(st.grow_mask(fs.size(), grad_above), split_scale > 0.0 ? std::optional<double>(split_scale) : std::nullopt,
                                             torch::Tensor(), seed, nullptr, &n_split);
    steps();
    const int64_t before = fs.size();
    fs.prune(std::nullopt, std::nullopt, st.big_mask(fs.size(), max_screen_radius));
    std::cout << "densify added " << parents.size(0) << " splits " << n_split << " pruned " << (before - fs.size()) << " size " << fs.size() << std::endl;
    steps();
    cv.clear(fs.size(), 0);
    fs.resort();
    steps();
    const int64_t Pn = fs.size();
    dump_rows(fs, d);
    save_raw(d + "/out_covis_bits.i32", cv.bits.narrow(0, 0, Pn));
    save_raw(d + "/out_covis_frame.i64", cv.frame_counts(Pn, last));
    save_raw(d + "/out_covis_seen.i32", cv.seen_count(Pn));
    save_raw(d + "/out_covis_red.i64", cv.redundant(Pn, 1));
    save_raw(d + "/out_covis_fewer.u8", cv.seen_by_fewer_than(Pn, 2).to(torch::kByte));
    save_raw(d + "/out_covis_overlap.f32", cv.overlap(Pn, last));
    if (n_frames <= GSLIC_COVIS_MAX_PAIR_FRAMES) save_raw(d + "/out_covis_pair.i64", cv.pair_counts(Pn));
    return 0;
}
