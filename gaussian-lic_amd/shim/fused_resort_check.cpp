// fused_resort_check.cpp — keeping the map in Morton order from C++ (gslic::FusedStep::resort / set_resort_fraction of shim/include/gslic_fused.h)
// between fused training steps, so a test can hold the C++ host against the Python host (trainer.GaussianModel.to_morton_order / resort / the
// resort_fraction rule).  Same file protocol as fused_densify_check.cpp:
//   fused_resort_check <dir> <P> <W> <H> <deg> <iters> <n_points> <fraction> <min_opacity> <max_scale> <w_min>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt,err}.f32 (err: the [H,W] error image), scalars.f32 (tanfovx, tanfovy,
// 4 lims, fx, fy, cx, cy) and one LiDAR frame {pts,col}.f32 [n_points,3], rsp.f32 [n_points], Rcw.f32 [3,3], tcw.f32 [3].  The map starts in
// INSERTION order.  The run: <iters> steps; one view accumulated with the error image; resort() (the first sort: the tie rank is created);
// set_resort_fraction(<fraction>); <iters> steps; extend() with the frame (its tail passes the fraction: the rule re-sorts); <iters> steps;
// prune() with the two limits (activated domain); resort(); <iters> steps.  Writes the raw bytes of all 19 arrays —
// out_{xyz,dc,rest,opacity,scaling,rotation}.f32, out_m_<name>.f32, out_v_<name>.f32, out_tie.i32 — of out_err_sum.i64 and of the three
// permutations out_perm{0,1,2}.i64, printing "resort extended <k> resorts <n> pruned <r> size <P'>".  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 12, "usage: fused_resort_check <dir> <P> <W> <H> <deg> <iters> <n_points> <fraction> <min_opacity> <max_scale> <w_min>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const int64_t n_pts = std::stoll(argv[7]);
    const double fraction = std::stod(argv[8]), min_opacity = std::stod(argv[9]), max_scale = std::stod(argv[10]);
    const float w_min = std::stof(argv[11]);
    const Inputs in = read_inputs(d, P, W, H, deg, 10);
    const gslic::FusedCamera& cam = in.cam;
    const float* s = in.scalars.data();
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), err = load(d + "/err.f32", {H, W});
    torch::Tensor pts = load(d + "/pts.f32", {n_pts, 3}), col = load(d + "/col.f32", {n_pts, 3}), rsp = load(d + "/rsp.f32", {n_pts});
    torch::Tensor Rcw = load(d + "/Rcw.f32", {3, 3}), tcw = load(d + "/tcw.f32", {3});

    gslic::FusedStep fs = make_step(in, deg);
    auto steps = [&]() {
        for (int it = 0; it < iters; it++) {
            torch::Tensor terms = fs.step(cam, gt);
            std::cout << "loss " << fs.loss_value(terms) << std::endl;
        }
    };
    steps();
    gslic::ContributionStats st;
    fs.accumulate_contribution(cam, st, w_min, err);
    const torch::Tensor perm0 = fs.resort(&st);              // the first sort, from insertion order
    TORCH_CHECK(fs.tie_rank().defined() && fs.sorted_rows() == P && fs.resorts() == 1);
    fs.set_resort_fraction(fraction);
    steps();
    const int64_t k = fs.extend(cam, pts, col, rsp, Rcw, tcw, s[6], s[7], s[8], s[9], 1.0f, &st);   // the appended tail passes the fraction: re-sorted
    const int64_t resorts = fs.resorts();
    const torch::Tensor perm1 = fs.last_resort().clone();
    steps();
    const int64_t before = fs.size();
    fs.prune(min_opacity > 0.0 ? std::optional<double>(min_opacity) : std::nullopt, max_scale > 0.0 ? std::optional<double>(max_scale) : std::nullopt,
             torch::Tensor(), torch::Tensor(), true, &st);
    const int64_t removed = before - fs.size();
    const torch::Tensor perm2 = fs.resort(&st);
    steps();
    std::cout << "resort extended " << k << " resorts " << resorts << " pruned " << removed << " size " << fs.size() << std::endl;
    dump_rows(fs, d);
    save_raw(d + "/out_err_sum.i64", st.err_sum.narrow(0, 0, fs.size()));
    save_raw(d + "/out_perm0.i64", perm0); save_raw(d + "/out_perm1.i64", perm1); save_raw(d + "/out_perm2.i64", perm2);
    return 0;
}
