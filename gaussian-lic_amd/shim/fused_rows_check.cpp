// fused_rows_check.cpp — BOTH statistics objects carried through all four row changes from C++ (gslic::ContributionStats with its error and
// free-space arrays and gslic::GradientStats, through gslic::FusedStep::densify / extend / prune / resort of shim/include/gslic_fused.h) between
// fused training steps, so a test can hold the C++ host against the Python host (trainer.ContributionStats / GradientStats attached to one
// trainer.GaussianModel).  Same file protocol and LiDAR frame inputs as fused_resort_check.cpp:
//   fused_rows_check <dir> <P> <W> <H> <deg> <iters> <n_points> <fraction> <w_min> <grad_above> <split_scale> <seed> <max_screen_radius>
// reads  the inputs of fused_check_io.h with scalars.f32 = (tanfovx, tanfovy, 4 lims, fx, fy, cx, cy), {gt,err,near}.f32 (err: the [H,W] error
// image, near: the [H,W] near-bound image) and one LiDAR frame {pts,col}.f32 [n_points,3], rsp.f32 [n_points], Rcw.f32 [3,3], tcw.f32 [3].  The map
// starts in INSERTION order.  The run: the gradient statistics attached, <iters> steps; one view accumulated with the error image and one with the
// near-bound image; densify() of grow_mask(<grad_above>) splitting above <split_scale>, with the contribution statistics; <iters> steps; resort()
// (the first sort: the tie rank is created) and set_resort_fraction(<fraction>); extend() with the frame (its tail passes the fraction: the rule
// re-sorts); <iters> steps; one more free-space view; prune() of big_mask(<max_screen_radius>); resort(); <iters> steps.  Writes the 19 row arrays
// (dump_rows), out_{max_w,n_pix}.i32, out_{sum_w,err_sum,free_sum,meas_sum}.i64, out_grad_sum.f32, out_n_seen.i32, out_max_radius.i32 over
// [0, size()) and the three permutations out_perm{0,1,2}.i64, printing
// "rows densified <k> splits <s> extended <k2> resorts <n> pruned <r> size <P'> views <v>".
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 14, "usage: fused_rows_check <dir> <P> <W> <H> <deg> <iters> <n_points> <fraction> <w_min> <grad_above> <split_scale> <seed> "
                            "<max_screen_radius>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const int64_t n_pts = std::stoll(argv[7]);
    const double fraction = std::stod(argv[8]);
    const float w_min = std::stof(argv[9]), grad_above = (float)std::stod(argv[10]);
    const double split_scale = std::stod(argv[11]);
    const uint32_t seed = (uint32_t)std::stoul(argv[12]);
    const int32_t max_screen_radius = (int32_t)std::stol(argv[13]);
    const Inputs in = read_inputs(d, P, W, H, deg, 10);
    const gslic::FusedCamera& cam = in.cam;
    const float* s = in.scalars.data();
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), err = load(d + "/err.f32", {H, W}), near = load(d + "/near.f32", {H, W});
    torch::Tensor pts = load(d + "/pts.f32", {n_pts, 3}), col = load(d + "/col.f32", {n_pts, 3}), rsp = load(d + "/rsp.f32", {n_pts});
    torch::Tensor Rcw = load(d + "/Rcw.f32", {3, 3}), tcw = load(d + "/tcw.f32", {3});

    gslic::FusedStep fs = make_step(in, deg);
    auto steps = [&]() {
        for (int it = 0; it < iters; it++) {
            torch::Tensor terms = fs.step(cam, gt);
            std::cout << "loss " << fs.loss_value(terms) << std::endl;
        }
    };
    gslic::GradientStats gst;
    fs.set_gradient_stats(&gst);
    steps();
    gslic::ContributionStats st;
    fs.accumulate_contribution(cam, st, w_min, err);
    fs.accumulate_free_space(cam, st, w_min, near);
    int64_t n_split = 0;
    const torch::Tensor parents = fs.densify(gst.grow_mask(fs.size(), grad_above), split_scale, torch::Tensor(), seed, &st, &n_split);
    steps();
    const torch::Tensor perm0 = fs.resort(&st);              // the first sort, from insertion order
    fs.set_resort_fraction(fraction);
    const int64_t k2 = fs.extend(cam, pts, col, rsp, Rcw, tcw, s[6], s[7], s[8], s[9], 1.0f, &st);   // the appended tail passes the fraction: re-sorted
    const int64_t resorts = fs.resorts();
    const torch::Tensor perm1 = fs.last_resort().clone();
    steps();
    fs.accumulate_free_space(cam, st, w_min, near);
    const int64_t before = fs.size();
    fs.prune(std::nullopt, std::nullopt, gst.big_mask(fs.size(), max_screen_radius), torch::Tensor(), true, &st);
    const int64_t removed = before - fs.size();
    const torch::Tensor perm2 = fs.resort(&st);
    steps();
    std::cout << "rows densified " << parents.size(0) << " splits " << n_split << " extended " << k2 << " resorts " << resorts << " pruned " << removed
              << " size " << fs.size() << " views " << st.views << std::endl;
    dump_rows(fs, d);
    const int64_t Pn = fs.size();
    auto rows = [&](const torch::Tensor& t) { return t.narrow(0, 0, Pn); };
    save_raw(d + "/out_max_w.i32", rows(st.max_w)); save_raw(d + "/out_n_pix.i32", rows(st.n_pix)); save_raw(d + "/out_sum_w.i64", rows(st.sum_w));
    save_raw(d + "/out_err_sum.i64", rows(st.err_sum)); save_raw(d + "/out_free_sum.i64", rows(st.free_sum)); save_raw(d + "/out_meas_sum.i64", rows(st.meas_sum));
    save_raw(d + "/out_grad_sum.f32", rows(gst.grad_sum)); save_raw(d + "/out_n_seen.i32", rows(gst.n_seen)); save_raw(d + "/out_max_radius.i32", rows(gst.max_radius));
    save_raw(d + "/out_perm0.i64", perm0); save_raw(d + "/out_perm1.i64", perm1); save_raw(d + "/out_perm2.i64", perm2);
    return 0;
}
