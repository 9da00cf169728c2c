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
#include "gslic_fused.h"

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

static torch::Tensor load(const std::string& path, std::vector<int64_t> shape)
{
    int64_t n = 1;
    for (auto s : shape) n *= s;
    std::vector<float> buf(n);
    std::ifstream f(path, std::ios::binary);
    TORCH_CHECK(f.good(), "cannot open ", path);
    f.read(reinterpret_cast<char*>(buf.data()), n * sizeof(float));
    return torch::from_blob(buf.data(), shape, torch::kFloat32).clone().to(torch::kCUDA);
}
static void save_raw(const std::string& path, const torch::Tensor& t)   // the tensor's bytes as they are
{
    torch::Tensor c = t.detach().to(torch::kCPU).contiguous();
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(c.data_ptr()), (std::streamsize)c.nbytes());
}

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 12, "usage: fused_resort_check <dir> <P> <W> <H> <deg> <iters> <n_points> <fraction> <min_opacity> <max_scale> <w_min>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const int64_t n_pts = std::stoll(argv[7]);
    const double fraction = std::stod(argv[8]), min_opacity = std::stod(argv[9]), max_scale = std::stod(argv[10]);
    const float w_min = std::stof(argv[11]);
    const int64_t M = deg > 0 ? 15 : 0;
    torch::Tensor xyz = load(d + "/xyz.f32", {P, 3}), scaling = load(d + "/scaling.f32", {P, 3}), rotation = load(d + "/rotation.f32", {P, 4});
    torch::Tensor opacity = load(d + "/opacity.f32", {P, 1}), dc = load(d + "/dc.f32", {P, 1, 3});
    torch::Tensor rest = M > 0 ? load(d + "/rest.f32", {P, M, 3}) : torch::zeros({P, 0, 3}, torch::kCUDA);
    gslic::FusedCamera cam;
    cam.image_width = (int)W; cam.image_height = (int)H;
    cam.world_view_transform = load(d + "/view.f32", {4, 4}); cam.full_proj_transform = load(d + "/proj.f32", {4, 4}); cam.camera_center = load(d + "/campos.f32", {3});
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), err = load(d + "/err.f32", {H, W});
    torch::Tensor pts = load(d + "/pts.f32", {n_pts, 3}), col = load(d + "/col.f32", {n_pts, 3}), rsp = load(d + "/rsp.f32", {n_pts});
    torch::Tensor Rcw = load(d + "/Rcw.f32", {3, 3}), tcw = load(d + "/tcw.f32", {3});
    torch::Tensor sc = load(d + "/scalars.f32", {10}).to(torch::kCPU);
    const float* s = sc.data_ptr<float>();
    cam.tanfovx = s[0]; cam.tanfovy = s[1]; cam.limx_neg = s[2]; cam.limx_pos = s[3]; cam.limy_neg = s[4]; cam.limy_pos = s[5];

    // trainingSetup (gaussian.cpp:399-418) with config/fastlivo.yaml learning rates
    gslic::FusedStep fs({xyz, dc, rest, opacity, scaling, rotation}, {1.6e-4f, 2.5e-3f, (float)(2.5e-3 / 20.0), 5e-2f, 5e-3f, 1e-3f}, deg);
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
    const char* names[6] = {"xyz", "dc", "rest", "opacity", "scaling", "rotation"};
    for (int g = 0; g < 6; g++) {
        if (g == 2 && M == 0) continue;
        save_raw(d + "/out_" + names[g] + ".f32", fs.param(g));
        save_raw(d + "/out_m_" + names[g] + ".f32", fs.exp_avg(g));
        save_raw(d + "/out_v_" + names[g] + ".f32", fs.exp_avg_sq(g));
    }
    save_raw(d + "/out_tie.i32", fs.tie_rank());
    save_raw(d + "/out_err_sum.i64", st.err_sum.narrow(0, 0, fs.size()));
    save_raw(d + "/out_perm0.i64", perm0); save_raw(d + "/out_perm1.i64", perm1); save_raw(d + "/out_perm2.i64", perm2);
    return 0;
}
