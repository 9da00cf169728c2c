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
    TORCH_CHECK(argc == 11, "usage: fused_gradient_stats_check <dir> <P> <W> <H> <deg> <iters> <grad_above> <max_screen_radius> <split_scale> <seed>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float grad_above = (float)std::stod(argv[7]);
    const int32_t max_screen_radius = (int32_t)std::stol(argv[8]);
    const double split_scale = std::stod(argv[9]);
    const uint32_t seed = (uint32_t)std::stoul(argv[10]);
    const int64_t M = deg > 0 ? 15 : 0;
    torch::Tensor xyz = load(d + "/xyz.f32", {P, 3}), scaling = load(d + "/scaling.f32", {P, 3}), rotation = load(d + "/rotation.f32", {P, 4});
    torch::Tensor opacity = load(d + "/opacity.f32", {P, 1}), dc = load(d + "/dc.f32", {P, 1, 3});
    torch::Tensor rest = M > 0 ? load(d + "/rest.f32", {P, M, 3}) : torch::zeros({P, 0, 3}, torch::kCUDA);
    gslic::FusedCamera cam;
    cam.image_width = (int)W; cam.image_height = (int)H;
    cam.world_view_transform = load(d + "/view.f32", {4, 4}); cam.full_proj_transform = load(d + "/proj.f32", {4, 4}); cam.camera_center = load(d + "/campos.f32", {3});
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W});
    torch::Tensor sc = load(d + "/scalars.f32", {6}).to(torch::kCPU);
    const float* s = sc.data_ptr<float>();
    cam.tanfovx = s[0]; cam.tanfovy = s[1]; cam.limx_neg = s[2]; cam.limx_pos = s[3]; cam.limy_neg = s[4]; cam.limy_pos = s[5];

    // trainingSetup (gaussian.cpp:399-418) with config/fastlivo.yaml learning rates
    gslic::FusedStep fs({xyz, dc, rest, opacity, scaling, rotation}, {1.6e-4f, 2.5e-3f, (float)(2.5e-3 / 20.0), 5e-2f, 5e-3f, 1e-3f}, deg);
    {
        std::ifstream probe(d + "/tie_rank.f32", std::ios::binary);
        if (probe.good()) fs.set_tie_rank(load(d + "/tie_rank.f32", {P}).to(torch::kInt32));
    }
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
    const char* names[6] = {"xyz", "dc", "rest", "opacity", "scaling", "rotation"};
    for (int g = 0; g < 6; g++) {
        if (g == 2 && M == 0) continue;
        save_raw(d + "/out_" + names[g] + ".f32", fs.param(g));
        save_raw(d + "/out_m_" + names[g] + ".f32", fs.exp_avg(g));
        save_raw(d + "/out_v_" + names[g] + ".f32", fs.exp_avg_sq(g));
    }
    save_raw(d + "/out_tie.i32", fs.tie_rank());
    save_raw(d + "/out_grad_sum.f32", st.grad_sum.narrow(0, 0, fs.size()));
    save_raw(d + "/out_n_seen.i32", st.n_seen.narrow(0, 0, fs.size()));
    save_raw(d + "/out_max_radius.i32", st.max_radius.narrow(0, 0, fs.size()));
    return 0;
}
