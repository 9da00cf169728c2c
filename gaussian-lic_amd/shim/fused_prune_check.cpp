// fused_prune_check.cpp — pruning the map from C++ (gslic::FusedStep::prune of shim/include/gslic_fused.h) between fused training steps, so a
// test can hold the C++ host against the Python host (trainer.GaussianModel.prune).  Same file protocol as fused_check.cpp:
//   fused_prune_check <dir> <P> <W> <H> <deg> <iters> <min_opacity> <max_scale>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims) and, when present,
// tie_rank.f32 (the rows' original indices of a map stored in a permuted order), runs <iters> steps, prunes with the two limits (activated
// domain; <= 0 disables one), runs <iters> more steps and writes <dir>/out_kept.f32 (the kept rows' old indices, as floats: P < 2^24),
// out_{xyz,scaling,rotation,opacity,dc,rest}.f32 and out_m_xyz.f32 / out_v_xyz.f32 (Adam moments of the positions), printing
// "prune removed <n> size <P'>".  LibTorch and libgslic_hip.so only.
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
static void save(const std::string& path, const torch::Tensor& t)
{
    torch::Tensor c = t.detach().to(torch::kFloat32).to(torch::kCPU).contiguous();
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(c.data_ptr<float>()), c.numel() * sizeof(float));
}

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 9, "usage: fused_prune_check <dir> <P> <W> <H> <deg> <iters> <min_opacity> <max_scale>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const double min_opacity = std::stod(argv[7]), max_scale = std::stod(argv[8]);
    TORCH_CHECK(P < (1 << 24), "out_kept.f32 holds row indices as floats");
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
    for (int it = 0; it < iters; it++) fs.step(cam, gt);
    const torch::Tensor kept = fs.prune(min_opacity > 0.0 ? std::optional<double>(min_opacity) : std::nullopt,
                                        max_scale > 0.0 ? std::optional<double>(max_scale) : std::nullopt);
    std::cout << "prune removed " << (P - kept.size(0)) << " size " << fs.size() << std::endl;
    for (int it = 0; it < iters; it++) {
        torch::Tensor terms = fs.step(cam, gt);
        std::cout << "iter " << (iters + it) << " loss " << fs.loss_value(terms) << " visible " << fs.visible().sum().item<int>() << std::endl;
    }
    save(d + "/out_kept.f32", kept);
    save(d + "/out_xyz.f32", fs.param(0)); save(d + "/out_dc.f32", fs.param(1));
    if (M > 0) save(d + "/out_rest.f32", fs.param(2));
    save(d + "/out_opacity.f32", fs.param(3)); save(d + "/out_scaling.f32", fs.param(4)); save(d + "/out_rotation.f32", fs.param(5));
    save(d + "/out_m_xyz.f32", fs.exp_avg(0)); save(d + "/out_v_xyz.f32", fs.exp_avg_sq(0));
    return 0;
}
