// fused_contribution_check.cpp — per-Gaussian contribution statistics from C++ (gslic::FusedStep::accumulate_contribution and the statistics
// carried through gslic::FusedStep::prune, shim/include/gslic_fused.h), held against arrays the Python host (trainer.ContributionStats) dumped:
//   fused_contribution_check <dir> <P> <W> <H> <deg> <w_min> <pixels_below>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims), when present tie_rank.f32,
// and the expected arrays exp1_{max,npix}.i32, exp1_sum.i64 (one accumulated view), exp_kept.i32 (the rows kept by a prune that drops every row
// with fewer than <pixels_below> counted pixels), exp2_{max,npix}.i32, exp2_sum.i64 (the carried statistics plus the same view accumulated on the
// pruned map).  Every comparison is on the bits.  Prints "contribution check ok rows <P> kept <P'>"; a mismatch exits with status 1.
#include "gslic_fused.h"

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

static torch::Tensor load(const std::string& path, std::vector<int64_t> shape, torch::ScalarType dt = torch::kFloat32)
{
    int64_t n = 1;
    for (auto s : shape) n *= s;
    const size_t bytes = (size_t)n * torch::elementSize(dt);
    std::vector<char> buf(bytes);
    std::ifstream f(path, std::ios::binary);
    TORCH_CHECK(f.good(), "cannot open ", path);
    f.read(buf.data(), (std::streamsize)bytes);
    TORCH_CHECK((size_t)f.gcount() == bytes, path, " is shorter than ", bytes, " bytes");
    return torch::from_blob(buf.data(), shape, dt).clone().to(torch::kCUDA);
}

static bool same(const char* what, const torch::Tensor& got, const torch::Tensor& want)
{
    const bool ok = got.sizes() == want.sizes() && torch::equal(got, want);
    if (!ok) std::cout << "MISMATCH " << what << ": " << (got.sizes() == want.sizes() ? (got != want).sum().item<int64_t>() : (int64_t)-1) << " rows differ" << std::endl;
    return ok;
}

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 8, "usage: fused_contribution_check <dir> <P> <W> <H> <deg> <w_min> <pixels_below>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]);
    const float w_min = std::stof(argv[6]);
    const int64_t pixels_below = std::stoll(argv[7]);
    const int64_t M = deg > 0 ? 15 : 0;
    torch::Tensor xyz = load(d + "/xyz.f32", {P, 3}), scaling = load(d + "/scaling.f32", {P, 3}), rotation = load(d + "/rotation.f32", {P, 4});
    torch::Tensor opacity = load(d + "/opacity.f32", {P, 1}), dc = load(d + "/dc.f32", {P, 1, 3});
    torch::Tensor rest = M > 0 ? load(d + "/rest.f32", {P, M, 3}) : torch::zeros({P, 0, 3}, torch::kCUDA);
    gslic::FusedCamera cam;
    cam.image_width = (int)W; cam.image_height = (int)H;
    cam.world_view_transform = load(d + "/view.f32", {4, 4}); cam.full_proj_transform = load(d + "/proj.f32", {4, 4}); cam.camera_center = load(d + "/campos.f32", {3});
    torch::Tensor sc = load(d + "/scalars.f32", {6}).to(torch::kCPU);
    const float* s = sc.data_ptr<float>();
    cam.tanfovx = s[0]; cam.tanfovy = s[1]; cam.limx_neg = s[2]; cam.limx_pos = s[3]; cam.limy_neg = s[4]; cam.limy_pos = s[5];

    gslic::FusedStep fs({xyz, dc, rest, opacity, scaling, rotation}, {1.6e-4f, 2.5e-3f, (float)(2.5e-3 / 20.0), 5e-2f, 5e-3f, 1e-3f}, deg);
    {
        std::ifstream probe(d + "/tie_rank.f32", std::ios::binary);
        if (probe.good()) fs.set_tie_rank(load(d + "/tie_rank.f32", {P}).to(torch::kInt32));
    }
    gslic::ContributionStats st;
    fs.accumulate_contribution(cam, st, w_min);
    bool ok = st.views == 1;
    ok &= same("max_w (view 1)", st.max_w.narrow(0, 0, P), load(d + "/exp1_max.i32", {P}, torch::kInt32));
    ok &= same("n_pix (view 1)", st.n_pix.narrow(0, 0, P), load(d + "/exp1_npix.i32", {P}, torch::kInt32));
    ok &= same("sum_w (view 1)", st.sum_w.narrow(0, 0, P), load(d + "/exp1_sum.i64", {P}, torch::kInt64));
    // the Python host's drop_mask(pixels_below = k): an integer comparison on the counts
    const torch::Tensor drop = (st.n_pix.narrow(0, 0, P).to(torch::kInt64).bitwise_and(0xffffffffLL) < pixels_below).to(torch::kByte);
    const torch::Tensor kept = fs.prune(std::nullopt, std::nullopt, drop, torch::Tensor(), true, &st);
    const int64_t Pn = fs.size();
    ok &= kept.size(0) == Pn;
    ok &= same("kept rows", kept.to(torch::kInt32), load(d + "/exp_kept.i32", {Pn}, torch::kInt32));
    fs.accumulate_contribution(cam, st, w_min);
    ok &= st.views == 2;
    ok &= same("max_w (pruned, view 2)", st.max_w.narrow(0, 0, Pn), load(d + "/exp2_max.i32", {Pn}, torch::kInt32));
    ok &= same("n_pix (pruned, view 2)", st.n_pix.narrow(0, 0, Pn), load(d + "/exp2_npix.i32", {Pn}, torch::kInt32));
    ok &= same("sum_w (pruned, view 2)", st.sum_w.narrow(0, 0, Pn), load(d + "/exp2_sum.i64", {Pn}, torch::kInt64));
    ok &= bool((st.max_w.narrow(0, Pn, st.max_w.size(0) - Pn) == 0).all().item<bool>());   // rows behind the map stay zero
    if (!ok) return 1;
    std::cout << "contribution check ok rows " << P << " kept " << Pn << std::endl;
    return 0;
}
