// fused_free_space_check.cpp — the free-space statistics from C++ (gslic::FusedStep::accumulate_free_space of shim/include/gslic_fused.h, and the
// two accumulators carried through prune() and resort()) between fused training steps, so a test can hold the C++ host against the Python host
// (trainer.ContributionStats.accumulate(free_space=...), floater_mask, GaussianModel.prune / to_morton_order).  Same file protocol as
// fused_resort_check.cpp:
//   fused_free_space_check <dir> <P> <W> <H> <deg> <iters> <w_min> <free_fraction_above> <min_measured>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,gt}.f32, two cameras {view,proj,campos}.f32 and {view2,proj2,campos2}.f32 with the shared
// scalars.f32 (tanfovx, tanfovy, 4 lims), and their near-bound images near1.f32 / near2.f32 [H,W].  The map is in INSERTION order.  The run:
// <iters> steps; view 1 and view 2 accumulated with their bounds; the floater mask by trainer.contribution_floater_mask's rule, computed here
// on the unsigned 64-bit values; prune(drop = mask); view 1 again on the pruned map; resort() (the first sort: the tie rank is created);
// <iters> steps.  Writes the raw bytes of all 19 arrays — out_{xyz,dc,rest,opacity,scaling,rotation}.f32, out_m_<name>.f32, out_v_<name>.f32,
// out_tie.i32 — of the five accumulators out_{max_w,n_pix}.i32, out_{sum_w,free_sum,meas_sum}.i64, of out_mask.u8, out_kept.i64 and
// out_perm.i64, printing "free space pruned <r> size <P'>".  LibTorch and libgslic_hip.so only.
#include "gslic_fused.h"

#include <cmath>
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
static double fixed_to_weight(uint64_t q) { return (double)(q >> 32) + (double)(q & 0xffffffffull) / 4294967296.0; }   // trainer.fixed_to_weight

// trainer.contribution_floater_mask: measured >= round(min_measured 2^32) (unsigned), measured != 0, free_weight > fraction * measured_weight
static torch::Tensor floater_mask(const torch::Tensor& free_sum, const torch::Tensor& meas_sum, int64_t P, double fraction, double min_measured)
{
    const torch::Tensor fr = free_sum.narrow(0, 0, P).to(torch::kCPU).contiguous(), ms = meas_sum.narrow(0, 0, P).to(torch::kCPU).contiguous();
    const uint64_t lim = (uint64_t)std::nearbyint(min_measured * 4294967296.0);   // round to nearest, ties to even
    torch::Tensor mask = torch::zeros({P}, torch::kUInt8);
    const uint64_t* f = reinterpret_cast<const uint64_t*>(fr.data_ptr<int64_t>());
    const uint64_t* m = reinterpret_cast<const uint64_t*>(ms.data_ptr<int64_t>());
    uint8_t* o = mask.data_ptr<uint8_t>();
    for (int64_t i = 0; i < P; i++) o[i] = (m[i] >= lim && m[i] != 0 && fixed_to_weight(f[i]) > fraction * fixed_to_weight(m[i])) ? 1 : 0;
    return mask;
}

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 10, "usage: fused_free_space_check <dir> <P> <W> <H> <deg> <iters> <w_min> <free_fraction_above> <min_measured>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float w_min = std::stof(argv[7]);
    const double fraction = std::stod(argv[8]), min_measured = std::stod(argv[9]);
    const int64_t M = deg > 0 ? 15 : 0;
    torch::Tensor xyz = load(d + "/xyz.f32", {P, 3}), scaling = load(d + "/scaling.f32", {P, 3}), rotation = load(d + "/rotation.f32", {P, 4});
    torch::Tensor opacity = load(d + "/opacity.f32", {P, 1}), dc = load(d + "/dc.f32", {P, 1, 3});
    torch::Tensor rest = M > 0 ? load(d + "/rest.f32", {P, M, 3}) : torch::zeros({P, 0, 3}, torch::kCUDA);
    torch::Tensor sc = load(d + "/scalars.f32", {6}).to(torch::kCPU);
    const float* s = sc.data_ptr<float>();
    gslic::FusedCamera cam[2];
    const char* tag[2] = {"", "2"};
    for (int c = 0; c < 2; c++) {
        cam[c].image_width = (int)W; cam[c].image_height = (int)H;
        cam[c].world_view_transform = load(d + "/view" + tag[c] + ".f32", {4, 4}); cam[c].full_proj_transform = load(d + "/proj" + tag[c] + ".f32", {4, 4});
        cam[c].camera_center = load(d + "/campos" + tag[c] + ".f32", {3});
        cam[c].tanfovx = s[0]; cam[c].tanfovy = s[1]; cam[c].limx_neg = s[2]; cam[c].limx_pos = s[3]; cam[c].limy_neg = s[4]; cam[c].limy_pos = s[5];
    }
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), near1 = load(d + "/near1.f32", {H, W}), near2 = load(d + "/near2.f32", {H, W});

    // trainingSetup (gaussian.cpp:399-418) with config/fastlivo.yaml learning rates
    gslic::FusedStep fs({xyz, dc, rest, opacity, scaling, rotation}, {1.6e-4f, 2.5e-3f, (float)(2.5e-3 / 20.0), 5e-2f, 5e-3f, 1e-3f}, deg);
    auto steps = [&]() {
        for (int it = 0; it < iters; it++) {
            torch::Tensor terms = fs.step(cam[0], gt);
            std::cout << "loss " << fs.loss_value(terms) << std::endl;
        }
    };
    steps();
    gslic::ContributionStats st;
    fs.accumulate_free_space(cam[0], st, w_min, near1);
    fs.accumulate_free_space(cam[1], st, w_min, near2);
    const torch::Tensor mask = floater_mask(st.free_sum, st.meas_sum, P, fraction, min_measured);
    const torch::Tensor kept = fs.prune(std::nullopt, std::nullopt, mask.to(torch::kCUDA), torch::Tensor(), true, &st);
    const int64_t removed = P - fs.size();
    fs.accumulate_free_space(cam[0], st, w_min, near1);
    const torch::Tensor perm = fs.resort(&st);               // the first sort, from insertion order
    TORCH_CHECK(fs.tie_rank().defined() && st.views == 3);
    steps();
    std::cout << "free space pruned " << removed << " size " << fs.size() << std::endl;
    const char* names[6] = {"xyz", "dc", "rest", "opacity", "scaling", "rotation"};
    for (int g = 0; g < 6; g++) {
        if (g == 2 && M == 0) continue;
        save_raw(d + "/out_" + names[g] + ".f32", fs.param(g));
        save_raw(d + "/out_m_" + names[g] + ".f32", fs.exp_avg(g));
        save_raw(d + "/out_v_" + names[g] + ".f32", fs.exp_avg_sq(g));
    }
    const int64_t Pn = fs.size();
    save_raw(d + "/out_tie.i32", fs.tie_rank());
    save_raw(d + "/out_max_w.i32", st.max_w.narrow(0, 0, Pn)); save_raw(d + "/out_n_pix.i32", st.n_pix.narrow(0, 0, Pn));
    save_raw(d + "/out_sum_w.i64", st.sum_w.narrow(0, 0, Pn)); save_raw(d + "/out_free_sum.i64", st.free_sum.narrow(0, 0, Pn));
    save_raw(d + "/out_meas_sum.i64", st.meas_sum.narrow(0, 0, Pn));
    save_raw(d + "/out_mask.u8", mask); save_raw(d + "/out_kept.i64", kept); save_raw(d + "/out_perm.i64", perm);
    return 0;
}
