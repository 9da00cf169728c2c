// fused_contribution_check.cpp — per-Gaussian contribution statistics from C++ (gslic::FusedStep::accumulate_contribution and the statistics
// carried through gslic::FusedStep::prune, shim/include/gslic_fused.h), held against arrays the Python host (trainer.ContributionStats) dumped:
//   fused_contribution_check <dir> <P> <W> <H> <deg> <w_min> <pixels_below>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims), when present tie_rank.f32,
// and the expected arrays exp1_{max,npix}.i32, exp1_sum.i64 (one accumulated view), exp_kept.i32 (the rows kept by a prune that drops every row
// with fewer than <pixels_below> counted pixels), exp2_{max,npix}.i32, exp2_sum.i64 (the carried statistics plus the same view accumulated on the
// pruned map).  Every comparison is on the bits.  Prints "contribution check ok rows <P> kept <P'>"; a mismatch exits with status 1.
#include "fused_check_io.h"

using namespace check_io;

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
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera& cam = in.cam;

    gslic::FusedStep fs = make_step(in, deg);
    probe_tie_rank(fs, d, P);
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
