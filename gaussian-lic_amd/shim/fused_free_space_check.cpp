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
#include "fused_check_io.h"

#include <cmath>

using namespace check_io;

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
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera cam[2] = {in.cam, read_camera(d, W, H, in.scalars.data(), "2")};
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W}), near1 = load(d + "/near1.f32", {H, W}), near2 = load(d + "/near2.f32", {H, W});

    gslic::FusedStep fs = make_step(in, deg);
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
    dump_rows(fs, d);
    const int64_t Pn = fs.size();
    save_raw(d + "/out_max_w.i32", st.max_w.narrow(0, 0, Pn)); save_raw(d + "/out_n_pix.i32", st.n_pix.narrow(0, 0, Pn));
    save_raw(d + "/out_sum_w.i64", st.sum_w.narrow(0, 0, Pn)); save_raw(d + "/out_free_sum.i64", st.free_sum.narrow(0, 0, Pn));
    save_raw(d + "/out_meas_sum.i64", st.meas_sum.narrow(0, 0, Pn));
    save_raw(d + "/out_mask.u8", mask); save_raw(d + "/out_kept.i64", kept); save_raw(d + "/out_perm.i64", perm);
    return 0;
}
