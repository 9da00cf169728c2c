// fused_geometry_check.cpp — the per-pixel geometry images from C++ (gslic::FusedStep::geometry_images and gslic::GeometryImages of
// shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host (trainer.geometry_images).  Same file protocol as
// fused_contribution_check.cpp:
//   fused_geometry_check <dir> <P> <W> <H> <deg> <a_min>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos}.f32, scalars.f32 (tanfovx, tanfovy, 4 lims) and, when present,
// tie_rank.f32.  The run: all seven images of the view; then the default set (an empty GeometryImages) into a second object, which must hold
// exactly opacity / depth_norm / depth_median / top_row with the bits of the first; then the same call again into the first object, which must
// reuse its tensors and repeat its bits.  Writes the raw bytes of out_{transmittance,opacity,depth_sum,depth_norm,depth_median,top_weight}.f32 and
// out_top_row.i32 and prints "geometry check ok rows <P> pixels <H*W>"; a mismatch exits with status 1.  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

static const char* const kImages[7] = {"transmittance", "opacity", "depth_sum", "depth_norm", "depth_median", "top_row", "top_weight"};

static bool same_bits(const torch::Tensor& a, const torch::Tensor& b)
{
    return a.defined() && b.defined() && a.sizes() == b.sizes() && torch::equal(a.view(torch::kInt32), b.view(torch::kInt32));
}

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 7, "usage: fused_geometry_check <dir> <P> <W> <H> <deg> <a_min>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]);
    const float a_min = std::stof(argv[6]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera& cam = in.cam;

    gslic::FusedStep fs = make_step(in, deg);
    probe_tie_rank(fs, d, P);
    gslic::GeometryImages all;
    all.make(H, W, torch::kCUDA, {true, true, true, true, true, true, true});
    fs.geometry_images(cam, all, a_min);
    std::array<torch::Tensor, 7> first;
    std::array<void*, 7> address;
    for (int i = 0; i < 7; i++) { first[i] = all.all()[i]->clone(); address[i] = all.all()[i]->data_ptr(); }

    gslic::GeometryImages some;   // nothing defined: the default set
    fs.geometry_images(cam, some, a_min);
    bool ok = !some.transmittance.defined() && !some.depth_sum.defined() && !some.top_weight.defined();
    ok &= same_bits(some.opacity, first[1]) && same_bits(some.depth_norm, first[3]) && same_bits(some.depth_median, first[4]) && same_bits(some.top_row, first[5]);
    if (!ok) std::cout << "MISMATCH: the default set differs from the all-images call" << std::endl;

    fs.geometry_images(cam, all, a_min);   // again: the same tensors, the same bits
    for (int i = 0; i < 7; i++) {
        const bool same = all.all()[i]->data_ptr() == address[i] && same_bits(*all.all()[i], first[i]);
        if (!same) std::cout << "MISMATCH: " << kImages[i] << " changed between two calls" << std::endl;
        ok &= same;
    }
    for (int i = 0; i < 7; i++) save_raw(d + "/out_" + kImages[i] + (i == 5 ? ".i32" : ".f32"), *all.all()[i]);
    if (!ok) return 1;
    std::cout << "geometry check ok rows " << P << " pixels " << H * W << std::endl;
    return 0;
}
