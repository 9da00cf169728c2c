// fused_check_io.h — the file protocol the shim/fused_*_check.cpp programs share (included by them only, never by gslic_fused.h): raw little-endian
// arrays under <dir>, written by the tests with numpy's tofile and read back with numpy's fromfile.
//   inputs   <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32 (the six raw parameter groups of P rows; rest only at SH degree > 0),
//            {view,proj,campos}<tag>.f32 (one camera), scalars.f32 (tanfovx, tanfovy, 4 lims, then whatever the program documents) and, when
//            present, tie_rank.f32 (the rows' original indices of a map handed over in a permuted order)
//   outputs  <dir>/out_<name>: out_{xyz,dc,rest,opacity,scaling,rotation}.f32, out_m_<name>.f32, out_v_<name>.f32 and out_tie.i32 are the 19 row
//            arrays (dump_rows); everything else is the program's own
#pragma once
#include "gslic_fused.h"

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace check_io {

inline bool exists(const std::string& path) { return std::ifstream(path, std::ios::binary).good(); }

// a device tensor of `shape` from the file's first bytes (a shorter file is an error)
inline torch::Tensor load(const std::string& path, std::vector<int64_t> shape, torch::ScalarType dt = torch::kFloat32)
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
inline void save_raw(const std::string& path, const torch::Tensor& t)   // the tensor's bytes as they are
{
    torch::Tensor c = t.detach().to(torch::kCPU).contiguous();
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(c.data_ptr()), (std::streamsize)c.nbytes());
}
inline void save(const std::string& path, const torch::Tensor& t) { save_raw(path, t.detach().to(torch::kFloat32)); }   // as floats

// one camera: {view,proj,campos}<tag>.f32 and the first six scalars
inline gslic::FusedCamera read_camera(const std::string& d, int64_t W, int64_t H, const float* s, const std::string& tag = "")
{
    gslic::FusedCamera cam;
    cam.image_width = (int)W; cam.image_height = (int)H;
    cam.world_view_transform = load(d + "/view" + tag + ".f32", {4, 4}); cam.full_proj_transform = load(d + "/proj" + tag + ".f32", {4, 4});
    cam.camera_center = load(d + "/campos" + tag + ".f32", {3});
    cam.tanfovx = s[0]; cam.tanfovy = s[1]; cam.limx_neg = s[2]; cam.limx_pos = s[3]; cam.limy_neg = s[4]; cam.limy_pos = s[5];
    return cam;
}

struct Inputs {
    std::array<torch::Tensor, 6> params;   // xyz, dc, rest, opacity, scaling, rotation: the group order of trainingSetup (gaussian.cpp:399-418)
    gslic::FusedCamera cam;
    std::vector<float> scalars;
    int64_t M = 0;                         // SH rest coefficients per row
};
inline Inputs read_inputs(const std::string& d, int64_t P, int64_t W, int64_t H, int deg, int64_t n_scalars = 6)
{
    Inputs in;
    in.M = deg > 0 ? 15 : 0;
    in.params = {load(d + "/xyz.f32", {P, 3}), load(d + "/dc.f32", {P, 1, 3}),
                 in.M > 0 ? load(d + "/rest.f32", {P, in.M, 3}) : torch::zeros({P, 0, 3}, torch::kCUDA),
                 load(d + "/opacity.f32", {P, 1}), load(d + "/scaling.f32", {P, 3}), load(d + "/rotation.f32", {P, 4})};
    const torch::Tensor sc = load(d + "/scalars.f32", {n_scalars}).to(torch::kCPU);
    in.scalars.assign(sc.data_ptr<float>(), sc.data_ptr<float>() + n_scalars);
    in.cam = read_camera(d, W, H, in.scalars.data());
    return in;
}
// the step on these parameters: trainingSetup (gaussian.cpp:399-418) with config/fastlivo.yaml learning rates (times lr_scale)
inline gslic::FusedStep make_step(const Inputs& in, int deg, float ls = 1.0f)
{
    return gslic::FusedStep(in.params, {1.6e-4f * ls, 2.5e-3f * ls, (float)(2.5e-3 / 20.0) * ls, 5e-2f * ls, 5e-3f * ls, 1e-3f * ls}, deg);
}
// optional <dir>/tie_rank.f32: the rows' original indices of a map handed over in a permuted (Morton) order
inline void probe_tie_rank(gslic::FusedStep& fs, const std::string& d, int64_t P)
{
    if (exists(d + "/tie_rank.f32")) fs.set_tie_rank(load(d + "/tie_rank.f32", {P}).to(torch::kInt32));
}

static const char* const kNames[6] = {"xyz", "dc", "rest", "opacity", "scaling", "rotation"};
// out_<name>.f32 of the six parameter groups as they are now (rest only at SH degree > 0)
inline void dump_params(const gslic::FusedStep& fs, const std::string& d)
{
    for (int g = 0; g < 6; g++) {
        if (g == 2 && fs.param(g).numel() == 0) continue;
        save_raw(d + "/out_" + kNames[g] + ".f32", fs.param(g));
    }
}
// the raw bytes of all 19 row arrays: 6 parameters, 12 moments and the tie rank (when there is one)
inline void dump_rows(const gslic::FusedStep& fs, const std::string& d)
{
    dump_params(fs, d);
    for (int g = 0; g < 6; g++) {
        if (g == 2 && fs.param(g).numel() == 0) continue;
        save_raw(d + "/out_m_" + kNames[g] + ".f32", fs.exp_avg(g));
        save_raw(d + "/out_v_" + kNames[g] + ".f32", fs.exp_avg_sq(g));
    }
    if (fs.tie_rank().defined()) save_raw(d + "/out_tie.i32", fs.tie_rank());
}

}  // namespace check_io
