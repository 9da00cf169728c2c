// fused_check.cpp — the fused training step driven from C++ (shim/include/gslic_fused.h): the program a Gaussian-LIC maintainer's
// optimize() loop turns into when it adopts the fused entry points.  Same file protocol as dropin_check.cpp (shim/fused_check_io.h):
//   fused_check <dir> <P> <W> <H> <deg> <iters> [timed_iters [lr_scale]]
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest,view,proj,campos,gt}.f32 and scalars.f32 (tanfovx, tanfovy, 4 lims),
// writes <dir>/out_{image,xyz,scaling,rotation,opacity,dc,rest}.f32 after <iters> steps; with timed_iters > 0 it then times that many
// further steps (wall clock between two device synchronisations) and prints "views_per_s <v> ms_per_step <t>".
// When <dir>/frame_pts.f32 exists (+ frame_col.f32 [n,3], frame_rsp.f32 [n], frame_pose.f32 = R_cw[9] | t_cw[3] | fx fy cx cy, frame_n.f32 = n),
// one extend() with that LiDAR frame follows the <iters> steps, then <iters> more steps, and "extend inserted <k>" is printed.
// Needs no reference source: LibTorch + libgslic_hip.so only.
#include "fused_check_io.h"

#include <chrono>
#include <cstdlib>

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc >= 7 && argc <= 9, "usage: fused_check <dir> <P> <W> <H> <deg> <iters> [timed_iters [lr_scale]]");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]), timed = argc >= 8 ? std::stoi(argv[7]) : 0;
    const float ls = argc >= 9 ? std::stof(argv[8]) : 1.0f;   // bench.py times a static synthetic scene at scaled-down rates
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera& cam = in.cam;
    torch::Tensor gt = load(d + "/gt.f32", {3, H, W});

    gslic::FusedStep fs = make_step(in, deg, ls);
    probe_tie_rank(fs, d, P);
    if (std::getenv("GSLIC_CHECK_POSE")) {   // the camera-pose gradient of the initial map (before any step), six numbers
        const auto g = fs.pose_gradient(cam, gt);
        std::cout.precision(9);
        std::cout << "pose_gradient " << g[0] << " " << g[1] << " " << g[2] << " " << g[3] << " " << g[4] << " " << g[5] << std::endl;
    }
    auto steps = [&](int first) {
        for (int it = 0; it < iters; it++) {
            torch::Tensor terms = fs.step(cam, gt);
            std::cout << "iter " << (first + it) << " loss " << fs.loss_value(terms) << " visible " << fs.visible().sum().item<int>() << std::endl;
        }
    };
    steps(0);
    if (exists(d + "/frame_n.f32")) {
        const int64_t n = (int64_t)load(d + "/frame_n.f32", {1}).item<float>();
        torch::Tensor pts = load(d + "/frame_pts.f32", {n, 3}), col = load(d + "/frame_col.f32", {n, 3}), rsp = load(d + "/frame_rsp.f32", {n});
        torch::Tensor pose = load(d + "/frame_pose.f32", {16}).to(torch::kCPU);
        const float* q = pose.data_ptr<float>();
        torch::Tensor Rcw = pose.narrow(0, 0, 9).reshape({3, 3}).clone(), tcw = pose.narrow(0, 9, 3).clone();
        const int64_t k = fs.extend(cam, pts, col, rsp, Rcw, tcw, q[12], q[13], q[14], q[15]);
        std::cout << "extend inserted " << k << " size " << fs.size() << " capacity " << fs.capacity() << std::endl;
        steps(iters);
    }
    save(d + "/out_image.f32", fs.image());
    dump_params(fs, d);
    if (timed > 0) {
        for (int it = 0; it < 5; it++) fs.step(cam, gt);
        torch::cuda::synchronize();
        const auto t0 = std::chrono::steady_clock::now();
        for (int it = 0; it < timed; it++) fs.step(cam, gt);
        torch::cuda::synchronize();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::cout << "views_per_s " << timed / sec << " ms_per_step " << 1e3 * sec / timed << std::endl;
    }
    return 0;
}
