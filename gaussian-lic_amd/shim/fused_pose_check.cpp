// fused_pose_check.cpp — trainable keyframe poses driven from C++ (gslic::PoseSet and the pose-set overload of gslic::FusedStep::pose_gradient,
// shim/include/gslic_fused.h), so a test can hold the C++ host against the Python host (trainer.pose_gradient(poses=, view=, do_step=True)).
// Same file protocol as fused_check.cpp:
//   fused_pose_check <dir> <P> <W> <H> <deg> <iters> <lr_trans> <lr_rot>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32, two cameras {view,proj,campos}.f32 / {view,proj,campos}2.f32 with scalars.f32 (tanfovx,
// tanfovy, 4 lims: both cameras), their targets gt.f32 / gt2.f32 and projection.f32 [16], the projection the views share; loads the two cameras
// into a set of two rows and runs <iters> pose steps with the map fixed, step i on row i % 2, and writes out_pose_view.f32, out_pose_proj.f32
// [2,16], out_pose_campos.f32 [2,3], out_pose_m.f32, out_pose_v.f32 [2,6], out_pose_steps.i32 [2] and out_pose_grads.f32 [iters,6] (every
// step's dL/d(rho, phi)); then clones the set, resets row 0's moments in the clone and writes out_clone_view.f32, out_clone_m.f32,
// out_clone_steps.i32, out_clone_grad.f32 and out_pose_steps_after_clone.i32 (the original's counts, untouched).  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 9, "usage: fused_pose_check <dir> <P> <W> <H> <deg> <iters> <lr_trans> <lr_rot>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float lr_trans = std::stof(argv[7]), lr_rot = std::stof(argv[8]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera cams[2] = {in.cam, read_camera(d, W, H, in.scalars.data(), "2")};
    const torch::Tensor gts[2] = {load(d + "/gt.f32", {3, H, W}), load(d + "/gt2.f32", {3, H, W})};

    gslic::FusedStep fs = make_step(in, deg);
    gslic::PoseSet ps(2, load(d + "/projection.f32", {16}), torch::kCUDA, lr_rot, lr_trans);
    ps.load(0, cams[0]);
    ps.load(1, cams[1]);
    std::vector<torch::Tensor> grads;
    for (int it = 0; it < iters; it++) grads.push_back(fs.pose_gradient(cams[0], gts[it % 2], &ps, it % 2, /*do_step=*/true).clone());
    save_raw(d + "/out_pose_view.f32", ps.view);
    save_raw(d + "/out_pose_proj.f32", ps.proj);
    save_raw(d + "/out_pose_campos.f32", ps.campos);
    save_raw(d + "/out_pose_m.f32", ps.m);
    save_raw(d + "/out_pose_v.f32", ps.v);
    save_raw(d + "/out_pose_steps.i32", ps.steps);
    if (!grads.empty()) save_raw(d + "/out_pose_grads.f32", torch::stack(grads));
    gslic::PoseSet copy = ps.clone();   // by value: the rows and the gradient of `ps`, then row 0's moments and count reset in the copy alone
    copy.reset_moments(0);
    save_raw(d + "/out_clone_view.f32", copy.view);
    save_raw(d + "/out_clone_m.f32", copy.m);
    save_raw(d + "/out_clone_steps.i32", copy.steps);
    save_raw(d + "/out_clone_grad.f32", copy.grad);
    save_raw(d + "/out_pose_steps_after_clone.i32", ps.steps);
    return 0;
}
