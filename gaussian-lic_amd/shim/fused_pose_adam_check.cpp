// fused_pose_adam_check.cpp — the joint map + pose iteration driven from C++ (gslic::FusedStep::step_with_pose, shim/include/gslic_fused.h), so a
// test can hold the C++ host against the Python host (trainer.training_step_with_pose(poses=, view=, adam_in_backward=True)).  Same file protocol
// as fused_pose_check.cpp:
//   fused_pose_adam_check <dir> <P> <W> <H> <deg> <iters> <lr_trans> <lr_rot> <lambda_depth>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32, two cameras {view,proj,campos}.f32 / {view,proj,campos}2.f32 with scalars.f32 (tanfovx,
// tanfovy, 4 lims: both cameras), their targets gt.f32 / gt2.f32, gt_depth.f32 [H,W] (used when lambda_depth != 0) and projection.f32 [16], the
// projection the views share; loads the two cameras into a set of two rows and runs <iters> joint steps, step i on row i % 2, and writes the 18 row
// arrays of the map (dump_rows), out_pose_view.f32, out_pose_proj.f32 [2,16], out_pose_campos.f32 [2,3], out_pose_m.f32, out_pose_v.f32 [2,6],
// out_pose_steps.i32 [2], out_pose_grads.f32 [iters,6] (every step's dL/d(rho, phi)) and out_terms.f32 [iters, 2 or 3].  LibTorch and
// libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 10, "usage: fused_pose_adam_check <dir> <P> <W> <H> <deg> <iters> <lr_trans> <lr_rot> <lambda_depth>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float lr_trans = std::stof(argv[7]), lr_rot = std::stof(argv[8]), lambda_depth = std::stof(argv[9]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera cams[2] = {in.cam, read_camera(d, W, H, in.scalars.data(), "2")};
    const torch::Tensor gts[2] = {load(d + "/gt.f32", {3, H, W}), load(d + "/gt2.f32", {3, H, W})};
    const torch::Tensor gt_depth = lambda_depth != 0.0f ? load(d + "/gt_depth.f32", {H, W}) : torch::Tensor();

    gslic::FusedStep fs = make_step(in, deg);
    gslic::PoseSet ps(2, load(d + "/projection.f32", {16}), torch::kCUDA, lr_rot, lr_trans);
    ps.load(0, cams[0]);
    ps.load(1, cams[1]);
    std::vector<torch::Tensor> grads, terms;
    for (int it = 0; it < iters; it++) {
        terms.push_back(fs.step_with_pose(cams[0], gts[it % 2], &ps, it % 2, gt_depth, lambda_depth).clone());
        grads.push_back(ps.grad.clone());
    }
    dump_rows(fs, d);
    save_raw(d + "/out_pose_view.f32", ps.view);
    save_raw(d + "/out_pose_proj.f32", ps.proj);
    save_raw(d + "/out_pose_campos.f32", ps.campos);
    save_raw(d + "/out_pose_m.f32", ps.m);
    save_raw(d + "/out_pose_v.f32", ps.v);
    save_raw(d + "/out_pose_steps.i32", ps.steps);
    if (!grads.empty()) {
        save_raw(d + "/out_pose_grads.f32", torch::stack(grads));
        save_raw(d + "/out_terms.f32", torch::stack(terms));
    }
    return 0;
}
