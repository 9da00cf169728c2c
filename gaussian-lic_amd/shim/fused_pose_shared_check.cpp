// fused_pose_shared_check.cpp — the shared extrinsic / time-offset calibration of a pose set driven from C++ (gslic::PoseSet with shared = true,
// FusedStep::step_with_pose and the pose-set overload of FusedStep::pose_gradient with shared = true, shim/include/gslic_fused.h), so a test can hold
// the C++ host against the Python host (trainer.training_step_with_pose(poses=, shared=True, adam_in_backward=True), trainer.pose_gradient(poses=,
// do_step=True, shared=True), PoseSet.load(calibrated=True)).  The file protocol of fused_pose_adam_check.cpp, with a third view and the twists:
//   fused_pose_shared_check <dir> <P> <W> <H> <deg> <iters> <lr_trans> <lr_rot> <lr_time>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32, three cameras {view,proj,campos}{,2,3}.f32 with scalars.f32, their targets gt.f32 / gt2.f32 /
// gt3.f32, projection.f32 [16] and twist.f32 [3,6]; loads the three cameras with their twists into a shared set, runs <iters> joint steps (step i on
// row i % 3), then one pose_gradient(do_step) on row 1, then loads row 2 again from its camera with calibrated = true, and writes the 18 row arrays of
// the map (dump_rows), out_pose_{view,proj,campos}.f32, out_shared_{sm,sv,X,tau}.f32, out_shared_ssteps.i32, out_shared_grads.f32 [iters + 1,7] and
// out_terms.f32 [iters,2].  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 10, "usage: fused_pose_shared_check <dir> <P> <W> <H> <deg> <iters> <lr_trans> <lr_rot> <lr_time>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), iters = std::stoi(argv[6]);
    const float lr_trans = std::stof(argv[7]), lr_rot = std::stof(argv[8]), lr_time = std::stof(argv[9]);
    const Inputs in = read_inputs(d, P, W, H, deg);
    const gslic::FusedCamera cams[3] = {in.cam, read_camera(d, W, H, in.scalars.data(), "2"), read_camera(d, W, H, in.scalars.data(), "3")};
    const torch::Tensor gts[3] = {load(d + "/gt.f32", {3, H, W}), load(d + "/gt2.f32", {3, H, W}), load(d + "/gt3.f32", {3, H, W})};
    const torch::Tensor twist = load(d + "/twist.f32", {3, 6});

    gslic::FusedStep fs = make_step(in, deg);
    gslic::PoseSet ps(3, load(d + "/projection.f32", {16}), torch::kCUDA, lr_rot, lr_trans, 0.9f, 0.999f, 1e-8f, /*shared=*/true, lr_time);
    for (int i = 0; i < 3; i++) ps.load(i, cams[i], twist[i]);
    std::vector<torch::Tensor> grads, terms;
    for (int it = 0; it < iters; it++) {
        terms.push_back(fs.step_with_pose(cams[0], gts[it % 3], &ps, it % 3, torch::Tensor(), 0.0f, torch::Tensor(), torch::Tensor(), 0.0f, /*shared=*/true).clone());
        grads.push_back(ps.shared_grad.clone());
    }
    grads.push_back(fs.pose_gradient(cams[0], gts[1], &ps, 1, /*do_step=*/true, torch::Tensor(), 0.0f, nullptr, torch::Tensor(), torch::Tensor(), 0.0f,
                                     /*shared=*/true).clone());
    ps.load(2, cams[2], twist[2], /*calibrated=*/true);
    dump_rows(fs, d);
    save_raw(d + "/out_pose_view.f32", ps.view);
    save_raw(d + "/out_pose_proj.f32", ps.proj);
    save_raw(d + "/out_pose_campos.f32", ps.campos);
    save_raw(d + "/out_shared_sm.f32", ps.sm);
    save_raw(d + "/out_shared_sv.f32", ps.sv);
    save_raw(d + "/out_shared_ssteps.i32", ps.ssteps);
    save_raw(d + "/out_shared_X.f32", ps.X);
    save_raw(d + "/out_shared_tau.f32", ps.tau);
    save_raw(d + "/out_shared_grads.f32", torch::stack(grads));
    if (!terms.empty()) save_raw(d + "/out_terms.f32", torch::stack(terms));
    return 0;
}
