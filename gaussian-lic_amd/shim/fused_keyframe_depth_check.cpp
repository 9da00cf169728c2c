// fused_keyframe_depth_check.cpp — the keyframe store's depth slabs driven from C++ (gslic::KeyframeStore with depths, shim/include/gslic_fused.h)
// feeding one depth-supervised fused training step, so a test can hold the C++ host against the Python host (trainer.KeyframeStore.depth_target and
// trainer.training_step_fused).  Same file protocol as fused_check.cpp:
//   fused_keyframe_depth_check <dir> <P> <W> <H> <deg> <level> <level2> <slot> <n_frames> <depth_weights 0|1>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32, one camera {view,proj,campos}.f32 with scalars.f32 (tanfovx, tanfovy, 4 lims, lambda_depth,
// depth_huber, depth_step) — the camera of the LEVEL: W >> level by H >> level pixels —, frames.u8 [n_frames,H,W,3] and depths.f32 [n_frames,H,W]
// (added together with add_u8; the LAST frame is added without depth), with depth weights dweights.f32 [n_frames,H,W], and late.f32 [H,W] (a depth
// image that replaces the depth of slot 0 through put_depth, without a weight); decodes <slot> at <level> and at <level2>, runs ONE depth step on the
// decoded colour and depth target of <level>, prints "loss <loss> visible <n>" and writes out_depth_slab.u16 [n_frames,H,W], out_dweight_slab.u8 (with
// depth weights), out_depth.f32 / out_dweight.f32 [H_l,W_l], out_depth2.f32 / out_dweight2.f32 (level2), out_terms.f32 [3] and the 19 row arrays
// (dump_rows).  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 11, "usage: fused_keyframe_depth_check <dir> <P> <W> <H> <deg> <level> <level2> <slot> <n_frames> <depth_weights 0|1>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), level = std::stoi(argv[6]), level2 = std::stoi(argv[7]), slot = std::stoi(argv[8]), n_frames = std::stoi(argv[9]);
    const bool weights = std::stoi(argv[10]) != 0;
    const Inputs in = read_inputs(d, P, W >> level, H >> level, deg, 9);
    const float lambda_depth = in.scalars[6], depth_huber = in.scalars[7], depth_step = in.scalars[8];

    gslic::KeyframeStore store((int)W, (int)H, n_frames, torch::kCUDA, false, true, depth_step, weights);
    TORCH_CHECK(store.has_depths() && store.has_depth_weights() == weights && store.nbytes() == n_frames * H * W * (weights ? 6 : 5),
                "KeyframeStore: the depth slabs are not what the constructor was asked for");
    const torch::Tensor frames = load(d + "/frames.u8", {n_frames, H, W, 3}, torch::kByte);
    const torch::Tensor depths = load(d + "/depths.f32", {n_frames, H, W});
    const torch::Tensor dweights = weights ? load(d + "/dweights.f32", {n_frames, H, W}) : torch::Tensor();
    for (int i = 0; i + 1 < n_frames; i++) store.add_u8(frames[i], torch::Tensor(), false, depths[i], weights ? dweights[i] : torch::Tensor());
    store.add_u8(frames[n_frames - 1]);   // no depth: nothing measured
    store.put_depth(0, load(d + "/late.f32", {H, W}));
    TORCH_CHECK(store.serial(0) == 1 && store.n() == n_frames, "KeyframeStore: put_depth did not bump the serial number of slot 0");
    save_raw(d + "/out_depth_slab.u16", store.depth);
    if (weights) save_raw(d + "/out_dweight_slab.u8", store.dweight);

    const gslic::KeyframeTarget t = store.target(slot, level);
    const gslic::KeyframeDepthTarget dt = store.depth_target(slot, level), dt2 = store.depth_target(slot, level2);
    save_raw(d + "/out_depth.f32", dt.depth);
    save_raw(d + "/out_depth2.f32", dt2.depth);
    if (weights) {
        save_raw(d + "/out_dweight.f32", dt.weight);
        save_raw(d + "/out_dweight2.f32", dt2.weight);
    }

    gslic::FusedStep fs = make_step(in, deg);
    const torch::Tensor terms = fs.step(in.cam, t.image, dt.depth, lambda_depth, torch::Tensor(), dt.weight, depth_huber);
    std::cout << "loss " << fs.loss_value(terms) << " visible " << fs.visible().sum().item<int>() << std::endl;
    save_raw(d + "/out_terms.f32", terms);
    dump_rows(fs, d);
    return 0;
}
