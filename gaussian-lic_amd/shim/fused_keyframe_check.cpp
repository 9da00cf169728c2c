// fused_keyframe_check.cpp — the keyframe store driven from C++ (gslic::KeyframeStore, shim/include/gslic_fused.h) feeding one fused training step,
// so a test can hold the C++ host against the Python host (trainer.KeyframeStore.target and trainer.training_step_fused).  Same file protocol as
// fused_check.cpp:
//   fused_keyframe_check <dir> <P> <W> <H> <deg> <level> <slot> <n_frames> <masks 0|1>
// reads  <dir>/{xyz,scaling,rotation,opacity,dc,rest}.f32, one camera {view,proj,campos}.f32 with scalars.f32 (tanfovx, tanfovy, 4 lims) — the camera
// of the LEVEL: W >> level by H >> level pixels —, frames.u8 [n_frames,H,W,3] (added with add_u8), image.f32 [3,H,W] (a float image that replaces slot
// 0 through put: the encode kernel) and, with masks, masks.u8 [n_frames,H,W]; decodes <slot> at <level>, runs ONE step on the decoded target (the
// weighted step with masks), prints "loss <loss> visible <n>" and writes out_target.f32 [3,H_l,W_l], out_weight.f32 [H_l,W_l] (with masks),
// out_slot0.u8 [H,W,3] (the re-encoded slot 0), out_terms.f32 [2] and the 19 row arrays (dump_rows).  LibTorch and libgslic_hip.so only.
#include "fused_check_io.h"

using namespace check_io;

int main(int argc, char** argv)
{
    TORCH_CHECK(argc == 10, "usage: fused_keyframe_check <dir> <P> <W> <H> <deg> <level> <slot> <n_frames> <masks 0|1>");
    const std::string d = argv[1];
    const int64_t P = std::stoll(argv[2]), W = std::stoll(argv[3]), H = std::stoll(argv[4]);
    const int deg = std::stoi(argv[5]), level = std::stoi(argv[6]), slot = std::stoi(argv[7]), n_frames = std::stoi(argv[8]);
    const bool masks = std::stoi(argv[9]) != 0;
    const Inputs in = read_inputs(d, P, W >> level, H >> level, deg);

    gslic::KeyframeStore store((int)W, (int)H, n_frames, torch::kCUDA, masks);
    const torch::Tensor frames = load(d + "/frames.u8", {n_frames, H, W, 3}, torch::kByte);
    const torch::Tensor mask_frames = masks ? load(d + "/masks.u8", {n_frames, H, W}, torch::kByte) : torch::Tensor();
    for (int i = 0; i < n_frames; i++) store.add_u8(frames[i], masks ? mask_frames[i] : torch::Tensor());
    store.put(0, load(d + "/image.f32", {3, H, W}));
    TORCH_CHECK(store.serial(0) == 1 && store.n() == n_frames, "KeyframeStore: put did not bump the serial number of slot 0");
    save_raw(d + "/out_slot0.u8", store.color[0]);

    const gslic::KeyframeTarget t = store.target(slot, level);
    save_raw(d + "/out_target.f32", t.image);
    if (masks) save_raw(d + "/out_weight.f32", t.weight);

    gslic::FusedStep fs = make_step(in, deg);
    const torch::Tensor terms = masks ? fs.step(in.cam, t.image, torch::Tensor(), 0.0f, t.weight) : fs.step(in.cam, t.image);
    std::cout << "loss " << fs.loss_value(terms) << " visible " << fs.visible().sum().item<int>() << std::endl;
    save_raw(d + "/out_terms.f32", terms);
    dump_rows(fs, d);
    return 0;
}
