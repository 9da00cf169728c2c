// keyframes_depth.hip — the keyframe store's depth slabs, in a module of their own beside keyframes.hip (whose kernels stay as they compile alone).
// The LiDAR depth of a slot as 16-bit codes (0 = not measured, k >= 1 = depth k * step, step a power of two) and an optional 8-bit weight; the
// rules are written out in include/gslic_hip.h (gslic_keyframe_decode_depth / gslic_keyframe_encode_depth).  The decode is an UNSIGNED MINIMUM of
// integer keys — key = code, or (code << 8) | (255 - weight) with a weight slab — and ONE float multiply per output; the encode one exact float
// multiply, one add and a floor.  Both are streams shaped like the colour pair: the decode reads 3 * 4^l bytes (2 * 4^l without weights) and
// writes 8 (4) per output pixel; a lane of the fast path owns FOUR consecutive output pixels, reads 8 << l bytes of codes and 4 << l bytes of
// weights per source row (non-temporal; kf_load_row at the widths of the colour path) into four running minima and stores 16 bytes per plane.
#include "gslic_common.h"
#include "kernels.h"
#include "keyframe_rows.h"

namespace gslic {

static constexpr uint32_t KF_NO_RETURN = 0xffffffffu;   // above every key: a key is at most (65535 << 8) | 255

struct KeyframeDepthArgs {
    int W, H, Wl, Hl, level, n_frames;
    const uint16_t* depth;    // [capacity, H, W] codes
    const uint8_t* dweight;   // [capacity, H, W] or NULL
    const int32_t* frame;     // device word: the slot
    float* depth_out;         // [Hl, Wl]
    float* dweight_out;       // [Hl, Wl] or NULL
    float step;               // 2^e
};

// the key of one pixel: KF_NO_RETURN where nothing was measured, so that the minimum of a block is its nearest return (largest weight among equals)
template <bool HAS_W>
__device__ __forceinline__ uint32_t kf_depth_key(uint32_t code, uint32_t wcode)
{
    const uint32_t key = HAS_W ? ((code << 8) | (255u - wcode)) : code;
    return code ? key : KF_NO_RETURN;
}

template <bool HAS_W>
__device__ __forceinline__ float kf_depth_of(uint32_t m, float step)
{
    return m == KF_NO_RETURN ? 0.0f : (float)(HAS_W ? (m >> 8) : m) * step;
}

__device__ __forceinline__ float kf_dweight_of(uint32_t m)
{
    return m == KF_NO_RETURN ? 0.0f : (float)(255u - (m & 255u)) * (1.0f / 255.0f);
}

template <int L, bool HAS_W>
__global__ __launch_bounds__(KF_THREADS) void keyframe_decode_depth_kernel(KeyframeDepthArgs a)
{
    const int32_t f = a.frame[0];
    if (f < 0 || f >= a.n_frames) return;
    const size_t g = (size_t)blockIdx.x * KF_THREADS + threadIdx.x;
    const int gpr = a.Wl >> 2;                                  // groups per output row
    if (g >= (size_t)gpr * (size_t)a.Hl) return;
    const int Y = (int)(g / (size_t)gpr), X = 4 * (int)(g % (size_t)gpr);
    const size_t pix = (size_t)a.H * (size_t)a.W;
    const size_t first = (size_t)f * pix + (size_t)(Y << L) * (size_t)a.W + (size_t)(X << L);
    const uint8_t* crow = reinterpret_cast<const uint8_t*>(a.depth + first);   // 8 << L bytes of codes per source row
    const uint8_t* wrow = HAS_W ? a.dweight + first : nullptr;                 // 4 << L bytes of weights
    uint32_t m[4] = {KF_NO_RETURN, KF_NO_RETURN, KF_NO_RETURN, KF_NO_RETURN};
    for (int r = 0; r < (1 << L); r++) {
        uint32_t c[2 << L], w[1 << L];
        kf_load_row<L + 1, 1>(crow, c);                         // level 0: one 8-byte load, level 1: one 16-byte load, then 1 << (L - 1) of them
        if constexpr (HAS_W) kf_load_row<L, 1>(wrow, w);        // level 0: one dword, level 1: one 8-byte load, then 1 << (L - 2) 16-byte loads
#pragma unroll
        for (int p = 0; p < (4 << L); p++) {                    // pixel p of the segment belongs to output pixel p >> L
            const uint32_t code = (c[p >> 1] >> (16 * (p & 1))) & 0xffffu;
            uint32_t wc = 0u;
            if constexpr (HAS_W) wc = (w[p >> 2] >> (8 * (p & 3))) & 0xffu;
            m[p >> L] = min(m[p >> L], kf_depth_key<HAS_W>(code, wc));
        }
        crow += (size_t)a.W * 2;
        if constexpr (HAS_W) wrow += a.W;
    }
    const size_t o = (size_t)Y * (size_t)a.Wl + (size_t)X;
    const gs_v4f d = {kf_depth_of<HAS_W>(m[0], a.step), kf_depth_of<HAS_W>(m[1], a.step), kf_depth_of<HAS_W>(m[2], a.step), kf_depth_of<HAS_W>(m[3], a.step)};
    *reinterpret_cast<gs_v4f*>(a.depth_out + o) = d;
    if constexpr (HAS_W) {
        const gs_v4f wv = {kf_dweight_of(m[0]), kf_dweight_of(m[1]), kf_dweight_of(m[2]), kf_dweight_of(m[3])};
        *reinterpret_cast<gs_v4f*>(a.dweight_out + o) = wv;
    }
}

// every other width: one lane per output pixel, the block read code by code
__global__ __launch_bounds__(KF_THREADS) void keyframe_decode_depth_scalar_kernel(KeyframeDepthArgs a)
{
    const int32_t f = a.frame[0];
    if (f < 0 || f >= a.n_frames) return;
    const size_t i = (size_t)blockIdx.x * KF_THREADS + threadIdx.x;
    if (i >= (size_t)a.Hl * (size_t)a.Wl) return;
    const int Y = (int)(i / (size_t)a.Wl), X = (int)(i % (size_t)a.Wl);
    const int n = 1 << a.level;
    const size_t first = (size_t)f * (size_t)a.H * (size_t)a.W + (size_t)(Y << a.level) * (size_t)a.W + (size_t)(X << a.level);
    const uint16_t* c0 = a.depth + first;
    uint32_t m = KF_NO_RETURN;
    if (a.dweight) {
        const uint8_t* w0 = a.dweight + first;
        for (int r = 0; r < n; r++) {
            for (int k = 0; k < n; k++) m = min(m, kf_depth_key<true>(__builtin_nontemporal_load(c0 + k), __builtin_nontemporal_load(w0 + k)));
            c0 += a.W; w0 += a.W;
        }
        a.depth_out[i] = kf_depth_of<true>(m, a.step);
        a.dweight_out[i] = kf_dweight_of(m);
    } else {
        for (int r = 0; r < n; r++) {
            for (int k = 0; k < n; k++) m = min(m, kf_depth_key<false>(__builtin_nontemporal_load(c0 + k), 0u));
            c0 += a.W;
        }
        a.depth_out[i] = kf_depth_of<false>(m, a.step);
    }
}

// code = k = floorf(d / step + 0.5) where d > 0 is finite and 1 <= k <= 65535, else 0 (not measured: never clamped to a wrong depth); the quotient
// is the exact product with 1 / step, rounded on its own
__device__ __forceinline__ uint32_t kf_depth_code(float d, float inv_step)
{
#pragma clang fp contract(off)
    if (!(d > 0.0f && d < __builtin_inff())) return 0u;
    const float k = floorf(__fmul_rn(d, inv_step) + 0.5f);
    return (k >= 1.0f && k <= 65535.0f) ? (uint32_t)k : 0u;
}

// float depth [N] (and weight [N] or NULL: every weight 255) -> codes [N] (and bytes [N] when wslot != NULL).  QUADS: N % 4 == 0 and every pointer
// aligned to its access: a lane takes four pixels, one 8-byte store of codes and one dword store of weights; otherwise one pixel per lane
template <bool QUADS>
__global__ __launch_bounds__(KF_THREADS) void keyframe_encode_depth_kernel(size_t N, const float* __restrict__ depth, const float* __restrict__ weight,
                                                                          uint16_t* __restrict__ cslot, uint8_t* __restrict__ wslot, float inv_step)
{
    const size_t t = (size_t)blockIdx.x * KF_THREADS + threadIdx.x;
    if constexpr (QUADS) {
        const size_t i = 4 * t;
        if (i >= N) return;
        const gs_v4f d = *reinterpret_cast<const gs_v4f*>(depth + i);
        kf_u2 c;
        c.x = kf_depth_code(d[0], inv_step) | (kf_depth_code(d[1], inv_step) << 16);
        c.y = kf_depth_code(d[2], inv_step) | (kf_depth_code(d[3], inv_step) << 16);
        *reinterpret_cast<kf_u2*>(cslot + i) = c;
        if (wslot) {
            uint32_t q = 0xffffffffu;
            if (weight) {
                const gs_v4f v = *reinterpret_cast<const gs_v4f*>(weight + i);
                q = kf_quantise(v[0]) | (kf_quantise(v[1]) << 8) | (kf_quantise(v[2]) << 16) | (kf_quantise(v[3]) << 24);
            }
            *reinterpret_cast<uint32_t*>(wslot + i) = q;
        }
    } else {
        if (t >= N) return;
        cslot[t] = (uint16_t)kf_depth_code(depth[t], inv_step);
        if (wslot) wslot[t] = weight ? (uint8_t)kf_quantise(weight[t]) : (uint8_t)255;
    }
}

static bool kf_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

int keyframe_decode_depth(int W, int H, int level, const uint16_t* depth, const uint8_t* dweight, const int32_t* frame, int n_frames, float step,
                          float* depth_out, float* dweight_out, hipStream_t s)
{
    KeyframeDepthArgs a{};
    a.W = W; a.H = H; a.Wl = W >> level; a.Hl = H >> level; a.level = level; a.n_frames = n_frames;
    a.depth = depth; a.dweight = dweight; a.frame = frame; a.depth_out = depth_out; a.dweight_out = dweight ? dweight_out : nullptr; a.step = step;
    const size_t plane = (size_t)a.Hl * (size_t)a.Wl;
    // as for colour: the fast path's accesses are aligned when the slabs and the outputs are (checked by the caller) and W is a multiple of 4 << level
    if (W % (4 << level) == 0) {
        const dim3 grid((unsigned)div_up_sz(plane / 4, KF_THREADS)), block(KF_THREADS);
#define KF_DEPTH_CASE(L) \
        if (dweight) GS_LAUNCH(K_GATHER_ROWS, (keyframe_decode_depth_kernel<L, true>), grid, block, 0, s, a); \
        else GS_LAUNCH(K_GATHER_ROWS, (keyframe_decode_depth_kernel<L, false>), grid, block, 0, s, a); \
        break
        switch (level) {
        case 0: KF_DEPTH_CASE(0);
        case 1: KF_DEPTH_CASE(1);
        case 2: KF_DEPTH_CASE(2);
        case 3: KF_DEPTH_CASE(3);
        default: KF_DEPTH_CASE(4);
        }
#undef KF_DEPTH_CASE
    } else {
        GS_LAUNCH(K_GATHER_ROWS, keyframe_decode_depth_scalar_kernel, dim3((unsigned)div_up_sz(plane, KF_THREADS)), dim3(KF_THREADS), 0, s, a);
    }
    return GSLIC_OK;
}

int keyframe_encode_depth(int W, int H, const float* depth, const float* weight, uint16_t* depth_slot, uint8_t* dweight_slot, float step, hipStream_t s)
{
    const size_t N = (size_t)H * (size_t)W;
    const float inv_step = 1.0f / step;   // exact: step is a power of two
    const dim3 block(KF_THREADS);
    if (N % 4 == 0 && kf_aligned16(depth) && kf_aligned16(weight) && kf_aligned8(depth_slot) && kf_aligned4(dweight_slot))
        GS_LAUNCH(K_GATHER_ROWS, (keyframe_encode_depth_kernel<true>), dim3((unsigned)div_up_sz(N / 4, KF_THREADS)), block, 0, s, N, depth, weight,
                  depth_slot, dweight_slot, inv_step);
    else
        GS_LAUNCH(K_GATHER_ROWS, (keyframe_encode_depth_kernel<false>), dim3((unsigned)div_up_sz(N, KF_THREADS)), block, 0, s, N, depth, weight,
                  depth_slot, dweight_slot, inv_step);
    return GSLIC_OK;
}

}  // namespace gslic
