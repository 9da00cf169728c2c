// keyframes.hip — the keyframe store's two kernels: 8-bit interleaved slots decoded into the planar float32 target of a pyramid level, and planar
// float32 images encoded into a slot.  The rules are written out in include/gslic_hip.h (gslic_keyframe_decode / gslic_keyframe_encode); the decode is
// an integer sum and ONE float multiply, the encode one float multiply, one add and a floor (fp contract off: the product is rounded on its own).
//
// Both kernels are streams: the decode reads 3 * 4^l bytes and writes 12 bytes per output pixel (4^l and 4 for the mask), the encode reads 12 and
// writes 3.  A lane owns a group of FOUR consecutive output pixels of one row:
//   decode, fast path (W % (4 << l) == 0: every group is whole, no remainder column exists, and every address below is aligned to its access):
//     the group's source is, per source row, 12 << l contiguous bytes (4 << l for the mask) — level 0: three dword loads, level 1: three 8-byte
//     loads, level >= 2: 3 << (l - 2) 16-byte loads per row, 2^l rows — summed per pixel and channel in integer registers, then one 16-byte store
//     into each plane.  The slab is read once: non-temporal loads.  The output is what the loss kernels read next: ordinary stores.
//   decode, scalar path (every other width): a lane owns ONE output pixel, reads its block byte by byte and stores three floats (and the weight).
//   encode: W % 4 == 0 reads one 16-byte quad per plane and writes three dwords (one for the mask); other widths go pixel by pixel.
// The decode reads the slot index from a device word; a word outside [0, n_frames) makes every lane return before its first load.  No atomics, no
// allocation, no read-back: capturable in a graph.
#include "gslic_common.h"
#include "kernels.h"
#include "keyframe_rows.h"

namespace gslic {

// One group of the fast path: output pixels (X .. X + 3, Y) of a CH-channel slot [H, W, CH] -> planes out + c * plane (plane = H_l * W_l floats)
template <int L, int CH>
__device__ __forceinline__ void kf_decode_group(const uint8_t* __restrict__ slot, int W, int Wl, int X, int Y, float scale, float* __restrict__ out,
                                                size_t plane)
{
    uint32_t acc[4][CH];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int c = 0; c < CH; c++) acc[j][c] = 0u;
    const uint8_t* row = slot + ((size_t)(Y << L) * (size_t)W + (size_t)(X << L)) * CH;
    for (int r = 0; r < (1 << L); r++) {
        uint32_t w[CH << L];
        kf_load_row<L, CH>(row, w);
#pragma unroll
        for (int b = 0; b < ((4 * CH) << L); b++) {   // byte b of the segment: pixel b / CH of the 4 << L, channel b % CH
            const uint32_t v = (w[b >> 2] >> (8 * (b & 3))) & 0xffu;
            acc[(b / CH) >> L][b % CH] += v;
        }
        row += (size_t)W * CH;
    }
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const gs_v4f o = {(float)acc[0][c] * scale, (float)acc[1][c] * scale, (float)acc[2][c] * scale, (float)acc[3][c] * scale};
        *reinterpret_cast<gs_v4f*>(out + (size_t)c * plane + (size_t)Y * (size_t)Wl + (size_t)X) = o;
    }
}

struct KeyframeDecodeArgs {
    int W, H, Wl, Hl, level, n_frames;
    const uint8_t* color;     // [capacity, H, W, 3]
    const uint8_t* mask;      // [capacity, H, W] or NULL
    const int32_t* frame;     // device word: the slot
    float* out;               // [3, Hl, Wl]
    float* weight;            // [Hl, Wl] or NULL
    float scale;              // c_l
};

template <int L>
__global__ __launch_bounds__(KF_THREADS) void keyframe_decode_kernel(KeyframeDecodeArgs a)
{
    const int32_t f = a.frame[0];
    if (f < 0 || f >= a.n_frames) return;
    const size_t g = (size_t)blockIdx.x * KF_THREADS + threadIdx.x;
    const int gpr = a.Wl >> 2;                                  // groups per output row
    if (g >= (size_t)gpr * (size_t)a.Hl) return;
    const int Y = (int)(g / (size_t)gpr), X = 4 * (int)(g % (size_t)gpr);
    const size_t pix = (size_t)a.H * (size_t)a.W, plane = (size_t)a.Hl * (size_t)a.Wl;
    kf_decode_group<L, 3>(a.color + (size_t)f * pix * 3, a.W, a.Wl, X, Y, a.scale, a.out, plane);
    if (a.mask) kf_decode_group<L, 1>(a.mask + (size_t)f * pix, a.W, a.Wl, X, Y, a.scale, a.weight, plane);
}

// every other width: one lane per output pixel, the block read byte by byte
__global__ __launch_bounds__(KF_THREADS) void keyframe_decode_scalar_kernel(KeyframeDecodeArgs a)
{
    const int32_t f = a.frame[0];
    if (f < 0 || f >= a.n_frames) return;
    const size_t i = (size_t)blockIdx.x * KF_THREADS + threadIdx.x;
    const size_t plane = (size_t)a.Hl * (size_t)a.Wl;
    if (i >= plane) return;
    const int Y = (int)(i / (size_t)a.Wl), X = (int)(i % (size_t)a.Wl);
    const int n = 1 << a.level;
    const size_t pix = (size_t)a.H * (size_t)a.W;
    const size_t first = (size_t)(Y << a.level) * (size_t)a.W + (size_t)(X << a.level);
    const uint8_t* c0 = a.color + (size_t)f * pix * 3 + first * 3;
    uint32_t s0 = 0u, s1 = 0u, s2 = 0u;
    for (int r = 0; r < n; r++) {
        for (int k = 0; k < n; k++) {
            s0 += __builtin_nontemporal_load(c0 + 3 * k);
            s1 += __builtin_nontemporal_load(c0 + 3 * k + 1);
            s2 += __builtin_nontemporal_load(c0 + 3 * k + 2);
        }
        c0 += (size_t)a.W * 3;
    }
    a.out[i] = (float)s0 * a.scale;
    a.out[plane + i] = (float)s1 * a.scale;
    a.out[2 * plane + i] = (float)s2 * a.scale;
    if (a.mask) {
        const uint8_t* m0 = a.mask + (size_t)f * pix + first;
        uint32_t s = 0u;
        for (int r = 0; r < n; r++) {
            for (int k = 0; k < n; k++) s += __builtin_nontemporal_load(m0 + k);
            m0 += a.W;
        }
        a.weight[i] = (float)s * a.scale;
    }
}

// planar float [CH, N] -> interleaved bytes [N, CH]; QUADS: N % 4 == 0 and the planes are 16-byte aligned: a lane takes four pixels, reads one quad per
// plane and writes CH dwords; otherwise one pixel per lane
template <int CH, bool QUADS>
__global__ __launch_bounds__(KF_THREADS) void keyframe_encode_kernel(size_t N, const float* __restrict__ image, uint8_t* __restrict__ slot)
{
    const size_t t = (size_t)blockIdx.x * KF_THREADS + threadIdx.x;
    if constexpr (QUADS) {
        const size_t i = 4 * t;
        if (i >= N) return;
        uint32_t q[4][CH];
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const gs_v4f v = *reinterpret_cast<const gs_v4f*>(image + (size_t)c * N + i);
#pragma unroll
            for (int j = 0; j < 4; j++) q[j][c] = kf_quantise(v[j]);
        }
        uint32_t w[CH];
#pragma unroll
        for (int k = 0; k < CH; k++) w[k] = 0u;
#pragma unroll
        for (int b = 0; b < 4 * CH; b++) w[b >> 2] |= q[b / CH][b % CH] << (8 * (b & 3));
        uint32_t* dst = reinterpret_cast<uint32_t*>(slot + i * CH);
#pragma unroll
        for (int k = 0; k < CH; k++) dst[k] = w[k];
    } else {
        if (t >= N) return;
#pragma unroll
        for (int c = 0; c < CH; c++) slot[t * CH + c] = (uint8_t)kf_quantise(image[(size_t)c * N + t]);
    }
}

int keyframe_decode(int W, int H, int level, const uint8_t* color, const uint8_t* mask, const int32_t* frame, int n_frames, float* out, float* weight,
                    hipStream_t s)
{
    KeyframeDecodeArgs a{};
    a.W = W; a.H = H; a.Wl = W >> level; a.Hl = H >> level; a.level = level; a.n_frames = n_frames;
    a.color = color; a.mask = mask; a.frame = frame; a.out = out; a.weight = mask ? weight : nullptr;
    a.scale = ldexpf(1.0f / 255.0f, -2 * level);
    const size_t plane = (size_t)a.Hl * (size_t)a.Wl;
    // the fast path's accesses are aligned when the slabs and the outputs are (checked by the caller) and W is a multiple of 4 << level
    if (W % (4 << level) == 0) {
        const dim3 grid((unsigned)div_up_sz(plane / 4, KF_THREADS)), block(KF_THREADS);
        switch (level) {
        case 0: GS_LAUNCH(K_GATHER_ROWS, keyframe_decode_kernel<0>, grid, block, 0, s, a); break;
        case 1: GS_LAUNCH(K_GATHER_ROWS, keyframe_decode_kernel<1>, grid, block, 0, s, a); break;
        case 2: GS_LAUNCH(K_GATHER_ROWS, keyframe_decode_kernel<2>, grid, block, 0, s, a); break;
        case 3: GS_LAUNCH(K_GATHER_ROWS, keyframe_decode_kernel<3>, grid, block, 0, s, a); break;
        default: GS_LAUNCH(K_GATHER_ROWS, keyframe_decode_kernel<4>, grid, block, 0, s, a); break;
        }
    } else {
        GS_LAUNCH(K_GATHER_ROWS, keyframe_decode_scalar_kernel, dim3((unsigned)div_up_sz(plane, KF_THREADS)), dim3(KF_THREADS), 0, s, a);
    }
    return GSLIC_OK;
}

int keyframe_encode(int W, int H, const float* image, const float* mask, uint8_t* color_slot, uint8_t* mask_slot, hipStream_t s)
{
    const size_t N = (size_t)H * (size_t)W;
    const dim3 block(KF_THREADS), quads((unsigned)div_up_sz(div_up_sz(N, 4), KF_THREADS)), pixels((unsigned)div_up_sz(N, KF_THREADS));
    if (image) {
        if (N % 4 == 0 && kf_aligned16(image) && kf_aligned4(color_slot))
            GS_LAUNCH(K_GATHER_ROWS, (keyframe_encode_kernel<3, true>), quads, block, 0, s, N, image, color_slot);
        else
            GS_LAUNCH(K_GATHER_ROWS, (keyframe_encode_kernel<3, false>), pixels, block, 0, s, N, image, color_slot);
    }
    if (mask) {
        if (N % 4 == 0 && kf_aligned16(mask) && kf_aligned4(mask_slot))
            GS_LAUNCH(K_GATHER_ROWS, (keyframe_encode_kernel<1, true>), quads, block, 0, s, N, mask, mask_slot);
        else
            GS_LAUNCH(K_GATHER_ROWS, (keyframe_encode_kernel<1, false>), pixels, block, 0, s, N, mask, mask_slot);
    }
    return GSLIC_OK;
}

}  // namespace gslic
