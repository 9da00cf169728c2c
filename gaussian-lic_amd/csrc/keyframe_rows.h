// keyframe_rows.h — what the keyframe store's two modules share (keyframes.hip: the colour and mask slabs; keyframes_depth.hip: the depth slabs):
// the workgroup size, the aligned non-temporal row loader of the four-pixel paths, the byte quantiser of the encode rule and the alignment tests.
#pragma once
#include "gslic_common.h"

namespace gslic {

static constexpr int KF_THREADS = 256;

typedef uint32_t kf_u2 __attribute__((ext_vector_type(2)));
typedef uint32_t kf_u4 __attribute__((ext_vector_type(4)));

// the CH << L dwords of one source row of a group (4 << L pixels of CH bytes), at an address aligned to min(16, 4 << L) bytes
template <int L, int CH>
__device__ __forceinline__ void kf_load_row(const uint8_t* __restrict__ p, uint32_t (&w)[CH << L])
{
    constexpr int ND = CH << L;
    if constexpr (L == 0) {
#pragma unroll
        for (int k = 0; k < ND; k++) w[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p) + k);
    } else if constexpr (L == 1) {
#pragma unroll
        for (int k = 0; k < ND / 2; k++) {
            const kf_u2 v = __builtin_nontemporal_load(reinterpret_cast<const kf_u2*>(p) + k);
            w[2 * k] = v.x; w[2 * k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < ND / 4; k++) {
            const kf_u4 v = __builtin_nontemporal_load(reinterpret_cast<const kf_u4*>(p) + k);
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    }
}

// q = (uint8) floorf(x' * 255 + 0.5), x' = x clamped to [0, 1] with NaN -> 0 (saturate_f); the product rounded on its own
__device__ __forceinline__ uint32_t kf_quantise(float x)
{
#pragma clang fp contract(off)
    const float p = __fmul_rn(saturate_f(x), 255.0f);
    return (uint32_t)floorf(p + 0.5f);
}

static bool kf_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static bool kf_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }   // a slot of a 16-byte aligned slab when N % 4 == 0

}  // namespace gslic
