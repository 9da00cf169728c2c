// row_rules.h — the per-row predicates of the map edits, written once: the flag kernels of prune and densify, densify_parent_kernel
// and the zero segments of row_ops_kernel must agree on them exactly (the two launches of an emission each decide "split" on their own).
#pragma once
#include <hip/hip_runtime.h>

namespace gslic {

__device__ __forceinline__ bool not_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u; }   // +-inf or NaN

// some of the 14 floats the rules look at is not finite (features_rest is not scanned): opacity, scaling, rotation, then xyz[j], features_dc[j]
__device__ __forceinline__ bool row_not_finite(const float* __restrict__ xyz, const float* __restrict__ dc, const float* __restrict__ opacity,
                                               const float* __restrict__ scaling, const float* __restrict__ rotation, size_t r)
{
    const float4 q = reinterpret_cast<const float4*>(rotation)[r];
    bool bad = not_finite(opacity[r]) || not_finite(scaling[3 * r]) || not_finite(scaling[3 * r + 1]) || not_finite(scaling[3 * r + 2]) ||
               not_finite(q.x) || not_finite(q.y) || not_finite(q.z) || not_finite(q.w);
#pragma unroll
    for (int j = 0; j < 3; j++) bad = bad || not_finite(xyz[3 * r + j]) || not_finite(dc[3 * r + j]);
    return bad;
}

// some raw scaling strictly above the threshold: "too large" of the prune rule, "split" of the densify rule (a row at the threshold clones)
__device__ __forceinline__ bool any_above(float s0, float s1, float s2, float thr) { return (s0 > thr) || (s1 > thr) || (s2 > thr); }

// the 32-bit finaliser of the counter generator (include/gslic_hip.h): the host mixes the seed with it once, the device every key
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

}  // namespace gslic
