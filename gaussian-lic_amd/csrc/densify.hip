// densify.hip — growing the map where the image is badly reconstructed: which rows clone or split, and the new rows of every per-row
// array.  The reference has no densification (its map grows from LiDAR returns only); a LibTorch host would write it as 18 index + cat launches plus
// the rewrite of the split parents.  Here:
//   densify_flag_kernel     one thread per row: the eligibility rule of include/gslic_hip.h on the RAW parameters (comparisons, bit tests and one float32 sum of squares in a stated order, so a
//                           torch expression on the same float32 threshold reproduces it exactly), scattered to the row's ORIGINAL index; the split
//                           rows are counted with one integer atomic per wave
//   (u32 scan)              rank of every eligible original index among the eligible ones
//   densify_compact_kernel  parent_index[rank of row i's original index] = i
//   row_ops_kernel          (row_ops.hip, shared with gslic_gather_rows) the WIDE part of the emission, cut along the destination: three copy
//                           segments for the copied fields of the new rows (features_dc, features_rest, opacity — fields no thread writes) and up to
//                           twelve zero segments for the moments of the new rows and of the split parents, contiguous dwords per wave, no atomics.
//                           It decides "split" from the parents' scaling, so it runs FIRST
//   densify_parent_kernel   one thread per parent, the SECOND launch: reads xyz / scaling / rotation of its parent once and writes xyz, scaling,
//                           rotation and tie of the new row and, for a split, xyz and scaling of the parent's row (child 0) — the only thread that
//                           touches those two rows of those arrays
// The row predicates and fmix32 are those of row_rules.h: the flag kernel, the zero segments and the parent kernel decide "split" by one any_above().
// The flag, compact and parent launches go through GS_LAUNCH under the prune_select class (no profiler id of their own), the wide one under gather_rows.
#include "gslic_common.h"
#include "kernels.h"
#include "row_rules.h"

namespace gslic {

__global__ __launch_bounds__(256) void densify_flag_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ dc,
                                                           const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                           const float* __restrict__ rotation, const uint8_t* __restrict__ grow,
                                                           const uint8_t* __restrict__ protect, const uint32_t* __restrict__ tie_rank, float split_above,
                                                           uint32_t* __restrict__ flags_by_tie /* zeroed when tie_rank */, uint32_t* __restrict__ n_split /* zeroed */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool eligible = false, split = false;
    if (i < P) {
        const size_t r = (size_t)i;
        const float s0 = scaling[3 * r], s1 = scaling[3 * r + 1], s2 = scaling[3 * r + 2];
        const float4 q = reinterpret_cast<const float4*>(rotation)[r];
        const bool bad = row_not_finite(xyz, dc, opacity, scaling, rotation, r);
        // |q|^2 > 0 on the float32 sum of squares densify_parent_kernel divides by (same order, products and sums rounded one by one): a quaternion
        // whose squares all underflow has no direction in float32 and is not eligible
        const bool zero_q = !((((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w) > 0.0f);
        uint32_t o = (uint32_t)i;
        if (tie_rank) o = tie_rank[r];
        eligible = grow[r] != 0 && !(protect && protect[r]) && !bad && !zero_q && o < (uint32_t)P;   // (an index outside 0..P-1 is never an address)
        split = eligible && any_above(s0, s1, s2, split_above);
        if (tie_rank) { if (eligible) flags_by_tie[o] = 1u; }
        else flags_by_tie[r] = eligible ? 1u : 0u;
    }
    const unsigned long long b = __builtin_amdgcn_ballot_w64(split);
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicAdd(n_split, (uint32_t)__builtin_popcountll(b));   // (an integer count: any order gives it)
}

__global__ __launch_bounds__(256) void densify_compact_kernel(int P, const uint32_t* __restrict__ flags_by_tie, const uint32_t* __restrict__ rank_by_tie,
                                                              const uint32_t* __restrict__ tie_rank, uint32_t* __restrict__ parent_index)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint32_t o = (uint32_t)i;
    if (tie_rank) o = tie_rank[i];
    if (o >= (uint32_t)P || !flags_by_tie[o]) return;
    parent_index[rank_by_tie[o]] = (uint32_t)i;   // rank < number of eligible rows <= P
}

int densify_select(int P, const float* xyz, const float* dc, const float* opacity, const float* scaling, const float* rotation, const uint8_t* grow,
                   const uint8_t* protect, const uint32_t* tie_rank, float split_above, gslic_alloc_fn alloc, void* ctx, uint32_t* parent_index,
                   int32_t* count, int32_t* count_split, hipStream_t s)
{
    const size_t n = (size_t)P;
    size_t bytes;
    {
        Carver c(nullptr);
        c.take<uint32_t>(n); c.take<uint32_t>(n); c.take<uint32_t>(scan_temp_elems(n)); c.take<uint32_t>(64);
        bytes = c.used(nullptr) + 256;
    }
    char* base = alloc(ctx, bytes);
    if (!base) return set_error(GSLIC_ERR_ALLOC, "densify scratch allocator returned NULL for %zu bytes", bytes);
    Carver c(base);
    uint32_t* flags_by_tie = c.take<uint32_t>(n);
    uint32_t* rank_by_tie = c.take<uint32_t>(n);
    uint32_t* stemp = c.take<uint32_t>(scan_temp_elems(n));
    uint32_t* n_split = c.take<uint32_t>(64);
    if (tie_rank) GS_HIP(hipMemsetAsync(flags_by_tie, 0, n * sizeof(uint32_t), s));
    GS_HIP(hipMemsetAsync(n_split, 0, sizeof(uint32_t), s));
    GS_LAUNCH(K_PRUNE_SELECT, densify_flag_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, xyz, dc, opacity, scaling, rotation, grow, protect, tie_rank,
              split_above, flags_by_tie, n_split);
    GS_TRY(scan_u32(flags_by_tie, rank_by_tie, n, true, stemp, s));
    GS_LAUNCH(K_PRUNE_SELECT, densify_compact_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, (const uint32_t*)flags_by_tie,
              (const uint32_t*)rank_by_tie, tie_rank, parent_index);
    uint32_t splits = 0;
    GS_TRY(scan_count(rank_by_tie, flags_by_tie, n, s, count, n_split, &splits));   // the host sizes the new rows from the count
    *count_split = (int32_t)splits;
    return GSLIC_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The counter generator of include/gslic_hip.h: keyed by the ORIGINAL index, so every rank and both row orders draw the same noise.
__device__ __forceinline__ float dn_uniform(uint32_t key, uint32_t n)   // (2 (word >> 9) + 1) 2^-24: exact, inside (0, 1)
{
    const uint32_t word = fmix32(key + 0x9E3779B9u * (n + 1u));
    return (float)(2u * (word >> 9) + 1u) * 5.9604644775390625e-08f;
}
__device__ __forceinline__ float3 dn_normal3(uint32_t key, uint32_t child)
{
    const float u0 = dn_uniform(key, 4u * child), u1 = dn_uniform(key, 4u * child + 1u), u2 = dn_uniform(key, 4u * child + 2u),
                u3 = dn_uniform(key, 4u * child + 3u);
    const float r0 = sqrtf(-2.0f * logf(u0)), r2 = sqrtf(-2.0f * logf(u2));
    float s1, c1;
    sincospif(2.0f * u1, &s1, &c1);   // (2 u is exact: cos(2 pi u), sin(2 pi u))
    return make_float3(r0 * c1, r0 * s1, r2 * cospif(2.0f * u3));
}

__global__ __launch_bounds__(256) void densify_parent_kernel(uint32_t P, uint32_t count, const uint32_t* __restrict__ parent_index, float* xyz,
                                                             float* scaling, float* rotation, uint32_t* tie_rank, float split_above, uint32_t seed_mixed)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= count) return;
    const uint32_t p = parent_index[j];
    if (p >= P) return;
    const size_t rp = (size_t)p, rn = (size_t)P + j;
    const float x0 = xyz[3 * rp], x1 = xyz[3 * rp + 1], x2 = xyz[3 * rp + 2];
    const float s0 = scaling[3 * rp], s1 = scaling[3 * rp + 1], s2 = scaling[3 * rp + 2];
    const float4 q = reinterpret_cast<const float4*>(rotation)[rp];
    reinterpret_cast<float4*>(rotation)[rn] = q;
    uint32_t o = p;
    if (tie_rank) { o = tie_rank[rp]; tie_rank[rn] = P + j; }
    const bool split = any_above(s0, s1, s2, split_above);
    if (!split) {
        xyz[3 * rn] = x0; xyz[3 * rn + 1] = x1; xyz[3 * rn + 2] = x2;
        scaling[3 * rn] = s0; scaling[3 * rn + 1] = s1; scaling[3 * rn + 2] = s2;
        return;
    }
    // R(q / |q|) of the 3DGS build_rotation (q = (r, x, y, z)), the parent's activated scales, two draws of N(0, diag(scale^2)) in the parent's frame
    const float inv = 1.0f / sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
    const float r = q.x * inv, x = q.y * inv, y = q.z * inv, z = q.w * inv;
    const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
    const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
    const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
    const float e0 = expf(s0), e1 = expf(s1), e2 = expf(s2);
    const uint32_t key = fmix32(seed_mixed ^ o);
    const float shrink = 0.4700036292457356f;   // (float)log(1.6)
    const float c0 = s0 - shrink, c1 = s1 - shrink, c2 = s2 - shrink;
#pragma unroll
    for (uint32_t child = 0; child < 2; child++) {
        const float3 n = dn_normal3(key, child);
        const float v0 = e0 * n.x, v1 = e1 * n.y, v2 = e2 * n.z;
        const size_t rc = child == 0 ? rp : rn;
        xyz[3 * rc] = x0 + ((R00 * v0 + R01 * v1) + R02 * v2);
        xyz[3 * rc + 1] = x1 + ((R10 * v0 + R11 * v1) + R12 * v2);
        xyz[3 * rc + 2] = x2 + ((R20 * v0 + R21 * v1) + R22 * v2);
        scaling[3 * rc] = c0; scaling[3 * rc + 1] = c1; scaling[3 * rc + 2] = c2;
    }
}

int densify_emit(int P, int count, const uint32_t* parent_index, int M, float* const param[6], float* const exp_avg[6], float* const exp_avg_sq[6],
                 uint32_t* tie_rank, float split_above, uint32_t seed, hipStream_t s)
{
    const uint32_t widths[6] = {3u, 3u, 3u * (uint32_t)M, 1u, 3u, 4u};   // xyz, features_dc, features_rest, opacity, scaling, rotation
    // The wide launch: src = the array, dst = its row P; a copy segment reads the parent's row, a zero segment zeroes the new row and a split parent's.
    RowOpsArgs a{};
    a.n_rows = (uint32_t)count;
    a.src_rows = (uint32_t)P;     // a parent outside the map is never an address; select writes none
    a.index = parent_index;
    a.scaling = param[4];
    a.split_above = split_above;
    bool ok = true;
    auto add = [&](float* base, uint32_t w) { ok = ok && row_ops_add(a, base, base + (size_t)P * w, w); };
    for (int g : {1, 2, 3}) add(param[g], widths[g]);   // the copied fields: no thread of either launch writes a parent's row of them
    a.n_copy = a.n_segments;
    for (int g = 0; g < 6; g++) { add(exp_avg[g], widths[g]); add(exp_avg_sq[g], widths[g]); }
    if (!ok) return set_error(GSLIC_ERR_INVALID_ARG, "densify emit: too many rows for one launch");
    // ORDER: the wide launch decides "split" from the parents' raw scaling, so it runs BEFORE densify_parent_kernel rewrites the split parents' scaling
    GS_TRY(launch_row_ops(a, s));
    // the seed is mixed once, on the host; a parent's key is fmix32(fmix32(seed) ^ original index)
    GS_LAUNCH(K_PRUNE_SELECT, densify_parent_kernel, dim3((unsigned)div_up(count, 256)), dim3(256), 0, s, (uint32_t)P, (uint32_t)count, parent_index,
              param[0], param[4], param[5], tie_rank, split_above, fmix32(seed));
    return GSLIC_OK;
}

}  // namespace gslic
