// densify.hip — growing the map where the image is badly reconstructed: which rows clone or split, and the new rows of every per-row
// array.  The reference has no densification (its map grows from LiDAR returns only); a LibTorch host would write it as 18 index + cat launches plus
// the rewrite of the split parents.  Here:
//   densify_flag_kernel     one thread per row: the eligibility rule of include/gslic_hip.h on the RAW parameters (comparisons, bit tests and one float32 sum of squares in a stated order, so a
//                           torch expression on the same float32 threshold reproduces it exactly), scattered to the row's ORIGINAL index; the split
//                           rows are counted with one integer atomic per wave
//   (u32 scan)              rank of every eligible original index among the eligible ones
//   densify_compact_kernel  parent_index[rank of row i's original index] = i
//   densify_rows_kernel     the WIDE part of the emission, cut along the destination like gather_rows_kernel: the copied fields of the new rows
//                           (features_dc, features_rest, opacity — fields no thread writes) and the zeroed moments of the new rows and of the split
//                           parents, contiguous dwords per wave, no atomics.  It decides "split" from the parents' scaling, so it runs FIRST
//   densify_parent_kernel   one thread per parent, the SECOND launch: reads xyz / scaling / rotation of its parent once and writes xyz, scaling,
//                           rotation and tie of the new row and, for a split, xyz and scaling of the parent's row (child 0) — the only thread that
//                           touches those two rows of those arrays
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

__device__ __forceinline__ bool dn_not_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u; }   // +-inf or NaN

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
        bool bad = dn_not_finite(opacity[r]) || dn_not_finite(s0) || dn_not_finite(s1) || dn_not_finite(s2) || dn_not_finite(q.x) || dn_not_finite(q.y) ||
                   dn_not_finite(q.z) || dn_not_finite(q.w);
#pragma unroll
        for (int j = 0; j < 3; j++) bad = bad || dn_not_finite(xyz[3 * r + j]) || dn_not_finite(dc[3 * r + j]);
        // |q|^2 > 0 on the float32 sum of squares densify_parent_kernel divides by (same order, products and sums rounded one by one): a quaternion
        // whose squares all underflow has no direction in float32 and is not eligible
        const bool zero_q = !((((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w) > 0.0f);
        uint32_t o = (uint32_t)i;
        if (tie_rank) o = tie_rank[r];
        eligible = grow[r] != 0 && !(protect && protect[r]) && !bad && !zero_q && o < (uint32_t)P;   // (an index outside 0..P-1 is never an address)
        split = eligible && ((s0 > split_above) || (s1 > split_above) || (s2 > split_above));
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
    hipLaunchKernelGGL(densify_flag_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, xyz, dc, opacity, scaling, rotation, grow, protect, tie_rank,
                       split_above, flags_by_tie, n_split);
    GS_HIP(hipGetLastError());
    GS_TRY(scan_u32(flags_by_tie, rank_by_tie, n, true, stemp, s));
    hipLaunchKernelGGL(densify_compact_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, (const uint32_t*)flags_by_tie, (const uint32_t*)rank_by_tie,
                       tie_rank, parent_index);
    GS_HIP(hipGetLastError());
    uint32_t last[3] = {0, 0, 0};
    GS_HIP(hipMemcpyAsync(&last[0], rank_by_tie + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipMemcpyAsync(&last[1], flags_by_tie + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipMemcpyAsync(&last[2], n_split, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));  // the host sizes the new rows from the count: the call's one synchronisation
    *count = (int32_t)(last[0] + last[1]);
    *count_split = (int32_t)last[2];
    return GSLIC_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The wide part.  A workgroup owns `rows_per_block` consecutive NEW rows of one array: one contiguous run of about DENSIFY_CHUNK destination
// dwords, walked dword by dword by its lanes (256 contiguous bytes per wave-instruction, as in gather_rows_kernel).  A copy segment reads the
// parent's row of the same array; a moment segment stores zeros to the new row and, when the parent splits, to the parent's row as well.
static constexpr int DENSIFY_MAX_SEGMENTS = 16;      // 3 copied arrays + 12 moment arrays (features_rest and its moments absent at SH degree 0)
static constexpr uint32_t DENSIFY_CHUNK = 4096;      // destination dwords per workgroup: 16 per thread
struct DensifyRowsArgs {
    uint32_t* arr[DENSIFY_MAX_SEGMENTS];             // base pointer of the array (row 0)
    uint32_t width[DENSIFY_MAX_SEGMENTS];            // dwords per row (> 0)
    uint32_t rows_per_block[DENSIFY_MAX_SEGMENTS];   // max(1, DENSIFY_CHUNK / width)
    uint32_t block_end[DENSIFY_MAX_SEGMENTS];        // exclusive end of the segment's workgroups in the grid
    int n_copy;                                      // segments [0, n_copy) copy, [n_copy, n_segments) zero
    int n_segments;
    uint32_t P, count;
    float split_above;
    const float* scaling;                            // [P,3] the parents' raw scaling: NOT yet rewritten when this kernel runs
    const uint32_t* parent_index;
};

__device__ __forceinline__ bool dn_splits(const float* __restrict__ scaling, uint32_t p, float split_above)
{
    const float* s = scaling + 3 * (size_t)p;
    return (s[0] > split_above) || (s[1] > split_above) || (s[2] > split_above);
}

template <uint32_t W>   // W = 0: the width is a run-time value
__device__ __forceinline__ void densify_run(const DensifyRowsArgs& a, uint32_t* __restrict__ arr, bool copy, uint32_t width, uint32_t row0, uint32_t rows)
{
    const uint32_t w = W ? W : width;
    uint32_t* const out = arr + ((size_t)a.P + row0) * w;
    if ((size_t)rows * w <= DENSIFY_CHUNK) {
        const uint32_t total = rows * w;          // <= DENSIFY_CHUNK: 32-bit arithmetic throughout
#pragma unroll 4
        for (uint32_t e = threadIdx.x; e < total; e += 256) {
            const uint32_t r = e / w, col = e - r * w;
            const uint32_t p = a.parent_index[row0 + r];
            if (p >= a.P) continue;               // (a parent outside the map is never an address; select writes none)
            if (copy) {
                __builtin_nontemporal_store(__builtin_nontemporal_load(arr + (size_t)p * w + col), out + e);
            } else {
                __builtin_nontemporal_store(0u, out + e);
                if (dn_splits(a.scaling, p, a.split_above)) arr[(size_t)p * w + col] = 0u;
            }
        }
    } else {
        // a row wider than DENSIFY_CHUNK dwords (rows == 1): the lanes along the row
        const uint32_t p = a.parent_index[row0];
        if (p >= a.P) return;
        const bool sp = !copy && dn_splits(a.scaling, p, a.split_above);
        for (uint32_t col = threadIdx.x; col < w; col += 256) {
            if (copy) out[col] = arr[(size_t)p * w + col];
            else { out[col] = 0u; if (sp) arr[(size_t)p * w + col] = 0u; }
        }
    }
}

__global__ __launch_bounds__(256) void densify_rows_kernel(const DensifyRowsArgs a)
{
    int k = 0;
    while (k < a.n_segments - 1 && blockIdx.x >= a.block_end[k]) k++;   // (wave-uniform: scalar loads of the argument block)
    const uint32_t first = k ? a.block_end[k - 1] : 0u;
    const uint32_t rpb = a.rows_per_block[k];
    const uint32_t row0 = (blockIdx.x - first) * rpb;
    if (row0 >= a.count) return;
    const uint32_t rows = min(rpb, a.count - row0);
    const uint32_t w = a.width[k];
    uint32_t* const arr = a.arr[k];
    const bool copy = k < a.n_copy;
    switch (w) {
    case 1: densify_run<1>(a, arr, copy, w, row0, rows); break;
    case 3: densify_run<3>(a, arr, copy, w, row0, rows); break;
    case 4: densify_run<4>(a, arr, copy, w, row0, rows); break;
    case 45: densify_run<45>(a, arr, copy, w, row0, rows); break;
    default: densify_run<0>(a, arr, copy, w, row0, rows); break;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The counter generator of include/gslic_hip.h: keyed by the ORIGINAL index, so every rank and both row orders draw the same noise.
__device__ __forceinline__ uint32_t dn_fmix32(uint32_t h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ float dn_uniform(uint32_t key, uint32_t n)   // (2 (word >> 9) + 1) 2^-24: exact, inside (0, 1)
{
    const uint32_t word = dn_fmix32(key + 0x9E3779B9u * (n + 1u));
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
    const bool split = (s0 > split_above) || (s1 > split_above) || (s2 > split_above);
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
    const uint32_t key = dn_fmix32(seed_mixed ^ o);
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
    DensifyRowsArgs a;
    a.n_segments = 0;
    a.P = (uint32_t)P; a.count = (uint32_t)count; a.split_above = split_above;
    a.scaling = param[4]; a.parent_index = parent_index;
    uint64_t blocks = 0;
    auto add = [&](float* base, uint32_t w) {
        if (w == 0) return true;                    // features_rest at SH degree 0
        const int k = a.n_segments++;
        a.arr[k] = reinterpret_cast<uint32_t*>(base);
        a.width[k] = w;
        a.rows_per_block[k] = w >= DENSIFY_CHUNK ? 1u : DENSIFY_CHUNK / w;
        blocks += ((uint64_t)count + a.rows_per_block[k] - 1) / a.rows_per_block[k];
        a.block_end[k] = (uint32_t)blocks;
        return blocks <= 0x7fffffffull;
    };
    bool ok = true;
    for (int g : {1, 2, 3}) ok = ok && add(param[g], widths[g]);   // the copied fields: no thread of either launch writes a parent's row of them
    a.n_copy = a.n_segments;
    for (int g = 0; g < 6; g++) ok = ok && add(exp_avg[g], widths[g]) && add(exp_avg_sq[g], widths[g]);
    if (!ok) return set_error(GSLIC_ERR_INVALID_ARG, "densify emit: too many rows for one launch");
    for (int k = a.n_segments; k < DENSIFY_MAX_SEGMENTS; k++) { a.arr[k] = nullptr; a.width[k] = 0; a.rows_per_block[k] = 0; a.block_end[k] = 0; }
    hipLaunchKernelGGL(densify_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    GS_HIP(hipGetLastError());
    // the seed is mixed once, on the host (fmix32); a parent's key is fmix32(fmix32(seed) ^ original index)
    uint32_t h = seed;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    hipLaunchKernelGGL(densify_parent_kernel, dim3((unsigned)div_up(count, 256)), dim3(256), 0, s, (uint32_t)P, (uint32_t)count, parent_index, param[0],
                       param[4], param[5], tie_rank, split_above, h);
    GS_HIP(hipGetLastError());
    return GSLIC_OK;
}

}  // namespace gslic
