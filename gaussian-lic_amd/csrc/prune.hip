// prune.hip — removing rows from the map on the device: which rows stay, and the compaction of every per-row array in one launch.
// The reference has no pruning at all (its map only grows: extend() appends, nothing removes); a LibTorch host would write it as 19 boolean-index
// launches with 19 temporaries (6 groups x {parameter, exp_avg, exp_avg_sq} + tie_rank).  Here:
//   prune_flag_kernel     one thread per row: the keep rule of include/gslic_hip.h on the RAW parameters (comparisons and bit tests only, so a
//                         torch expression on the same float32 thresholds reproduces it exactly); with tie_rank also the keep flag scattered to
//                         the row's ORIGINAL index
//   (u32 scans)           exclusive positions of the kept rows in storage order, and of the kept original indices in original order
//   prune_compact_kernel  kept_index[pos[i]] = i (stable), new_tie[pos[i]] = dense rank of row i's original index among the kept ones
//   row_ops_kernel        (row_ops.hip, shared with densify.hip, as are the row predicates of row_rules.h) dst_a[k, :] = src_a[index[k], :] for up to
//                         ROW_OPS_MAX_SEGMENTS row arrays of any widths in ONE launch: gather_rows() below only fills its copy segments
#include "gslic_common.h"
#include "kernels.h"
#include "row_rules.h"

namespace gslic {

__global__ __launch_bounds__(256) void prune_flag_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ dc,
                                                         const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                         const float* __restrict__ rotation, float opacity_min, float scaling_max, int drop_nonfinite,
                                                         const uint8_t* __restrict__ drop, const uint8_t* __restrict__ protect,
                                                         const uint32_t* __restrict__ tie_rank, uint32_t* __restrict__ flags,
                                                         uint32_t* __restrict__ flags_by_tie /* zeroed */)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t r = (size_t)i;
    const bool bad = drop_nonfinite && row_not_finite(xyz, dc, opacity, scaling, rotation, r);
    const bool hit = (drop && drop[r]) || (opacity[r] < opacity_min) || any_above(scaling[3 * r], scaling[3 * r + 1], scaling[3 * r + 2], scaling_max);
    const bool keep = !bad && ((protect && protect[r]) || !hit);
    flags[r] = keep ? 1u : 0u;
    if (tie_rank) {
        const uint32_t t = tie_rank[r];
        if (t < (uint32_t)P) flags_by_tie[t] = keep ? 1u : 0u;   // (tie_rank is a permutation of 0..P-1; a value outside it is never used as an address)
    }
}

__global__ __launch_bounds__(256) void prune_compact_kernel(int P, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos,
                                                            const uint32_t* __restrict__ tie_rank, const uint32_t* __restrict__ rank_by_tie,
                                                            uint32_t* __restrict__ kept_index, uint32_t* __restrict__ new_tie)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || !flags[i]) return;
    const uint32_t k = pos[i];   // < number of kept rows <= P
    kept_index[k] = (uint32_t)i;
    if (new_tie) {
        const uint32_t t = tie_rank[i];
        new_tie[k] = (t < (uint32_t)P) ? rank_by_tie[t] : 0u;
    }
}

int prune_select(int P, const float* xyz, const float* dc, const float* opacity, const float* scaling, const float* rotation, float opacity_min,
                 float scaling_max, int drop_nonfinite, const uint8_t* drop, const uint8_t* protect, const uint32_t* tie_rank, int split_row,
                 gslic_alloc_fn alloc, void* ctx, uint32_t* kept_index, uint32_t* new_tie, int32_t* count, int32_t* count_below, hipStream_t s)
{
    const bool ties = tie_rank != nullptr && new_tie != nullptr;
    const size_t n = (size_t)P;
    size_t bytes;
    {
        Carver c(nullptr);
        c.take<uint32_t>(n); c.take<uint32_t>(n); c.take<uint32_t>(scan_temp_elems(n));
        if (ties) { c.take<uint32_t>(n); c.take<uint32_t>(n); }
        bytes = c.used(nullptr) + 256;
    }
    char* base = alloc(ctx, bytes);
    if (!base) return set_error(GSLIC_ERR_ALLOC, "prune scratch allocator returned NULL for %zu bytes", bytes);
    Carver c(base);
    uint32_t* flags = c.take<uint32_t>(n);
    uint32_t* pos = c.take<uint32_t>(n);
    uint32_t* stemp = c.take<uint32_t>(scan_temp_elems(n));
    uint32_t* flags_by_tie = ties ? c.take<uint32_t>(n) : nullptr;
    uint32_t* rank_by_tie = ties ? c.take<uint32_t>(n) : nullptr;
    if (ties) GS_HIP(hipMemsetAsync(flags_by_tie, 0, n * sizeof(uint32_t), s));
    GS_LAUNCH(K_PRUNE_SELECT, prune_flag_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, xyz, dc, opacity, scaling, rotation, opacity_min, scaling_max,
              drop_nonfinite, drop, protect, ties ? tie_rank : (const uint32_t*)nullptr, flags, flags_by_tie);
    GS_TRY(scan_u32(flags, pos, n, true, stemp, s));
    if (ties) GS_TRY(scan_u32(flags_by_tie, rank_by_tie, n, true, stemp, s));   // (the same temp: the scans run one after the other on the stream)
    GS_LAUNCH(K_PRUNE_SELECT, prune_compact_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, (const uint32_t*)flags, (const uint32_t*)pos,
              ties ? tie_rank : (const uint32_t*)nullptr, (const uint32_t*)rank_by_tie, kept_index, ties ? new_tie : (uint32_t*)nullptr);
    const bool inside = split_row > 0 && split_row < P;
    uint32_t below = 0;
    GS_TRY(scan_count(pos, flags, n, s, count, inside ? pos + split_row : nullptr, &below));   // the host sizes the new storage from the count
    *count_below = split_row <= 0 ? 0 : (inside ? (int32_t)below : *count);
    return GSLIC_OK;
}

int gather_rows(const gslic_row_array* arrays, int n_arrays, const uint32_t* index, int n_rows, hipStream_t s)
{
    int done = 0;
    while (done < n_arrays) {   // (the map has 19 arrays: one launch; more are served by further launches)
        RowOpsArgs a{};
        a.n_rows = (uint32_t)n_rows;
        a.src_rows = 0xffffffffu;   // the index is the caller's to bound: no guard
        a.index = index;
        for (; done < n_arrays && a.n_segments < ROW_OPS_MAX_SEGMENTS; done++)
            if (!row_ops_add(a, arrays[done].src, arrays[done].dst, arrays[done].row_dwords))
                return set_error(GSLIC_ERR_INVALID_ARG, "gather rows: too many rows for one launch");
        a.n_copy = a.n_segments;
        GS_TRY(launch_row_ops(a, s));
    }
    return GSLIC_OK;
}

}  // namespace gslic
