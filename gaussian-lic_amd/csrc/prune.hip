// prune.hip — removing rows from the map on the device: which rows stay, and the compaction of every per-row array in one launch.
// The reference has no pruning at all (its map only grows: extend() appends, nothing removes); a LibTorch host would write it as 19 boolean-index
// launches with 19 temporaries (6 groups x {parameter, exp_avg, exp_avg_sq} + tie_rank).  Here:
//   prune_flag_kernel     one thread per row: the keep rule of include/gslic_hip.h on the RAW parameters (comparisons and bit tests only, so a
//                         torch expression on the same float32 thresholds reproduces it exactly); with tie_rank also the keep flag scattered to
//                         the row's ORIGINAL index
//   (u32 scans)           exclusive positions of the kept rows in storage order, and of the kept original indices in original order
//   prune_compact_kernel  kept_index[pos[i]] = i (stable), new_tie[pos[i]] = dense rank of row i's original index among the kept ones
//   gather_rows_kernel    dst_a[k, :] = src_a[index[k], :] for up to GATHER_MAX_ARRAYS row arrays of any widths in ONE launch
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

__device__ __forceinline__ bool not_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u; }   // +-inf or NaN

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
    const float o = opacity[r];
    const float s0 = scaling[3 * r], s1 = scaling[3 * r + 1], s2 = scaling[3 * r + 2];
    bool bad = false;
    if (drop_nonfinite) {
        const float4 q = reinterpret_cast<const float4*>(rotation)[r];
        bad = not_finite(o) || not_finite(s0) || not_finite(s1) || not_finite(s2) || not_finite(q.x) || not_finite(q.y) || not_finite(q.z) || not_finite(q.w);
#pragma unroll
        for (int j = 0; j < 3; j++) bad = bad || not_finite(xyz[3 * r + j]) || not_finite(dc[3 * r + j]);
    }
    const bool hit = (drop && drop[r]) || (o < opacity_min) || (s0 > scaling_max) || (s1 > scaling_max) || (s2 > scaling_max);
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
    uint32_t last[3] = {0, 0, 0};
    GS_HIP(hipMemcpyAsync(&last[0], pos + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipMemcpyAsync(&last[1], flags + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (split_row > 0 && split_row < P) GS_HIP(hipMemcpyAsync(&last[2], pos + split_row, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));  // the host sizes the new storage from the count: the call's one synchronisation
    *count = (int32_t)(last[0] + last[1]);
    *count_below = split_row <= 0 ? 0 : (split_row < P ? (int32_t)last[2] : *count);
    return GSLIC_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Row gather.  The work is cut along the DESTINATION: a workgroup owns `rows_per_block` consecutive destination rows of one array, i.e. one
// contiguous run of about GATHER_CHUNK dwords, and its lanes walk that run dword by dword — every wave-instruction stores 256 contiguous bytes
// (the shape that streams at the plain-store rate on this part), and reads 256 bytes that are contiguous inside a source row and, for the ascending
// index of a compaction, mostly across rows too.  A 45-dword row is read by 45 neighbouring lanes, never by one lane looping over it.
// The row of a dword is (local dword) / width: a 32-bit division by a compile-time constant for the widths the map has (1, 3, 4, 45).
static constexpr int GATHER_MAX_ARRAYS = 32;      // arrays per launch (the map has 19); more are served by further launches
static constexpr uint32_t GATHER_CHUNK = 4096;    // destination dwords per workgroup: 16 per thread
struct GatherArgs {
    const uint32_t* src[GATHER_MAX_ARRAYS];
    uint32_t* dst[GATHER_MAX_ARRAYS];
    uint32_t width[GATHER_MAX_ARRAYS];            // dwords per row (> 0)
    uint32_t rows_per_block[GATHER_MAX_ARRAYS];   // max(1, GATHER_CHUNK / width)
    uint32_t block_end[GATHER_MAX_ARRAYS];        // exclusive end of the array's workgroups in the grid
    int n_arrays;
    uint32_t n_rows;
};

template <uint32_t W>   // W = 0: the width is a run-time value
__device__ __forceinline__ void gather_run(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint32_t* __restrict__ index,
                                           uint32_t width, uint32_t row0, uint32_t rows)
{
    const uint32_t w = W ? W : width;
    uint32_t* const out = dst + (size_t)row0 * w;
    if ((size_t)rows * w <= GATHER_CHUNK) {
        const uint32_t total = rows * w;          // <= GATHER_CHUNK: 32-bit arithmetic throughout
#pragma unroll 4
        for (uint32_t e = threadIdx.x; e < total; e += 256) {
            const uint32_t r = e / w, col = e - r * w;
            const uint32_t v = __builtin_nontemporal_load(src + (size_t)index[row0 + r] * w + col);
            __builtin_nontemporal_store(v, out + e);
        }
    } else {
        // a row wider than GATHER_CHUNK dwords (rows == 1): the lanes along the row
        const uint32_t* const in = src + (size_t)index[row0] * w;
        for (uint32_t col = threadIdx.x; col < w; col += 256) __builtin_nontemporal_store(__builtin_nontemporal_load(in + col), out + col);
    }
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const GatherArgs a, const uint32_t* __restrict__ index)
{
    int k = 0;
    while (k < a.n_arrays - 1 && blockIdx.x >= a.block_end[k]) k++;   // (wave-uniform: scalar loads of the argument block)
    const uint32_t first = k ? a.block_end[k - 1] : 0u;
    const uint32_t rpb = a.rows_per_block[k];
    const uint32_t row0 = (blockIdx.x - first) * rpb;
    if (row0 >= a.n_rows) return;
    const uint32_t rows = min(rpb, a.n_rows - row0);
    const uint32_t w = a.width[k];
    const uint32_t* const src = a.src[k];
    uint32_t* const dst = a.dst[k];
    switch (w) {
    case 1: gather_run<1>(src, dst, index, w, row0, rows); break;
    case 3: gather_run<3>(src, dst, index, w, row0, rows); break;
    case 4: gather_run<4>(src, dst, index, w, row0, rows); break;
    case 45: gather_run<45>(src, dst, index, w, row0, rows); break;
    default: gather_run<0>(src, dst, index, w, row0, rows); break;
    }
}

int gather_rows(const gslic_row_array* arrays, int n_arrays, const uint32_t* index, int n_rows, hipStream_t s)
{
    int done = 0;
    while (done < n_arrays) {
        GatherArgs g;
        g.n_arrays = 0;
        g.n_rows = (uint32_t)n_rows;
        uint64_t blocks = 0;
        for (; done < n_arrays && g.n_arrays < GATHER_MAX_ARRAYS; done++) {
            const gslic_row_array& r = arrays[done];
            if (r.row_dwords == 0) continue;   // an empty array (features_rest at SH degree 0)
            const int k = g.n_arrays++;
            g.src[k] = static_cast<const uint32_t*>(r.src);
            g.dst[k] = static_cast<uint32_t*>(r.dst);
            g.width[k] = r.row_dwords;
            g.rows_per_block[k] = r.row_dwords >= GATHER_CHUNK ? 1u : GATHER_CHUNK / r.row_dwords;
            blocks += ((uint64_t)n_rows + g.rows_per_block[k] - 1) / g.rows_per_block[k];
            if (blocks > 0x7fffffffull) return set_error(GSLIC_ERR_INVALID_ARG, "gather rows: too many rows for one launch");
            g.block_end[k] = (uint32_t)blocks;
        }
        if (g.n_arrays == 0) continue;
        for (int k = g.n_arrays; k < GATHER_MAX_ARRAYS; k++) { g.src[k] = nullptr; g.dst[k] = nullptr; g.width[k] = 0; g.rows_per_block[k] = 0; g.block_end[k] = 0; }
        GS_LAUNCH(K_GATHER_ROWS, gather_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, g, index);
    }
    return GSLIC_OK;
}

}  // namespace gslic
