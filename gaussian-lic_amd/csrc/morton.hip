// morton.hip — keeping the map's rows in Morton order on the device: gslic_morton_order (which old row becomes row s) and
// gslic_permute_rows (every per-row array re-ordered in place through a staging buffer).  The reference has no counterpart (its rows stay in
// insertion order); a LibTorch host writes it as ten elementwise int64 kernels, torch.sort and 19 index + copy round trips.  Here:
//   morton_key_kernel   one thread per row: the key rule of include/gslic_hip.h — every step ONE float32 operation rounded on its own (this file is
//                       built with -ffp-contract=off and a true division), so a numpy float32 transcription gives the same keys bit for bit
//   radix_sort_u32      (radix_sort.hip) the stable argsort over the 30 key bits; its ping-pong is arranged so that the LAST pass writes the
//                       caller's perm (and keys_sorted) directly: nothing is copied afterwards
//   row_ops_kernel      (row_ops.hip, through prune.hip's gather_rows) staging_a[s, :] = a[perm[s], :] for every array in one launch
//   hipMemcpyAsync      the way back, staging -> arrays: one device-to-device copy per array on the stream (measured faster than the one-launch
//                       copy below: DESIGN.md §8)
//   row_copy_kernel     the same way back as ONE launch with the gather's grid cut (a workgroup owns one contiguous run of about 4096 dwords of
//                       one array): kept for the A/B, GSLIC_PERMUTE_COPY=kernel
// The key kernel is booked under the prune_select class and the copy under gather_rows, as densify.hip books its launches (no profiler id of
// their own); the sort under sort_hist / sort_scatter.  No atomics, no stream synchronisation, no host read-back.
#include "gslic_common.h"
#include "kernels.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace gslic {

__device__ __forceinline__ uint32_t spread10(uint32_t x)   // 10 bits -> every third bit (knn.hip's prep_morton)
{
    x = (x | (x << 16)) & 0x030000FF;
    x = (x | (x << 8)) & 0x0300F00F;
    x = (x | (x << 4)) & 0x030C30C3;
    x = (x | (x << 2)) & 0x09249249;
    return x;
}

__global__ __launch_bounds__(256) void morton_key_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ box,
                                                         uint32_t* __restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint32_t c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float lo = box[k], hi = box[3 + k];
        const float ext = hi - lo;
        const float d = (ext > 1e-30f) ? ext : 1e-30f;               // max(hi - lo, 1e-30f); a NaN extent (inf - inf) reads as 1e-30f
        const float t = (xyz[3 * (size_t)i + k] - lo) / d;
        const float cl = (t > 0.0f) ? ((t < 1.0f) ? t : 1.0f) : 0.0f;   // min(max(t, 0), 1); NaN -> 0
        c[k] = spread10((uint32_t)(cl * 1023.0f));                  // 0 <= cl * 1023 <= 1023: the cast truncates
    }
    keys[i] = c[0] | (c[1] << 1) | (c[2] << 2);
}

int morton_order(int P, const float* xyz, const float* box, gslic_alloc_fn alloc, void* ctx, uint32_t* perm, uint32_t* keys_sorted, hipStream_t s)
{
    const size_t n = (size_t)P;
    const SortPlan plan = sort_plan(n, 30);
    const int out = plan.passes & 1;   // the side the sort's result lands on: the caller's arrays stand there
    size_t bytes;
    {
        Carver c(nullptr);
        c.take<uint32_t>(n); c.take<uint32_t>(n); c.take<uint32_t>(n);
        c.take<char>(sort_scratch_bytes(plan));
        bytes = c.used(nullptr) + 256;
    }
    char* base = alloc(ctx, bytes);
    if (!base) return set_error(GSLIC_ERR_ALLOC, "morton order scratch allocator returned NULL for %zu bytes", bytes);
    Carver c(base);
    uint32_t* const keys_other = c.take<uint32_t>(n);
    uint32_t* const vals_other = c.take<uint32_t>(n);
    uint32_t* const keys_own = c.take<uint32_t>(n);     // stands in for keys_sorted when the caller wants none
    void* const sort_scratch = c.take<char>(sort_scratch_bytes(plan));
    SortBuffers sb;
    sb.keys[out] = keys_sorted ? keys_sorted : keys_own; sb.keys[out ^ 1] = keys_other;
    sb.v0[out] = perm; sb.v0[out ^ 1] = vals_other;
    sb.v1[0] = sb.v1[1] = nullptr; sb.v2[0] = sb.v2[1] = nullptr;
    sb.v0_identity = true;             // pass 0 takes the row index as the payload: v0[0] is written before it is ever read
    GS_LAUNCH(K_PRUNE_SELECT, morton_key_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, xyz, box, sb.keys[0]);
    return radix_sort_u32(sb, plan, sort_scratch, false, K_SORT_HIST, K_SORT_SCATTER, s);
}

// ---------------------------------------------------------------------------------------------------------
// The copy back.  The argument block is a gather's (row_ops_add cut the grid): src[k] is the staging run of array k, dst[k] the array; the
// index is not read.  A workgroup's rows are one contiguous run of dwords on both sides.
__global__ __launch_bounds__(256) void row_copy_kernel(const RowOpsArgs a)
{
    int k = 0;
    while (k < a.n_segments - 1 && blockIdx.x >= a.block_end[k]) k++;   // (wave-uniform: scalar loads of the argument block)
    const uint32_t first = k ? a.block_end[k - 1] : 0u;
    const uint32_t rpb = a.rows_per_block[k];
    const uint32_t row0 = (blockIdx.x - first) * rpb;
    if (row0 >= a.n_rows) return;
    const uint32_t rows = min(rpb, a.n_rows - row0);
    const uint32_t w = a.width[k];
    const size_t total = (size_t)rows * w;                  // about 4096 dwords; one row of any width when it is wider than that
    const uint32_t* __restrict__ const in = a.src[k] + (size_t)row0 * w;
    uint32_t* __restrict__ const out = a.dst[k] + (size_t)row0 * w;
#pragma unroll 4
    for (size_t e = threadIdx.x; e < total; e += 256) __builtin_nontemporal_store(__builtin_nontemporal_load(in + e), out + e);
}

size_t permute_rows_bytes(const gslic_row_array* arrays, int n_arrays, int n_rows)
{
    size_t bytes = 0;
    for (int i = 0; i < n_arrays; i++) bytes += (size_t)arrays[i].row_dwords * sizeof(uint32_t) * (size_t)n_rows;
    return bytes;
}

// GSLIC_PERMUTE_COPY=kernel: the way back as the one copy launch instead of one hipMemcpyAsync per array (the A/B of DESIGN.md §8; same result).
// Read at every call, so that one process can alternate the two (tools/resort_probe.py).
static bool copy_back_by_kernel()
{
    const char* e = getenv("GSLIC_PERMUTE_COPY");
    return e && !strcmp(e, "kernel");
}

int permute_rows(const gslic_row_array* arrays, int n_arrays, const uint32_t* perm, int n_rows, void* staging, hipStream_t s)
{
    // array i's rows go to staging + sum over j < i of row_dwords_j * 4 * n_rows: dword aligned, which is all the row kernels ask for
    std::vector<gslic_row_array> out((size_t)n_arrays);
    char* at = static_cast<char*>(staging);
    for (int i = 0; i < n_arrays; i++) {
        out[i].src = arrays[i].dst;
        out[i].dst = at;
        out[i].row_dwords = arrays[i].row_dwords;
        at += (size_t)arrays[i].row_dwords * sizeof(uint32_t) * (size_t)n_rows;
    }
    GS_TRY(gather_rows(out.data(), n_arrays, perm, n_rows, s));
    if (!copy_back_by_kernel()) {
        for (int i = 0; i < n_arrays; i++)
            if (out[i].row_dwords)
                GS_HIP(hipMemcpyAsync(arrays[i].dst, out[i].dst, (size_t)out[i].row_dwords * sizeof(uint32_t) * (size_t)n_rows, hipMemcpyDeviceToDevice, s));
        return GSLIC_OK;
    }
    int done = 0;
    while (done < n_arrays) {   // (the map has 19 arrays: one launch, as in gather_rows)
        RowOpsArgs a{};
        a.n_rows = (uint32_t)n_rows;
        for (; done < n_arrays && a.n_segments < ROW_OPS_MAX_SEGMENTS; done++)
            if (!row_ops_add(a, out[done].dst, arrays[done].dst, out[done].row_dwords))
                return set_error(GSLIC_ERR_INVALID_ARG, "permute rows: too many rows for one launch");
        a.n_copy = a.n_segments;
        if (a.n_segments == 0) continue;
        GS_LAUNCH(K_GATHER_ROWS, row_copy_kernel, dim3(a.block_end[a.n_segments - 1]), dim3(256), 0, s, a);
    }
    return GSLIC_OK;
}

}  // namespace gslic
