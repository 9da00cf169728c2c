// row_ops.hip — the one segmented row kernel of the map edits: gslic_gather_rows and the wide launch of gslic_densify_emit.
// A launch serves up to ROW_OPS_MAX_SEGMENTS segments, one per row array of any width, over the same n_rows destination rows and one index:
//   copy segment   dst[row, :] = src[index[row], :]
//   zero segment   dst[row, :] = 0, and src[index[row], :] = 0 as well when the row of `scaling` at index[row] has a component above split_above
//                  (the Adam moments of a densification's new rows and of its split parents)
// The work is cut along the DESTINATION: a workgroup owns `rows_per_block` consecutive destination rows of one segment, i.e. one contiguous run
// of about ROW_OPS_CHUNK dwords, and its lanes walk that run dword by dword — every wave-instruction stores 256 contiguous bytes (the shape that
// streams at the plain-store rate on this part), and reads 256 bytes that are contiguous inside a source row and, for the ascending index of a
// compaction, mostly across rows too.  A 45-dword row is read by 45 neighbouring lanes, never by one lane looping over it.  The row of a dword
// is (local dword) / width: a 32-bit division by a compile-time constant for the widths the map has (1, 3, 4, 45).
// Which segment a workgroup serves and whether it copies or zeroes are decided from blockIdx and the argument block alone: scalar loads and
// branches.  No atomics: a destination dword has one writer, and a split parent's row of an array is zeroed by the threads that own its new row.
#include "gslic_common.h"
#include "kernels.h"
#include "row_rules.h"

namespace gslic {

static constexpr uint32_t ROW_OPS_CHUNK = 4096;   // destination dwords per workgroup: 16 per thread

// The copy of one chunk, compiled twice per width and chosen by a scalar branch: without the test (src_rows = 0xffffffff, the gather) its index
// loads and then its row loads go out four at a time; a conditional store between them (the densification) keeps every load behind that store.
template <uint32_t W, bool GUARDED>
__device__ __forceinline__ void copy_rows(const uint32_t* __restrict__ src, uint32_t* __restrict__ out, const uint32_t* __restrict__ index,
                                          uint32_t width, uint32_t row0, uint32_t total, uint32_t src_rows)
{
    const uint32_t w = W ? W : width;
#pragma unroll 4
    for (uint32_t e = threadIdx.x; e < total; e += 256) {
        const uint32_t r = e / w, col = e - r * w;
        const uint32_t p = index[row0 + r];
        if (GUARDED && p >= src_rows) continue;   // (an index outside the source is never an address)
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + (size_t)p * w + col), out + e);
    }
}

template <uint32_t W>   // W = 0: the width is a run-time value
__device__ __forceinline__ void row_run(const RowOpsArgs& a, uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                        const uint32_t* __restrict__ index, bool copy, uint32_t width, uint32_t row0, uint32_t rows)
{
    const uint32_t w = W ? W : width;
    uint32_t* const out = dst + (size_t)row0 * w;
    if ((size_t)rows * w <= ROW_OPS_CHUNK) {
        const uint32_t total = rows * w;          // <= ROW_OPS_CHUNK: 32-bit arithmetic throughout
        if (copy) {
            if (a.src_rows == 0xffffffffu) copy_rows<W, false>(src, out, index, w, row0, total, a.src_rows);
            else copy_rows<W, true>(src, out, index, w, row0, total, a.src_rows);
        } else {
#pragma unroll 4
            for (uint32_t e = threadIdx.x; e < total; e += 256) {
                const uint32_t r = e / w, col = e - r * w;
                const uint32_t p = index[row0 + r];
                if (p >= a.src_rows) continue;
                __builtin_nontemporal_store(0u, out + e);
                const float* const sc = a.scaling + 3 * (size_t)p;
                if (any_above(sc[0], sc[1], sc[2], a.split_above)) src[(size_t)p * w + col] = 0u;
            }
        }
    } else {
        // a row wider than ROW_OPS_CHUNK dwords (rows == 1): the lanes along the row
        const uint32_t p = index[row0];
        if (p >= a.src_rows) return;
        uint32_t* const in = src + (size_t)p * w;
        if (copy) {
            for (uint32_t col = threadIdx.x; col < w; col += 256) __builtin_nontemporal_store(__builtin_nontemporal_load(in + col), out + col);
        } else {
            const float* const sc = a.scaling + 3 * (size_t)p;
            const bool split = any_above(sc[0], sc[1], sc[2], a.split_above);
            for (uint32_t col = threadIdx.x; col < w; col += 256) {
                __builtin_nontemporal_store(0u, out + col);
                if (split) in[col] = 0u;
            }
        }
    }
}

__global__ __launch_bounds__(256) void row_ops_kernel(const RowOpsArgs a)
{
    int k = 0;
    while (k < a.n_segments - 1 && blockIdx.x >= a.block_end[k]) k++;   // (wave-uniform: scalar loads of the argument block)
    const uint32_t first = k ? a.block_end[k - 1] : 0u;
    const uint32_t rpb = a.rows_per_block[k];
    const uint32_t row0 = (blockIdx.x - first) * rpb;
    if (row0 >= a.n_rows) return;
    const uint32_t rows = min(rpb, a.n_rows - row0);
    const uint32_t w = a.width[k];
    uint32_t* const src = a.src[k];
    uint32_t* const dst = a.dst[k];
    const bool copy = k < a.n_copy;
    switch (w) {
    case 1: row_run<1>(a, src, dst, a.index, copy, w, row0, rows); break;
    case 3: row_run<3>(a, src, dst, a.index, copy, w, row0, rows); break;
    case 4: row_run<4>(a, src, dst, a.index, copy, w, row0, rows); break;
    case 45: row_run<45>(a, src, dst, a.index, copy, w, row0, rows); break;
    default: row_run<0>(a, src, dst, a.index, copy, w, row0, rows); break;
    }
}

bool row_ops_add(RowOpsArgs& a, const void* src, void* dst, uint32_t width)
{
    if (width == 0) return true;   // an empty array (features_rest at SH degree 0)
    const int k = a.n_segments++;
    a.src[k] = static_cast<uint32_t*>(const_cast<void*>(src));
    a.dst[k] = static_cast<uint32_t*>(dst);
    a.width[k] = width;
    a.rows_per_block[k] = width >= ROW_OPS_CHUNK ? 1u : ROW_OPS_CHUNK / width;
    const uint64_t blocks = (k ? a.block_end[k - 1] : 0u) + ((uint64_t)a.n_rows + a.rows_per_block[k] - 1) / a.rows_per_block[k];
    a.block_end[k] = (uint32_t)blocks;
    return blocks <= 0x7fffffffull;
}

int launch_row_ops(const RowOpsArgs& a, hipStream_t s)
{
    if (a.n_segments == 0) return GSLIC_OK;
    GS_LAUNCH(K_GATHER_ROWS, row_ops_kernel, dim3(a.block_end[a.n_segments - 1]), dim3(256), 0, s, a);
    return GSLIC_OK;
}

}  // namespace gslic
