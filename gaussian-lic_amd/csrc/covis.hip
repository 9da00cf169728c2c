// covis.hip — covisibility sets (include/gslic_hip.h, gslic_covis_*): one bit per (row, frame) in uint32 [P, Wd] rows, Wd = ceil(F / 32).
//   covis_record_kernel        one thread per row: a plain load and store of the ONE word that holds the frame's bit (replace, not OR)
//   covis_pair_counts_kernel   F <= 128 (Wd <= 4): a thread owns a row, walks its set pairs f <= g and bumps the workgroup's LDS counter of the
//                              upper triangle (33 KB at F = 128); the workgroup then adds its non-zero counters to pair[] by integer atomics
//   covis_frame_counts_kernel  any F: rows that have the frame's bit walk their set bits into F LDS counters
//   covis_row_counts_kernel    n_seen[r] = popcount(row & mask); rows with n_seen >= need walk their set bits into F LDS counters
// The queries are streaming passes over P * Wd dwords: a lane reads its row with 16-byte loads where Wd % 4 == 0 (at Wd = 4 a wave-instruction
// reads 1 KiB contiguous), the grids are capped and stride over the rows, and the only per-row divergence is the walk over the set bits.
// Every counter is an unsigned integer: the sums do not depend on the order of the adds.  Bits f >= F of a row's last word are masked off
// before they index anything.  No launch here has a profiler id of its own (the id table is pinned): plain launches.
#include "gslic_common.h"
#include "kernels.h"
#include <algorithm>

namespace gslic {

static constexpr int COVIS_THREADS = 256;
static constexpr int COVIS_MAX_BLOCKS = 2048;   // the queries stride over the rows behind this many workgroups (256 CUs x 8)
static constexpr int COVIS_PAIR_F = GSLIC_COVIS_MAX_PAIR_FRAMES;
static constexpr int COVIS_TRI = COVIS_PAIR_F * (COVIS_PAIR_F + 1) / 2;   // 8256 counters

__global__ __launch_bounds__(COVIS_THREADS) void covis_record_kernel(int row_begin, int row_end, int F, uint32_t wd, uint32_t* __restrict__ bits,
                                                                     const int32_t* __restrict__ radii, const uint8_t* __restrict__ visible,
                                                                     const int32_t* __restrict__ frame_word, const int32_t* __restrict__ skip)
{
    const int r = row_begin + (int)(blockIdx.x * (unsigned)COVIS_THREADS + threadIdx.x);
    if (r >= row_end) return;
    if (skip && skip[0] != 0) return;
    const int f = frame_word[0];
    if (f < 0 || f >= F) return;
    const bool seen = radii ? radii[r] > 0 : (visible ? visible[r] != 0 : false);
    uint32_t* const w = bits + (size_t)r * wd + ((uint32_t)f >> 5);
    const uint32_t m = 1u << (f & 31);
    *w = (*w & ~m) | (seen ? m : 0u);
}

// the valid bits of word k of a row (bits f >= F are not part of the state)
__device__ __forceinline__ uint32_t covis_word_mask(int F, uint32_t wd, uint32_t k)
{
    return (k + 1 == wd && (F & 31)) ? ((1u << (F & 31)) - 1u) : 0xffffffffu;
}

// counter of the pair f <= g in the packed upper triangle of an F x F matrix
__device__ __forceinline__ uint32_t covis_tri(uint32_t F, uint32_t f, uint32_t g) { return f * F - (f * (f - 1u)) / 2u + (g - f); }

template <int WD>
__global__ __launch_bounds__(COVIS_THREADS) void covis_pair_counts_kernel(int P, int F, bool vec, const uint32_t* __restrict__ bits,
                                                                          uint32_t* __restrict__ pair)
{
    __shared__ uint32_t tri[COVIS_TRI];
    const uint32_t n_tri = (uint32_t)F * ((uint32_t)F + 1u) / 2u;
    for (uint32_t e = threadIdx.x; e < n_tri; e += COVIS_THREADS) tri[e] = 0u;
    __syncthreads();
    for (size_t r = (size_t)blockIdx.x * COVIS_THREADS + threadIdx.x; r < (size_t)P; r += (size_t)gridDim.x * COVIS_THREADS) {
        uint32_t w[WD];
#pragma unroll
        for (int k = 0; k < WD; k++) w[k] = 0u;
        if constexpr (WD == 4) {
            if (vec) {   // (wave-uniform: an argument)
                const uint4 q = *reinterpret_cast<const uint4*>(bits + r * 4);
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
            }
        }
        if (WD != 4 || !vec) {
#pragma unroll
            for (int k = 0; k < WD; k++) w[k] = bits[r * WD + k];
        }
        w[WD - 1] &= covis_word_mask(F, WD, WD - 1);
#pragma unroll
        for (int a = 0; a < WD; a++) {
            uint32_t wa = w[a];
            while (wa) {
                const uint32_t fb = (uint32_t)__builtin_ctz(wa);
                wa &= wa - 1u;
                const uint32_t f = 32u * a + fb;
                const uint32_t base = covis_tri((uint32_t)F, f, f) - f;   // + g: the counter of (f, g)
                uint32_t m = w[a] & (0xffffffffu << fb);                  // g >= f in f's own word
                while (m) {
                    const uint32_t gb = (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                    atomicAdd(&tri[base + 32u * a + gb], 1u);
                }
#pragma unroll
                for (int b = a + 1; b < WD; b++) {
                    m = w[b];
                    while (m) {
                        const uint32_t gb = (uint32_t)__builtin_ctz(m);
                        m &= m - 1u;
                        atomicAdd(&tri[base + 32u * b + gb], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < (uint32_t)F * (uint32_t)F; e += COVIS_THREADS) {
        const uint32_t f = e / (uint32_t)F, g = e - f * (uint32_t)F;
        if (f > g) continue;
        const uint32_t c = tri[covis_tri((uint32_t)F, f, g)];
        if (!c) continue;
        atomicAdd(pair + e, c);
        if (f != g) atomicAdd(pair + (size_t)g * F + f, c);
    }
}

// Adds 1 to cnt[g] for every set bit g of the row at `row` (wd words, the last one masked): 16-byte loads where VEC
template <bool VEC>
__device__ __forceinline__ void covis_walk_row(const uint32_t* __restrict__ row, int F, uint32_t wd, uint32_t* cnt)
{
    if (VEC) {
        for (uint32_t k = 0; k < wd; k += 4) {
            const uint4 q = *reinterpret_cast<const uint4*>(row + k);
            uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                uint32_t m = w[j] & covis_word_mask(F, wd, k + j);
                while (m) {
                    const uint32_t gb = (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                    atomicAdd(&cnt[32u * (k + j) + gb], 1u);
                }
            }
        }
    } else {
        for (uint32_t k = 0; k < wd; k++) {
            uint32_t m = row[k] & covis_word_mask(F, wd, k);
            while (m) {
                const uint32_t gb = (uint32_t)__builtin_ctz(m);
                m &= m - 1u;
                atomicAdd(&cnt[32u * k + gb], 1u);
            }
        }
    }
}

// the workgroup's F counters to the output (non-zero ones only)
__device__ __forceinline__ void covis_flush(const uint32_t* cnt, int F, uint32_t* __restrict__ out)
{
    for (int g = threadIdx.x; g < F; g += COVIS_THREADS)
        if (cnt[g]) atomicAdd(out + g, cnt[g]);
}

template <bool VEC>
__global__ __launch_bounds__(COVIS_THREADS) void covis_frame_counts_kernel(int P, int F, uint32_t wd, const uint32_t* __restrict__ bits,
                                                                           const int32_t* __restrict__ frame_word, uint32_t* __restrict__ out)
{
    __shared__ uint32_t cnt[GSLIC_COVIS_MAX_FRAMES];
    const int f = frame_word[0];
    if (f < 0 || f >= F) return;   // (uniform: the whole grid leaves, out stays zero)
    for (int g = threadIdx.x; g < F; g += COVIS_THREADS) cnt[g] = 0u;
    __syncthreads();
    const uint32_t fw = (uint32_t)f >> 5, fm = 1u << (f & 31);
    for (size_t r = (size_t)blockIdx.x * COVIS_THREADS + threadIdx.x; r < (size_t)P; r += (size_t)gridDim.x * COVIS_THREADS) {
        const uint32_t* const row = bits + r * wd;
        if (row[fw] & fm) covis_walk_row<VEC>(row, F, wd, cnt);
    }
    __syncthreads();
    covis_flush(cnt, F, out);
}

template <bool VEC>
__global__ __launch_bounds__(COVIS_THREADS) void covis_row_counts_kernel(int P, int F, uint32_t wd, const uint32_t* __restrict__ bits,
                                                                         const uint32_t* __restrict__ frame_mask, int32_t* __restrict__ n_seen,
                                                                         int need, uint32_t* __restrict__ redundant)
{
    __shared__ uint32_t cnt[GSLIC_COVIS_MAX_FRAMES];
    if (redundant) {
        for (int g = threadIdx.x; g < F; g += COVIS_THREADS) cnt[g] = 0u;
        __syncthreads();
    }
    for (size_t r = (size_t)blockIdx.x * COVIS_THREADS + threadIdx.x; r < (size_t)P; r += (size_t)gridDim.x * COVIS_THREADS) {
        const uint32_t* const row = bits + r * wd;
        int n = 0;
        if (VEC) {
            for (uint32_t k = 0; k < wd; k += 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(row + k);
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    n += __popc(w[j] & covis_word_mask(F, wd, k + j) & (frame_mask ? frame_mask[k + j] : 0xffffffffu));
            }
        } else {
            for (uint32_t k = 0; k < wd; k++) n += __popc(row[k] & covis_word_mask(F, wd, k) & (frame_mask ? frame_mask[k] : 0xffffffffu));
        }
        n_seen[r] = n;
        if (redundant && n >= need) covis_walk_row<VEC>(row, F, wd, cnt);   // (the row's 128 bytes at most: an L1 hit)
    }
    if (redundant) {
        __syncthreads();
        covis_flush(cnt, F, redundant);
    }
}

#define COVIS_PLAIN_LAUNCH(kernel, grid, s, ...)                                                           \
    do {                                                                                                   \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(COVIS_THREADS), 0, s, __VA_ARGS__);                    \
        GS_HIP(hipGetLastError());                                                                         \
    } while (0)

static inline uint32_t covis_words(int F) { return (uint32_t)(F + 31) / 32u; }
static inline unsigned covis_grid(int P) { return (unsigned)std::min(div_up(P, COVIS_THREADS), COVIS_MAX_BLOCKS); }
// 16-byte loads of a row need rows that start on 16 bytes: Wd % 4 == 0 and an aligned base
static inline bool covis_vec(const uint32_t* bits, int F) { return covis_words(F) % 4u == 0 && (reinterpret_cast<uintptr_t>(bits) & 15u) == 0; }

int covis_record(int F, uint32_t* bits, const int32_t* radii, const uint8_t* visible, const int32_t* frame_word, const int32_t* skip, int row_begin,
                 int row_end, hipStream_t s)
{
    const int nrows = row_end - row_begin;
    if (nrows <= 0) return GSLIC_OK;
    COVIS_PLAIN_LAUNCH(covis_record_kernel, div_up(nrows, COVIS_THREADS), s, row_begin, row_end, F, covis_words(F), bits, radii, visible, frame_word, skip);
    return GSLIC_OK;
}

int covis_pair_counts(int P, int F, const uint32_t* bits, uint32_t* pair, hipStream_t s)
{
    GS_HIP(hipMemsetAsync(pair, 0, (size_t)F * (size_t)F * sizeof(uint32_t), s));
    if (P <= 0) return GSLIC_OK;
    const unsigned grid = covis_grid(P);
    const bool vec = covis_vec(bits, F);
    switch (covis_words(F)) {
    case 1: COVIS_PLAIN_LAUNCH(covis_pair_counts_kernel<1>, grid, s, P, F, vec, bits, pair); break;
    case 2: COVIS_PLAIN_LAUNCH(covis_pair_counts_kernel<2>, grid, s, P, F, vec, bits, pair); break;
    case 3: COVIS_PLAIN_LAUNCH(covis_pair_counts_kernel<3>, grid, s, P, F, vec, bits, pair); break;
    default: COVIS_PLAIN_LAUNCH(covis_pair_counts_kernel<4>, grid, s, P, F, vec, bits, pair); break;
    }
    return GSLIC_OK;
}

int covis_frame_counts(int P, int F, const uint32_t* bits, const int32_t* frame_word, uint32_t* out, hipStream_t s)
{
    GS_HIP(hipMemsetAsync(out, 0, (size_t)F * sizeof(uint32_t), s));
    if (P <= 0) return GSLIC_OK;
    if (covis_vec(bits, F)) COVIS_PLAIN_LAUNCH(covis_frame_counts_kernel<true>, covis_grid(P), s, P, F, covis_words(F), bits, frame_word, out);
    else COVIS_PLAIN_LAUNCH(covis_frame_counts_kernel<false>, covis_grid(P), s, P, F, covis_words(F), bits, frame_word, out);
    return GSLIC_OK;
}

int covis_row_counts(int P, int F, const uint32_t* bits, const uint32_t* frame_mask, int32_t* n_seen, int min_others, uint32_t* redundant, hipStream_t s)
{
    if (redundant) GS_HIP(hipMemsetAsync(redundant, 0, (size_t)F * sizeof(uint32_t), s));
    if (P <= 0) return GSLIC_OK;
    const int need = min_others >= 0x7fffffff ? 0x7fffffff : 1 + min_others;
    if (covis_vec(bits, F))
        COVIS_PLAIN_LAUNCH(covis_row_counts_kernel<true>, covis_grid(P), s, P, F, covis_words(F), bits, frame_mask, n_seen, need, redundant);
    else
        COVIS_PLAIN_LAUNCH(covis_row_counts_kernel<false>, covis_grid(P), s, P, F, covis_words(F), bits, frame_mask, n_seen, need, redundant);
    return GSLIC_OK;
}

}  // namespace gslic
