// contrib.hip — per-Gaussian contribution statistics from the lists of a completed forward (gslic_contribution_accumulate; no reference
// counterpart: the blend weight w = alpha T of a (pixel, Gaussian) pair only exists inside the blend loop).
//
// contribution_kernel: ONE WORKGROUP OF FOUR WAVES PER 16x16 TILE, thread i owns element i of the tile-major per-pixel arrays (tile_pix_x /
//   tile_pix_y: wave = 8x8 quadrant), i.e. it reads its n_contrib from pix_final[tile * 256 + i] with one coalesced load.  The tile's list is
//   walked front to back in batches of 64 entries (one record per lane of wave 0, parked in LDS, read back at a wave-uniform address); the
//   walk ends at the tile's largest n_contrib, a wave's at its quadrant's.  A pixel REPLAYS the forward's strict arithmetic (absolute pixel
//   coordinates, the products of the power rounded one by one, expf_core, min(0.99, opacity exp(power)), T (1 - alpha)) for the entries in
//   front of its n_contrib and skips power > 0 / alpha < 1/255 as the forward did: between two skipped entries nothing of the forward's
//   state is needed, and the stop at T < 1e-4 is what n_contrib records.  There is no fast-math variant (header: gslic_hip.h).
//   Per entry the wave reduces {sum w, max w, #(w >= w_min)} over its 64 pixels (butterfly: a fixed order), lane j keeps entry j's three values
//   in registers; entries no pixel of the wave blends cost the replay only.  Per batch the four waves' partials meet in LDS and wave 0 adds
//   them in wave order, so a tile's partial sum is one float formed in a fixed order; it is converted ONCE to 32.32 fixed point
//   (round to nearest) and leaves as one 64-bit integer atomic — at most one global atomic per statistic per (tile, entry), none for an entry
//   the tile does not blend.  Integer max / add / saturating add commute: the accumulators do not depend on the order in which tiles finish.
// contribution_error_kernel (gslic_contribution_accumulate_error): the same body (contrib_body.inc, CONTRIB_ERR = 1) which also reduces w e(p),
//   e = the caller's per-pixel error image clamped to [0, 4], into a fourth accumulator by the same route.
// contribution_free_space_kernel (gslic_contribution_accumulate_free_space): the same body (CONTRIB_FREE = 1) which also reduces w over the pixels
//   with a measured near bound, and over those of them the entry lies in front of (z_g < near_bound[p]), into two more accumulators by that route.
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

__device__ __forceinline__ float wave_sum_butterfly(float v)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);   // (a + b == b + a: every lane ends with the same bits)
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// n_pix[g] = min(2^32 - 1, n_pix[g] + c): below 2^31 a plain add cannot wrap (one launch adds less than 2^31 in total: the host checks
// 256 T < 2^31, and launches on one set of accumulators are ordered by their stream), above it a compare-and-swap loop saturates.  Both are
// the same function of the multiset of addends, whatever their order.
__device__ __forceinline__ void saturating_add_u32(uint32_t* p, uint32_t c)
{
    uint32_t cur = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur < 0x80000000u) { atomicAdd(p, c); return; }
    while (true) {
        const uint32_t want = cur > 0xffffffffu - c ? 0xffffffffu : cur + c;
        if (want == cur) return;
        const uint32_t seen = atomicCAS(p, cur, want);
        if (seen == cur) return;
        cur = seen;
    }
}

// e(p) of gslic_contribution_accumulate_error: err[p] clamped to [0, 4]; a negative value or a NaN reads as 0, +inf as 4
__device__ __forceinline__ float error_value(float e)
{
    return __builtin_amdgcn_fmed3f(e == e ? e : 0.0f, 0.0f, 4.0f);
}

__global__ __launch_bounds__(256) void contribution_kernel(ContribArgs a)
{
#define CONTRIB_ERR 0
#define CONTRIB_FREE 0
#include "contrib_body.inc"
#undef CONTRIB_FREE
#undef CONTRIB_ERR
}

__global__ __launch_bounds__(256) void contribution_error_kernel(ContribArgs a, const float* __restrict__ err, unsigned long long* __restrict__ err_sum)
{
#define CONTRIB_ERR 1
#define CONTRIB_FREE 0
#include "contrib_body.inc"
#undef CONTRIB_FREE
#undef CONTRIB_ERR
}

__global__ __launch_bounds__(256) void contribution_free_space_kernel(ContribArgs a, const float* __restrict__ near_bound,
                                                                      unsigned long long* __restrict__ free_sum, unsigned long long* __restrict__ meas_sum)
{
#define CONTRIB_ERR 0
#define CONTRIB_FREE 1
#include "contrib_body.inc"
#undef CONTRIB_FREE
#undef CONTRIB_ERR
}

int launch_contribution(const ContribArgs& a, hipStream_t s, const float* err, unsigned long long* err_sum, const float* near_bound,
                        unsigned long long* free_sum, unsigned long long* meas_sum)
{
    if (a.T <= 0) return GSLIC_OK;
    if ((uint64_t)a.T * GS_TILE_PIX >= 0x80000000ull) return set_error(GSLIC_ERR_INVALID_ARG, "contribution: %d tiles are more than one launch counts", a.T);
    if (free_sum) hipLaunchKernelGGL(contribution_free_space_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a, near_bound, free_sum, meas_sum);
    else if (err_sum) hipLaunchKernelGGL(contribution_error_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a, err, err_sum);
    else hipLaunchKernelGGL(contribution_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a);
    GS_HIP(hipGetLastError());
    return GSLIC_OK;
}

// geometry_images_kernel (gslic_geometry_images): the same launch geometry, staging and replay as contribution_kernel — one workgroup of four
//   waves per tile, thread i = tile-major pixel i, batches of 64 records parked in LDS (with the view depth and the row id) and read back at
//   wave-uniform addresses, a wave's walk ending at its quadrant's largest n_contrib, an entry no pixel of the wave blends skipped on a ballot —
//   but the per-pixel results STAY with the pixel: no cross-lane reduction, no LDS partials, no atomics.  Seven accumulators in registers
//   {T, A, D, zmed, found, top, wtop}; every pixel of the image stores up to seven values at the end (a NULL image is a scalar decision).
//   D = D + (z alpha) T is the strict depth forward's operation order (render_fwd_body.inc), T (1 - alpha) its transmittance: on a strict
//   forward's buffers T and D come out as that forward's final_T and depth, bit for bit.
__global__ __launch_bounds__(256) void geometry_images_kernel(GeometryArgs a)
{
#pragma clang fp contract(off)
    __shared__ float4 s_r0[GS_BUCKET];      // {mean.x, mean.y, conic.x, conic.y}
    __shared__ float2 s_r1[GS_BUCKET];      // {conic.z, opacity}
    __shared__ float s_z[GS_BUCKET];        // the entry's view depth (rec[3g + 2].y)
    __shared__ uint32_t s_gid[GS_BUCKET];
    __shared__ uint32_t s_nc[4];
    if (a.status[2] != 0u) return;   // capacity mode: the forward's lists did not fit — nothing of it is valid, nothing is written
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint2 range = a.ranges[tile];
    if (range.y > a.R) range.y = a.R;                                   // (a list never leaves the point list: R is the exact count or the capacity)
    const uint32_t n = range.y > range.x ? range.y - range.x : 0u;
    const int px = (tile % a.gx) * GS_TILE + tile_pix_x(tid), py = (tile / a.gx) * GS_TILE + tile_pix_y(tid);
    const bool inside = px < a.W && py < a.H;
    uint32_t nc = 0u;
    if (inside) nc = __float_as_uint(a.pix_final[(size_t)tile * GS_TILE_PIX + tid].w);   // last contributor, 1-based: entries [0, nc)
    nc = nc < n ? nc : n;
    const uint32_t wnc = wave_max_u32(nc);   // this quadrant's walk ends here
    if (lane == 0) s_nc[wave] = wnc;
    __syncthreads();
    const uint32_t tnc = max(max(s_nc[0], s_nc[1]), max(s_nc[2], s_nc[3]));   // the tile's (workgroup-uniform)
    const float fx = (float)px, fy = (float)py;
    const float kL2E = GS_EXP_L2E, kCC = GS_EXP_CC;
    float T = 1.0f, A = 0.0f, D = 0.0f, zmed = 0.0f, wtop = 0.0f;
    int32_t top = -1;
    bool found = false;
    for (uint32_t base = 0; base < tnc; base += GS_BUCKET) {
        const uint32_t m = (tnc - base) < GS_BUCKET ? (tnc - base) : GS_BUCKET;
        if (tid < (int)m) {
            const uint32_t g = a.point_list[range.x + base + (uint32_t)tid];
            float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
            float z = 0.0f;
            if (g < (uint32_t)a.P) {   // (else opacity 0: never blended)
                r0 = a.rec[GS_REC_F4 * (size_t)g]; r1 = a.rec[GS_REC_F4 * (size_t)g + 1];
                z = reinterpret_cast<const float*>(a.rec + GS_REC_F4 * (size_t)g + 2)[1];   // .y alone: one dword, not a third float4
            }
            s_r0[tid] = r0; s_r1[tid] = make_float2(r1.x, r1.y); s_z[tid] = z; s_gid[tid] = g;
        }
        __syncthreads();
        if (wnc > base) {
            const uint32_t mw = (wnc - base) < m ? (wnc - base) : m;
            for (uint32_t j = 0; j < mw; j++) {
                const float4 e0 = s_r0[j];
                const float2 e1 = s_r1[j];
                // contrib_body.inc's replay, line for line
                const float dxs = e0.x - fx, dys = e0.y - fy;
                const float s2 = (e0.z * dxs) * dxs + (e1.x * dys) * dys;
                const float power = __builtin_fmaf(-0.5f, s2, -((e0.w * dxs) * dys));
                const float alpha = __builtin_amdgcn_fmed3f(e1.y * expf_core(power, kL2E, kCC), -__builtin_inff(), 0.99f);
                const bool hit = (base + j < nc) & !(power > 0.0f) & !(alpha < 1.0f / 255.0f);
                if (!__builtin_amdgcn_ballot_w64(hit)) continue;   // wave-uniform: no pixel of the quadrant blends this entry
                if (hit) {
                    const float z = s_z[j];
                    const float w = alpha * T;
                    D = D + (z * alpha) * T;
                    A = A + w;
                    if (w > wtop) { wtop = w; top = (int32_t)s_gid[j]; }   // strict >: the frontmost wins a tie
                    T = T * (1.0f - alpha);
                    if (!found && T < 0.5f) { zmed = z; found = true; }     // the entry whose blending takes T below one half
                }
            }
        }
        __syncthreads();   // (the next batch is staged over this one)
    }
    if (!inside) return;
    const size_t pid = (size_t)py * a.W + px;
    if (a.transmittance) a.transmittance[pid] = T;
    if (a.opacity) a.opacity[pid] = A;
    if (a.depth_sum) a.depth_sum[pid] = D;
    if (a.depth_norm) a.depth_norm[pid] = A >= a.a_min ? D / A : 0.0f;   // one IEEE float32 division
    if (a.depth_median) a.depth_median[pid] = zmed;
    if (a.top_row) a.top_row[pid] = top;
    if (a.top_weight) a.top_weight[pid] = wtop;
}

// P == 0 or R == 0: no list exists — the rule's initial values for every pixel, the forward's buffers are not read
__global__ __launch_bounds__(256) void geometry_images_empty_kernel(GeometryArgs a)
{
    const size_t pid = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pid >= (size_t)a.W * a.H) return;
    if (a.transmittance) a.transmittance[pid] = 1.0f;
    if (a.opacity) a.opacity[pid] = 0.0f;
    if (a.depth_sum) a.depth_sum[pid] = 0.0f;
    if (a.depth_norm) a.depth_norm[pid] = 0.0f;
    if (a.depth_median) a.depth_median[pid] = 0.0f;
    if (a.top_row) a.top_row[pid] = -1;
    if (a.top_weight) a.top_weight[pid] = 0.0f;
}

int launch_geometry_images(const GeometryArgs& a, bool lists, hipStream_t s)
{
    if (a.T <= 0) return GSLIC_OK;
    if ((uint64_t)a.T * GS_TILE_PIX >= 0x80000000ull) return set_error(GSLIC_ERR_INVALID_ARG, "geometry images: %d tiles are more than one launch covers", a.T);
    if (lists) hipLaunchKernelGGL(geometry_images_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(geometry_images_empty_kernel, dim3((unsigned)(((size_t)a.W * a.H + 255) / 256)), dim3(256), 0, s, a);
    GS_HIP(hipGetLastError());
    return GSLIC_OK;
}

}  // namespace gslic
