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

__global__ __launch_bounds__(256) void contribution_kernel(ContribArgs a)
{
#pragma clang fp contract(off)
    __shared__ float4 s_r0[GS_BUCKET];      // {mean.x, mean.y, conic.x, conic.y}
    __shared__ float2 s_r1[GS_BUCKET];      // {conic.z, opacity}
    __shared__ uint32_t s_gid[GS_BUCKET];
    __shared__ float s_sum[4][GS_BUCKET];
    __shared__ uint32_t s_max[4][GS_BUCKET];
    __shared__ uint32_t s_cnt[4][GS_BUCKET];
    __shared__ uint32_t s_nc[4];
    if (a.status[2] != 0u) return;   // capacity mode: the forward's lists did not fit — nothing of it is valid (the rule of the backward)
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint2 range = a.ranges[tile];
    if (range.y > a.R) range.y = a.R;                                   // (a list never leaves the point list: R is the exact count or the capacity)
    const uint32_t n = range.y > range.x ? range.y - range.x : 0u;
    const int px = (tile % a.gx) * GS_TILE + tile_pix_x(tid), py = (tile / a.gx) * GS_TILE + tile_pix_y(tid);
    uint32_t nc = 0u;
    if (px < a.W && py < a.H) nc = __float_as_uint(a.pix_final[(size_t)tile * GS_TILE_PIX + tid].w);   // last contributor, 1-based: entries [0, nc)
    nc = nc < n ? nc : n;
    const uint32_t wnc = wave_max_u32(nc);   // this quadrant's walk ends here
    if (lane == 0) s_nc[wave] = wnc;
    __syncthreads();
    const uint32_t tnc = max(max(s_nc[0], s_nc[1]), max(s_nc[2], s_nc[3]));   // the tile's (workgroup-uniform)
    const float fx = (float)px, fy = (float)py;
    const float kL2E = GS_EXP_L2E, kCC = GS_EXP_CC;
    float T = 1.0f;
    for (uint32_t base = 0; base < tnc; base += GS_BUCKET) {
        const uint32_t m = (tnc - base) < GS_BUCKET ? (tnc - base) : GS_BUCKET;
        if (tid < (int)m) {
            const uint32_t g = a.point_list[range.x + base + (uint32_t)tid];
            float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
            if (g < (uint32_t)a.P) { r0 = a.rec[GS_REC_F4 * (size_t)g]; r1 = a.rec[GS_REC_F4 * (size_t)g + 1]; }   // (else opacity 0: never blended)
            s_r0[tid] = r0; s_r1[tid] = make_float2(r1.x, r1.y); s_gid[tid] = g;
        }
        __syncthreads();
        float esum = 0.0f;
        uint32_t emax = 0u, ecnt = 0u;   // lane j: entry base + j of this wave's quadrant
        if (wnc > base) {
            const uint32_t mw = (wnc - base) < m ? (wnc - base) : m;
            for (uint32_t j = 0; j < mw; j++) {
                const float4 e0 = s_r0[j];
                const float2 e1 = s_r1[j];
                // forward.cu:424-445 as render_fwd_body.inc's STRICT branch evaluates it
                const float dxs = e0.x - fx, dys = e0.y - fy;
                const float s2 = (e0.z * dxs) * dxs + (e1.x * dys) * dys;
                const float power = __builtin_fmaf(-0.5f, s2, -((e0.w * dxs) * dys));
                const float alpha = __builtin_amdgcn_fmed3f(e1.y * expf_core(power, kL2E, kCC), -__builtin_inff(), 0.99f);
                const bool hit = (base + j < nc) & !(power > 0.0f) & !(alpha < 1.0f / 255.0f);
                if (!__builtin_amdgcn_ballot_w64(hit)) continue;   // wave-uniform: no pixel of the quadrant blends this entry
                const float w = hit ? alpha * T : 0.0f;
                T = hit ? T * (1.0f - alpha) : T;
                const uint32_t cnt = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(hit & (w >= a.w_min)));
                const float sm = wave_sum_butterfly(w);
                const uint32_t mx = wave_max_u32(__float_as_uint(w));   // w >= 0: the bit patterns order like the values
                if (lane == (int)j) { esum = sm; emax = mx; ecnt = cnt; }
            }
        }
        s_sum[wave][lane] = esum; s_max[wave][lane] = emax; s_cnt[wave][lane] = ecnt;
        __syncthreads();
        if (wave == 0 && lane < (int)m) {
            const float sum = ((s_sum[0][lane] + s_sum[1][lane]) + s_sum[2][lane]) + s_sum[3][lane];   // fixed order; a wave that skipped adds +0
            const uint32_t mx = max(max(s_max[0][lane], s_max[1][lane]), max(s_max[2][lane], s_max[3][lane]));
            const uint32_t cnt = s_cnt[0][lane] + s_cnt[1][lane] + s_cnt[2][lane] + s_cnt[3][lane];
            const uint32_t g = s_gid[lane];
            if (mx != 0u && g < (uint32_t)a.P) {   // some pixel of the tile blended the entry (w > 0 for every blended pair)
                if (a.max_w) atomicMax(a.max_w + g, mx);
                if (a.n_pix && cnt != 0u) saturating_add_u32(a.n_pix + g, cnt);
                if (a.sum_w) {
                    const unsigned long long q = __float2ull_rn(sum * 4294967296.0f);   // <= 256 * 2^32; the scaling is exact
                    if (q != 0ull) atomicAdd(a.sum_w + g, q);
                }
            }
        }
        // (wave 0 stages the next batch behind its atomics; the other waves wait for it at the barrier above before they touch s_sum again)
    }
}

int launch_contribution(const ContribArgs& a, hipStream_t s)
{
    if (a.T <= 0) return GSLIC_OK;
    if ((uint64_t)a.T * GS_TILE_PIX >= 0x80000000ull) return set_error(GSLIC_ERR_INVALID_ARG, "contribution: %d tiles are more than one launch counts", a.T);
    hipLaunchKernelGGL(contribution_kernel, dim3((unsigned)a.T), dim3(256), 0, s, a);
    GS_HIP(hipGetLastError());
    return GSLIC_OK;
}

}  // namespace gslic
