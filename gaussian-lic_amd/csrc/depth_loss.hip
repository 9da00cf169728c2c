// depth_loss.hip — the masked depth L1 of LiDAR depth supervision (loss.depth_l1) and its gradient, in two launches:
//   mask = gt_depth > 0,  n = |mask|,  L_d = sum_mask |depth - gt_depth| / max(n, 1),
//   dL_ddepth = (lambda_depth / max(n, 1)) * sign(depth - gt_depth) on the mask, 0 off it (sign(0) = 0).
// That gradient is what autograd forms for lambda_depth * depth_l1(depth, gt_depth) (MulBackward: lambda, DivBackward: lambda / n as a float32
// quotient, Where / Abs backward: times sign or zero), so it is held bit for bit against it.
//
// Pass 1 (depth_loss_partials_kernel): per workgroup of DL_PIX pixels, the masked |difference| sum (fixed order: per-thread sum in pixel order, then a
// fixed shuffle tree) and the exact integer count.  Pass 2 (depth_loss_grad_kernel): every workgroup adds the counts (integers: exact in any order)
// to get n, then writes the gradient of its pixels; workgroup 0 also adds the float partial sums in a fixed order and writes L_d.  No atomics, no
// host synchronisation, no allocation: 8 + 8 + 4 = 20 bytes per pixel, graph-capturable.
#include "gslic_common.h"

namespace gslic {

static constexpr int DL_THREADS = 256;
static constexpr int DL_PER_THREAD = 8;
static constexpr int DL_PIX = DL_THREADS * DL_PER_THREAD;   // pixels per workgroup (2048: 1013 workgroups at 1920 x 1080)

__device__ __forceinline__ float dl_block_sum(float v, float* red /*[4]*/)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}
__device__ __forceinline__ uint32_t dl_block_count(uint32_t v, uint32_t* red /*[4]*/)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t r = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

// partials[2 b] = masked sum of workgroup b (float), partials[2 b + 1] = its count (uint32 bits)
__global__ __launch_bounds__(DL_THREADS) void depth_loss_partials_kernel(size_t N, const float* __restrict__ depth, const float* __restrict__ gt,
                                                                         float* __restrict__ partials)
{
    __shared__ float redf[4];
    __shared__ uint32_t redu[4];
    const size_t base = (size_t)blockIdx.x * DL_PIX + threadIdx.x;
    float d[DL_PER_THREAD], g[DL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {   // (all loads in flight before the arithmetic)
        const size_t i = base + (size_t)j * DL_THREADS;
        d[j] = i < N ? depth[i] : 0.f;
        g[j] = i < N ? gt[i] : 0.f;
    }
    float s = 0.f;
    uint32_t c = 0u;
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {
        if (g[j] > 0.f) {
            s += fabsf(d[j] - g[j]);
            c += 1u;
        }
    }
    const float bs = dl_block_sum(s, redf);
    const uint32_t bc = dl_block_count(c, redu);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = bs;
        partials[2 * (size_t)blockIdx.x + 1] = __uint_as_float(bc);
    }
}

__global__ __launch_bounds__(DL_THREADS) void depth_loss_grad_kernel(size_t N, size_t nblk, float lambda_depth, const float* __restrict__ depth,
                                                                     const float* __restrict__ gt, const float* __restrict__ partials,
                                                                     float* __restrict__ term, float* __restrict__ dL_ddepth)
{
    __shared__ float redf[4];
    __shared__ uint32_t redu[4];
    uint32_t c = 0u;
    for (size_t i = threadIdx.x; i < nblk; i += DL_THREADS) c += __float_as_uint(partials[2 * i + 1]);
    const uint32_t n = dl_block_count(c, redu);
    const float nf = (float)(n > 0u ? n : 1u);   // n.clamp_min(1).to(float32): round to nearest, as the integer-to-float conversion there
    if (blockIdx.x == 0) {
        float s = 0.f;
        for (size_t i = threadIdx.x; i < nblk; i += DL_THREADS) s += partials[2 * i];
        const float t = dl_block_sum(s, redf);
        if (threadIdx.x == 0) term[0] = t / nf;
    }
    const float w = lambda_depth / nf;
    const size_t base = (size_t)blockIdx.x * DL_PIX + threadIdx.x;
    float d[DL_PER_THREAD], g[DL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {
        const size_t i = base + (size_t)j * DL_THREADS;
        d[j] = i < N ? depth[i] : 0.f;
        g[j] = i < N ? gt[i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {
        const size_t i = base + (size_t)j * DL_THREADS;
        if (i >= N) break;
        const float diff = d[j] - g[j];
        dL_ddepth[i] = g[j] > 0.f ? (diff > 0.f ? w : (diff < 0.f ? -w : 0.f)) : 0.f;
    }
}

int64_t depth_loss_partials_count(int H, int W) { return 2 * (int64_t)div_up_sz((size_t)H * (size_t)W, DL_PIX) + 8; }

int depth_loss_forward_backward(int H, int W, float lambda_depth, const float* depth, const float* gt, float* partials, float* term, float* dL_ddepth,
                                hipStream_t s)
{
    const size_t N = (size_t)H * (size_t)W;
    const size_t nblk = div_up_sz(N, DL_PIX);
    GS_LAUNCH(K_DEPTH_LOSS, depth_loss_partials_kernel, dim3((unsigned)nblk), dim3(DL_THREADS), 0, s, N, depth, gt, partials);
    GS_LAUNCH(K_DEPTH_LOSS, depth_loss_grad_kernel, dim3((unsigned)nblk), dim3(DL_THREADS), 0, s, N, nblk, lambda_depth, depth, gt,
              (const float*)partials, term, dL_ddepth);
    return GSLIC_OK;
}

// ---- the weighted / Huber depth loss (gslic_depth_loss_weighted_forward_backward; the rule is written out in include/gslic_hip.h) ----
// The same two launches over the same DL_PIX-pixel workgroups, with the integer count replaced by the float weight sum S: pass 1 writes per
// workgroup the partials of T = sum w rho and of S (per-thread sums in pixel order, then dl_block_sum's tree); pass 2 has every workgroup add the
// S partials in one fixed order (the strided per-thread loop, then the same tree: every workgroup gets the same bits), forms k = lambda_depth / S
// and writes its pixels' gradient; workgroup 0 also adds the T partials and writes terms = [T / S, S].  12 + 12 + 4 = 28 bytes per pixel.
// WEIGHT (a weight image is given) and HUBER (delta > 0) are template parameters: with both off the arithmetic is the one of the kernels above,
// S a sum of ones (exact below 2^24 pixels), so the bits are theirs.  Every step is rounded on its own (fp contract off), as the header states.

__device__ __forceinline__ float dl_weight(float w) { return (w > 0.f && w < INFINITY) ? w : 0.f; }   // NaN, negative, +inf: 0; no clamp at 1

template <bool WEIGHT, bool HUBER>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_weighted_partials_kernel(size_t N, float delta, const float* __restrict__ depth,
                                                                                  const float* __restrict__ gt, const float* __restrict__ weight,
                                                                                  float* __restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ float redf[4];
    const size_t base = (size_t)blockIdx.x * DL_PIX + threadIdx.x;
    float d[DL_PER_THREAD], g[DL_PER_THREAD], w[DL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {   // (all loads in flight before the arithmetic)
        const size_t i = base + (size_t)j * DL_THREADS;
        d[j] = i < N ? depth[i] : 0.f;
        g[j] = i < N ? gt[i] : 0.f;
        w[j] = WEIGHT ? (i < N ? weight[i] : 0.f) : 1.f;
    }
    float t = 0.f, s = 0.f;
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {
        const float wj = WEIGHT ? dl_weight(w[j]) : 1.f;
        if (g[j] > 0.f && wj > 0.f) {
            const float a = fabsf(d[j] - g[j]);
            float rho = a;
            if (HUBER) rho = a < delta ? ((0.5f * a) * a) / delta : a - 0.5f * delta;
            t += WEIGHT ? wj * rho : rho;
            s += wj;
        }
    }
    const float bt = dl_block_sum(t, redf);
    const float bs = dl_block_sum(s, redf);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = bt;
        partials[2 * (size_t)blockIdx.x + 1] = bs;
    }
}

template <bool WEIGHT, bool HUBER>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_weighted_grad_kernel(size_t N, size_t nblk, float lambda_depth, float delta,
                                                                              const float* __restrict__ depth, const float* __restrict__ gt,
                                                                              const float* __restrict__ weight, const float* __restrict__ partials,
                                                                              float* __restrict__ terms, float* __restrict__ dL_ddepth)
{
#pragma clang fp contract(off)
    __shared__ float redf[4];
    const size_t base = (size_t)blockIdx.x * DL_PIX + threadIdx.x;
    float d[DL_PER_THREAD], g[DL_PER_THREAD], w[DL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {   // (the pixel loads are issued ahead of the partial sums they do not depend on)
        const size_t i = base + (size_t)j * DL_THREADS;
        d[j] = i < N ? depth[i] : 0.f;
        g[j] = i < N ? gt[i] : 0.f;
        w[j] = WEIGHT ? (i < N ? weight[i] : 0.f) : 1.f;
    }
    float sp = 0.f;
    for (size_t i = threadIdx.x; i < nblk; i += DL_THREADS) sp += partials[2 * i + 1];
    const float S = dl_block_sum(sp, redf);
    if (blockIdx.x == 0) {
        float tp = 0.f;
        for (size_t i = threadIdx.x; i < nblk; i += DL_THREADS) tp += partials[2 * i];
        const float T = dl_block_sum(tp, redf);
        if (threadIdx.x == 0) {
            terms[0] = S > 0.f ? T / S : 0.f;
            terms[1] = S;
        }
    }
    const float k = S > 0.f ? lambda_depth / S : 0.f;
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {
        const size_t i = base + (size_t)j * DL_THREADS;
        if (i >= N) break;
        const float wj = WEIGHT ? dl_weight(w[j]) : 1.f;
        const float kw = WEIGHT ? k * wj : k;
        const float r = d[j] - g[j];
        float v = r > 0.f ? kw : (r < 0.f ? -kw : 0.f);
        if (HUBER) {
            if (fabsf(r) < delta) v = kw * (r / delta);
        }
        dL_ddepth[i] = (g[j] > 0.f && wj > 0.f) ? v : 0.f;
    }
}

int64_t depth_loss_weighted_partials_count(int H, int W) { return 2 * (int64_t)div_up_sz((size_t)H * (size_t)W, DL_PIX) + 8; }

template <bool WEIGHT, bool HUBER>
static int depth_loss_weighted_launch(size_t N, float lambda_depth, float delta, const float* depth, const float* gt, const float* weight,
                                      float* partials, float* terms, float* dL_ddepth, hipStream_t s)
{
    const size_t nblk = div_up_sz(N, DL_PIX);
    GS_LAUNCH(K_DEPTH_LOSS, (depth_loss_weighted_partials_kernel<WEIGHT, HUBER>), dim3((unsigned)nblk), dim3(DL_THREADS), 0, s, N, delta, depth, gt,
              weight, partials);
    GS_LAUNCH(K_DEPTH_LOSS, (depth_loss_weighted_grad_kernel<WEIGHT, HUBER>), dim3((unsigned)nblk), dim3(DL_THREADS), 0, s, N, nblk, lambda_depth,
              delta, depth, gt, weight, (const float*)partials, terms, dL_ddepth);
    return GSLIC_OK;
}

int depth_loss_weighted_forward_backward(int H, int W, float lambda_depth, float delta, const float* depth, const float* gt, const float* weight,
                                         float* partials, float* terms, float* dL_ddepth, hipStream_t s)
{
    const size_t N = (size_t)H * (size_t)W;
    const bool huber = delta > 0.f;
    if (weight) {
        return huber ? depth_loss_weighted_launch<true, true>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s)
                     : depth_loss_weighted_launch<true, false>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s);
    }
    return huber ? depth_loss_weighted_launch<false, true>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s)
                 : depth_loss_weighted_launch<false, false>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s);
}

}  // namespace gslic
