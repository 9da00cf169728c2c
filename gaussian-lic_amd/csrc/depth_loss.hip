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

}  // namespace gslic
