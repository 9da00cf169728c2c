// depth_loss.hip — the depth loss of LiDAR depth supervision and its gradient, in two launches; one kernel pair behind both entry points.
//
// gslic_depth_loss_weighted_forward_backward (the rule is written out in include/gslic_hip.h): per-pixel weights w, a Huber threshold delta,
//   m = gt > 0 && w > 0,  S = sum_m w,  T = sum_m w rho(|depth - gt|),  terms = [T / S, S],  dL_ddepth = (lambda_depth / S) w rho'(depth - gt) on m.
// gslic_depth_l1_loss_forward_backward (loss.depth_l1) is the case without weight and threshold, where S = n = |mask| is a COUNT:
//   L_d = sum_mask |depth - gt| / max(n, 1),  dL_ddepth = (lambda_depth / max(n, 1)) * sign(depth - gt) on the mask, 0 off it (sign(0) = 0).
// That gradient is what autograd forms for lambda_depth * depth_l1(depth, gt_depth) (MulBackward: lambda, DivBackward: lambda / n as a float32
// quotient, Where / Abs backward: times sign or zero), and it is held bit for bit against it at every image size: a float sum of ones is exact
// only below 2^24 measured pixels, so the accumulator type of S is a template parameter, ACC —
//   float     the four instantiations of the weighted entry point (its header documents float partials),
//   uint32_t  the one of the plain entry point: exact for any count, stored in the partials as bits, converted once (round to nearest, as
//             n.to(float32) there); it writes term[0] only.
// Read off the code for ACC = uint32_t, WEIGHT = HUBER = false against the rule above: n == 0 gives terms[0] = +0 (the rule: 0 / 1 = +0) and a
// gradient of +0 everywhere (no pixel passes gt > 0, and the store writes the literal 0); nothing there is a product feeding a sum, so
// fp contract(off) changes nothing in it.
//
// Pass 1 (partials kernel): per workgroup of DL_PIX pixels the partials of T and of S — per-thread sums in pixel order, then block256_sum's fixed
// tree.  Pass 2 (grad kernel): every workgroup adds the S partials in one fixed order (the strided per-thread loop, then the same tree: every
// workgroup gets the same bits), forms k = lambda_depth / S and writes its pixels' gradient; workgroup 0 also adds the T partials and writes the
// terms.  No atomics, no host synchronisation, no allocation, graph-capturable: 8 + 8 + 4 = 20 bytes per pixel, 12 + 12 + 4 = 28 with a weight image.
// Every step is rounded on its own (fp contract off), as the header states.
#include "gslic_common.h"
#include <type_traits>

namespace gslic {

static constexpr int DL_THREADS = 256;
static constexpr int DL_PER_THREAD = 8;
static constexpr int DL_PIX = DL_THREADS * DL_PER_THREAD;   // pixels per workgroup (2048: 1013 workgroups at 1920 x 1080)

__device__ __forceinline__ float dl_weight(float w) { return (w > 0.f && w < INFINITY) ? w : 0.f; }   // NaN, negative, +inf: 0; no clamp at 1

// an S partial in the float scratch: the float itself, or the bits of the count
__device__ __forceinline__ float dl_to_partial(float v) { return v; }
__device__ __forceinline__ float dl_to_partial(uint32_t v) { return __uint_as_float(v); }
template <typename ACC>
__device__ __forceinline__ ACC dl_from_partial(float v)
{
    if constexpr (std::is_same<ACC, float>::value) return v;
    else return __float_as_uint(v);
}
template <typename ACC>
union DlRed { float t[4]; ACC s[4]; };   // block256_sum's LDS words, for the T sums and the S sums in turn

// partials[2 b] = the T partial of workgroup b (float), partials[2 b + 1] = its S partial (ACC)
template <typename ACC, bool WEIGHT, bool HUBER>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_weighted_partials_kernel(size_t N, float delta, const float* __restrict__ depth,
                                                                                  const float* __restrict__ gt, const float* __restrict__ weight,
                                                                                  float* __restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ DlRed<ACC> red;
    const size_t base = (size_t)blockIdx.x * DL_PIX + threadIdx.x;
    float d[DL_PER_THREAD], g[DL_PER_THREAD], w[DL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {   // (all loads in flight before the arithmetic)
        const size_t i = base + (size_t)j * DL_THREADS;
        d[j] = i < N ? depth[i] : 0.f;
        g[j] = i < N ? gt[i] : 0.f;
        w[j] = WEIGHT ? (i < N ? weight[i] : 0.f) : 1.f;
    }
    float t = 0.f;
    ACC s = 0;
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {
        const float wj = WEIGHT ? dl_weight(w[j]) : 1.f;
        if (g[j] > 0.f && wj > 0.f) {
            const float a = fabsf(d[j] - g[j]);
            float rho = a;
            if (HUBER) rho = a < delta ? ((0.5f * a) * a) / delta : a - 0.5f * delta;
            t += WEIGHT ? wj * rho : rho;
            s += (ACC)wj;
        }
    }
    const float bt = block256_sum(t, red.t);
    const ACC bs = block256_sum(s, red.s);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = bt;
        partials[2 * (size_t)blockIdx.x + 1] = dl_to_partial(bs);
    }
}

template <typename ACC, bool WEIGHT, bool HUBER>
__global__ __launch_bounds__(DL_THREADS) void depth_loss_weighted_grad_kernel(size_t N, size_t nblk, float lambda_depth, float delta,
                                                                              const float* __restrict__ depth, const float* __restrict__ gt,
                                                                              const float* __restrict__ weight, const float* __restrict__ partials,
                                                                              float* __restrict__ terms, float* __restrict__ dL_ddepth)
{
#pragma clang fp contract(off)
    __shared__ DlRed<ACC> red;
    const size_t base = (size_t)blockIdx.x * DL_PIX + threadIdx.x;
    float d[DL_PER_THREAD], g[DL_PER_THREAD], w[DL_PER_THREAD];
#pragma unroll
    for (int j = 0; j < DL_PER_THREAD; j++) {   // (the pixel loads are issued ahead of the partial sums they do not depend on)
        const size_t i = base + (size_t)j * DL_THREADS;
        d[j] = i < N ? depth[i] : 0.f;
        g[j] = i < N ? gt[i] : 0.f;
        w[j] = WEIGHT ? (i < N ? weight[i] : 0.f) : 1.f;
    }
    ACC sp = 0;
    for (size_t i = threadIdx.x; i < nblk; i += DL_THREADS) sp += dl_from_partial<ACC>(partials[2 * i + 1]);
    const float S = (float)block256_sum(sp, red.s);
    if (blockIdx.x == 0) {
        float tp = 0.f;
        for (size_t i = threadIdx.x; i < nblk; i += DL_THREADS) tp += partials[2 * i];
        const float T = block256_sum(tp, red.t);
        if (threadIdx.x == 0) {
            terms[0] = S > 0.f ? T / S : 0.f;
            if constexpr (std::is_same<ACC, float>::value) terms[1] = S;   // (the plain entry point's `term` is one float)
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

int64_t depth_loss_partials_count(int H, int W) { return 2 * (int64_t)div_up_sz((size_t)H * (size_t)W, DL_PIX) + 8; }
int64_t depth_loss_weighted_partials_count(int H, int W) { return 2 * (int64_t)div_up_sz((size_t)H * (size_t)W, DL_PIX) + 8; }

template <typename ACC, bool WEIGHT, bool HUBER>
static int depth_loss_launch(size_t N, float lambda_depth, float delta, const float* depth, const float* gt, const float* weight, float* partials,
                             float* terms, float* dL_ddepth, hipStream_t s)
{
    const size_t nblk = div_up_sz(N, DL_PIX);
    GS_LAUNCH(K_DEPTH_LOSS, (depth_loss_weighted_partials_kernel<ACC, WEIGHT, HUBER>), dim3((unsigned)nblk), dim3(DL_THREADS), 0, s, N, delta, depth,
              gt, weight, partials);
    GS_LAUNCH(K_DEPTH_LOSS, (depth_loss_weighted_grad_kernel<ACC, WEIGHT, HUBER>), dim3((unsigned)nblk), dim3(DL_THREADS), 0, s, N, nblk, lambda_depth,
              delta, depth, gt, weight, (const float*)partials, terms, dL_ddepth);
    return GSLIC_OK;
}

int depth_loss_forward_backward(int H, int W, float lambda_depth, const float* depth, const float* gt, float* partials, float* term, float* dL_ddepth,
                                hipStream_t s)
{
    return depth_loss_launch<uint32_t, false, false>((size_t)H * (size_t)W, lambda_depth, 0.f, depth, gt, nullptr, partials, term, dL_ddepth, s);
}

int depth_loss_weighted_forward_backward(int H, int W, float lambda_depth, float delta, const float* depth, const float* gt, const float* weight,
                                         float* partials, float* terms, float* dL_ddepth, hipStream_t s)
{
    const size_t N = (size_t)H * (size_t)W;
    const bool huber = delta > 0.f;
    if (weight) {
        return huber ? depth_loss_launch<float, true, true>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s)
                     : depth_loss_launch<float, true, false>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s);
    }
    return huber ? depth_loss_launch<float, false, true>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s)
                 : depth_loss_launch<float, false, false>(N, lambda_depth, delta, depth, gt, weight, partials, terms, dL_ddepth, s);
}

}  // namespace gslic
