// exposure.hip — the per-view exposure model (a 3x4 affine colour transform E on the rendered image) forward and backward, with the optional
// torch-style Adam update of E riding on the backward's second launch.  The rules are written out in include/gslic_hip.h
// (gslic_exposure_apply / gslic_exposure_backward); every product and sum here is one float32 operation rounded on its own (fp contract off).
//
// Both kernels stream planar [3,H,W] images: 12 B read + 12 B written per pixel (apply), 24 B read + 12 B written (backward).  The pixels are cut
// the same way in both and in every run: workgroup b takes the EX_PIX consecutive pixels from b * EX_PIX, thread t of it the EX_QUADS quads of four
// consecutive pixels q = t, t + 256, ... — an assignment that depends on H * W alone (not on the device's CU count and not on the pointers), which
// is what makes the twelve sums of dL_dE the same bits on every run and every device.  A quad is one 16-byte access per plane where the planes
// are 16-byte aligned (ALIGNED: every pointer is and H * W % 4 == 0), a dword-aligned 16-byte access otherwise; the one quad that crosses the end
// of the image is read and written pixel by pixel.
//
// Backward, launch 1: dL_dimage for the workgroup's pixels and its row of twelve partial sums (per-thread accumulators in pixel order -> xor-shuffle
// tree per wave64 -> (r0 + r1) + (r2 + r3) over the four waves through LDS).  Launch 2, ONE workgroup: thread t adds the rows t, t + 256, ... in that
// order, the 256 thread sums go through the same tree, threads 0..11 write dL_dE and — with an Adam descriptor — update E's row of the [V,12] arrays.
// No atomics, no allocation, no read-back: capturable in a graph.
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

static constexpr int EX_THREADS = 256;
static constexpr int EX_QUADS = 2;                            // quads of four pixels per thread
static constexpr int EX_PIX = EX_THREADS * EX_QUADS * 4;      // pixels per workgroup (2048: 1013 workgroups at 1920 x 1080)

template <bool ALIGNED>
struct ExQuad { typedef gs_v4f_u type; };
template <>
struct ExQuad<true> { typedef gs_v4f type; };

// the quad at pixel i of a plane: whole (one 16-byte access) when i + 4 <= N, otherwise the pixels below N (the others read as 0 and are not stored)
template <bool ALIGNED>
__device__ __forceinline__ gs_v4f ex_load(const float* __restrict__ plane, size_t i, size_t N)
{
    if (i + 4 <= N) return *reinterpret_cast<const typename ExQuad<ALIGNED>::type*>(plane + i);
    gs_v4f v = {0.f, 0.f, 0.f, 0.f};
    if (i < N) v.x = plane[i];
    if (i + 1 < N) v.y = plane[i + 1];
    if (i + 2 < N) v.z = plane[i + 2];
    return v;
}
template <bool ALIGNED>
__device__ __forceinline__ void ex_store(float* __restrict__ plane, size_t i, size_t N, const gs_v4f v)
{
    if (i + 4 <= N) { *reinterpret_cast<typename ExQuad<ALIGNED>::type*>(plane + i) = v; return; }
    if (i < N) plane[i] = v.x;
    if (i + 1 < N) plane[i + 1] = v.y;
    if (i + 2 < N) plane[i + 2] = v.z;
}

template <bool ALIGNED>
__global__ __launch_bounds__(EX_THREADS) void exposure_apply_kernel(size_t N, const float* __restrict__ E, const float* __restrict__ image,
                                                                    float* __restrict__ out)
{
#pragma clang fp contract(off)
    float e[12];
#pragma unroll
    for (int k = 0; k < 12; k++) e[k] = E[k];
    const size_t base = (size_t)blockIdx.x * EX_PIX;
    gs_v4f r[EX_QUADS], g[EX_QUADS], b[EX_QUADS];
#pragma unroll
    for (int j = 0; j < EX_QUADS; j++) {   // (all loads in flight before the arithmetic)
        const size_t i = base + 4 * ((size_t)threadIdx.x + (size_t)j * EX_THREADS);
        r[j] = ex_load<ALIGNED>(image, i, N);
        g[j] = ex_load<ALIGNED>(image + N, i, N);
        b[j] = ex_load<ALIGNED>(image + 2 * N, i, N);
    }
#pragma unroll
    for (int j = 0; j < EX_QUADS; j++) {
        const size_t i = base + 4 * ((size_t)threadIdx.x + (size_t)j * EX_THREADS);
        if (i >= N) break;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const gs_v4f o = ((e[4 * c] * r[j] + e[4 * c + 1] * g[j]) + e[4 * c + 2] * b[j]) + e[4 * c + 3];
            ex_store<ALIGNED>(out + (size_t)c * N, i, N, o);
        }
    }
}

// partials[12 b + 4 c + k] = the partial of dL_dE[c,k] of workgroup b
template <bool ALIGNED>
__global__ __launch_bounds__(EX_THREADS) void exposure_backward_kernel(size_t N, const float* __restrict__ E, const float* __restrict__ image,
                                                                       const float* __restrict__ dL_dout, float* __restrict__ dL_dimage,
                                                                       float* __restrict__ partials)
{
#pragma clang fp contract(off)
    __shared__ float red[4][12];
    float e[12];
#pragma unroll
    for (int k = 0; k < 12; k++) e[k] = E[k];
    const size_t base = (size_t)blockIdx.x * EX_PIX;
    gs_v4f x[EX_QUADS][3], g[EX_QUADS][3];
#pragma unroll
    for (int j = 0; j < EX_QUADS; j++) {
        const size_t i = base + 4 * ((size_t)threadIdx.x + (size_t)j * EX_THREADS);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x[j][c] = ex_load<ALIGNED>(image + (size_t)c * N, i, N);
            g[j][c] = ex_load<ALIGNED>(dL_dout + (size_t)c * N, i, N);
        }
    }
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < EX_QUADS; j++) {
        const size_t i = base + 4 * ((size_t)threadIdx.x + (size_t)j * EX_THREADS);
        if (i < N) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const gs_v4f d = (e[k] * g[j][0] + e[4 + k] * g[j][1]) + e[8 + k] * g[j][2];
                ex_store<ALIGNED>(dL_dimage + (size_t)k * N, i, N, d);
            }
        }
        // the pixels of the quad in order; a pixel at or past N adds nothing (not even a zero)
#pragma unroll
        for (int p = 0; p < 4; p++) {
            if (i + p < N) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float gc = g[j][c][p];
#pragma unroll
                    for (int k = 0; k < 3; k++) acc[4 * c + k] += gc * x[j][k][p];
                    acc[4 * c + 3] += gc;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
        float v = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        acc[k] = v;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int k = threadIdx.x;
        partials[12 * (size_t)blockIdx.x + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

struct ExposureAdamArgs {
    float *param, *m, *v;
    int32_t* step_count;
    const int32_t* view;
    const uint32_t* skip;
    float lr, beta1, beta2, eps;
    int on;
};

__global__ __launch_bounds__(EX_THREADS) void exposure_finalize_kernel(size_t nblk, const float* __restrict__ partials, float* __restrict__ dL_dE,
                                                                       ExposureAdamArgs ad)
{
#pragma clang fp contract(off)
    __shared__ float red[4][12];
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.f;
    for (size_t r = threadIdx.x; r < nblk; r += EX_THREADS) {
        const gs_v4f_u* row = reinterpret_cast<const gs_v4f_u*>(partials + 12 * r);
        const gs_v4f a = row[0], b = row[1], c = row[2];
#pragma unroll
        for (int k = 0; k < 4; k++) { acc[k] += a[k]; acc[4 + k] += b[k]; acc[8 + k] += c[k]; }
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
        float v = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        acc[k] = v;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x >= 12) return;
    const int k = threadIdx.x;
    const float g = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    dL_dE[k] = g;
    if (!ad.on) return;
    if (ad.skip && (ad.skip[0] & 27u) != 0) return;   // the step's forward did not complete (its status bits 1 | 2 | 8 | 16): nothing is updated
    const int32_t view = ad.view[0];
    // every one of the twelve threads reads the count before thread 0 stores the new one (they are lanes of one wave: the loads of this
    // instruction complete before the store below is issued)
    const int32_t t = ad.step_count[view] + 1;
    const size_t at = 12 * (size_t)view + k;
    // torch.optim.Adam: the two bias terms in double from the integer t, each rounded to float once; everything else float32
    const double bc1 = 1.0 - pow((double)ad.beta1, (double)t), bc2 = 1.0 - pow((double)ad.beta2, (double)t);
    const float step = (float)((double)ad.lr / bc1), rbc2 = (float)sqrt(bc2);
    const float m = ad.beta1 * ad.m[at] + (1.0f - ad.beta1) * g;
    const float v = ad.beta2 * ad.v[at] + ((1.0f - ad.beta2) * g) * g;
    const float denom = sqrtf(v) / rbc2 + ad.eps;
    ad.m[at] = m;
    ad.v[at] = v;
    ad.param[at] = ad.param[at] - (step * m) / denom;
    if (k == 0) ad.step_count[view] = t;
}

int64_t exposure_partials_count(int H, int W) { return 12 * (int64_t)div_up_sz((size_t)H * (size_t)W, EX_PIX); }

static bool ex_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int exposure_apply(int H, int W, const float* E, const float* image, float* out, hipStream_t s)
{
    const size_t N = (size_t)H * (size_t)W, nblk = div_up_sz(N, EX_PIX);
    if (N % 4 == 0 && ex_aligned16(image) && ex_aligned16(out))
        GS_LAUNCH(K_DEPTH_LOSS, exposure_apply_kernel<true>, dim3((unsigned)nblk), dim3(EX_THREADS), 0, s, N, E, image, out);
    else
        GS_LAUNCH(K_DEPTH_LOSS, exposure_apply_kernel<false>, dim3((unsigned)nblk), dim3(EX_THREADS), 0, s, N, E, image, out);
    return GSLIC_OK;
}

int exposure_backward(int H, int W, const float* E, const float* image, const float* dL_dout, float* dL_dimage, float* partials, float* dL_dE,
                      const gslic_exposure_adam* adam, hipStream_t s)
{
    const size_t N = (size_t)H * (size_t)W, nblk = div_up_sz(N, EX_PIX);
    ExposureAdamArgs ad{};
    if (adam) {
        ad.param = adam->param; ad.m = adam->m; ad.v = adam->v; ad.step_count = adam->step_count; ad.view = adam->view; ad.skip = adam->skip;
        ad.lr = adam->lr; ad.beta1 = adam->beta1; ad.beta2 = adam->beta2; ad.eps = adam->eps; ad.on = 1;
    }
    if (N % 4 == 0 && ex_aligned16(image) && ex_aligned16(dL_dout) && ex_aligned16(dL_dimage))
        GS_LAUNCH(K_DEPTH_LOSS, exposure_backward_kernel<true>, dim3((unsigned)nblk), dim3(EX_THREADS), 0, s, N, E, image, dL_dout, dL_dimage, partials);
    else
        GS_LAUNCH(K_DEPTH_LOSS, exposure_backward_kernel<false>, dim3((unsigned)nblk), dim3(EX_THREADS), 0, s, N, E, image, dL_dout, dL_dimage, partials);
    GS_LAUNCH(K_DEPTH_LOSS, exposure_finalize_kernel, dim3(1), dim3(EX_THREADS), 0, s, nblk, (const float*)partials, dL_dE, ad);
    return GSLIC_OK;
}

}  // namespace gslic
