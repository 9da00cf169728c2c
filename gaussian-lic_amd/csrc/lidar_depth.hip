// lidar_depth.hip — the per-pixel LiDAR range image the depth loss, the pose gradient under depth and the free-space statistics consume, built on
// the device.  The reference's host does it on the CPU (a device->host copy of every point and an unordered_map keyed by "x_y"
// strings, gaussian.cpp:554-572); a LibTorch host writes about twenty small launches ending in scatter_reduce_(amin).  Here, on a caller-owned
// z-buffer of W * H 64-bit keys {float bits of camera z, point index} (all ones = empty):
//   lidar_zbuffer_kernel   one thread per point: the projection rule of include/gslic_hip.h — every step ONE float32 operation rounded on its own
//                          (this file is built with -ffp-contract=off and a true division) — then ONE 64-bit atomicMin: the smallest z wins, equal z
//                          goes to the lowest index, whatever the arrival order.  Unlike extend.hip's kernel it drops z <= 0, NaN and +inf, so the
//                          bits of a positive float order like the value and need no re-mapping.
//   lidar_resolve_kernel   per pixel the minimum key over the (2r+1) x (2r+1) window clipped to the image (r = 0: the pixel's own key), decoded into
//                          depth / index / near bound, and the count of non-empty resolved pixels (one integer atomic per workgroup).
// The minimum filter is separable.  A workgroup of 256 owns a 64 x 16 pixel tile: tile plus halo (at most 80 x 32 cells; out-of-image cells read as
// empty) goes into LDS as 64-bit keys, a row minimum over 2r+1 cells goes into a second LDS array (64 x 32), a column minimum over 2r+1 rows comes
// out of it: two barriers.  Every wave walks ONE row with consecutive lanes on consecutive 8-byte cells, so each 32-lane half of a ds_read_b64 covers
// one 256-byte bank row (whatever the row stride or the window offset) and each 16-lane group of a ds_write_b64 covers 32 consecutive banks:
// conflict-free with no padding, and the global loads and stores of a wave are 512 / 256 contiguous bytes.
//   lidar_resolve_weighted_kernel   the same tile and passes, plus dist2 (squared pixel distance from the pixel to the nearest cell of its window
//                          whose OWN key is the window minimum) and weight = sigma_abs / (sigma_abs + sigma_rel d) * 1 / (1 + falloff dist2), each
//                          step rounded on its own.  dist2 separates as the minimum does: a window row holds the key iff its row minimum equals it,
//                          and the nearest copy inside that row is the smallest |dx| among the row's cells equal to the row minimum.  So the row
//                          pass keeps that |dx| (ties on equal keys to the smaller one) in a BYTE array s_dx beside s_row (64 x 32 bytes, 2 KB:
//                          38 928 B per workgroup, still four per CU) and the column pass takes min(dy^2 + dx^2) over the rows whose minimum equals
//                          the final key: 2r+1 byte reads per pixel on top of the 2r+1 key reads, no search of the (2r+1)^2 cells, no extra global
//                          reads.  Banks of s_dx: a wave's 64 lanes touch 64 consecutive bytes = 16 consecutive dwords, rows 64 bytes apart, so a
//                          ds_read_u8 / ds_write_b8 (32-lane halves, 32 dword banks) has each half on 8 distinct banks with four lanes inside
//                          every dword — one bank, one dword address.  The guide's rule (distinct addresses on one bank serialise, identical
//                          ones broadcast) is stated per dword; whether the four byte lanes of one dword merge in a byte WRITE has not been
//                          measured here.  If they do not, the one store per row pass (against 2r+1 key reads) is four-way, which the LDS
//                          write path's own issue cost covers up to two-way; the reads are dword-granular.  r = 0 skips LDS: dist2 = 0 / -1.
// The launches are booked under the extend class (no profiler id of their own).  No float atomics, no stream synchronisation, no allocation.
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

static constexpr unsigned long long LIDAR_EMPTY = ~0ull;
static constexpr int LD_TW = 64;                      // tile width: one wave per row
static constexpr int LD_TH = 16;                      // tile height: four rows per wave
static constexpr int LD_RMAX = 8;                     // largest footprint radius
static constexpr int LD_LW = LD_TW + 2 * LD_RMAX;     // 80 cells per LDS row of the tile
static constexpr int LD_LH = LD_TH + 2 * LD_RMAX;     // 32 LDS rows

__global__ __launch_bounds__(256) void lidar_zbuffer_kernel(int n, const float* __restrict__ pts, const float* __restrict__ Rcw,
                                                            const float* __restrict__ tcw, float fx, float fy, float cx, float cy, int W, int H,
                                                            unsigned long long* __restrict__ zbuf, uint32_t index_base)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p0 = pts[3 * (size_t)i], p1 = pts[3 * (size_t)i + 1], p2 = pts[3 * (size_t)i + 2];
    const float c0 = p0 * Rcw[0] + p1 * Rcw[1] + p2 * Rcw[2] + tcw[0];
    const float c1 = p0 * Rcw[3] + p1 * Rcw[4] + p2 * Rcw[5] + tcw[1];
    const float z = p0 * Rcw[6] + p1 * Rcw[7] + p2 * Rcw[8] + tcw[2];
    if (!(z > 0.0f) || !(z < __builtin_inff())) return;                        // z <= 0, NaN, +inf
    const float xf = floorf((c0 * fx) / z + cx), yf = floorf((c1 * fy) / z + cy);
    if (!(xf >= 0.0f && xf < (float)W && yf >= 0.0f && yf < (float)H)) return;  // compared as floats (a NaN fails): the casts below are in range
    const size_t id = (size_t)(int)yf * (size_t)W + (size_t)(int)xf;
    atomicMin(&zbuf[id], ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(index_base + (uint32_t)i));
}

__global__ __launch_bounds__(256) void lidar_resolve_kernel(int W, int H, const unsigned long long* __restrict__ zbuf, int r, float margin_abs,
                                                            float margin_rel, float* __restrict__ depth_out, int32_t* __restrict__ index_out,
                                                            float* __restrict__ near_out, uint32_t* __restrict__ n_measured)
{
    __shared__ unsigned long long s_tile[LD_LH * LD_LW];   // tile + halo, 20 KB
    __shared__ unsigned long long s_row[LD_LH * LD_TW];    // row minima of the LD_TH + 2r rows, 16 KB
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * LD_TW, y0 = blockIdx.y * LD_TH;
    const int x = x0 + lane;
    if (r > 0) {   // (wave-uniform: the argument)
        const int lw = LD_TW + 2 * r, lh = LD_TH + 2 * r;
        for (int ly = wave; ly < lh; ly += 4) {
            const int gy = y0 - r + ly;
            const bool row_in = gy >= 0 && gy < H;
            for (int lx = lane; lx < lw; lx += 64) {
                const int gx = x0 - r + lx;
                s_tile[ly * LD_LW + lx] = (row_in && gx >= 0 && gx < W) ? zbuf[(size_t)gy * W + gx] : LIDAR_EMPTY;
            }
        }
        __syncthreads();
        for (int ly = wave; ly < lh; ly += 4) {
            unsigned long long m = LIDAR_EMPTY;
            for (int k = 0; k <= 2 * r; k++) {
                const unsigned long long v = s_tile[ly * LD_LW + lane + k];
                m = v < m ? v : m;
            }
            s_row[ly * LD_TW + lane] = m;
        }
        __syncthreads();
    }
    uint32_t count = 0;
#pragma unroll
    for (int j = 0; j < LD_TH / 4; j++) {
        const int ty = wave + 4 * j, y = y0 + ty;
        if (x >= W || y >= H) continue;
        unsigned long long key;
        if (r > 0) {
            key = LIDAR_EMPTY;
            for (int k = 0; k <= 2 * r; k++) {
                const unsigned long long v = s_row[(ty + k) * LD_TW + lane];
                key = v < key ? v : key;
            }
        } else {
            key = zbuf[(size_t)y * W + x];
        }
        const bool hit = key != LIDAR_EMPTY;
        const float d = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        const size_t o = (size_t)y * W + x;
        if (depth_out) depth_out[o] = d;
        if (index_out) index_out[o] = hit ? (int32_t)(uint32_t)key : -1;
        if (near_out) {
            const float prod = margin_rel * d;
            const float margin = margin_abs + prod;
            near_out[o] = hit ? d - margin : 0.0f;
        }
        count += hit ? 1u : 0u;
    }
    if (n_measured) {   // (wave-uniform)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d, 64);
        if (lane == 0) s_cnt[wave] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            if (total) atomicAdd(n_measured, total);
        }
    }
}

// lidar_resolve_kernel with two more images: dist2 (the squared pixel distance to the cell the key came from) and weight (the range weight times
// a rational falloff in dist2) — the rule of gslic_lidar_zbuffer_resolve_weighted in include/gslic_hip.h.  Same tile, same two barriers; the row
// pass also leaves |dx| of the nearest cell holding the row minimum in s_dx, the column pass takes min(dy^2 + dx^2) over the rows whose minimum
// is the key.
__global__ __launch_bounds__(256) void lidar_resolve_weighted_kernel(int W, int H, const unsigned long long* __restrict__ zbuf, int r,
                                                                     float margin_abs, float margin_rel, float sigma_abs, float sigma_rel,
                                                                     float falloff, float* __restrict__ depth_out, int32_t* __restrict__ index_out,
                                                                     float* __restrict__ near_out, uint32_t* __restrict__ n_measured,
                                                                     float* __restrict__ weight_out, int32_t* __restrict__ dist2_out)
{
    __shared__ unsigned long long s_tile[LD_LH * LD_LW];   // tile + halo, 20 KB
    __shared__ unsigned long long s_row[LD_LH * LD_TW];    // row minima of the LD_TH + 2r rows, 16 KB
    __shared__ uint8_t s_dx[LD_LH * LD_TW];                // |dx| of the nearest cell of the row window that holds the row minimum, 2 KB
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * LD_TW, y0 = blockIdx.y * LD_TH;
    const int x = x0 + lane;
    if (r > 0) {   // (wave-uniform: the argument)
        const int lw = LD_TW + 2 * r, lh = LD_TH + 2 * r;
        for (int ly = wave; ly < lh; ly += 4) {
            const int gy = y0 - r + ly;
            const bool row_in = gy >= 0 && gy < H;
            for (int lx = lane; lx < lw; lx += 64) {
                const int gx = x0 - r + lx;
                s_tile[ly * LD_LW + lx] = (row_in && gx >= 0 && gx < W) ? zbuf[(size_t)gy * W + gx] : LIDAR_EMPTY;
            }
        }
        __syncthreads();
        for (int ly = wave; ly < lh; ly += 4) {
            unsigned long long m = LIDAR_EMPTY;
            int best = r;   // (of an all-empty row: never looked at, an empty row minimum equals no key)
            for (int k = 0; k <= 2 * r; k++) {
                const unsigned long long v = s_tile[ly * LD_LW + lane + k];
                const int adx = k < r ? r - k : k - r;
                const bool take = v < m || (v == m && adx < best);   // equal keys: the smaller |dx|
                m = take ? v : m;
                best = take ? adx : best;
            }
            s_row[ly * LD_TW + lane] = m;
            s_dx[ly * LD_TW + lane] = (uint8_t)best;
        }
        __syncthreads();
    }
    uint32_t count = 0;
#pragma unroll
    for (int j = 0; j < LD_TH / 4; j++) {
        const int ty = wave + 4 * j, y = y0 + ty;
        if (x >= W || y >= H) continue;
        unsigned long long key;
        int s2 = 0;
        if (r > 0) {
            key = LIDAR_EMPTY;
            for (int k = 0; k <= 2 * r; k++) {
                const unsigned long long v = s_row[(ty + k) * LD_TW + lane];
                const int dx = s_dx[(ty + k) * LD_TW + lane], dy = k - r;
                const int c = dy * dy + dx * dx;
                s2 = v < key ? c : (v == key && c < s2 ? c : s2);
                key = v < key ? v : key;
            }
        } else {
            key = zbuf[(size_t)y * W + x];
        }
        const bool hit = key != LIDAR_EMPTY;
        const float d = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        const size_t o = (size_t)y * W + x;
        if (depth_out) depth_out[o] = d;
        if (index_out) index_out[o] = hit ? (int32_t)(uint32_t)key : -1;
        if (near_out) {
            const float prod = margin_rel * d;
            const float margin = margin_abs + prod;
            near_out[o] = hit ? d - margin : 0.0f;
        }
        if (dist2_out) dist2_out[o] = hit ? s2 : -1;
        if (weight_out) {   // four steps, each one float32 operation (this file is built with -ffp-contract=off; '/' is the true division)
            const float prod = sigma_rel * d;
            const float a = sigma_abs + prod;
            const float rw = sigma_abs / a;
            const float fs = falloff * (float)s2;
            const float den = 1.0f + fs;
            const float f = 1.0f / den;
            weight_out[o] = hit ? rw * f : 0.0f;
        }
        count += hit ? 1u : 0u;
    }
    if (n_measured) {   // (wave-uniform)
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) count += __shfl_xor(count, d, 64);
        if (lane == 0) s_cnt[wave] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            if (total) atomicAdd(n_measured, total);
        }
    }
}

int lidar_zbuffer_add(int n, const float* points, const float* Rcw, const float* tcw, float fx, float fy, float cx, float cy, int W, int H,
                      unsigned long long* zbuf, bool clear, int32_t index_base, hipStream_t s)
{
    if (clear) GS_HIP(hipMemsetAsync(zbuf, 0xff, (size_t)W * H * sizeof(unsigned long long), s));
    if (n <= 0) return GSLIC_OK;
    GS_LAUNCH(K_EXTEND, lidar_zbuffer_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, n, points, Rcw, tcw, fx, fy, cx, cy, W, H, zbuf,
              (uint32_t)index_base);
    return GSLIC_OK;
}

int lidar_zbuffer_resolve(int W, int H, const unsigned long long* zbuf, int footprint, float margin_abs, float margin_rel, float* depth_out,
                          int32_t* index_out, float* near_out, uint32_t* n_measured_out, hipStream_t s)
{
    if (n_measured_out) GS_HIP(hipMemsetAsync(n_measured_out, 0, sizeof(uint32_t), s));
    GS_LAUNCH(K_EXTEND, lidar_resolve_kernel, dim3(div_up(W, LD_TW), div_up(H, LD_TH)), dim3(256), 0, s, W, H, zbuf, footprint, margin_abs,
              margin_rel, depth_out, index_out, near_out, n_measured_out);
    return GSLIC_OK;
}

int lidar_zbuffer_resolve_weighted(int W, int H, const unsigned long long* zbuf, int footprint, float margin_abs, float margin_rel, float sigma_abs,
                                   float sigma_rel, float falloff, float* depth_out, int32_t* index_out, float* near_out, uint32_t* n_measured_out,
                                   float* weight_out, int32_t* dist2_out, hipStream_t s)
{
    if (n_measured_out) GS_HIP(hipMemsetAsync(n_measured_out, 0, sizeof(uint32_t), s));
    GS_LAUNCH(K_EXTEND, lidar_resolve_weighted_kernel, dim3(div_up(W, LD_TW), div_up(H, LD_TH)), dim3(256), 0, s, W, H, zbuf, footprint, margin_abs,
              margin_rel, sigma_abs, sigma_rel, falloff, depth_out, index_out, near_out, n_measured_out, weight_out, dist2_out);
    return GSLIC_OK;
}

}  // namespace gslic
