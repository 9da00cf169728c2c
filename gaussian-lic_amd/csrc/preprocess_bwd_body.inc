// preprocess_bwd_body.inc — the body of preprocess_bwd_kernel / preprocess_bwd_defer_xyz_kernel (preprocess_bwd.hip), included inside each kernel
// with LDS_SH, BS, CAM, DEFER_XYZ and GSTAT (+ the GradStatArgs gs) in scope.  DEFER_XYZ: the fused Adam update skips group 0 (xyz), whose chain
// gradient goes to dL_dmean3D.  GSTAT: the gradient densification statistics are accumulated into gs (grad_stat_update); false: gs is never read.
    __shared__ __attribute__((aligned(16))) float lds_tab[LDS_SH ? BS * SHT : 4];   // {c_0..c_14, dRGB} per Gaussian; later the 14 small gradients
    __shared__ float lds_sk[LDS_SH ? BS * 15 : 4];                                    // q_k per Gaussian
    __shared__ uint8_t lds_vis[BS];
    // the 14 small-group gradients of every Gaussian of the block, group-major (xyz | dc | opacity | scale | rotation), for the
    // cooperative float4 Adam below: per-thread 4-byte accesses at stride 12 / 16 B cost this kernel 0.29 ms of 0.86
    float* const lds_g = lds_tab;  // overlays the table once the column pass is through (14 * BS <= SHT * BS)
    if (a.status[2] != 0u) return;  // capacity overflow in the forward: nothing of this step is valid — no gradients, no Adam
    const int idx = a.row_begin + blockIdx.x * BS + threadIdx.x;
    const int M = a.M;
    const int row0 = a.row_begin + blockIdx.x * BS;
    const int rows = (a.row_end - row0) < BS ? (a.row_end - row0) : BS;
    ShOut so;
    so.x = so.y = so.z = so.dR = so.dG = so.dB = 0.f;
    so.on = false;
    float sg[14];
#pragma unroll
    for (int k = 0; k < 14; k++) sg[k] = 0.f;
    // camera gradient (CAM): 27 sums over the Gaussians — d/dviewmatrix rows 0..2, d/dprojmatrix rows 0, 1, 3, d/dcampos — with the
    // three matrices treated as the independent inputs they are at this boundary (the reference returns no camera gradient at all:
    // rasterizer.cpp:181).  Each wave reduces its 64 Gaussians and writes one row of partials; cam_reduce_kernel adds the rows.
    float cg[CAM ? 27 : 1];
    if constexpr (CAM) {
#pragma unroll
        for (int k = 0; k < 27; k++) cg[k] = 0.f;
    }
    PartialSums ps;
    bool visible = false;
    if (idx < a.row_end) visible = bwd_gather(a, idx, LDS_SH, ps);
    if constexpr (GSTAT) {   // the densification statistics of this row, from the two sums dL_dmean2D would hold (rows of a failed forward never get here)
        if (visible) grad_stat_update(gs, idx, ps.mx, ps.my, a.radii[idx]);
    }
    lds_vis[threadIdx.x] = visible ? 1 : 0;
    if (a.vis_out && idx < a.row_end) a.vis_out[idx] = visible ? 1 : 0;                                            // the exchange payload's mask ...
    if (a.campos_out && blockIdx.x == 0 && threadIdx.x < 3) a.campos_out[threadIdx.x] = a.campos[threadIdx.x];     // ... and camera centre
    if constexpr (LDS_SH) {
        // ---- this Gaussian's row of the table (zeros when invisible: its gradient elements and products are then exact zeros)
        float trow[18];
#pragma unroll
        for (int k = 0; k < 18; k++) trow[k] = 0.f;
        if (visible) {
            const uint32_t clamp_bits = __float_as_uint(a.rec[GS_REC_F4 * (size_t)idx + 2].z);
            float dox, doy, doz, x, y, z;
            sh_dir(a.means[3 * idx], a.means[3 * idx + 1], a.means[3 * idx + 2], a.campos, dox, doy, doz, x, y, z);
            float c[15];
            sh_coefs(a.D, x, y, z, c);
#pragma unroll
            for (int k = 0; k < 15; k++) trow[k] = c[k];
            trow[15] = (clamp_bits & 1u) ? 0.f : ps.r; trow[16] = (clamp_bits & 2u) ? 0.f : ps.g; trow[17] = (clamp_bits & 4u) ? 0.f : ps.b;
        }
#pragma unroll
        for (int k = 0; k < 18; k++) lds_tab[threadIdx.x * SHT + k] = trow[k];
        __syncthreads();
        // ---- the column pass over the block's SH parameters (full blocks); the last, partial block goes row by row
        const bool sh_sink = a.dL_dsh || a.adam.on;
        if (rows == BS) {
            sh_columns_pass<BS>(a, lds_tab, lds_sk, lds_vis, row0);
        } else {
            const size_t base = (size_t)row0 * 45;
            if ((int)threadIdx.x < rows) {
#pragma clang fp contract(off)   // (as sh_columns_pass rounds them)
                const float* __restrict__ sh = a.shs + base + 45 * threadIdx.x;
                const float* __restrict__ tr = lds_tab + threadIdx.x * SHT;
#pragma unroll
                for (int k = 0; k < 15; k++) lds_sk[threadIdx.x * 15 + k] = (sh[3 * k] * tr[15] + sh[3 * k + 1] * tr[16]) + sh[3 * k + 2] * tr[17];
            }
            __syncthreads();   // every q_k has been formed from the parameters as they were
            const AdamFusedArgs& A = a.adam;
            if (sh_sink)
                for (int i = threadIdx.x; i < rows * 45; i += BS) {
                    const int r = i / 45, rem = i - 45 * r, k = rem / 3, ch = rem - 3 * k;
                    const float g = lds_tab[r * SHT + k] * lds_tab[r * SHT + 15 + ch];
                    if (a.dL_dsh) a.dL_dsh[base + i] = g;
                    if (A.on && lds_vis[r]) adam_scalar(A.p[2][base + i], g, A.m[2][base + i], A.v[2][base + i], A.lr[2], A.b1, A.b2, A.eps);
                }
        }
        __syncthreads();   // q_k complete; the table is free
        if (visible) bwd_rest<CAM, DEFER_XYZ>(a, idx, ps, nullptr, lds_sk + threadIdx.x * 15, so, sg, cg);
    } else {
        const float* sh_row = a.shs ? a.shs + (size_t)3 * M * idx : nullptr;
        if (visible) bwd_rest<CAM, DEFER_XYZ>(a, idx, ps, sh_row, nullptr, so, nullptr, cg);
    }
    if constexpr (CAM) {
#pragma unroll
        for (int k = 0; k < 27; k++) {
            float v = cg[k];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
            cg[k] = v;
        }
        if ((threadIdx.x & 63) == 0) {
            float* row = a.cam_partials + 32 * ((size_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6));
#pragma unroll
            for (int k = 0; k < 27; k++) row[k] = cg[k];
        }
    }
    if constexpr (LDS_SH) {
        // ---- small groups: the block's rows of xyz / dc / opacity / scale / rotation are contiguous in memory, so the Adam update runs
        // on float4 columns of those five regions (at most one float4 per thread and group, all fifteen loads issued before the math)
        const int t = threadIdx.x;
        lds_g[3 * t] = sg[0]; lds_g[3 * t + 1] = sg[1]; lds_g[3 * t + 2] = sg[2];
        lds_g[3 * BS + 3 * t] = sg[3]; lds_g[3 * BS + 3 * t + 1] = sg[4]; lds_g[3 * BS + 3 * t + 2] = sg[5];
        lds_g[6 * BS + t] = sg[6];
        lds_g[7 * BS + 3 * t] = sg[7]; lds_g[7 * BS + 3 * t + 1] = sg[8]; lds_g[7 * BS + 3 * t + 2] = sg[9];
        reinterpret_cast<float4*>(lds_g + 10 * BS)[t] = make_float4(sg[10], sg[11], sg[12], sg[13]);
        __syncthreads();
        float* const gout[5] = {a.dL_dmean3D, a.dL_drgb ? a.dL_drgb : a.dL_ddc, a.dL_dopacity, a.dL_dscale, a.dL_drot};
        small_groups_sink<BS, DEFER_XYZ>(a.adam, gout, lds_g, lds_vis, row0, rows);
    } else if (idx < a.row_end && M > 0 && (a.dL_dsh || a.adam.on)) {
        // generic row width: per-thread strided rows (dL_dsh zeros when invisible, when shs == NULL, above the active degree)
        const AdamFusedArgs& A = a.adam;
        float c[15];
        sh_coefs(a.D, so.x, so.y, so.z, c);
        const int nk = M < 15 ? M : 15;
        const float dR[3] = {so.dR, so.dG, so.dB};
        const size_t rb = (size_t)3 * M * idx;
        for (int k = 0; k < 3 * M; k++) {
            const float g = (so.on && k < 3 * nk) ? c[k / 3] * dR[k % 3] : 0.f;
            if (a.dL_dsh) a.dL_dsh[rb + k] = g;
            if (A.on && lds_vis[threadIdx.x]) adam_scalar(A.p[2][rb + k], g, A.m[2][rb + k], A.v[2][rb + k], A.lr[2], A.b1, A.b2, A.eps);
        }
    }
