// loss_bwd_body.inc — the body of the loss backward kernels of ssim.hip behind their LDS declarations, included twice:
//   LOSS_BWD_WEIGHTED 0  loss_bwd_kernel: the uniform upstream gradients w_ssim = -lambda/N and w_l1 = (1-lambda)/N (kernel arguments)
//   LOSS_BWD_WEIGHTED 1  loss_weighted_bwd_kernel: per pixel g_p = c_ssim * w_p and (c_l1 * w_p), the two coefficients read from `coef`
//                        (device memory, written by loss_weighted_reduce_kernel) and w_p = loss_weight(weight[p]), 0 outside the image.
// g_p is multiplied into the three derivative maps where the uniform kernel multiplies w_ssim, before the convolutions: no LDS of its own.
// Expects: grid, H, W, img1, img2, dm_dmu1, dm_dsigma1_sq, dm_dsigma12, dL_dimg1 and the LDS arrays s1, s2, s3 [SH_][SH_].
    int tile_x, tile_y, plane_i;
    size_t tile_linear;
    if (!ssim_tile(grid, tile_x, tile_y, plane_i, tile_linear)) return;   // (whole workgroup: before any barrier)
    const size_t plane = (size_t)plane_i * H * W;
    const int x0 = tile_x * ST, y0 = tile_y * ST;
    const int tid = threadIdx.x;
#if LOSS_BWD_WEIGHTED
    const float c_l1 = coef[0], c_ssim = coef[1];   // uniform: (1-lambda)/(CH S) and -lambda/(CH S), or 0, 0 when S == 0
#endif
    {
        float v1[HALO_TRIPS], v2[HALO_TRIPS], v3[HALO_TRIPS];
#if LOSS_BWD_WEIGHTED
        float g[HALO_TRIPS];
#endif
#pragma unroll
        for (int k = 0; k < HALO_TRIPS; k++) {
            const int t = tid + 256 * k;
            const int ly = t / SH_, lx = t - ly * SH_;
            const int y = y0 + ly - 5, x = x0 + lx - 5;
            const bool in = t < SH_ * SH_;
            v1[k] = in ? pix_or_zero(dm_dmu1 + plane, H, W, y, x) : 0.f;
            v2[k] = in ? pix_or_zero(dm_dsigma1_sq + plane, H, W, y, x) : 0.f;
            v3[k] = in ? pix_or_zero(dm_dsigma12 + plane, H, W, y, x) : 0.f;
#if LOSS_BWD_WEIGHTED
            g[k] = c_ssim * loss_weight(in ? pix_or_zero(weight, H, W, y, x) : 0.f);
#endif
        }
#pragma unroll
        for (int k = 0; k < HALO_TRIPS; k++) {
            const int t = tid + 256 * k;
#if LOSS_BWD_WEIGHTED
            if (t < SH_ * SH_) { (&s1[0][0])[t] = v1[k] * g[k]; (&s2[0][0])[t] = v2[k] * g[k]; (&s3[0][0])[t] = v3[k] * g[k]; }
#else
            if (t < SH_ * SH_) { (&s1[0][0])[t] = v1[k] * w_ssim; (&s2[0][0])[t] = v2[k] * w_ssim; (&s3[0][0])[t] = v3[k] * w_ssim; }
#endif
        }
    }
    __syncthreads();
    for (int t = tid; t < SH_ * ST; t += 256) {
        const int ly = t / ST, lx = t % ST;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int i = 0; i < 11; i++) {
            const float g = c_G[i];
            r0 += g * s1[ly][lx + i]; r1 += g * s2[ly][lx + i]; r2 += g * s3[ly][lx + i];
        }
        s1[ly][lx] = r0; s2[ly][lx] = r1; s3[ly][lx] = r2;
    }
    __syncthreads();
    const int lx = tid & 31;
    // four consecutive rows per thread, one sweep over the 14 rows of hs they share (ssim_fwd_column4): taps in ascending order per output
    const int ly0 = 4 * (tid >> 5);
    float w0[4] = {0.f, 0.f, 0.f, 0.f}, w1[4] = {0.f, 0.f, 0.f, 0.f}, w2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 14; r++) {
        const float a0 = s1[ly0 + r][lx], a1 = s2[ly0 + r][lx], a2 = s3[ly0 + r][lx];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = r - k;
            if (j >= 0 && j <= 10) {
                const float g = c_G[j];
                w0[k] += g * a0; w1[k] += g * a1; w2[k] += g * a2;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int ly = ly0 + q;
        const float v0 = w0[q], v1 = w1[q], v2 = w2[q];
        const int px = x0 + lx, py = y0 + ly;
        if (px < W && py < H) {
            const size_t o = plane + (size_t)py * W + px;
            const float pix1 = img1[o], pix2 = img2[o];
            const float d = pix1 - pix2;
            const float sgn = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);  // torch.sign (abs backward)
            float acc = 0.0f;
            acc += v0;
            acc += pix1 * 2.0f * v1;
            acc += pix2 * v2;
#if LOSS_BWD_WEIGHTED
            dL_dimg1[o] = (c_l1 * loss_weight(weight[(size_t)py * W + px])) * sgn + acc;
#else
            dL_dimg1[o] = w_l1 * sgn + acc;
#endif
        }
    }
