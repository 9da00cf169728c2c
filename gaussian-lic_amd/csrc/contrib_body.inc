// contrib_body.inc — the body of contribution_kernel (contrib.hip), included once per variant.
// CONTRIB_ERR = 0: gslic_contribution_accumulate.  CONTRIB_ERR = 1: gslic_contribution_accumulate_error, which also forms
// err_sum[g] += sum of w e(p) over the contributing pairs of g (kernel arguments `err`, `err_sum`): one more butterfly per blended (wave, entry),
// 1 KB more LDS, one more 64-bit atomic per (tile, entry); the other three accumulators are formed by the same operations in the same order.
// CONTRIB_FREE = 1: gslic_contribution_accumulate_free_space (kernel arguments `near_bound`, `free_sum`, `meas_sum`): the pixel is MEASURED when
// near_bound[p] > 0, and meas_sum[g] += sum of w over the measured pixels, free_sum[g] += sum of w over the measured pixels with z_g < near_bound[p]
// (z_g: the view depth in the entry's record, staged beside s_r1).  The per-pixel addend is w or +0: one comparison, two selects, two more
// butterflies per blended (wave, entry), 2.25 KB more LDS, up to two more 64-bit atomics per (tile, entry); the base three are formed as before.
#pragma clang fp contract(off)
    __shared__ float4 s_r0[GS_BUCKET];      // {mean.x, mean.y, conic.x, conic.y}
    __shared__ float2 s_r1[GS_BUCKET];      // {conic.z, opacity}
    __shared__ uint32_t s_gid[GS_BUCKET];
    __shared__ float s_sum[4][GS_BUCKET];
    __shared__ uint32_t s_max[4][GS_BUCKET];
    __shared__ uint32_t s_cnt[4][GS_BUCKET];
    __shared__ uint32_t s_nc[4];
#if CONTRIB_ERR
    __shared__ float s_err[4][GS_BUCKET];
#endif
#if CONTRIB_FREE
    __shared__ float s_z[GS_BUCKET];        // the entry's view depth (rec[3g + 2].y)
    __shared__ float s_free[4][GS_BUCKET];
    __shared__ float s_meas[4][GS_BUCKET];
#endif
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
#if CONTRIB_ERR
    float ep = 0.0f;   // this pixel's e(p); a pixel outside the image blends nothing (nc = 0)
    if (px < a.W && py < a.H) ep = error_value(err[(size_t)py * a.W + px]);
#endif
#if CONTRIB_FREE
    float nb = 0.0f;   // this pixel's near bound; a pixel outside the image blends nothing (nc = 0)
    if (px < a.W && py < a.H) nb = near_bound[(size_t)py * a.W + px];
    const bool measured = nb > 0.0f;   // NaN, 0 and negative values are not measured; +inf is
#endif
    const float kL2E = GS_EXP_L2E, kCC = GS_EXP_CC;
    float T = 1.0f;
    for (uint32_t base = 0; base < tnc; base += GS_BUCKET) {
        const uint32_t m = (tnc - base) < GS_BUCKET ? (tnc - base) : GS_BUCKET;
        if (tid < (int)m) {
            const uint32_t g = a.point_list[range.x + base + (uint32_t)tid];
            float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0;
            if (g < (uint32_t)a.P) { r0 = a.rec[GS_REC_F4 * (size_t)g]; r1 = a.rec[GS_REC_F4 * (size_t)g + 1]; }   // (else opacity 0: never blended)
            s_r0[tid] = r0; s_r1[tid] = make_float2(r1.x, r1.y); s_gid[tid] = g;
#if CONTRIB_FREE
            s_z[tid] = g < (uint32_t)a.P ? reinterpret_cast<const float*>(a.rec + GS_REC_F4 * (size_t)g + 2)[1] : 0.0f;   // .y alone: one dword, not a third float4
#endif
        }
        __syncthreads();
        float esum = 0.0f;
#if CONTRIB_ERR
        float eerr = 0.0f;
#endif
#if CONTRIB_FREE
        float efree = 0.0f, emeas = 0.0f;
#endif
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
#if CONTRIB_ERR
                const float we = wave_sum_butterfly(w * ep);   // the product rounded on its own (contract off); a lane that skips adds +0
                if (lane == (int)j) eerr = we;
#endif
#if CONTRIB_FREE
                const float wm = wave_sum_butterfly(measured ? w : 0.0f);                     // w or +0: no arithmetic on the addend
                const float wf = wave_sum_butterfly((measured & (s_z[j] < nb)) ? w : 0.0f);   // strict float32 <
                if (lane == (int)j) { emeas = wm; efree = wf; }
#endif
            }
        }
        s_sum[wave][lane] = esum; s_max[wave][lane] = emax; s_cnt[wave][lane] = ecnt;
#if CONTRIB_ERR
        s_err[wave][lane] = eerr;
#endif
#if CONTRIB_FREE
        s_free[wave][lane] = efree; s_meas[wave][lane] = emeas;
#endif
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
#if CONTRIB_ERR
                const float es = ((s_err[0][lane] + s_err[1][lane]) + s_err[2][lane]) + s_err[3][lane];   // wave order, like `sum`
                const unsigned long long qe = __float2ull_rn(es * 4294967296.0f);   // <= 1024 * 2^32 = 2^42
                if (qe != 0ull) atomicAdd(err_sum + g, qe);
#endif
#if CONTRIB_FREE
                const float ms = ((s_meas[0][lane] + s_meas[1][lane]) + s_meas[2][lane]) + s_meas[3][lane];   // wave order, like `sum`
                const float fs = ((s_free[0][lane] + s_free[1][lane]) + s_free[2][lane]) + s_free[3][lane];
                const unsigned long long qm = __float2ull_rn(ms * 4294967296.0f), qf = __float2ull_rn(fs * 4294967296.0f);   // each <= 256 * 2^32
                if (qm != 0ull) atomicAdd(meas_sum + g, qm);
                if (qf != 0ull) atomicAdd(free_sum + g, qf);
#endif
            }
        }
        // (wave 0 stages the next batch behind its atomics; the other waves wait for it at the barrier above before they touch s_sum again)
    }
