// pose.hip — the trainable keyframe pose set: gslic_pose_step (the se(3) chain of the three camera gradients, torch-style Adam on the six tangent
// coordinates, the exact retraction T_cw <- exp(delta^) T_cw, Gram-Schmidt on R and the three arrays the rasteriser reads, recomposed) and
// gslic_pose_load (row *view_word of the set copied into a step's static buffers).  The rule is written out in include/gslic_hip.h; every float32
// product and sum here is one operation rounded on its own (fp contract off), the Adam bias terms and the three exp coefficients are in double
// and rounded to float once, as the header names them.
//
// Both are ONE launch of ONE wave.  The step is a serial chain of a few hundred operations on 35 + 35 + 16 + 12 floats: lane 0 runs it from start
// to end in the order the header states — no cross-lane reduction, so no sum depends on a reduction order — and leaves the results in LDS; after the
// barrier the lanes store them (one lane per float: vector stores).  The cost is the launch, not the arithmetic.  No atomics, no allocation, no
// read-back: capturable in a graph.
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

static constexpr int POSE_THREADS = 64;
static constexpr double POSE_SERIES_BELOW = GSLIC_POSE_SERIES_THETA;   // theta below this: the series coefficients

// what a launch writes (block-uniform, decided by lane 0)
static constexpr int POSE_W_GRAD = 1, POSE_W_MOMENTS = 2, POSE_W_POSE = 4;

struct PoseStepArgs {
    float *view_all, *proj_all, *campos_all, *m, *v;
    int32_t* step_count;
    const float* projection;
    const int32_t* view;
    const uint32_t* skip;
    int32_t n_views;
    float lr_trans, lr_rot, beta1, beta2, eps;
};

__device__ __forceinline__ bool pose_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // (false for NaN and +-inf)

__global__ __launch_bounds__(POSE_THREADS) void pose_step_kernel(PoseStepArgs a, const float* __restrict__ dL_dview, const float* __restrict__ dL_dproj,
                                                                 const float* __restrict__ dL_dcampos, float* __restrict__ grad_out)
{
#pragma clang fp contract(off)
    __shared__ float s_view[16], s_proj[16], s_campos[3], s_m[6], s_v[6], s_g[6];
    __shared__ int32_t s_steps, s_what, s_row;
    if (threadIdx.x == 0) {
        int what = 0;
        const int32_t row = a.view[0];
        s_row = row;
        if (row >= 0 && row < a.n_views) {
            what = POSE_W_GRAD;
            const float* vw = a.view_all + 16 * (size_t)row;
            // V = [R | t] (element (r, c) at [4 c + r]), Pm the projection in the same layout
            float R[3][3], t[3], Pm[4][4];
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int r = 0; r < 3; r++) R[r][c] = vw[4 * c + r];
#pragma unroll
            for (int r = 0; r < 3; r++) t[r] = vw[12 + r];
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) Pm[r][c] = a.projection[4 * c + r];
            const float gc[3] = {dL_dcampos[0], dL_dcampos[1], dL_dcampos[2]};
            // ---- chain: G = dL/dV + Pm^T dL/d(PV), top three rows
            float G[3][4];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float s = ((Pm[0][r] * dL_dproj[4 * c] + Pm[1][r] * dL_dproj[4 * c + 1]) + Pm[2][r] * dL_dproj[4 * c + 2]) + Pm[3][r] * dL_dproj[4 * c + 3];
                    G[r][c] = dL_dview[4 * c + r] + s;
                }
            float GR[3][3], Gt[3], M[3][3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) GR[r][c] = G[r][c] - t[r] * gc[c];
                Gt[r] = G[r][3] - ((R[r][0] * gc[0] + R[r][1] * gc[1]) + R[r][2] * gc[2]);
            }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) M[r][c] = (GR[r][0] * R[c][0] + GR[r][1] * R[c][1]) + GR[r][2] * R[c][2];
            float g[6];
            g[0] = Gt[0]; g[1] = Gt[1]; g[2] = Gt[2];
            g[3] = (M[2][1] - M[1][2]) + (t[1] * Gt[2] - t[2] * Gt[1]);
            g[4] = (M[0][2] - M[2][0]) + (t[2] * Gt[0] - t[0] * Gt[2]);
            g[5] = (M[1][0] - M[0][1]) + (t[0] * Gt[1] - t[1] * Gt[0]);
            bool finite = true;
#pragma unroll
            for (int k = 0; k < 6; k++) { s_g[k] = g[k]; finite = finite && pose_finite(g[k]); }
            const bool skipped = a.skip && (a.skip[0] & 27u) != 0;
            if (finite && !skipped) {
                what |= POSE_W_MOMENTS;
                // ---- Adam (torch.optim.Adam with bias correction; the two bias terms in double from the integer step, each rounded once)
                const int32_t n = a.step_count[row] + 1;
                s_steps = n;
                const double bc1 = 1.0 - pow((double)a.beta1, (double)n), bc2 = 1.0 - pow((double)a.beta2, (double)n);
                const float s_tr = (float)((double)a.lr_trans / bc1), s_rot = (float)((double)a.lr_rot / bc1), q = (float)sqrt(bc2);
                float d[6];
                bool moved = false, d_finite = true;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    const float m = a.beta1 * a.m[6 * (size_t)row + k] + (1.0f - a.beta1) * g[k];
                    const float v = a.beta2 * a.v[6 * (size_t)row + k] + ((1.0f - a.beta2) * g[k]) * g[k];
                    s_m[k] = m;
                    s_v[k] = v;
                    d[k] = -(((k < 3 ? s_tr : s_rot) * m) / (sqrtf(v) / q + a.eps));
                    moved = moved || d[k] != 0.0f;
                    d_finite = d_finite && pose_finite(d[k]);
                }
                if (moved && d_finite) {
                    what |= POSE_W_POSE;
                    // ---- retraction: exp of (rho, phi) = (d[0..2], d[3..5]); theta and the three coefficients in double, rounded once
                    const float px = d[3], py = d[4], pz = d[5];
                    const double th2 = ((double)px * (double)px + (double)py * (double)py) + (double)pz * (double)pz;
                    const double th = sqrt(th2);
                    double ca, cb, cc;
                    if (th < POSE_SERIES_BELOW) {
                        ca = 1.0 - th2 / 6.0; cb = 0.5 - th2 / 24.0; cc = 1.0 / 6.0 - th2 / 120.0;
                    } else {
                        ca = sin(th) / th; cb = (1.0 - cos(th)) / th2; cc = (th - sin(th)) / (th2 * th);
                    }
                    const float fa = (float)ca, fb = (float)cb, fc = (float)cc;
                    const float K[3][3] = {{0.f, -pz, py}, {pz, 0.f, -px}, {-py, px, 0.f}};
                    // K^2 = phi phi^T - theta^2 I, written without the cancellation on the diagonal
                    const float K2[3][3] = {{-(py * py + pz * pz), px * py, px * pz}, {px * py, -(px * px + pz * pz), py * pz}, {px * pz, py * pz, -(px * px + py * py)}};
                    float Rm[3][3], Vm[3][3], Et[3];
#pragma unroll
                    for (int r = 0; r < 3; r++)
#pragma unroll
                        for (int c = 0; c < 3; c++) {
                            const float one = r == c ? 1.f : 0.f;
                            Rm[r][c] = (one + fa * K[r][c]) + fb * K2[r][c];
                            Vm[r][c] = (one + fb * K[r][c]) + fc * K2[r][c];
                        }
#pragma unroll
                    for (int r = 0; r < 3; r++) Et[r] = (Vm[r][0] * d[0] + Vm[r][1] * d[1]) + Vm[r][2] * d[2];
                    float Rn[3][3], tn[3];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int c = 0; c < 3; c++) Rn[r][c] = (Rm[r][0] * R[0][c] + Rm[r][1] * R[1][c]) + Rm[r][2] * R[2][c];
                        tn[r] = ((Rm[r][0] * t[0] + Rm[r][1] * t[1]) + Rm[r][2] * t[2]) + Et[r];
                    }
                    // ---- Gram-Schmidt on the rows, in the order 0, 1; row 2 = row 0 x row 1
                    const float n0 = sqrtf((Rn[0][0] * Rn[0][0] + Rn[0][1] * Rn[0][1]) + Rn[0][2] * Rn[0][2]);
                    const float r0[3] = {Rn[0][0] / n0, Rn[0][1] / n0, Rn[0][2] / n0};
                    const float dot = (r0[0] * Rn[1][0] + r0[1] * Rn[1][1]) + r0[2] * Rn[1][2];
                    const float u[3] = {Rn[1][0] - dot * r0[0], Rn[1][1] - dot * r0[1], Rn[1][2] - dot * r0[2]};
                    const float n1 = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
                    const float r1[3] = {u[0] / n1, u[1] / n1, u[2] / n1};
                    const float r2[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
                    float V[4][4];
#pragma unroll
                    for (int c = 0; c < 3; c++) { V[0][c] = r0[c]; V[1][c] = r1[c]; V[2][c] = r2[c]; V[3][c] = 0.f; }
                    V[0][3] = tn[0]; V[1][3] = tn[1]; V[2][3] = tn[2]; V[3][3] = 1.f;
                    // ---- recompose: view, proj = Pm V (k ascending), campos = -R^T t
#pragma unroll
                    for (int c = 0; c < 4; c++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            s_view[4 * c + r] = V[r][c];
                            s_proj[4 * c + r] = ((Pm[r][0] * V[0][c] + Pm[r][1] * V[1][c]) + Pm[r][2] * V[2][c]) + Pm[r][3] * V[3][c];
                        }
#pragma unroll
                    for (int c = 0; c < 3; c++) s_campos[c] = -((V[0][c] * tn[0] + V[1][c] * tn[1]) + V[2][c] * tn[2]);
                }
            }
        }
        s_what = what;
    }
    __syncthreads();
    const int what = s_what;
    const size_t row = (size_t)s_row;
    const int l = threadIdx.x;
    if ((what & POSE_W_GRAD) && l < 6) grad_out[l] = s_g[l];
    if (what & POSE_W_MOMENTS) {
        if (l < 6) { a.m[6 * row + l] = s_m[l]; a.v[6 * row + l] = s_v[l]; }
        if (l == 6) a.step_count[row] = s_steps;
    }
    if (what & POSE_W_POSE) {
        if (l < 16) { a.view_all[16 * row + l] = s_view[l]; a.proj_all[16 * row + l] = s_proj[l]; }
        if (l < 3) a.campos_all[3 * row + l] = s_campos[l];
    }
}

__global__ __launch_bounds__(POSE_THREADS) void pose_load_kernel(const float* __restrict__ view_all, const float* __restrict__ proj_all,
                                                                 const float* __restrict__ campos_all, const int32_t* __restrict__ view_word,
                                                                 int32_t n_views, float* __restrict__ view_out, float* __restrict__ proj_out,
                                                                 float* __restrict__ campos_out)
{
    const int32_t row = view_word[0];
    if (row < 0 || row >= n_views) return;   // (a host validates the index before it fills the word)
    const int l = threadIdx.x;
    if (l < 16) view_out[l] = view_all[16 * (size_t)row + l];
    else if (l < 32) proj_out[l - 16] = proj_all[16 * (size_t)row + (l - 16)];
    else if (l < 35) campos_out[l - 32] = campos_all[3 * (size_t)row + (l - 32)];
}

int pose_step(const gslic_pose_adam* d, const float* dL_dviewmatrix, const float* dL_dprojmatrix, const float* dL_dcampos, float* grad_out, hipStream_t s)
{
    PoseStepArgs a{};
    a.view_all = d->view_all; a.proj_all = d->proj_all; a.campos_all = d->campos_all; a.m = d->m; a.v = d->v; a.step_count = d->step_count;
    a.projection = d->projection; a.view = d->view; a.skip = d->skip; a.n_views = d->n_views;
    a.lr_trans = d->lr_trans; a.lr_rot = d->lr_rot; a.beta1 = d->beta1; a.beta2 = d->beta2; a.eps = d->eps;
    GS_LAUNCH(K_DEPTH_LOSS, pose_step_kernel, dim3(1), dim3(POSE_THREADS), 0, s, a, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, grad_out);
    return GSLIC_OK;
}

int pose_load(const float* view_all, const float* proj_all, const float* campos_all, const int32_t* view_word, int n_views, float* view_out,
              float* proj_out, float* campos_out, hipStream_t s)
{
    GS_LAUNCH(K_DEPTH_LOSS, pose_load_kernel, dim3(1), dim3(POSE_THREADS), 0, s, view_all, proj_all, campos_all, view_word, (int32_t)n_views, view_out,
              proj_out, campos_out);
    return GSLIC_OK;
}

}  // namespace gslic
