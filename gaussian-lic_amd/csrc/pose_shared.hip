// pose_shared.hip — the calibration a pose set's views share: gslic_pose_step_shared (gslic_pose_step's chain on row *view, the time-offset gradient
// xi_i . g, Adam on the seven coordinates (rho_x, phi_x, tau), then EVERY row moved by d_x + d_tau xi_j through gslic_pose_step's retraction,
// Gram-Schmidt and recomposition, the accumulated correction X by d_x and tau by d_tau) and gslic_pose_calibrate_rows (a freshly loaded row
// brought to the calibration: T <- exp((tau xi_j)^) (X T)).  The rule is written out in include/gslic_hip.h; every float32 product and sum here is
// one operation rounded on its own (fp contract off), the Adam bias terms and the three exp coefficients are in double and rounded to float once.
//
// The step is ONE launch of ONE workgroup (a second one would race with the moment update).  Thread 0 runs chain and Adam in the order the header
// states — no cross-lane reduction — and leaves the gradient, the moments, the seven deltas and the write decision in LDS; after the barrier the
// threads stride over the rows, each running one row's whole rule alone, so no result depends on a reduction order or on V.  The chain and the
// move are copies of pose.hip's statements (pose_step_kernel itself is not touched: its machine code stays what it was).  No atomics, no
// allocation, no read-back: capturable in a graph.  All stores are plain vector stores.
#include "gslic_common.h"
#include "kernels.h"

namespace gslic {

static constexpr int PSH_THREADS = 256;
static constexpr double PSH_SERIES_BELOW = GSLIC_POSE_SERIES_THETA;   // theta below this: the series coefficients

// what a launch writes (block-uniform, decided by thread 0)
static constexpr int PSH_W_GRAD = 1, PSH_W_MOMENTS = 2;

struct PoseSharedArgs {
    float *view_all, *proj_all, *campos_all;
    const float *projection, *twist;
    const int32_t* view;
    const uint32_t* skip;
    float *sm, *sv, *X, *tau;
    int32_t* ssteps;
    int32_t n_views;
    float lr_trans, lr_rot, lr_time, beta1, beta2, eps;
};

__device__ __forceinline__ bool psh_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // (false for NaN and +-inf)

// whether an increment moves anything: not zero in all six coordinates, and finite in every one
__device__ __forceinline__ bool psh_moves(const float d[6])
{
    bool moved = false, finite = true;
#pragma unroll
    for (int k = 0; k < 6; k++) { moved = moved || d[k] != 0.0f; finite = finite && psh_finite(d[k]); }
    return moved && finite;
}

// RETRACTION and RE-ORTHONORMALISATION of gslic_pose_step on a 3x4 [R | t]: Ro (rows r0, r1, r2), tn <- exp(d^) [R | t]
__device__ __forceinline__ void psh_retract(const float R[3][3], const float t[3], const float d[6], float Ro[3][3], float tn[3])
{
#pragma clang fp contract(off)
    const float px = d[3], py = d[4], pz = d[5];
    const double th2 = ((double)px * (double)px + (double)py * (double)py) + (double)pz * (double)pz;
    const double th = sqrt(th2);
    double ca, cb, cc;
    if (th < PSH_SERIES_BELOW) {
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
    float Rn[3][3];
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
#pragma unroll
    for (int c = 0; c < 3; c++) { Ro[0][c] = r0[c]; Ro[1][c] = r1[c]; Ro[2][c] = r2[c]; }
}

// RECOMPOSITION of gslic_pose_step: the row's view, proj = Pm V (k ascending) and campos = -R^T t, stored by the calling thread
__device__ __forceinline__ void psh_store_row(const float Ro[3][3], const float tn[3], const float* __restrict__ projection, float* view, float* proj,
                                              float* campos)
{
#pragma clang fp contract(off)
    float V[4][4], Pm[4][4];
#pragma unroll
    for (int c = 0; c < 3; c++) { V[0][c] = Ro[0][c]; V[1][c] = Ro[1][c]; V[2][c] = Ro[2][c]; V[3][c] = 0.f; }
    V[0][3] = tn[0]; V[1][3] = tn[1]; V[2][3] = tn[2]; V[3][3] = 1.f;
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) Pm[r][c] = projection[4 * c + r];
#pragma unroll
    for (int c = 0; c < 4; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            view[4 * c + r] = V[r][c];
            proj[4 * c + r] = ((Pm[r][0] * V[0][c] + Pm[r][1] * V[1][c]) + Pm[r][2] * V[2][c]) + Pm[r][3] * V[3][c];
        }
#pragma unroll
    for (int c = 0; c < 3; c++) campos[c] = -((V[0][c] * tn[0] + V[1][c] * tn[1]) + V[2][c] * tn[2]);
}

// [R | t] of a row's view array (element (r, c) at [4 c + r])
__device__ __forceinline__ void psh_load_row(const float* vw, float R[3][3], float t[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int r = 0; r < 3; r++) R[r][c] = vw[4 * c + r];
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] = vw[12 + r];
}

__global__ __launch_bounds__(PSH_THREADS) void pose_shared_step_kernel(PoseSharedArgs a, const float* __restrict__ dL_dview,
                                                                       const float* __restrict__ dL_dproj, const float* __restrict__ dL_dcampos,
                                                                       float* __restrict__ grad_out)
{
#pragma clang fp contract(off)
    __shared__ float s_m[7], s_v[7], s_g[7], s_d[7];
    __shared__ int32_t s_steps, s_what;
    if (threadIdx.x == 0) {
        int what = 0;
        const int32_t row = a.view[0];
        if (row >= 0 && row < a.n_views) {
            what = PSH_W_GRAD;
            float R[3][3], t[3], Pm[4][4];
            psh_load_row(a.view_all + 16 * (size_t)row, R, t);
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
            float g[7];
            g[0] = Gt[0]; g[1] = Gt[1]; g[2] = Gt[2];
            g[3] = (M[2][1] - M[1][2]) + (t[1] * Gt[2] - t[2] * Gt[1]);
            g[4] = (M[0][2] - M[2][0]) + (t[2] * Gt[0] - t[0] * Gt[2]);
            g[5] = (M[1][0] - M[0][1]) + (t[0] * Gt[1] - t[1] * Gt[0]);
            // ---- the time offset: xi_i . g, k ascending
            const float* xi = a.twist + 6 * (size_t)row;
            g[6] = ((((g[0] * xi[0] + g[1] * xi[1]) + g[2] * xi[2]) + g[3] * xi[3]) + g[4] * xi[4]) + g[5] * xi[5];
            bool finite = true;
#pragma unroll
            for (int k = 0; k < 7; k++) { s_g[k] = g[k]; finite = finite && psh_finite(g[k]); }
            const bool skipped = a.skip && (a.skip[0] & 27u) != 0;
            if (finite && !skipped) {
                what |= PSH_W_MOMENTS;
                // ---- Adam (torch.optim.Adam with bias correction; the two bias terms in double from the integer step, each rounded once)
                const int32_t n = a.ssteps[0] + 1;
                s_steps = n;
                const double bc1 = 1.0 - pow((double)a.beta1, (double)n), bc2 = 1.0 - pow((double)a.beta2, (double)n);
                const float s_tr = (float)((double)a.lr_trans / bc1), s_rot = (float)((double)a.lr_rot / bc1), s_time = (float)((double)a.lr_time / bc1);
                const float q = (float)sqrt(bc2);
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    const float m = a.beta1 * a.sm[k] + (1.0f - a.beta1) * g[k];
                    const float v = a.beta2 * a.sv[k] + ((1.0f - a.beta2) * g[k]) * g[k];
                    s_m[k] = m;
                    s_v[k] = v;
                    s_d[k] = -(((k < 3 ? s_tr : (k < 6 ? s_rot : s_time)) * m) / (sqrtf(v) / q + a.eps));
                }
            }
        }
        s_what = what;
    }
    __syncthreads();
    const int what = s_what;
    const int l = threadIdx.x;
    if ((what & PSH_W_GRAD) && l < 7) grad_out[l] = s_g[l];
    if (!(what & PSH_W_MOMENTS)) return;   // (block-uniform)
    if (l < 7) { a.sm[l] = s_m[l]; a.sv[l] = s_v[l]; }
    if (l == 7) a.ssteps[0] = s_steps;
    float dx[6];
#pragma unroll
    for (int k = 0; k < 6; k++) dx[k] = s_d[k];
    const float dtau = s_d[6];
    // ---- MOVE: every row by d_j = d_x + d_tau xi_j, one thread per row
    for (int32_t j = l; j < a.n_views; j += PSH_THREADS) {
        const float* xi = a.twist + 6 * (size_t)j;
        float d[6];
#pragma unroll
        for (int k = 0; k < 6; k++) d[k] = dx[k] + dtau * xi[k];
        if (!psh_moves(d)) continue;
        float R[3][3], t[3], Ro[3][3], tn[3];
        psh_load_row(a.view_all + 16 * (size_t)j, R, t);
        psh_retract(R, t, d, Ro, tn);
        psh_store_row(Ro, tn, a.projection, a.view_all + 16 * (size_t)j, a.proj_all + 16 * (size_t)j, a.campos_all + 3 * (size_t)j);
    }
    // ---- the accumulated correction: X by d_x (the 3x4 alone, rows of [R_x | t_x]), tau by d_tau
    if (l == PSH_THREADS - 1) {
        if (psh_moves(dx)) {
            float R[3][3], t[3], Ro[3][3], tn[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) R[r][c] = a.X[4 * r + c];
                t[r] = a.X[4 * r + 3];
            }
            psh_retract(R, t, dx, Ro, tn);
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) a.X[4 * r + c] = Ro[r][c];
                a.X[4 * r + 3] = tn[r];
            }
        }
        if (dtau != 0.0f && psh_finite(dtau)) a.tau[0] = a.tau[0] + dtau;
    }
}

// one thread per row of [first, first + count): T <- exp((tau xi_j)^) (X T)
__global__ __launch_bounds__(PSH_THREADS) void pose_calibrate_rows_kernel(PoseSharedArgs a, int32_t first, int32_t count)
{
#pragma clang fp contract(off)
    const int32_t k = (int32_t)(blockIdx.x * PSH_THREADS + threadIdx.x);
    if (k >= count) return;
    const int32_t j = first + k;
    if (j < 0 || j >= a.n_views) return;   // (the host validates the range)
    const float tau = a.tau[0];
    const float* xi = a.twist + 6 * (size_t)j;
    float d[6];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 6; c++) { d[c] = tau * xi[c]; finite = finite && psh_finite(d[c]); }
    if (!finite) return;
    float R[3][3], t[3], XR[3][3], Xt[3], A[3][3], At[3], Ro[3][3], tn[3];
    psh_load_row(a.view_all + 16 * (size_t)j, R, t);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) XR[r][c] = a.X[4 * r + c];
        Xt[r] = a.X[4 * r + 3];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) A[r][c] = (XR[r][0] * R[0][c] + XR[r][1] * R[1][c]) + XR[r][2] * R[2][c];
        At[r] = ((XR[r][0] * t[0] + XR[r][1] * t[1]) + XR[r][2] * t[2]) + Xt[r];
    }
    psh_retract(A, At, d, Ro, tn);
    psh_store_row(Ro, tn, a.projection, a.view_all + 16 * (size_t)j, a.proj_all + 16 * (size_t)j, a.campos_all + 3 * (size_t)j);
}

static PoseSharedArgs pose_shared_args(const gslic_pose_shared* d)
{
    PoseSharedArgs a{};
    a.view_all = d->view_all; a.proj_all = d->proj_all; a.campos_all = d->campos_all; a.projection = d->projection; a.twist = d->twist;
    a.view = d->view; a.skip = d->skip; a.sm = d->sm; a.sv = d->sv; a.X = d->X; a.tau = d->tau; a.ssteps = d->ssteps; a.n_views = d->n_views;
    a.lr_trans = d->lr_trans; a.lr_rot = d->lr_rot; a.lr_time = d->lr_time; a.beta1 = d->beta1; a.beta2 = d->beta2; a.eps = d->eps;
    return a;
}

int pose_step_shared(const gslic_pose_shared* d, const float* dL_dviewmatrix, const float* dL_dprojmatrix, const float* dL_dcampos, float* grad_out,
                     hipStream_t s)
{
    const PoseSharedArgs a = pose_shared_args(d);
    GS_LAUNCH(K_DEPTH_LOSS, pose_shared_step_kernel, dim3(1), dim3(PSH_THREADS), 0, s, a, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, grad_out);
    return GSLIC_OK;
}

int pose_calibrate_rows(const gslic_pose_shared* d, int first, int count, hipStream_t s)
{
    const PoseSharedArgs a = pose_shared_args(d);
    const unsigned nblk = (unsigned)((count + PSH_THREADS - 1) / PSH_THREADS);
    GS_LAUNCH(K_DEPTH_LOSS, pose_calibrate_rows_kernel, dim3(nblk), dim3(PSH_THREADS), 0, s, a, (int32_t)first, (int32_t)count);
    return GSLIC_OK;
}

}  // namespace gslic
