// ehr_intrinsics.hip -- intrinsics refinement: the one small kernel that follows the solver step's launch chain when the
// focal lengths and the principal point are fitted together with the camera pose (easyhec_amd/intrinsics_calib.py).
//
//   theta [4] float32, dimensionless:   fu = K0[0] exp(theta0)   fv = K0[4] exp(theta1)   cu = K0[2] + W theta2   cv = K0[5] + H theta3
//   intrinsics_backward_adam: grad_mvp [B,L,16] (written by the chain) -> d(sum_b loss_b) / d theta.  MVP_bl = P(K) @ A_bl with
//                        A_bl = F @ Tc @ link_poses[b,l], F = diag(1,-1,-1,1), Tc = tc_jac[0:16] (the pose that was rendered),
//                        and projection() is linear in fu, fv, cu, cv: P[0] = 2 fu / W, P[5] = 2 fv / H, P[2] = 1 - 2 cu / W,
//                        P[6] = 2 cv / H - 1.  With Q[r,k] = sum_{b,l} sum_c grad_mvp[b,l][r,c] A_bl[k,c]:
//                            s0 = fu (2/W) Q[0,0]    s1 = fv (2/H) Q[1,1]    s2 = -2 Q[0,2]    s3 = 2 Q[1,2]
//                        -> the Adam update (group_adam) on the free elements -> the K the next step's vertex head reads.
//
// The kernel does not allocate, synchronise or use an atomic: results are bit-reproducible from run to run.
#include "ehr_host.h"
#include "ehr_pose_core.h"
#include "ehr_group_adam.h"

namespace ehr {

// One entry of K from K0 and its parameter, evaluated in float64 and rounded once.  i: 0 fu, 1 fv, 2 cu, 3 cv.  A parameter
// that is exactly zero gives K0's bits (selected, not left to exp(0.0) == 1.0).
__device__ __forceinline__ float intrinsics_entry(const float* __restrict__ K0, float th, int i, int H, int W) {
    const float k0 = K0[i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 2 : 5))];
    double x;
    if (i < 2)
        x = (double)k0 * exp((double)th);
    else
        x = (double)k0 + (double)(i == 2 ? W : H) * (double)th;
    return th == 0.f ? k0 : (float)x;
}

// Q[0,0], Q[1,1], Q[0,2], Q[1,2] of one camera; call with all 256 threads of the single workgroup.  Thread t adds pairs t,
// t + 256, ... in order into four float64 accumulators of its own (products and sums float64 from float32 inputs); every wave
// combines with wave_sum_f64 and leaves its four sums in S[wave][0..3], which the caller adds in order: ((S0 + S1) + S2) + S3.
// Ends on a barrier (S is readable); its write to S comes after a barrier of its own, so a caller may read S and call again.
__device__ __forceinline__ void intrinsics_sums(const float* __restrict__ grad_mvp, const float* __restrict__ tc_jac,
                                                const float* __restrict__ link_poses, int B, int L, double (*S)[4]) {
    const int tid = threadIdx.x;
    double T[3][4];  // rows 0..2 of Tc = tc_jac[0:16]: the pose this step rendered
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) T[k][j] = (double)tc_jac[4 * k + j];
    double q00 = 0.0, q11 = 0.0, q02 = 0.0, q12 = 0.0;
    const int BL = B * L;
    for (int i = tid; i < BL; i += 256) {
        float g[8], lp[16];
#pragma unroll
        for (int k = 0; k < 16; k++) lp[k] = link_poses[(size_t)i * 16 + k];
#pragma unroll
        for (int k = 0; k < 8; k++) g[k] = grad_mvp[(size_t)i * 16 + k];
        double A[3][4];  // rows 0..2 of F @ Tc @ lp
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const double a = ((T[k][0] * (double)lp[c] + T[k][1] * (double)lp[4 + c]) + T[k][2] * (double)lp[8 + c]) +
                                 T[k][3] * (double)lp[12 + c];
                A[k][c] = k == 0 ? a : -a;
            }
        q00 += ((double)g[0] * A[0][0] + (double)g[1] * A[0][1]) + ((double)g[2] * A[0][2] + (double)g[3] * A[0][3]);
        q11 += ((double)g[4] * A[1][0] + (double)g[5] * A[1][1]) + ((double)g[6] * A[1][2] + (double)g[7] * A[1][3]);
        q02 += ((double)g[0] * A[2][0] + (double)g[1] * A[2][1]) + ((double)g[2] * A[2][2] + (double)g[3] * A[2][3]);
        q12 += ((double)g[4] * A[2][0] + (double)g[5] * A[2][1]) + ((double)g[6] * A[2][2] + (double)g[7] * A[2][3]);
    }
    q00 = wave_sum_f64(q00);
    q11 = wave_sum_f64(q11);
    q02 = wave_sum_f64(q02);
    q12 = wave_sum_f64(q12);
    __syncthreads();  // (a previous call's S has been read)
    if ((tid & 63) == 0) {
        S[tid >> 6][0] = q00;
        S[tid >> 6][1] = q11;
        S[tid >> 6][2] = q02;
        S[tid >> 6][3] = q12;
    }
    __syncthreads();
}

// The group's Adam and the new K; call with all 256 threads, behind intrinsics_sums' barrier.  The work is wave 0's alone, so
// it needs no barrier and no LDS of its own: element i < 4 is lane i's (its sum s_i in float64; fu, fv as rendered, i.e. from
// theta before this update; group_adam), which also writes its entry of K; lanes 4..8 write the entries that are K0's.  The
// verdict is the chain's own (red[0..7] finite) and every FREE element's float32 sum finite.  A reported step leaves K alone.
__device__ __forceinline__ void intrinsics_adam(double (*S)[4], const float* __restrict__ red, const float* __restrict__ K0,
                                                const int* __restrict__ free4, int tie_focal, int H, int W,
                                                float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v,
                                                int* __restrict__ step_k, float lr, float b1, float b2, float eps, float wd,
                                                float* __restrict__ K, float* __restrict__ grad_out) {
    const int tid = threadIdx.x & 63;  // the lane: wave 0 goes on alone
    if (threadIdx.x >= 64) return;
    const bool mine = tid < 4 && free4[tid] != 0;
    double d = 0.0;
    if (tid < 4) {
        const double q = ((S[0][tid] + S[1][tid]) + S[2][tid]) + S[3][tid];
        if (tid < 2)
            d = (double)intrinsics_entry(K0, theta[tid], tid, H, W) * (2.0 / (double)(tid == 0 ? W : H)) * q;
        else
            d = (tid == 2 ? -2.0 : 2.0) * q;
    }
    const double other = wave_xor<1>(d);  // (lanes 0 and 1: each other's sum)
    if (tie_focal != 0 && tid < 2) d = tid == 0 ? d + other : other + d;  // s0 + s1 for both
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) ok = ok && (fabsf(red[k]) < 3.0e38f);
    ok = ok && __ballot(mine && !(fabsf((float)d) < 3.0e38f)) == 0;
    const int t = step_k[0] + 1;
    if (tid < 4) group_adam(tid, mine, ok, [&]() { return d; }, red[7], t, theta, m, v, lr, b1, b2, eps, wd, grad_out);
    if (tid < 9 && ok) {
        const int i = tid == 0 ? 0 : (tid == 1 ? 4 : (tid == 2 ? 2 : (tid == 3 ? 5 : -1)));  // lane i < 4: its entry of K
        const int rest = tid == 4 ? 1 : (tid == 5 ? 3 : tid);  // lanes 4..8: entries 1, 3, 6, 7, 8
        if (i >= 0)
            K[i] = intrinsics_entry(K0, theta[tid], tid, H, W);
        else
            K[rest] = K0[rest];
    }
    if (tid == 0 && ok) step_k[0] = t;
}

// Single workgroup of 256 threads: the sums, then the group's Adam and the K of the next step.
__global__ void __launch_bounds__(256) intrinsics_backward_adam_kernel(
    const float* __restrict__ grad_mvp, const float* __restrict__ tc_jac, const float* __restrict__ link_poses, int B, int L,
    int H, int W, const float* __restrict__ red, const float* __restrict__ K0, const int* __restrict__ free4, int tie_focal,
    float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v, int* __restrict__ step_k, float lr, float b1,
    float b2, float eps, float wd, float* __restrict__ K, float* __restrict__ grad_out) {
    __shared__ double S[4][4];
    intrinsics_sums(grad_mvp, tc_jac, link_poses, B, L, S);
    intrinsics_adam(S, red, K0, free4, tie_focal, H, W, theta, m, v, step_k, lr, b1, b2, eps, wd, K, grad_out);
}

}  // namespace ehr

using namespace ehr;

extern "C" {

int ehr_intrinsics_backward_adam(const float* grad_mvp, const float* tc_jac, const float* link_poses, int B, int L, int H,
                                 int W, const float* red, const float* K0, const int32_t* free4, int tie_focal, float* theta,
                                 float* adam_m, float* adam_v, int32_t* step_k, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, float* K, float* grad_out, void* stream) {
    if (!grad_mvp || !tc_jac || !link_poses || !red || !K0 || !free4 || !theta || !adam_m || !adam_v || !step_k || !K)
        return fail(EHR_ERR_INVALID, "ehr_intrinsics_backward_adam: NULL tensor");
    if (L < 1 || B < 1 || (long long)B * L > 0x7fffffffll / 16 || H < 1 || W < 1)
        return fail(EHR_ERR_INVALID, "ehr_intrinsics_backward_adam: bad sizes (L %d, B %d, H %d, W %d)", L, B, H, W);
    intrinsics_backward_adam_kernel<<<1, 256, 0, (hipStream_t)stream>>>(grad_mvp, tc_jac, link_poses, B, L, H, W, red, K0,
                                                                        free4, tie_focal, theta, adam_m, adam_v, step_k, lr,
                                                                        beta1, beta2, eps, weight_decay, K, grad_out);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
