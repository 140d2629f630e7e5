// ehr_lm.hip -- Levenberg-Marquardt on the information matrix of the mask loss (easyhec_amd/lm.py): the
// two small kernels that surround ehr_mask_information in one iteration
//
//     [ehr_joint_forward]  ->  ehr_lm_linearize  ->  ehr_mask_information  ->  ehr_lm_update        on one stream.
//
//   lm_linearize : dof, K as rendered, link_poses [, joint_frames] -> mvp [B,L,16] (ehr_pose_forward's, bit for bit: the same
//                  device functions of ehr_pose_core.h) and the tangents dmvp [N,B,L,16] = d MVP[b,l] / d theta_k, evaluated in
//                  float64 at the float32 parameters and rounded once.  One thread per (k, b, l) matrix.
//   lm_update    : the call's info / grad / loss / count -> accept or reject the trial, the damping's schedule, the damped
//                  normal equations (H_acc + lambda D) delta = -g_acc / 2 by a Cholesky factorisation of the scaled system, the
//                  predicted reduction, the stopping rule, and the next trial's parameters (or the accepted ones).  One
//                  workgroup of one wave, float64 throughout, every sum in a fixed order.
//
//   lm_linearize_multi, lm_update_multi : the same two for P hypotheses of ONE problem (easyhec_amd/lm_multi.py, section 6m):
//                  virtual view p * Bv + j takes dof[p] and link_poses[j]; one workgroup per hypothesis updates its own state
//                  block.  Both call the device functions the solo kernels call, so hypothesis p has its solo solve's bits.
//
//   lm_linearize_multi_calib, lm_update_multi_calib<PRIOR> : P hypotheses that each own dof, offsets, theta, K, link poses, joint
//                  frames and prior rows (section 6q): any layout of free joints and intrinsics, the same device functions again.
//
//   lm_update_rig : the update for C cameras that share the joint offsets (easyhec_amd/lm_rig.py, section 6o): ONE system of
//                  6 C + F parameters summed from the cameras' own (6 + F) matrices; its own gathering head, then the steps
//                  every update shares (lm_update_rest) over the rig's parameter accessor.
//
//   lm_update_rig_arrow<PRIOR> : the rig's update on its BLOCK-ARROW system (section 6r): every camera may free its own intrinsics,
//                  which ride in that camera's diagonal block, and N goes up to 182.  One workgroup of 256 threads eliminates
//                  the camera blocks side by side and factors the Schur complement of the shared offsets: the dense
//                  factorisation's arithmetic in the dense order with the structurally zero blocks skipped.
//
//   lm_update<true>, lm_update_rig<true> : the two under a diagonal Gaussian prior sum_k p_k (theta_k - mu_k)^2 (section 6p): its
//                  term joins the objective the accept test sees, p_k and 2 p_k (theta_acc_k - mu_k) the system that is solved;
//                  the stored linearisation stays the data's.  The <false> forms are compiled without any of it.
//
// No kernel here allocates, synchronises or uses an atomic: results are bit-reproducible from run to run.
#include "ehr_host.h"
#include "ehr_pose_core.h"

#define EHR_LM_MAX_RETRIES 8  // non-positive pivots in a row (lambda raised each time) before the solve gives up

namespace ehr {

// ---- float64 forward mode with ONE partial: the exponential map of ehr_pose_core.h (se3_exp_dual) restated in float64 ----------
struct DD {
    double v, d;
};
__device__ __forceinline__ DD dd(double v, double d = 0.0) {
    DD r;
    r.v = v;
    r.d = d;
    return r;
}
__device__ __forceinline__ DD operator+(const DD& a, const DD& b) { return dd(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ DD operator-(const DD& a, const DD& b) { return dd(a.v - b.v, a.d - b.d); }
__device__ __forceinline__ DD operator*(const DD& a, const DD& b) { return dd(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ __forceinline__ DD operator/(const DD& a, const DD& b) {
    const double inv = 1.0 / b.v, q = a.v * inv;
    return dd(q, (a.d - q * b.d) * inv);
}
__device__ __forceinline__ DD ddsqrt(const DD& a) {
    const double s = sqrt(a.v);
    return dd(s, a.d * (0.5 / s));
}
__device__ __forceinline__ DD ddsin(const DD& a) { return dd(sin(a.v), a.d * cos(a.v)); }
__device__ __forceinline__ DD ddcos(const DD& a) { return dd(cos(a.v), -a.d * sin(a.v)); }

// Tc = se3_exp_map(dof) (row-major, [[R, t], [0, 1]]) and d Tc / d dof[which] (which < 0: values only), in float64 at the
// float32 dof; the squared angle is clamped at 1e-4 and the gradient passes only where it is not (torch.clamp).
__device__ void se3_exp_f64(const float* dof, int which, double* T, double* dT) {
    DD x[6];
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = dd((double)dof[i], i == which ? 1.0 : 0.0);
    const DD w0 = x[3], w1 = x[4], w2 = x[5];
    DD nrms = w0 * w0 + w1 * w1 + w2 * w2;
    if (!(nrms.v >= 1e-4)) nrms = dd(1e-4);
    const DD th = ddsqrt(nrms), one = dd(1.0), zero = dd(0.0);
    const DD inv = one / th;
    const DD fac1 = inv * ddsin(th);
    const DD fac2 = inv * inv * (one - ddcos(th));
    const DD fv1 = (one - ddcos(th)) / (th * th);
    const DD fv2 = (th - ddsin(th)) / (th * th * th);
    const DD Kx[9] = {zero, zero - w2, w1, w2, zero, zero - w0, zero - w1, w0, zero};
    DD K2[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) K2[3 * r + c] = Kx[3 * r] * Kx[c] + Kx[3 * r + 1] * Kx[3 + c] + Kx[3 * r + 2] * Kx[6 + c];
    for (int r = 0; r < 3; r++) {
        DD t = zero;
        for (int c = 0; c < 3; c++) {
            const DD I = dd(r == c ? 1.0 : 0.0);
            const DD R = fac1 * Kx[3 * r + c] + fac2 * K2[3 * r + c] + I;
            T[4 * r + c] = R.v;
            dT[4 * r + c] = R.d;
            const DD V = I + Kx[3 * r + c] * fv1 + K2[3 * r + c] * fv2;
            t = t + V * x[c];
        }
        T[4 * r + 3] = t.v;
        dT[4 * r + 3] = t.d;
    }
    for (int c = 0; c < 4; c++) {
        T[12 + c] = c == 3 ? 1.0 : 0.0;
        dT[12 + c] = 0.0;
    }
}

__device__ __forceinline__ void mat4_mul_f64(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++)
            C[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
}

// Which intrinsics element(s) the q-th free intrinsics parameter moves: the order is "f" (tied: elements 0 and 1 together) or
// "fx", "fy", then "cx", "cy" (easyhec_amd/intrinsics_calib.py).  Returns the first element, or -1 past the end.
__device__ __forceinline__ int lm_intrinsics_element(int q, int free4_mask, int tie_focal) {
    if (tie_focal) {
        if (q == 0) return 0;
        q -= 1;
    } else {
        for (int i = 0; i < 2; i++)
            if ((free4_mask >> i) & 1) {
                if (q == 0) return i;
                q -= 1;
            }
    }
    for (int i = 2; i < 4; i++)
        if ((free4_mask >> i) & 1) {
            if (q == 0) return i;
            q -= 1;
        }
    return -1;
}

// One (k, b, l) matrix of the linearisation, for both kernels below: k < 0 -> the matrix itself into `o` (16 floats), else the
// tangent d MVP[b,l] / d theta_k.  dof: the 6 pose coordinates of this view's hypothesis; lpf: link_poses[b,l]; b, l: the view
// and link the joint tables are read at (free joints only).
__device__ __forceinline__ void lm_linearize_matrix(const float* __restrict__ dof, const float* __restrict__ K,
                                                    const float* __restrict__ lpf, int k, int b, int l, int H, int W, float n,
                                                    float f, const float* __restrict__ joint_frames,
                                                    const unsigned* __restrict__ upstream, const int* __restrict__ joint_kind,
                                                    const int* __restrict__ free_list, int F, int J, int free4_mask,
                                                    int tie_focal, float* __restrict__ o) {
    if (k < 0) {  // the matrix itself: pose_forward_kernel's expressions
        Dual<1> T[16];
        se3_exp_dual<1>(dof, 1e-4f, T);
        float Tc[16], P[16], C[16];
        for (int e = 0; e < 16; e++) Tc[e] = T[e].v;
        projection(K, H, W, n, f, P);
        mvp_from_pose(Tc, P, lpf, C);
        for (int e = 0; e < 16; e++) o[e] = C[e];
        return;
    }
    double Tc[16], dTc[16], lp[16], M[16], A[16], out[16];
    se3_exp_f64(dof, k < 6 ? k : -1, Tc, dTc);
    for (int e = 0; e < 16; e++) lp[e] = (double)lpf[e];
    const double fu = (double)K[0], fv = (double)K[4], cu = (double)K[2], cv = (double)K[5];
    const double nn = (double)n, ff = (double)f;
    double PF[16];  // proj(K) @ diag(1,-1,-1,1), in float64 from the float32 K
    for (int e = 0; e < 16; e++) PF[e] = 0.0;
    PF[0] = 2.0 * fu / (double)W;
    PF[2] = -(-2.0 * cu / (double)W + 1.0);
    PF[5] = -(2.0 * fv / (double)H);
    PF[6] = -(2.0 * cv / (double)H - 1.0);
    PF[10] = (ff + nn) / (ff - nn);
    PF[11] = -2.0 * ff * nn / (ff - nn);
    PF[14] = 1.0;
    for (int e = 0; e < 16; e++) out[e] = 0.0;
    if (k < 6) {  // PF @ dTc/ddof_k @ lp
        mat4_mul_f64(dTc, lp, M);
        mat4_mul_f64(PF, M, out);
    } else if (k < 6 + F) {  // PF @ Tc @ D_blj
        const int j = free_list[k - 6];
        const int kind = (j >= 0 && j < J) ? joint_kind[j] : 0;
        if (j >= 0 && j < J && ((upstream[l] >> j) & 1u) && (kind == 1 || kind == 2)) {
            const float* jf = joint_frames + ((size_t)b * J + j) * 6;
            const double a[3] = {(double)jf[0], (double)jf[1], (double)jf[2]};
            double D[16];
            for (int e = 0; e < 16; e++) D[e] = 0.0;
            if (kind == 1) {  // [a]x R_l | a x (t_l - p)
                const double d[3] = {lp[3] - (double)jf[3], lp[7] - (double)jf[4], lp[11] - (double)jf[5]};
                for (int c = 0; c < 3; c++) {
                    D[c] = a[1] * lp[8 + c] - a[2] * lp[4 + c];
                    D[4 + c] = a[2] * lp[c] - a[0] * lp[8 + c];
                    D[8 + c] = a[0] * lp[4 + c] - a[1] * lp[c];
                }
                D[3] = a[1] * d[2] - a[2] * d[1];
                D[7] = a[2] * d[0] - a[0] * d[2];
                D[11] = a[0] * d[1] - a[1] * d[0];
            } else {          // 0 | a
                D[3] = a[0];
                D[7] = a[1];
                D[11] = a[2];
            }
            mat4_mul_f64(Tc, D, M);
            mat4_mul_f64(PF, M, out);
        }
    } else {  // d proj / d theta @ diag(1,-1,-1,1) @ Tc @ lp: the derivatives that ehr_intrinsics_backward_adam's s0..s3 imply
        const int el = lm_intrinsics_element(k - 6 - F, free4_mask, tie_focal);
        mat4_mul_f64(Tc, lp, A);
        for (int c = 0; c < 4; c++) {
            A[4 + c] = -A[4 + c];
            A[8 + c] = -A[8 + c];
        }
        for (int c = 0; c < 4; c++) {
            if (el == 0) out[c] = (2.0 * fu / (double)W) * A[c];
            if (el == 1 || (el == 0 && tie_focal)) out[4 + c] = (2.0 * fv / (double)H) * A[4 + c];
            if (el == 2) out[c] = -2.0 * A[8 + c];
            if (el == 3) out[4 + c] = 2.0 * A[8 + c];
        }
    }
    for (int e = 0; e < 16; e++) o[e] = (float)out[e];
}

__global__ void __launch_bounds__(256) lm_linearize_kernel(const float* __restrict__ dof, const float* __restrict__ K,
                                                           const float* __restrict__ link_poses, int B, int L, int H, int W,
                                                           float n, float f, const float* __restrict__ joint_frames,
                                                           const unsigned* __restrict__ upstream,
                                                           const int* __restrict__ joint_kind, const int* __restrict__ free_list,
                                                           int F, int J, int free4_mask, int tie_focal, int N,
                                                           float* __restrict__ mvp, float* __restrict__ dmvp) {
    const int BL = B * L;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)(N + 1) * BL) return;
    const int k = (int)(idx / BL) - 1, i = (int)(idx % BL);
    const int b = i / L, l = i - b * L;
    lm_linearize_matrix(dof, K, link_poses + (size_t)i * 16, k, b, l, H, W, n, f, joint_frames, upstream, joint_kind, free_list, F,
                        J, free4_mask, tie_focal, k < 0 ? mvp + (size_t)i * 16 : dmvp + ((size_t)k * BL + i) * 16);
}

// P hypotheses: virtual view b = p * Bv + j takes dof[p] and link_poses[j] (ehr_solver_step_multi's layout); pose only.
__global__ void __launch_bounds__(256) lm_linearize_multi_kernel(const float* __restrict__ dof, const float* __restrict__ K,
                                                                 const float* __restrict__ link_poses, int P, int Bv, int L,
                                                                 int H, int W, float n, float f, float* __restrict__ mvp,
                                                                 float* __restrict__ dmvp) {
    const int BL = P * Bv * L;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 7ll * BL) return;
    const int k = (int)(idx / BL) - 1, i = (int)(idx % BL);
    const int b = i / L, l = i - b * L;
    const int p = b / Bv, j = b - p * Bv;
    lm_linearize_matrix(dof + 6 * (size_t)p, K, link_poses + ((size_t)j * L + l) * 16, k, j, l, H, W, n, f, nullptr, nullptr,
                        nullptr, nullptr, 0, 0, 0, 0, k < 0 ? mvp + (size_t)i * 16 : dmvp + ((size_t)k * BL + i) * 16);
}

// P hypotheses with everything of their own (section 6q): virtual view b = p * Bv + j takes dof[p], K[p], ITS link pose and ITS
// joint-frame rows (ehr_joint_forward_multi's layout); any layout of free joints and intrinsics.
__global__ void __launch_bounds__(256) lm_linearize_multi_calib_kernel(
    const float* __restrict__ dof, const float* __restrict__ K, const float* __restrict__ link_poses, int P, int Bv, int L, int H,
    int W, float n, float f, const float* __restrict__ joint_frames, const unsigned* __restrict__ upstream,
    const int* __restrict__ joint_kind, const int* __restrict__ free_list, int F, int J, int free4_mask, int tie_focal, int N,
    float* __restrict__ mvp, float* __restrict__ dmvp) {
    const int BL = P * Bv * L;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)(N + 1) * BL) return;
    const int k = (int)(idx / BL) - 1, i = (int)(idx % BL);
    const int b = i / L, l = i - b * L;
    const int p = b / Bv;
    lm_linearize_matrix(dof + 6 * (size_t)p, K + 9 * (size_t)p, link_poses + (size_t)i * 16, k, b, l, H, W, n, f, joint_frames,
                        upstream, joint_kind, free_list, F, J, free4_mask, tie_focal,
                        k < 0 ? mvp + (size_t)i * 16 : dmvp + ((size_t)k * BL + i) * 16);
}

// ---- the update ---------------------------------------------------------------------------------------------------------------
// ehr_intrinsics.hip's intrinsics_entry (the "writing K" rule of ehr_intrinsics_backward_adam), restated: one entry of K from K0
// and its parameter in float64, rounded once; a parameter that is exactly zero gives K0's bits.
__device__ __forceinline__ float lm_intrinsics_entry(const float* __restrict__ K0, float th, int i, int H, int W) {
    const float k0 = K0[i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 2 : 5))];
    double x;
    if (i < 2)
        x = (double)k0 * exp((double)th);
    else
        x = (double)k0 + (double)(i == 2 ? W : H) * (double)th;
    return th == 0.f ? k0 : (float)x;
}

struct LmParams {  // where the N parameters live: dof, then the free joints' offsets, then the free intrinsics
    float* dof;
    float* offset;
    const int* free_list;
    int F, J;
    float* theta;
    int free4_mask, tie_focal;
    const float* K0;
    float* K;
    int H, W;
};
__device__ __forceinline__ float lm_param_read(const LmParams& p, int k) {
    if (k < 6) return p.dof[k];
    if (k < 6 + p.F) {
        const int j = p.free_list[k - 6];  // (device memory: an index outside the offsets is read nowhere)
        return (j >= 0 && j < p.J) ? p.offset[j] : 0.f;
    }
    return p.theta[lm_intrinsics_element(k - 6 - p.F, p.free4_mask, p.tie_focal)];
}
__device__ __forceinline__ void lm_param_write(const LmParams& p, int k, float x) {
    if (k < 6) {
        p.dof[k] = x;
    } else if (k < 6 + p.F) {
        const int j = p.free_list[k - 6];
        if (j >= 0 && j < p.J) p.offset[j] = x;
    } else {
        const int el = lm_intrinsics_element(k - 6 - p.F, p.free4_mask, p.tie_focal);
        p.theta[el] = x;
        if (p.tie_focal && el == 0) p.theta[1] = x;  // both focal entries move together
    }
}
// K from theta: call with >= 9 threads behind a barrier that follows the writes to theta
__device__ __forceinline__ void lm_write_K(const LmParams& p, int tid) {
    if (p.free4_mask == 0 || tid >= 9) return;
    const int i = tid == 0 ? 0 : (tid == 1 ? 4 : (tid == 2 ? 2 : (tid == 3 ? 5 : -1)));
    const int rest = tid == 4 ? 1 : (tid == 5 ? 3 : tid);
    if (i >= 0)
        p.K[i] = lm_intrinsics_entry(p.K0, p.theta[tid], tid, p.H, p.W);
    else
        p.K[rest] = p.K0[rest];
}

__device__ __forceinline__ bool lm_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// the spacing of float32 at |x| (numpy.spacing of the float32), from the exponent bits: exact, no denormal arithmetic
__device__ __forceinline__ double lm_spacing_f32(float x) {
    const int e = (__float_as_int(x) >> 23) & 0xff;
    return ldexp(1.0, (e == 0 ? 1 : e) - 150);
}

// What the pieces of one update share in LDS; the kernel declares ONE of these and hands it to them.
struct LmShared {
    double Hm[EHR_LM_MAX_PARAMS][EHR_LM_MAX_PARAMS + 1];  // the call's sum, then H_acc
    double A[EHR_LM_MAX_PARAMS][EHR_LM_MAX_PARAMS + 1];   // the scaled, damped system and its factor
    double gv[EHR_LM_MAX_PARAMS], sv[EHR_LM_MAX_PARAMS], yv[EHR_LM_MAX_PARAMS], rv[EHR_LM_MAX_PARAMS], hy[EHR_LM_MAX_PARAMS],
        dl[EHR_LM_MAX_PARAMS];
    double F, cnt, lambda, nu;
    int accept, fail, small;
};
template <bool PRIOR>
struct LmPriorArgs {  // the prior's two device arrays as a kernel argument; without a prior an empty one
    const double *weight, *mean;
};
template <>
struct LmPriorArgs<false> {};
__device__ __forceinline__ const double* lm_prior_weight(const LmPriorArgs<true>& a) { return a.weight; }
__device__ __forceinline__ const double* lm_prior_mean(const LmPriorArgs<true>& a) { return a.mean; }
__device__ __forceinline__ const double* lm_prior_weight(const LmPriorArgs<false>&) { return nullptr; }
__device__ __forceinline__ const double* lm_prior_mean(const LmPriorArgs<false>&) { return nullptr; }
struct LmPriorShared {  // under a prior only: its weights p_k, its means mu_k and its term at the trial
    double pw[EHR_LM_MAX_PARAMS], pm[EHR_LM_MAX_PARAMS];
    double Fp;
};

// An update is three pieces, each called by all 64 threads of the one wave: lm_update_restore (finalize or done: only the
// accepted parameters are written back), a gathering head (step 1: lm_update_gather for one problem's views, the rig's own
// in lm_update_rig_kernel) and lm_update_rest (steps 2-6).  The two that write parameters do so through an accessor P:
// lm_param_read(p, k), lm_param_write(p, k, x) and lm_write_K(p, tid) overloaded for it.
template <class P>
__device__ __forceinline__ bool lm_update_restore(int N, const P& p, int finalize, const double* __restrict__ st) {
    const int tid = threadIdx.x;
    if (finalize == 0 && st[EHR_LM_DONE] == 0.0) return false;
    const bool have = st[EHR_LM_ACCEPTED] > 0.0;  // a point has been accepted
    if (have && tid < N) lm_param_write(p, tid, (float)st[EHR_LM_THETA + tid]);
    __syncthreads();
    if (have) lm_write_K(p, tid);
    return true;
}

// 1. the call's sums, in view order, into sh.Hm, sh.gv, sh.F, sh.cnt; returns this thread's "a sum is bad"
__device__ __forceinline__ int lm_update_gather(const double* __restrict__ info, const double* __restrict__ grad,
                                                const long long* __restrict__ count, const float* __restrict__ loss, int B,
                                                int N, LmShared& sh) {
    const int tid = threadIdx.x;
    int bad = 0;
    for (int e = tid; e < N * N; e += 64) {
        const int r = e / N, c = e - r * N;
        double s = 0.0;
        for (int b = 0; b < B; b++) s += info[((size_t)b * N + r) * N + c];
        sh.Hm[r][c] = s;
        bad |= !lm_finite(s);
    }
    if (tid < N) {
        double s = 0.0;
        for (int b = 0; b < B; b++) s += grad[(size_t)b * N + tid];
        sh.gv[tid] = s;
        bad |= !lm_finite(s);
    }
    if (tid == 0) {
        double s = 0.0, c = 0.0;
        for (int b = 0; b < B; b++) {
            s += (double)loss[b];
            bad |= count[b] < 0;
            c += (double)count[b];
        }
        bad |= !lm_finite(s);
        sh.F = s;
        sh.cnt = c;
    }
    return bad;
}

// Steps 2-6 on what a head left in sh (bad: the head's per-thread flag; it is joined here).
// prior_weight, prior_mean ([N] float64, both or neither): a Gaussian prior sum_k p_k (theta_k - mu_k)^2 beside the data's loss.
// Its term at the trial joins F ahead of step 3 (EHR_LM_F and EHR_LM_F_TRIAL hold the total, EHR_LM_F_PRIOR the term at the
// accepted point); H_acc, g_acc stay the data's own, and p_k, 2 p_k (theta_acc_k - mu_k) are added to the system that steps 4-6
// solve, in both branches of step 3.  A parameter without data information but with p_k > 0 is therefore NOT left out: the prior
// alone pulls it towards mu_k.  PRIOR is a template parameter: the kernels without a prior are compiled without any of it, so
// not one operation of theirs differs from the kernel that had none (ps, prior_weight, prior_mean: unused, may be NULL).
template <bool PRIOR, class P>
__device__ __forceinline__ void lm_update_rest(LmShared& sh, int bad, int N, const P& p, double ftol, double lambda_max,
                                               double* __restrict__ st, double* __restrict__ log, int log_rows,
                                               LmPriorShared* ps, const double* __restrict__ prior_weight,
                                               const double* __restrict__ prior_mean) {
    auto &Hm = sh.Hm, &A = sh.A;  // (the names the steps below were written with)
    auto &gv = sh.gv, &sv = sh.sv, &yv = sh.yv, &rv = sh.rv, &hy = sh.hy, &dl = sh.dl;
    double &sh_F = sh.F, &sh_cnt = sh.cnt, &sh_lambda = sh.lambda, &sh_nu = sh.nu;
    int &sh_accept = sh.accept, &sh_fail = sh.fail, &sh_small = sh.small;
    const int tid = threadIdx.x;
    double* const th_acc = st + EHR_LM_THETA;
    double* const H_acc = st + EHR_LM_H;
    double* const g_acc = st + EHR_LM_G;
    const bool have = st[EHR_LM_ACCEPTED] > 0.0;  // a point has been accepted
    const int it = (int)st[EHR_LM_ITERATIONS];
    double* const row = (log && it < log_rows) ? log + (size_t)it * 4 : nullptr;  // (thread 0's)
    constexpr bool prior = PRIOR;
    // the prior's term at the trial (the parameters as the pointers hold them): Fp = sum_k (p_k d_k) d_k, d_k = theta_k - mu_k,
    // k ascending from 0.0, p_k == 0 skipped; a bad weight, a bad mean under a weight or a non-finite Fp reports the call
    if (prior) {
        if (tid < N) {
            const double w = prior_weight[tid], m = prior_mean[tid];
            double t = 0.0;
            if (!(w >= 0.0) || !lm_finite(w)) {
                bad = 1;
            } else if (w != 0.0) {
                bad |= !lm_finite(m);
                const double d = (double)lm_param_read(p, tid) - m;
                t = (w * d) * d;
            }
            ps->pw[tid] = w;
            ps->pm[tid] = m;
            hy[tid] = t;  // (free until step 4)
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int k = 0; k < N; k++)
                if (ps->pw[k] != 0.0) s += hy[k];
            bad |= !lm_finite(s);
            ps->Fp = s;
        }
    }
    bad = __syncthreads_or(bad);
    // 2. a reported call: the trial is discarded, nothing else moves
    if (bad) {
        if (have && tid < N) lm_param_write(p, tid, (float)th_acc[tid]);
        if (tid == 0) {
            st[EHR_LM_REPORTED] += 1.0;
            st[EHR_LM_ITERATIONS] = (double)(it + 1);
            st[EHR_LM_LAST] = -1.0;
            if (row) {
                row[0] = __longlong_as_double(0x7ff8000000000000ll);
                row[1] = -1.0;
                row[2] = st[EHR_LM_LAMBDA];
                row[3] = __longlong_as_double(0x7ff8000000000000ll);
            }
        }
        __syncthreads();
        if (have) lm_write_K(p, tid);
        return;
    }
    // 3. accept or reject
    if (tid == 0) {
        const double F = prior ? sh_F + ps->Fp : sh_F, F_acc = st[EHR_LM_F];
        double lambda = st[EHR_LM_LAMBDA], nu = st[EHR_LM_NU], rho = 0.0;
        const int accept = !have || F < F_acc;
        if (accept) {
            if (have) {
                rho = (F_acc - F) / st[EHR_LM_PRED];
                const double t = 2.0 * rho - 1.0;
                lambda *= fmax(1.0 / 3.0, 1.0 - t * t * t);
            }
            nu = 2.0;
            st[EHR_LM_F] = F;
            if (prior) st[EHR_LM_F_PRIOR] = ps->Fp;  // (the data's loss at the accepted point: F_acc - F_prior)
            st[EHR_LM_COUNT] = sh_cnt;
            st[EHR_LM_RHO] = rho;
            st[EHR_LM_ACCEPTED] += 1.0;
        } else {
            lambda *= nu;
            nu *= 2.0;
            st[EHR_LM_REJECTED] += 1.0;
        }
        st[EHR_LM_ITERATIONS] = (double)(it + 1);
        st[EHR_LM_LAST] = accept ? 1.0 : 0.0;
        st[EHR_LM_F_TRIAL] = F;
        sh_accept = accept;
        sh_lambda = lambda;
        sh_nu = nu;
        if (row) {
            row[0] = F;
            row[1] = accept ? 1.0 : 0.0;
            row[3] = accept ? rho : __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    __syncthreads();
    if (sh_accept) {
        for (int e = tid; e < N * N; e += 64) {
            const int r = e / N, c = e - r * N;
            H_acc[r * EHR_LM_MAX_PARAMS + c] = Hm[r][c];
        }
        if (tid < N) {
            g_acc[tid] = gv[tid];
            th_acc[tid] = (double)lm_param_read(p, tid);
        }
    } else {  // the stored linearisation: the inputs of this call are not read again
        for (int e = tid; e < N * N; e += 64) {
            const int r = e / N, c = e - r * N;
            Hm[r][c] = H_acc[r * EHR_LM_MAX_PARAMS + c];
        }
        if (tid < N) gv[tid] = g_acc[tid];
    }
    __syncthreads();
    // the prior joins the system that is solved, never the stored one: a rejected call rebuilds what the accepting call solved
    if (prior) {
        if (tid < N && ps->pw[tid] != 0.0) {
            Hm[tid][tid] += ps->pw[tid];
            gv[tid] += 2.0 * ps->pw[tid] * (th_acc[tid] - ps->pm[tid]);
        }
        __syncthreads();
    }
    // 4. (H_acc + lambda D) delta = -g_acc / 2, D = diag H_acc, on the scaled system  (S H S + lambda I) y = -S g / 2,
    //    S = D^-1/2, delta = S y; a parameter whose diagonal entry is <= 0 is left out
    if (tid < N) {
        const double d = Hm[tid][tid];
        sv[tid] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
    }
    __syncthreads();
    int retries = 0;
    for (;;) {
        const double lambda = sh_lambda;
        for (int e = tid; e < N * N; e += 64) {
            const int r = e / N, c = e - r * N;
            double a = Hm[r][c] * sv[r] * sv[c];
            if (r == c) a = sv[r] > 0.0 ? a + lambda : 1.0;
            A[r][c] = a;
        }
        if (tid < N) rv[tid] = -0.5 * gv[tid] * sv[tid];
        if (tid == 0) sh_fail = 0;
        __syncthreads();
        for (int j = 0; j < N; j++) {  // Cholesky, right-looking, the lower triangle in place
            if (tid == 0) {
                double piv = A[j][j];
                if (!(piv > 0.0) || !lm_finite(piv)) {
                    sh_fail = 1;
                    piv = 1.0;
                }
                A[j][j] = sqrt(piv);
            }
            __syncthreads();
            if (tid > j && tid < N) A[tid][j] = A[tid][j] / A[j][j];
            __syncthreads();
            if (tid > j && tid < N)
                for (int k = j + 1; k <= tid; k++) A[tid][k] -= A[tid][j] * A[k][j];
            __syncthreads();
        }
        if (!sh_fail || retries >= EHR_LM_MAX_RETRIES) break;
        retries++;
        __syncthreads();
        if (tid == 0) {  // a non-positive pivot: raise lambda like a rejection and factor again
            sh_lambda *= sh_nu;
            sh_nu *= 2.0;
        }
        __syncthreads();
    }
    if (sh_fail) {  // the factorisation keeps failing: stop on the accepted point
        if (tid < N) lm_param_write(p, tid, (float)th_acc[tid]);
        if (tid == 0) {
            st[EHR_LM_LAMBDA] = sh_lambda;
            st[EHR_LM_NU] = sh_nu;
            st[EHR_LM_RETRIES] += (double)retries;
            st[EHR_LM_DONE] = 1.0;
            st[EHR_LM_WHY] = 4.0;
            if (row) row[2] = sh_lambda;
        }
        __syncthreads();
        lm_write_K(p, tid);
        return;
    }
    for (int j = 0; j < N; j++) {  // L z = r
        if (tid == 0) yv[j] = rv[j] / A[j][j];
        __syncthreads();
        if (tid > j && tid < N) rv[tid] -= A[tid][j] * yv[j];
        __syncthreads();
    }
    for (int j = N - 1; j >= 0; j--) {  // L^T y = z
        if (tid == 0) yv[j] = yv[j] / A[j][j];
        __syncthreads();
        if (tid < j) yv[tid] -= A[j][tid] * yv[j];
        __syncthreads();
    }
    if (tid < N) {
        double s = 0.0;
        for (int c = 0; c < N; c++) s += (Hm[tid][c] * sv[tid] * sv[c]) * yv[c];
        hy[tid] = s;
        dl[tid] = yv[tid] * sv[tid];
        st[EHR_LM_DELTA + tid] = dl[tid];
    }
    __syncthreads();
    // 5, 6. the predicted reduction, the stopping rule, the next trial
    if (tid == 0) {
        const double lambda = sh_lambda;
        double pred = 0.0;
        for (int k = 0; k < N; k++) pred += yv[k] * hy[k] + 2.0 * lambda * (yv[k] * yv[k]);
        int small = 1;
        for (int k = 0; k < N; k++) small = small && (dl[k] == 0.0 || fabs(dl[k]) < lm_spacing_f32((float)th_acc[k]));
        int why = 0;
        if (pred <= ftol * st[EHR_LM_F])
            why = 1;
        else if (lambda >= lambda_max)
            why = 2;
        else if (small)
            why = 3;
        st[EHR_LM_LAMBDA] = lambda;
        st[EHR_LM_NU] = sh_nu;
        st[EHR_LM_PRED] = pred;
        st[EHR_LM_RETRIES] += (double)retries;
        if (why) {
            st[EHR_LM_DONE] = 1.0;
            st[EHR_LM_WHY] = (double)why;
        }
        if (row) row[2] = lambda;
        sh_small = why;
    }
    __syncthreads();
    if (tid < N) lm_param_write(p, tid, sh_small ? (float)th_acc[tid] : (float)(th_acc[tid] + dl[tid]));
    __syncthreads();
    lm_write_K(p, tid);
}

template <bool PRIOR>
__global__ void __launch_bounds__(64) lm_update_kernel(const double* __restrict__ info, const double* __restrict__ grad,
                                                       const long long* __restrict__ count, const float* __restrict__ loss,
                                                       int B, int N, LmParams p, double ftol, double lambda_max, int finalize,
                                                       double* __restrict__ st, double* __restrict__ log, int log_rows,
                                                       LmPriorArgs<PRIOR> prior) {
    __shared__ LmShared sh;
    LmPriorShared* ps = nullptr;
    if constexpr (PRIOR) {
        __shared__ LmPriorShared prior_s;
        ps = &prior_s;
    }
    if (lm_update_restore(N, p, finalize, st)) return;
    const int bad = lm_update_gather(info, grad, count, loss, B, N, sh);
    lm_update_rest<PRIOR>(sh, bad, N, p, ftol, lambda_max, st, log, log_rows, ps, lm_prior_weight(prior), lm_prior_mean(prior));
}

// P hypotheses, one workgroup each: hypothesis p owns views [p Bv, (p + 1) Bv), dof[p], state block p and log rows p.  Reported,
// done and finalize are per hypothesis: a workgroup returns or restores by its own block alone.
__global__ void __launch_bounds__(64) lm_update_multi_kernel(const double* __restrict__ info, const double* __restrict__ grad,
                                                             const long long* __restrict__ count,
                                                             const float* __restrict__ loss, int Bv, int N,
                                                             float* __restrict__ dof, double ftol, double lambda_max,
                                                             int finalize, double* __restrict__ st, double* __restrict__ log,
                                                             int log_rows) {
    __shared__ LmShared sh;
    const size_t h = blockIdx.x, v = h * (size_t)Bv;
    const LmParams p = {dof + 6 * h, nullptr, nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr, 0, 0};
    st += h * EHR_LM_STATE_DOUBLES;
    log = log ? log + h * (size_t)log_rows * 4 : nullptr;
    if (lm_update_restore(N, p, finalize, st)) return;
    const int bad = lm_update_gather(info + v * N * N, grad + v * N, count + v, loss + v, Bv, N, sh);
    lm_update_rest<false>(sh, bad, N, p, ftol, lambda_max, st, log, log_rows, nullptr, nullptr, nullptr);  // (pose only: no prior)
}

// P hypotheses that each own a full parameter set (section 6q), one workgroup each: `all` holds the [P,...] arrays' bases, and
// workgroup h builds its LmParams on the slices dof + 6 h, offset + J h, theta + 4 h, K + 9 h (K0 and free_list are shared),
// its state block, its log rows and, under a prior, rows h of prior_weight / prior_mean [P,N].  Then the solo kernel's pieces.
template <bool PRIOR>
__global__ void __launch_bounds__(64) lm_update_multi_calib_kernel(const double* __restrict__ info, const double* __restrict__ grad,
                                                                   const long long* __restrict__ count,
                                                                   const float* __restrict__ loss, int Bv, int N, LmParams all,
                                                                   double ftol, double lambda_max, int finalize,
                                                                   double* __restrict__ st, double* __restrict__ log,
                                                                   int log_rows, LmPriorArgs<PRIOR> prior) {
    __shared__ LmShared sh;
    LmPriorShared* ps = nullptr;
    if constexpr (PRIOR) {
        __shared__ LmPriorShared prior_s;
        ps = &prior_s;
    }
    const size_t h = blockIdx.x, v = h * (size_t)Bv;
    const LmParams p = {all.dof + 6 * h,
                        all.offset ? all.offset + (size_t)all.J * h : nullptr,
                        all.free_list,
                        all.F,
                        all.J,
                        all.theta ? all.theta + 4 * h : nullptr,
                        all.free4_mask,
                        all.tie_focal,
                        all.K0,
                        all.K ? all.K + 9 * h : nullptr,
                        all.H,
                        all.W};
    st += h * EHR_LM_STATE_DOUBLES;
    log = log ? log + h * (size_t)log_rows * 4 : nullptr;
    if (lm_update_restore(N, p, finalize, st)) return;
    const int bad = lm_update_gather(info + v * N * N, grad + v * N, count + v, loss + v, Bv, N, sh);
    const double* pw = lm_prior_weight(prior);
    const double* pm = lm_prior_mean(prior);
    lm_update_rest<PRIOR>(sh, bad, N, p, ftol, lambda_max, st, log, log_rows, ps, pw ? pw + h * (size_t)N : nullptr,
                          pm ? pm + h * (size_t)N : nullptr);
}

// ---- the rig: C cameras, one system of N = 6 C + F parameters (easyhec_amd/lm_rig.py) -------------------
#define EHR_LM_RIG_MAX_CAMERAS (EHR_LM_MAX_PARAMS / 6)

struct LmRigCameras {  // the host's array, by value in the kernel's arguments (unused entries zeroed)
    ehr_lm_rig_camera c[EHR_LM_RIG_MAX_CAMERAS];
};

struct LmRigParams {  // cam0.dof[0..5], cam1.dof[0..5], ..., then the free joints' SHARED offsets; cams: the array in LDS
    const ehr_lm_rig_camera* cams;
    int C;
    float* offset;
    const int* free_list;
    int F, J;
};
__device__ __forceinline__ float lm_param_read(const LmRigParams& p, int k) {
    if (k < 6 * p.C) return p.cams[k / 6].dof[k % 6];
    const int j = p.free_list[k - 6 * p.C];
    return (j >= 0 && j < p.J) ? p.offset[j] : 0.f;
}
__device__ __forceinline__ void lm_param_write(const LmRigParams& p, int k, float x) {
    if (k < 6 * p.C) {
        p.cams[k / 6].dof[k % 6] = x;
    } else {
        const int j = p.free_list[k - 6 * p.C];
        if (j >= 0 && j < p.J) p.offset[j] = x;
    }
}
__device__ __forceinline__ void lm_write_K(const LmRigParams&, int) {}  // (no intrinsics in a rig)

// One workgroup of one wave.  The head: per camera the solo sums (from 0.0, in view order) of its [Nc,Nc] matrix, [Nc] gradient,
// loss and count, Nc = 6 + F, embedded in camera order into the cleared [N,N] system -- local i < 6 -> 6 c + i, local 6 + f ->
// 6 C + f.  Camera c's local entry (r, col) is thread (r Nc + col) % 64's for every c, so the entries that several cameras add
// to (the offsets' block) are added by ONE thread in camera order.  Any camera's bad sum reports the call for the whole rig.
template <bool PRIOR>
__global__ void __launch_bounds__(64) lm_update_rig_kernel(LmRigCameras cams, int C, float* __restrict__ offset,
                                                           const int* __restrict__ free_list, int F, int J, double ftol,
                                                           double lambda_max, int finalize, double* __restrict__ st,
                                                           double* __restrict__ log, int log_rows,
                                                           LmPriorArgs<PRIOR> prior) {
    __shared__ LmShared sh;
    LmPriorShared* ps = nullptr;
    if constexpr (PRIOR) {
        __shared__ LmPriorShared prior_s;
        ps = &prior_s;
    }
    __shared__ ehr_lm_rig_camera cam_s[EHR_LM_RIG_MAX_CAMERAS];
    const int tid = threadIdx.x;
    // the by-value array into LDS, every index a constant: a per-thread run-time index into it would put it in scratch
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < EHR_LM_RIG_MAX_CAMERAS; c++) cam_s[c] = cams.c[c];
    }
    __syncthreads();
    const int N = 6 * C + F, Nc = 6 + F;
    const LmRigParams p = {cam_s, C, offset, free_list, F, J};
    if (lm_update_restore(N, p, finalize, st)) return;
    for (int e = tid; e < N * N; e += 64) sh.Hm[e / N][e % N] = 0.0;
    if (tid < N) sh.gv[tid] = 0.0;
    __syncthreads();
    int bad = 0;
    double Fsum = 0.0, nsum = 0.0;  // (thread 0's)
    for (int c = 0; c < C; c++) {
        const double* __restrict__ info = cam_s[c].info;
        const double* __restrict__ grad = cam_s[c].grad;
        const int B = cam_s[c].B;
        for (int e = tid; e < Nc * Nc; e += 64) {
            const int r = e / Nc, col = e - r * Nc;
            double s = 0.0;
            for (int b = 0; b < B; b++) s += info[((size_t)b * Nc + r) * Nc + col];
            bad |= !lm_finite(s);
            sh.Hm[r < 6 ? 6 * c + r : 6 * C + (r - 6)][col < 6 ? 6 * c + col : 6 * C + (col - 6)] += s;
        }
        if (tid < Nc) {
            double s = 0.0;
            for (int b = 0; b < B; b++) s += grad[(size_t)b * Nc + tid];
            bad |= !lm_finite(s);
            sh.gv[tid < 6 ? 6 * c + tid : 6 * C + (tid - 6)] += s;
        }
        if (tid == 0) {
            const long long* __restrict__ count = cam_s[c].count;
            const float* __restrict__ loss = cam_s[c].loss;
            double s = 0.0, n = 0.0;
            for (int b = 0; b < B; b++) {
                s += (double)loss[b];
                bad |= count[b] < 0;
                n += (double)count[b];
            }
            bad |= !lm_finite(s);
            Fsum += s;
            nsum += n;
        }
    }
    if (tid == 0) {
        bad |= !lm_finite(Fsum);
        sh.F = Fsum;
        sh.cnt = nsum;
    }
    lm_update_rest<PRIOR>(sh, bad, N, p, ftol, lambda_max, st, log, log_rows, ps, lm_prior_weight(prior), lm_prior_mean(prior));
}

// ---- the rig on its block-arrow system: per-camera intrinsics, N up to 182 (easyhec_amd/lm_rig.py) -------
// The rig's matrix is block-arrow: one diagonal block per camera (pose + its free intrinsics, P_c <= 10), one border per camera
// (its coupling to the F shared offsets) and one shared corner; the block between two cameras is exactly 0.0.  Eliminating the
// camera blocks one by one IS the dense right-looking Cholesky in the system's order with the structurally zero updates left
// out.  One workgroup of 256 threads: 16 lanes per camera factor the camera panels side by side, every sum in the dense
// kernel's order.  Steps 2-3 and 5-6 are lm_update_rest's restated: that function is bound to the dense [32][32] LmShared and
// to one wave, and sharing it would have changed the existing kernels' code.
#define LM_ARROW_THREADS 256
#define LM_ARROW_PB EHR_LM_ARROW_MAX_BLOCK
#define LM_ARROW_FS EHR_LM_ARROW_MAX_SHARED
#define LM_ARROW_ROWS (LM_ARROW_PB + LM_ARROW_FS)

struct LmArrowCameras {  // the host's array, by value in the kernel's arguments (unused entries zeroed)
    ehr_lm_rig_arrow_camera c[EHR_LM_ARROW_MAX_CAMERAS];
};

struct LmArrowShared {
    // per camera: rows i < P_c its scaled damped block -> L_c; rows 10 + f the border's row of offset f -> (W_c^T)[f]
    double T[EHR_LM_ARROW_MAX_CAMERAS][LM_ARROW_ROWS][LM_ARROW_PB];
    double Cn[LM_ARROW_FS][LM_ARROW_FS];  // the scaled damped corner -> its Schur complement -> L_s
    double gv[EHR_LM_ARROW_MAX_PARAMS];   // the call's g, then g_acc (+ the prior's); after the solve: delta
    double sv[EHR_LM_ARROW_MAX_PARAMS], yv[EHR_LM_ARROW_MAX_PARAMS];
    double rv[EHR_LM_ARROW_MAX_PARAMS];   // the right-hand side; before step 4 the prior's terms, after the solve (S H S) y
    double dg[EHR_LM_ARROW_MAX_PARAMS];   // the diagonal of the system that is solved: H_acc's (+ the prior's weights)
    double F, cnt, lambda, nu, Fp;
    int accept, fail, why;
    int base[EHR_LM_ARROW_MAX_CAMERAS + 1], P[EHR_LM_ARROW_MAX_CAMERAS];
    ehr_lm_rig_arrow_camera cam[EHR_LM_ARROW_MAX_CAMERAS];
};

struct LmArrowParams {  // cam0.dof, cam0.theta[...], cam1.dof, ..., then the free joints' SHARED offsets; cams, base: in LDS
    const ehr_lm_rig_arrow_camera* cams;
    const int* base;  // [C + 1]: where camera c's block starts; base[C] = S0
    int C;
    float* offset;
    const int* free_list;
    int F, J;
};
// camera c's own parameters as the solo accessor sees them (dof, no joints, its intrinsics): local index i of its block
__device__ __forceinline__ LmParams lm_arrow_camera(const LmArrowParams& p, int c) {
    const ehr_lm_rig_arrow_camera& k = p.cams[c];
    return LmParams{k.dof, nullptr, nullptr, 0, 0, k.theta, k.free4_mask, k.tie_focal, k.K0, k.K, k.H, k.W};
}
__device__ __forceinline__ int lm_arrow_owner(const LmArrowParams& p, int k) {
    int c = 0;
    while (c + 1 < p.C && k >= p.base[c + 1]) c++;
    return c;
}
__device__ __forceinline__ float lm_param_read(const LmArrowParams& p, int k) {
    if (k < p.base[p.C]) {
        const int c = lm_arrow_owner(p, k);
        return lm_param_read(lm_arrow_camera(p, c), k - p.base[c]);
    }
    const int j = p.free_list[k - p.base[p.C]];
    return (j >= 0 && j < p.J) ? p.offset[j] : 0.f;
}
__device__ __forceinline__ void lm_param_write(const LmArrowParams& p, int k, float x) {
    if (k < p.base[p.C]) {
        const int c = lm_arrow_owner(p, k);
        lm_param_write(lm_arrow_camera(p, c), k - p.base[c], x);
    } else {
        const int j = p.free_list[k - p.base[p.C]];
        if (j >= 0 && j < p.J) p.offset[j] = x;
    }
}
// every camera's K from its theta (9 threads per camera; a camera without free intrinsics: untouched)
__device__ __forceinline__ void lm_write_K(const LmArrowParams& p, int tid) {
    const int c = tid / 9;
    if (c < p.C) lm_write_K(lm_arrow_camera(p, c), tid - 9 * c);
}

// the packed H_acc of the arrow state block: camera c's panel (block + border), its border's transpose, the corner
__device__ __forceinline__ double* lm_arrow_panel(double* st, int c) { return st + EHR_LM_ARROW_H + c * EHR_LM_ARROW_CAMERA_STRIDE; }
__device__ __forceinline__ double* lm_arrow_border_t(double* st, int c) { return lm_arrow_panel(st, c) + EHR_LM_ARROW_BORDER_T; }
__device__ __forceinline__ double* lm_arrow_corner(double* st) { return st + EHR_LM_ARROW_CORNER; }
// camera-local index of ehr_lm_linearize's order (dof, offsets, intrinsics) -> index in the camera's block, or -1 - f for offset f
__device__ __forceinline__ int lm_arrow_local(int r, int F) { return r < 6 ? r : (r < 6 + F ? -1 - (r - 6) : r - F); }

template <bool PRIOR>
__global__ void __launch_bounds__(LM_ARROW_THREADS) lm_update_rig_arrow_kernel(LmArrowCameras cams, int C, float* __restrict__ offset,
                                                                              const int* __restrict__ free_list, int F, int J,
                                                                              double ftol, double lambda_max, int finalize,
                                                                              double* st, double* __restrict__ log, int log_rows,
                                                                              LmPriorArgs<PRIOR> prior) {
    __shared__ LmArrowShared sh;
    constexpr int NT = LM_ARROW_THREADS, PB = LM_ARROW_PB, ST = EHR_LM_ARROW_PANEL_STRIDE;
    const int tid = threadIdx.x;
    // the by-value array into LDS, every index a constant: a per-thread run-time index into it would put it in scratch
    if (tid == 0) {
#pragma unroll
        for (int c = 0; c < EHR_LM_ARROW_MAX_CAMERAS; c++) sh.cam[c] = cams.c[c];
        int b = 0;
        for (int c = 0; c < C; c++) {
            const int m = sh.cam[c].free4_mask;
            const int Pc = 6 + (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1) - (sh.cam[c].tie_focal != 0 ? 1 : 0);
            sh.base[c] = b;
            sh.P[c] = Pc;
            b += Pc;
        }
        sh.base[C] = b;
    }
    __syncthreads();
    const int S0 = sh.base[C], N = S0 + F;
    const LmArrowParams p = {sh.cam, sh.base, C, offset, free_list, F, J};
    if (lm_update_restore(N, p, finalize, st)) return;
    const double* const prior_weight = lm_prior_weight(prior);
    const double* const prior_mean = lm_prior_mean(prior);
    double* const th_acc = st + EHR_LM_ARROW_THETA;
    double* const g_acc = st + EHR_LM_ARROW_G;
    const bool have = st[EHR_LM_ACCEPTED] > 0.0;  // a point has been accepted
    const int it = (int)st[EHR_LM_ITERATIONS];
    double* const row = (log && it < log_rows) ? log + (size_t)it * 4 : nullptr;  // (thread 0's)
    // where this thread's parameter (tid < N) lives: camera mc and index mi of its block, or mc = -1 and offset mi
    int mc = -1, mi = tid - S0;
    if (tid < S0) {
        mc = lm_arrow_owner(p, tid);
        mi = tid - sh.base[mc];
    }
    // 1. the head: every camera's sums in view order; g embedded with += in camera order; H is summed again where it is stored
    if (tid < N) sh.gv[tid] = 0.0;
    __syncthreads();
    int bad = 0;
    double Fsum = 0.0, nsum = 0.0;  // (thread 0's)
    for (int c = 0; c < C; c++) {
        const double* __restrict__ info = sh.cam[c].info;
        const double* __restrict__ grad = sh.cam[c].grad;
        const int B = sh.cam[c].B, Nc = sh.P[c] + F;
        for (int e = tid; e < Nc * Nc; e += NT) {
            double s = 0.0;
            for (int b = 0; b < B; b++) s += info[(size_t)b * Nc * Nc + e];
            bad |= !lm_finite(s);
        }
        if (tid < Nc) {  // local index tid is this thread's for every camera: an offset's C terms are added by ONE thread
            double s = 0.0;
            for (int b = 0; b < B; b++) s += grad[(size_t)b * Nc + tid];
            bad |= !lm_finite(s);
            const int l = lm_arrow_local(tid, F);
            sh.gv[l >= 0 ? sh.base[c] + l : S0 + (-1 - l)] += s;
        }
        if (tid == 0) {
            const long long* __restrict__ count = sh.cam[c].count;
            const float* __restrict__ loss = sh.cam[c].loss;
            double s = 0.0, n = 0.0;
            for (int b = 0; b < B; b++) {
                s += (double)loss[b];
                bad |= count[b] < 0;
                n += (double)count[b];
            }
            bad |= !lm_finite(s);
            Fsum += s;
            nsum += n;
        }
    }
    if (tid == 0) {
        bad |= !lm_finite(Fsum);
        sh.F = Fsum;
        sh.cnt = nsum;
    }
    // the prior's term at the trial: lm_update_rest's
    if (PRIOR) {
        if (tid < N) {
            const double w = prior_weight[tid], m = prior_mean[tid];
            double t = 0.0;
            if (!(w >= 0.0) || !lm_finite(w)) {
                bad = 1;
            } else if (w != 0.0) {
                bad |= !lm_finite(m);
                const double d = (double)lm_param_read(p, tid) - m;
                t = (w * d) * d;
            }
            sh.rv[tid] = t;  // (free until step 4)
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int k = 0; k < N; k++)
                if (prior_weight[k] != 0.0) s += sh.rv[k];
            bad |= !lm_finite(s);
            sh.Fp = s;
        }
    }
    bad = __syncthreads_or(bad);
    // 2. a reported call: the trial is discarded, nothing else moves
    if (bad) {
        if (have && tid < N) lm_param_write(p, tid, (float)th_acc[tid]);
        if (tid == 0) {
            st[EHR_LM_REPORTED] += 1.0;
            st[EHR_LM_ITERATIONS] = (double)(it + 1);
            st[EHR_LM_LAST] = -1.0;
            if (row) {
                row[0] = __longlong_as_double(0x7ff8000000000000ll);
                row[1] = -1.0;
                row[2] = st[EHR_LM_LAMBDA];
                row[3] = __longlong_as_double(0x7ff8000000000000ll);
            }
        }
        __syncthreads();
        if (have) lm_write_K(p, tid);
        return;
    }
    // 3. accept or reject
    if (tid == 0) {
        const double Fv = PRIOR ? sh.F + sh.Fp : sh.F, F_acc = st[EHR_LM_F];
        double lambda = st[EHR_LM_LAMBDA], nu = st[EHR_LM_NU], rho = 0.0;
        const int accept = !have || Fv < F_acc;
        if (accept) {
            if (have) {
                rho = (F_acc - Fv) / st[EHR_LM_PRED];
                const double t = 2.0 * rho - 1.0;
                lambda *= fmax(1.0 / 3.0, 1.0 - t * t * t);
            }
            nu = 2.0;
            st[EHR_LM_F] = Fv;
            if (PRIOR) st[EHR_LM_F_PRIOR] = sh.Fp;
            st[EHR_LM_COUNT] = sh.cnt;
            st[EHR_LM_RHO] = rho;
            st[EHR_LM_ACCEPTED] += 1.0;
        } else {
            lambda *= nu;
            nu *= 2.0;
            st[EHR_LM_REJECTED] += 1.0;
        }
        st[EHR_LM_ITERATIONS] = (double)(it + 1);
        st[EHR_LM_LAST] = accept ? 1.0 : 0.0;
        st[EHR_LM_F_TRIAL] = Fv;
        sh.accept = accept;
        sh.lambda = lambda;
        sh.nu = nu;
        if (row) {
            row[0] = Fv;
            row[1] = accept ? 1.0 : 0.0;
            row[3] = accept ? rho : __longlong_as_double(0x7ff8000000000000ll);
        }
    }
    __syncthreads();
    if (sh.accept) {
        // the call's H into the packed H_acc: the same sums again (the same bits), every entry by one owner
        for (int c = 0; c < C; c++) {
            const double* __restrict__ info = sh.cam[c].info;
            const int B = sh.cam[c].B, Nc = sh.P[c] + F;
            double* const panel = lm_arrow_panel(st, c);
            double* const bt = lm_arrow_border_t(st, c);
            for (int e = tid; e < Nc * Nc; e += NT) {
                const int r = lm_arrow_local(e / Nc, F), col = lm_arrow_local(e % Nc, F);
                if (r < 0 && col < 0) continue;  // (the corner: below)
                double s = 0.0;
                for (int b = 0; b < B; b++) s += info[(size_t)b * Nc * Nc + e];
                if (r >= 0)
                    panel[r * ST + (col >= 0 ? col : PB + (-1 - col))] = s;
                else
                    bt[(-1 - r) * PB + col] = s;
            }
        }
        for (int e = tid; e < F * F; e += NT) {  // the shared corner: its C terms one camera at a time
            const int f = e / F, g = e - f * F;
            double acc = 0.0;
            for (int c = 0; c < C; c++) {
                const double* __restrict__ info = sh.cam[c].info;
                const int B = sh.cam[c].B, Nc = sh.P[c] + F;
                double s = 0.0;
                for (int b = 0; b < B; b++) s += info[((size_t)b * Nc + 6 + f) * Nc + 6 + g];
                acc += s;
            }
            lm_arrow_corner(st)[f * LM_ARROW_FS + g] = acc;
        }
        if (tid < N) {
            g_acc[tid] = sh.gv[tid];
            th_acc[tid] = (double)lm_param_read(p, tid);
        }
    } else if (tid < N) {  // the stored linearisation: the inputs of this call are not read again
        sh.gv[tid] = g_acc[tid];
    }
    __syncthreads();
    // the diagonal of the system that is solved; the prior joins it and g, never the stored ones
    if (tid < N) {
        double d = mc >= 0 ? lm_arrow_panel(st, mc)[mi * ST + mi] : lm_arrow_corner(st)[mi * LM_ARROW_FS + mi];
        if (PRIOR) {
            const double w = prior_weight[tid];
            if (w != 0.0) {
                d += w;
                sh.gv[tid] += 2.0 * w * (th_acc[tid] - prior_mean[tid]);
            }
        }
        sh.dg[tid] = d;
        sh.sv[tid] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
    }
    __syncthreads();
    // 4. (S H S + lambda I) y = -S g / 2 by block elimination in the system's order
    const int gc = tid >> 4, gl = tid & 15;  // this thread's camera panel and its lane there
    const int gP = gc < C ? sh.P[gc] : 0, gb = gc < C ? sh.base[gc] : 0;
    double(*const T)[PB] = sh.T[gc];
    int retries = 0;
    for (;;) {
        const double lambda = sh.lambda;
        for (int e = tid; e < C * LM_ARROW_ROWS * PB; e += NT) {
            const int c = e / (LM_ARROW_ROWS * PB), rem = e - c * (LM_ARROW_ROWS * PB), r = rem / PB, j = rem - r * PB;
            const int Pc = sh.P[c], b = sh.base[c];
            double a = 0.0;
            if (j < Pc) {
                if (r < PB) {
                    if (r < Pc) {
                        a = (r == j ? sh.dg[b + r] : lm_arrow_panel(st, c)[r * ST + j]) * sh.sv[b + r] * sh.sv[b + j];
                        if (r == j) a = sh.sv[b + r] > 0.0 ? a + lambda : 1.0;
                    }
                } else if (r - PB < F) {
                    a = lm_arrow_border_t(st, c)[(r - PB) * PB + j] * sh.sv[S0 + r - PB] * sh.sv[b + j];
                }
            }
            sh.T[c][r][j] = a;
        }
        for (int e = tid; e < F * F; e += NT) {
            const int f = e / F, g = e - f * F;
            double a = (f == g ? sh.dg[S0 + f] : lm_arrow_corner(st)[f * LM_ARROW_FS + g]) * sh.sv[S0 + f] * sh.sv[S0 + g];
            if (f == g) a = sh.sv[S0 + f] > 0.0 ? a + lambda : 1.0;
            sh.Cn[f][g] = a;
        }
        if (tid < N) sh.rv[tid] = -0.5 * sh.gv[tid] * sh.sv[tid];
        if (tid == 0) sh.fail = 0;
        __syncthreads();
        // the camera panels side by side: A_c = L_c L_c^T right-looking, W_c^T = B_c^T L_c^-T, z_c = L_c^-1 r_c
        for (int j = 0; j < PB; j++) {
            const bool on = j < gP;
            if (on && gl == 0) {
                double piv = T[j][j];
                if (!(piv > 0.0) || !lm_finite(piv)) {
                    sh.fail = 1;
                    piv = 1.0;
                }
                T[j][j] = sqrt(piv);
            }
            __syncthreads();
            if (on) {
                const double d = T[j][j];
                for (int r = gl; r < LM_ARROW_ROWS; r += 16)
                    if (r < PB ? (r > j && r < gP) : (r - PB < F)) T[r][j] = T[r][j] / d;
                if (gl == 0) sh.yv[gb + j] = sh.rv[gb + j] / d;
            }
            __syncthreads();
            if (on) {
                for (int r = gl; r < LM_ARROW_ROWS; r += 16) {
                    if (r < PB) {
                        if (r > j && r < gP) {
                            for (int k = j + 1; k <= r; k++) T[r][k] -= T[r][j] * T[k][j];
                            sh.rv[gb + r] -= T[r][j] * sh.yv[gb + j];
                        }
                    } else if (r - PB < F) {
                        for (int k = j + 1; k < gP; k++) T[r][k] -= T[r][j] * T[k][j];
                    }
                }
            }
            __syncthreads();
        }
        // the corner and its right-hand side lose W_c^T W_c and W_c^T z_c: camera order, then row order k, one owner per entry
        for (int e = tid; e < F * F; e += NT) {
            const int f = e / F, g = e - f * F;
            if (g > f) continue;
            double acc = sh.Cn[f][g];
            for (int c = 0; c < C; c++)
                for (int k = 0; k < sh.P[c]; k++) acc -= sh.T[c][PB + f][k] * sh.T[c][PB + g][k];
            sh.Cn[f][g] = acc;
        }
        if (tid < F) {
            double acc = sh.rv[S0 + tid];
            for (int c = 0; c < C; c++)
                for (int k = 0; k < sh.P[c]; k++) acc -= sh.T[c][PB + tid][k] * sh.yv[sh.base[c] + k];
            sh.rv[S0 + tid] = acc;
        }
        __syncthreads();
        for (int j = 0; j < F; j++) {  // the Schur complement's Cholesky: the dense kernel's
            if (tid == 0) {
                double piv = sh.Cn[j][j];
                if (!(piv > 0.0) || !lm_finite(piv)) {
                    sh.fail = 1;
                    piv = 1.0;
                }
                sh.Cn[j][j] = sqrt(piv);
            }
            __syncthreads();
            if (tid > j && tid < F) sh.Cn[tid][j] = sh.Cn[tid][j] / sh.Cn[j][j];
            __syncthreads();
            if (tid > j && tid < F)
                for (int k = j + 1; k <= tid; k++) sh.Cn[tid][k] -= sh.Cn[tid][j] * sh.Cn[k][j];
            __syncthreads();
        }
        if (!sh.fail || retries >= EHR_LM_MAX_RETRIES) break;
        retries++;
        __syncthreads();
        if (tid == 0) {  // a non-positive pivot: raise lambda like a rejection and factor again
            sh.lambda *= sh.nu;
            sh.nu *= 2.0;
        }
        __syncthreads();
    }
    if (sh.fail) {  // the factorisation keeps failing: stop on the accepted point
        if (tid < N) lm_param_write(p, tid, (float)th_acc[tid]);
        if (tid == 0) {
            st[EHR_LM_LAMBDA] = sh.lambda;
            st[EHR_LM_NU] = sh.nu;
            st[EHR_LM_RETRIES] += (double)retries;
            st[EHR_LM_DONE] = 1.0;
            st[EHR_LM_WHY] = 4.0;
            if (row) row[2] = sh.lambda;
        }
        __syncthreads();
        lm_write_K(p, tid);
        return;
    }
    for (int j = 0; j < F; j++) {  // L_s z_s = r_s
        if (tid == 0) sh.yv[S0 + j] = sh.rv[S0 + j] / sh.Cn[j][j];
        __syncthreads();
        if (tid > j && tid < F) sh.rv[S0 + tid] -= sh.Cn[tid][j] * sh.yv[S0 + j];
        __syncthreads();
    }
    for (int j = F - 1; j >= 0; j--) {  // L_s^T y_s = z_s
        if (tid == 0) sh.yv[S0 + j] = sh.yv[S0 + j] / sh.Cn[j][j];
        __syncthreads();
        if (tid < j) sh.yv[S0 + tid] -= sh.Cn[j][tid] * sh.yv[S0 + j];
        __syncthreads();
    }
    // y_c = L_c^-T (z_c - W_c y_s): the offsets' terms last to first, then the camera's own rows, as the dense back-substitution
    if (gl < gP) {
        double acc = sh.yv[gb + gl];
        for (int f = F - 1; f >= 0; f--) acc -= T[PB + f][gl] * sh.yv[S0 + f];
        sh.yv[gb + gl] = acc;
    }
    __syncthreads();
    for (int j = PB - 1; j >= 0; j--) {
        const bool on = j < gP;
        if (on && gl == 0) sh.yv[gb + j] = sh.yv[gb + j] / T[j][j];
        __syncthreads();
        if (on && gl < j) sh.yv[gb + gl] -= T[j][gl] * sh.yv[gb + j];
        __syncthreads();
    }
    // hy = (S H S) y per row over its structurally non-zero columns, ascending; H_acc is read back from the state block
    if (tid < N) {
        const double sk = sh.sv[tid];
        double s = 0.0;
        if (mc >= 0) {
            const double* const panel = lm_arrow_panel(st, mc);
            const int b = sh.base[mc], Pc = sh.P[mc];
            for (int j = 0; j < Pc; j++) s += ((j == mi ? sh.dg[tid] : panel[mi * ST + j]) * sk * sh.sv[b + j]) * sh.yv[b + j];
            for (int f = 0; f < F; f++) s += (panel[mi * ST + PB + f] * sk * sh.sv[S0 + f]) * sh.yv[S0 + f];
        } else {
            for (int c = 0; c < C; c++) {
                const double* const bt = lm_arrow_border_t(st, c);
                const int b = sh.base[c], Pc = sh.P[c];
                for (int j = 0; j < Pc; j++) s += (bt[mi * PB + j] * sk * sh.sv[b + j]) * sh.yv[b + j];
            }
            const double* const corner = lm_arrow_corner(st);
            for (int f = 0; f < F; f++)
                s += ((f == mi ? sh.dg[tid] : corner[mi * LM_ARROW_FS + f]) * sk * sh.sv[S0 + f]) * sh.yv[S0 + f];
        }
        sh.rv[tid] = s;                   // (S H S) y
        sh.gv[tid] = sh.yv[tid] * sk;     // delta
        st[EHR_LM_ARROW_DELTA + tid] = sh.gv[tid];
    }
    __syncthreads();
    // 5, 6. the predicted reduction, the stopping rule, the next trial
    if (tid == 0) {
        const double lambda = sh.lambda;
        double pred = 0.0;
        for (int k = 0; k < N; k++) pred += sh.yv[k] * sh.rv[k] + 2.0 * lambda * (sh.yv[k] * sh.yv[k]);
        int small = 1;
        for (int k = 0; k < N; k++) small = small && (sh.gv[k] == 0.0 || fabs(sh.gv[k]) < lm_spacing_f32((float)th_acc[k]));
        int why = 0;
        if (pred <= ftol * st[EHR_LM_F])
            why = 1;
        else if (lambda >= lambda_max)
            why = 2;
        else if (small)
            why = 3;
        st[EHR_LM_LAMBDA] = lambda;
        st[EHR_LM_NU] = sh.nu;
        st[EHR_LM_PRED] = pred;
        st[EHR_LM_RETRIES] += (double)retries;
        if (why) {
            st[EHR_LM_DONE] = 1.0;
            st[EHR_LM_WHY] = (double)why;
        }
        if (row) row[2] = lambda;
        sh.why = why;
    }
    __syncthreads();
    if (tid < N) lm_param_write(p, tid, sh.why ? (float)th_acc[tid] : (float)(th_acc[tid] + sh.gv[tid]));
    __syncthreads();
    lm_write_K(p, tid);
}

}  // namespace ehr

using namespace ehr;

extern "C" {

int ehr_lm_linearize(const float* dof, const float* K, const float* link_poses, int B, int L, int H, int W, float near_plane,
                     float far_plane, const float* joint_frames, const uint32_t* upstream, const int32_t* joint_kind,
                     const int32_t* free_list, int F, int J, int free4_mask, int tie_focal, int N, float* mvp, float* dmvp,
                     void* stream) {
    if (!dof || !K || !link_poses || !mvp || !dmvp) return fail(EHR_ERR_INVALID, "ehr_lm_linearize: NULL tensor");
    if (F < 0 || (F > 0 && (!joint_frames || !upstream || !joint_kind || !free_list || J < 1 || J > 32)))
        return fail(EHR_ERR_INVALID, "ehr_lm_linearize: free joints need joint_frames, upstream, joint_kind and the list (J %d <= 32)", J);
    int Fi = 0;
    if (free4_mask < 0 || free4_mask > 15 || (tie_focal != 0 && (free4_mask & 3) != 3))
        return fail(EHR_ERR_INVALID, "ehr_lm_linearize: bad free intrinsics (mask %d, tie_focal %d)", free4_mask, tie_focal);
    for (int i = 0; i < 4; i++) Fi += (free4_mask >> i) & 1;
    if (tie_focal != 0) Fi -= 1;
    if (N != 6 + F + Fi || N > EHR_LM_MAX_PARAMS)
        return fail(EHR_ERR_INVALID, "ehr_lm_linearize: N %d is not 6 + %d free joints + %d free intrinsics, or exceeds %d", N, F,
                    Fi, EHR_LM_MAX_PARAMS);
    if (B < 1 || L < 1 || H < 1 || W < 1 || (long long)B * L * (N + 1) > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID, "ehr_lm_linearize: bad sizes (B %d, L %d, H %d, W %d)", B, L, H, W);
    const long long total = (long long)B * L * (N + 1);
    lm_linearize_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        dof, K, link_poses, B, L, H, W, near_plane, far_plane, joint_frames, upstream, joint_kind, free_list, F, J, free4_mask,
        tie_focal, N, mvp, dmvp);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

// what the two prior pointers must be, for both forms: both NULL (no prior) or both given
static int lm_prior_check(const char* who, const double* prior_weight, const double* prior_mean) {
    if ((prior_weight == nullptr) != (prior_mean == nullptr))
        return fail(EHR_ERR_INVALID, "%s: prior_weight and prior_mean go together (both NULL: no prior); got %s NULL", who,
                    prior_weight ? "prior_mean" : "prior_weight");
    return EHR_OK;
}

static int lm_update_launch(const char* who, const double* info, const double* grad, const long long* count, const float* loss,
                            int B, int N, float* dof, float* offset, const int32_t* free_list, int F, int J, float* theta,
                            int free4_mask, int tie_focal, const float* K0, float* K, int H, int W, double ftol, double lambda_max,
                            int finalize, double* state, double* log, int log_rows, const double* prior_weight,
                            const double* prior_mean, void* stream) {
    if (!info || !grad || !count || !loss || !dof || !state) return fail(EHR_ERR_INVALID, "%s: NULL tensor", who);
    if (F < 0 || (F > 0 && (!offset || !free_list || J < 1 || J > 32)))
        return fail(EHR_ERR_INVALID, "%s: free joints need offset and the list (J %d <= 32)", who, J);
    if (free4_mask < 0 || free4_mask > 15 || (tie_focal != 0 && (free4_mask & 3) != 3) ||
        (free4_mask != 0 && (!theta || !K0 || !K || H < 1 || W < 1)))
        return fail(EHR_ERR_INVALID, "%s: bad free intrinsics (mask %d, tie_focal %d), or no theta / K0 / K", who, free4_mask,
                    tie_focal);
    int Fi = 0;
    for (int i = 0; i < 4; i++) Fi += (free4_mask >> i) & 1;
    if (tie_focal != 0) Fi -= 1;
    // (N < 6 without free joints or intrinsics: the first N pose coordinates alone)
    if ((N != 6 + F + Fi && !(F == 0 && Fi == 0 && N >= 1 && N < 6)) || N > EHR_LM_MAX_PARAMS || B < 1)
        return fail(EHR_ERR_INVALID, "%s: N %d is not 6 + %d free joints + %d free intrinsics, or exceeds %d (B %d)", who, N, F, Fi,
                    EHR_LM_MAX_PARAMS, B);
    if (int rc = lm_prior_check(who, prior_weight, prior_mean)) return rc;
    LmParams p = {dof, offset, free_list, F, J, theta, free4_mask, tie_focal, K0, K, H, W};
    double* const lg = log && log_rows > 0 ? log : nullptr;
    if (prior_weight)
        lm_update_kernel<true><<<1, 64, 0, (hipStream_t)stream>>>(info, grad, count, loss, B, N, p, ftol, lambda_max, finalize,
                                                                 state, lg, log_rows,
                                                                 LmPriorArgs<true>{prior_weight, prior_mean});
    else
        lm_update_kernel<false><<<1, 64, 0, (hipStream_t)stream>>>(info, grad, count, loss, B, N, p, ftol, lambda_max, finalize,
                                                                  state, lg, log_rows, LmPriorArgs<false>{});
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_lm_update(const double* info, const double* grad, const long long* count, const float* loss, int B, int N, float* dof,
                  float* offset, const int32_t* free_list, int F, int J, float* theta, int free4_mask, int tie_focal,
                  const float* K0, float* K, int H, int W, double ftol, double lambda_max, int finalize, double* state, double* log, int log_rows,
                  void* stream) {
    return lm_update_launch("ehr_lm_update", info, grad, count, loss, B, N, dof, offset, free_list, F, J, theta, free4_mask,
                            tie_focal, K0, K, H, W, ftol, lambda_max, finalize, state, log, log_rows, nullptr, nullptr, stream);
}

int ehr_lm_update_prior(const double* info, const double* grad, const long long* count, const float* loss, int B, int N,
                        float* dof, float* offset, const int32_t* free_list, int F, int J, float* theta, int free4_mask,
                        int tie_focal, const float* K0, float* K, int H, int W, double ftol, double lambda_max, int finalize,
                        double* state, double* log, int log_rows, const double* prior_weight, const double* prior_mean,
                        void* stream) {
    return lm_update_launch("ehr_lm_update_prior", info, grad, count, loss, B, N, dof, offset, free_list, F, J, theta, free4_mask,
                            tie_focal, K0, K, H, W, ftol, lambda_max, finalize, state, log, log_rows, prior_weight, prior_mean,
                            stream);
}

int ehr_lm_linearize_multi(const float* dof, const float* K, const float* link_poses, int P, int Bv, int L, int H, int W,
                           float near_plane, float far_plane, float* mvp, float* dmvp, void* stream) {
    if (!dof || !K || !link_poses || !mvp || !dmvp) return fail(EHR_ERR_INVALID, "ehr_lm_linearize_multi: NULL tensor");
    if (P < 1 || Bv < 1 || L < 1 || H < 1 || W < 1 || (long long)P * Bv * L * 7 > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID, "ehr_lm_linearize_multi: bad sizes (P %d, Bv %d, L %d, H %d, W %d)", P, Bv, L, H, W);
    const long long total = (long long)P * Bv * L * 7;
    lm_linearize_multi_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        dof, K, link_poses, P, Bv, L, H, W, near_plane, far_plane, mvp, dmvp);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_lm_update_multi(const double* info, const double* grad, const long long* count, const float* loss, int P, int Bv, int N,
                        float* dof, double ftol, double lambda_max, int finalize, double* state, double* log, int log_rows,
                        void* stream) {
    if (!info || !grad || !count || !loss || !dof || !state) return fail(EHR_ERR_INVALID, "ehr_lm_update_multi: NULL tensor");
    if (P < 1 || Bv < 1 || N < 1 || N > 6 || (long long)P * Bv > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID, "ehr_lm_update_multi: bad sizes (P %d, Bv %d), or N %d outside 1..6 (the pose alone)", P, Bv,
                    N);
    lm_update_multi_kernel<<<(unsigned)P, 64, 0, (hipStream_t)stream>>>(info, grad, count, loss, Bv, N, dof, ftol, lambda_max,
                                                                       finalize, state, log && log_rows > 0 ? log : nullptr,
                                                                       log_rows);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

// free intrinsics of a mask (tied focal: one parameter for both), or -1 for a mask / tying that is not one
static int lm_free_intrinsics(int free4_mask, int tie_focal) {
    if (free4_mask < 0 || free4_mask > 15 || (tie_focal != 0 && (free4_mask & 3) != 3)) return -1;
    int Fi = 0;
    for (int i = 0; i < 4; i++) Fi += (free4_mask >> i) & 1;
    return tie_focal != 0 ? Fi - 1 : Fi;
}

int ehr_lm_linearize_multi_calib(const float* dof, const float* K, const float* link_poses, int P, int Bv, int L, int H, int W,
                                 float near_plane, float far_plane, const float* joint_frames, const uint32_t* upstream,
                                 const int32_t* joint_kind, const int32_t* free_list, int F, int J, int free4_mask,
                                 int tie_focal, int N, float* mvp, float* dmvp, void* stream) {
    const char* who = "ehr_lm_linearize_multi_calib";
    if (!dof || !K || !link_poses || !mvp || !dmvp) return fail(EHR_ERR_INVALID, "%s: NULL tensor", who);
    if (F < 0 || (F > 0 && (!joint_frames || !upstream || !joint_kind || !free_list || J < 1 || J > 32)))
        return fail(EHR_ERR_INVALID, "%s: free joints need joint_frames, upstream, joint_kind and the list (J %d <= 32)", who, J);
    const int Fi = lm_free_intrinsics(free4_mask, tie_focal);
    if (Fi < 0) return fail(EHR_ERR_INVALID, "%s: bad free intrinsics (mask %d, tie_focal %d)", who, free4_mask, tie_focal);
    if (N != 6 + F + Fi || N > EHR_LM_MAX_PARAMS)
        return fail(EHR_ERR_INVALID, "%s: N %d is not 6 + %d free joints + %d free intrinsics, or exceeds %d", who, N, F, Fi,
                    EHR_LM_MAX_PARAMS);
    if (P < 1 || Bv < 1 || L < 1 || H < 1 || W < 1 || (long long)P * Bv * L * (N + 1) > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID, "%s: bad sizes (P %d, Bv %d, L %d, H %d, W %d)", who, P, Bv, L, H, W);
    const long long total = (long long)P * Bv * L * (N + 1);
    lm_linearize_multi_calib_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        dof, K, link_poses, P, Bv, L, H, W, near_plane, far_plane, joint_frames, upstream, joint_kind, free_list, F, J,
        free4_mask, tie_focal, N, mvp, dmvp);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_lm_update_multi_calib(const double* info, const double* grad, const long long* count, const float* loss, int P, int Bv,
                              int N, float* dof, float* offset, const int32_t* free_list, int F, int J, float* theta,
                              int free4_mask, int tie_focal, const float* K0, float* K, int H, int W, double ftol,
                              double lambda_max, int finalize, double* state, double* log, int log_rows,
                              const double* prior_weight, const double* prior_mean, void* stream) {
    const char* who = "ehr_lm_update_multi_calib";
    if (!info || !grad || !count || !loss || !dof || !state) return fail(EHR_ERR_INVALID, "%s: NULL tensor", who);
    if (F < 0 || (F > 0 && (!offset || !free_list || J < 1 || J > 32)))
        return fail(EHR_ERR_INVALID, "%s: free joints need offset and the list (J %d <= 32)", who, J);
    const int Fi = lm_free_intrinsics(free4_mask, tie_focal);
    if (Fi < 0 || (free4_mask != 0 && (!theta || !K0 || !K || H < 1 || W < 1)))
        return fail(EHR_ERR_INVALID, "%s: bad free intrinsics (mask %d, tie_focal %d), or no theta / K0 / K", who, free4_mask,
                    tie_focal);
    // (N < 6 without free joints or intrinsics: the first N pose coordinates alone, as for ehr_lm_update)
    if ((N != 6 + F + Fi && !(F == 0 && Fi == 0 && N >= 1 && N < 6)) || N > EHR_LM_MAX_PARAMS)
        return fail(EHR_ERR_INVALID, "%s: N %d is not 6 + %d free joints + %d free intrinsics, or exceeds %d", who, N, F, Fi,
                    EHR_LM_MAX_PARAMS);
    if (P < 1 || Bv < 1 || (long long)P * Bv > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID, "%s: bad sizes (P %d, Bv %d)", who, P, Bv);
    if (int rc = lm_prior_check(who, prior_weight, prior_mean)) return rc;
    LmParams all = {dof, offset, free_list, F, J, theta, free4_mask, tie_focal, K0, K, H, W};
    double* const lg = log && log_rows > 0 ? log : nullptr;
    if (prior_weight)
        lm_update_multi_calib_kernel<true><<<(unsigned)P, 64, 0, (hipStream_t)stream>>>(
            info, grad, count, loss, Bv, N, all, ftol, lambda_max, finalize, state, lg, log_rows,
            LmPriorArgs<true>{prior_weight, prior_mean});
    else
        lm_update_multi_calib_kernel<false><<<(unsigned)P, 64, 0, (hipStream_t)stream>>>(
            info, grad, count, loss, Bv, N, all, ftol, lambda_max, finalize, state, lg, log_rows, LmPriorArgs<false>{});
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

static int lm_update_rig_launch(const char* who, const ehr_lm_rig_camera* cams, int C, float* offset, const int32_t* free_list,
                                int F, int J, double ftol, double lambda_max, int finalize, double* state, double* log,
                                int log_rows, const double* prior_weight, const double* prior_mean, void* stream) {
    if (!cams || !state) return fail(EHR_ERR_INVALID, "%s: NULL cameras or state", who);
    if (F < 0 || (F > 0 && (!offset || !free_list || J < 1 || J > 32)))
        return fail(EHR_ERR_INVALID, "%s: free joints need offset and the list (J %d <= 32)", who, J);
    if (C < 1 || C > EHR_LM_RIG_MAX_CAMERAS || 6 * C + F > EHR_LM_MAX_PARAMS)
        return fail(EHR_ERR_INVALID, "%s: %d cameras and %d free joints are N = %d parameters; 1 <= C and N <= %d", who, C, F,
                    6 * C + F, EHR_LM_MAX_PARAMS);
    LmRigCameras by_value = {};
    for (int c = 0; c < C; c++) {  // (a HOST array: every field can be judged here)
        const ehr_lm_rig_camera& k = cams[c];
        if (!k.info || !k.grad || !k.count || !k.loss || !k.dof)
            return fail(EHR_ERR_INVALID, "%s: camera %d has a NULL pointer", who, c);
        if (k.B < 1) return fail(EHR_ERR_INVALID, "%s: camera %d has B %d < 1", who, c, k.B);
        by_value.c[c] = k;
    }
    if (int rc = lm_prior_check(who, prior_weight, prior_mean)) return rc;
    double* const lg = log && log_rows > 0 ? log : nullptr;
    if (prior_weight)
        lm_update_rig_kernel<true><<<1, 64, 0, (hipStream_t)stream>>>(by_value, C, offset, free_list, F, J, ftol, lambda_max,
                                                                     finalize, state, lg, log_rows,
                                                                     LmPriorArgs<true>{prior_weight, prior_mean});
    else
        lm_update_rig_kernel<false><<<1, 64, 0, (hipStream_t)stream>>>(by_value, C, offset, free_list, F, J, ftol, lambda_max,
                                                                      finalize, state, lg, log_rows, LmPriorArgs<false>{});
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_lm_update_rig(const ehr_lm_rig_camera* cams, int C, float* offset, const int32_t* free_list, int F, int J, double ftol,
                      double lambda_max, int finalize, double* state, double* log, int log_rows, void* stream) {
    return lm_update_rig_launch("ehr_lm_update_rig", cams, C, offset, free_list, F, J, ftol, lambda_max, finalize, state, log,
                                log_rows, nullptr, nullptr, stream);
}

int ehr_lm_update_rig_prior(const ehr_lm_rig_camera* cams, int C, float* offset, const int32_t* free_list, int F, int J,
                            double ftol, double lambda_max, int finalize, double* state, double* log, int log_rows,
                            const double* prior_weight, const double* prior_mean, void* stream) {
    return lm_update_rig_launch("ehr_lm_update_rig_prior", cams, C, offset, free_list, F, J, ftol, lambda_max, finalize, state,
                                log, log_rows, prior_weight, prior_mean, stream);
}

int ehr_lm_update_rig_arrow(const ehr_lm_rig_arrow_camera* cams, int C, float* offset, const int32_t* free_list, int F, int J,
                            double ftol, double lambda_max, int finalize, double* state, double* log, int log_rows,
                            const double* prior_weight, const double* prior_mean, void* stream) {
    const char* who = "ehr_lm_update_rig_arrow";
    if (!cams || !state) return fail(EHR_ERR_INVALID, "%s: NULL cameras or state", who);
    if (F < 0 || (F > 0 && (!offset || !free_list || J < 1 || J > 32)))
        return fail(EHR_ERR_INVALID, "%s: free joints need offset and the list (J %d <= 32)", who, J);
    if (C < 1 || C > EHR_LM_ARROW_MAX_CAMERAS)
        return fail(EHR_ERR_INVALID, "%s: %d cameras; 1 <= C <= %d", who, C, EHR_LM_ARROW_MAX_CAMERAS);
    LmArrowCameras by_value = {};
    for (int c = 0; c < C; c++) {  // (a HOST array: every field can be judged here)
        const ehr_lm_rig_arrow_camera& k = cams[c];
        if (!k.info || !k.grad || !k.count || !k.loss || !k.dof)
            return fail(EHR_ERR_INVALID, "%s: camera %d has a NULL pointer", who, c);
        if (k.B < 1) return fail(EHR_ERR_INVALID, "%s: camera %d has B %d < 1", who, c, k.B);
        const int Fi = lm_free_intrinsics(k.free4_mask, k.tie_focal);
        if (Fi < 0)
            return fail(EHR_ERR_INVALID, "%s: camera %d has bad free intrinsics (mask %d, tie_focal %d)", who, c, k.free4_mask,
                        k.tie_focal);
        if (k.free4_mask != 0 && (!k.theta || !k.K0 || !k.K || k.H < 1 || k.W < 1))
            return fail(EHR_ERR_INVALID, "%s: camera %d has free intrinsics (mask %d) but no theta / K0 / K (H %d, W %d)", who, c,
                        k.free4_mask, k.H, k.W);
        if (F + Fi > EHR_LM_ARROW_MAX_SHARED)
            return fail(EHR_ERR_INVALID, "%s: camera %d has %d free joints + %d free intrinsics; F + I_c <= %d", who, c, F, Fi,
                        EHR_LM_ARROW_MAX_SHARED);
        by_value.c[c] = k;
    }
    if (int rc = lm_prior_check(who, prior_weight, prior_mean)) return rc;
    double* const lg = log && log_rows > 0 ? log : nullptr;
    if (prior_weight)
        lm_update_rig_arrow_kernel<true><<<1, LM_ARROW_THREADS, 0, (hipStream_t)stream>>>(
            by_value, C, offset, free_list, F, J, ftol, lambda_max, finalize, state, lg, log_rows,
            LmPriorArgs<true>{prior_weight, prior_mean});
    else
        lm_update_rig_arrow_kernel<false><<<1, LM_ARROW_THREADS, 0, (hipStream_t)stream>>>(
            by_value, C, offset, free_list, F, J, ftol, lambda_max, finalize, state, lg, log_rows, LmPriorArgs<false>{});
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
