// ehr_joint.hip -- joint-offset calibration: the small kernels that surround the solver step's launch chain when the
// joint zero errors are fitted together with the camera pose (easyhec_amd/joint_calib.py).
//
//   joint_forward      : qpos[b] + offset -> forward kinematics of the flat table (UrdfChain.joint_table), in float64 ->
//                        link_poses [B,L,16] float32 (what ehr_solver_step reads) and joint_frames [B,J,6] float32 = the
//                        world axis a and a world point p on the axis of every active joint.
//   joint_forward_multi: the same for P hypotheses of one arm: virtual view p * Bv + j walks qpos[j] + offset[p] (the multi-start
//                        Levenberg-Marquardt solve, easyhec_amd/lm_multi.py); the body is the solo kernel's device function.
//   joint_forward_mounted: both of the above for a camera bolted to a link of the arm (eye-in-hand): link_poses = inv(F_m) F_l
//                        and joint_frames in the mount's frame with the sign of the axes of the joints that move the mount
//                        folded in, so that every kernel below and in ehr_lm.hip differentiates them unchanged.
//   joint_backward_adam: grad_mvp [B,L,16] (written by the chain) -> d(sum_b loss_b) / d offset_j =
//                        sum_{b,l: j upstream of l} <(PF @ Tc)^T grad_mvp[b,l], D_blj>, with
//                            revolute  D = [[a]x R_l | a x (t_l - p); 0 0],   prismatic  D = [0 | a; 0 0]
//                        -> the Adam update of pose_adam_apply on the free joints' offsets.
//                        <G, D> is evaluated as a . (tau + (t_l - p) x f) (revolute) and a . f (prismatic) with
//                        tau = vee(G3 R_l^T - R_l G3^T), f = G[0:3,3]: per (view, link) pair once, then three products per joint.
//   rig_backward_adam  : C cameras that watch one arm (easyhec_amd/rig_calib.py): the sum above per camera, added over the
//                        cameras in order, then every camera's pose Adam and the shared offsets' Adam -- or, if any camera's
//                        step is reported, nothing at all.  One launch instead of a joint_backward_adam per camera.
//
// No kernel here allocates, synchronises or uses an atomic: results are bit-reproducible from run to run.
#include "ehr_host.h"
#include "ehr_pose_core.h"
#include "ehr_group_adam.h"

#include "ehr_joint_core.h"  // joint_forward_view, EHR_JOINT_MAX_LINKS, EHR_JOINT_MAX_JOINTS

#define EHR_JOINT_TILE 256  // (view, link) pairs whose wrench one pass of the backward kernel keeps in LDS
#define EHR_RIG_MAX_CAMERAS 16

namespace ehr {

__global__ void __launch_bounds__(64) joint_forward_kernel(const int* __restrict__ parent, const double* __restrict__ origin,
                                                          const int* __restrict__ kind, const double* __restrict__ axis,
                                                          const int* __restrict__ qidx, const int* __restrict__ use, int N,
                                                          int J, int L, const double* __restrict__ qpos,
                                                          const float* __restrict__ offset, float* __restrict__ link_poses,
                                                          float* __restrict__ joint_frames) {
    const size_t b = blockIdx.x;
    joint_forward_view<64>(parent, origin, kind, axis, qidx, use, N, J, L, qpos + b * J, offset, link_poses + b * L * 16,
                       joint_frames + b * J * 6);
}

// P hypotheses of one arm (easyhec_amd/lm_multi.py): virtual view b = p * Bv + j walks qpos[j] + offset[p].
__global__ void __launch_bounds__(64) joint_forward_multi_kernel(const int* __restrict__ parent, const double* __restrict__ origin,
                                                                const int* __restrict__ kind, const double* __restrict__ axis,
                                                                const int* __restrict__ qidx, const int* __restrict__ use,
                                                                int N, int J, int L, const double* __restrict__ qpos,
                                                                const float* __restrict__ offset, int Bv,
                                                                float* __restrict__ link_poses,
                                                                float* __restrict__ joint_frames) {
    const size_t b = blockIdx.x, p = b / (size_t)Bv, j = b - p * (size_t)Bv;
    joint_forward_view<64>(parent, origin, kind, axis, qidx, use, N, J, L, qpos + j * J, offset + p * J, link_poses + b * L * 16,
                       joint_frames + b * J * 6);
}

// Eye-in-hand (a camera on table node `mount`): the two kernels above with joint_forward_view's MOUNTED branch, which writes the
// poses and the sign-folded joint frames in the mount's frame.  Kernels of their own: the unmounted ones keep their code.
__global__ void __launch_bounds__(64) joint_forward_mounted_kernel(const int* __restrict__ parent, const double* __restrict__ origin,
                                                                  const int* __restrict__ kind, const double* __restrict__ axis,
                                                                  const int* __restrict__ qidx, const int* __restrict__ use,
                                                                  int N, int J, int L, int mount, unsigned mount_upstream,
                                                                  const double* __restrict__ qpos,
                                                                  const float* __restrict__ offset, int Bv,
                                                                  float* __restrict__ link_poses,
                                                                  float* __restrict__ joint_frames) {
    // (Bv == 0: the solo layout, one offset row; otherwise virtual view b = p * Bv + j walks qpos[j] + offset[p])
    const size_t b = blockIdx.x, p = Bv ? b / (size_t)Bv : 0, j = Bv ? b - p * (size_t)Bv : b;
    joint_forward_view<64, true>(parent, origin, kind, axis, qidx, use, N, J, L, qpos + j * J, offset + p * J,
                                 link_poses + b * L * 16, joint_frames + b * J * 6, mount, mount_upstream);
}

// The sum of one camera's offset gradient, shared by joint_backward_adam_kernel and rig_backward_adam_kernel; call with all
// 256 threads of the single workgroup.  Per tile of EHR_JOINT_TILE pairs: a thread per pair forms the pair's wrench (tau, f)
// and keeps it with t_l in LDS; then thread (j = t & 31, s = t >> 5) adds joint j's products over pairs s, s + 8, ... of the
// tile.  Every thread has ONE float64 accumulator and adds in a fixed order; the eight partial sums of a joint are combined by
// one shuffle (lanes j, j + 32 of a wave) and left per wave in S, which the caller adds in order: ((S0 + S1) + S2) + S3.
// A [16], Wr and S are the caller's LDS; ends on a barrier (S is readable), and its first write to S comes after a barrier of
// its own, so a caller may read S and call again without one in between.
__device__ __forceinline__ void joint_offset_sums(const float* __restrict__ grad_mvp, const float* __restrict__ tc_jac,
                                                  const float* __restrict__ K, int B, int L, int J, int H, int W, float n,
                                                  float f, const float* __restrict__ link_poses,
                                                  const float* __restrict__ joint_frames,
                                                  const unsigned* __restrict__ upstream,
                                                  const int* __restrict__ joint_kind, const int* __restrict__ free_j,
                                                  bool& mine, double* A, double (*Wr)[9],
                                                  double (*S)[EHR_JOINT_MAX_JOINTS]) {
    const int tid = threadIdx.x;
    if (tid < 16) {
        float P[16];
        projection(K, H, W, n, f, P);
        for (int r = 0; r < 4; r++) {  // PF = proj @ opencv2blender, as in pose_backward_prefetch
            P[4 * r + 1] = -P[4 * r + 1];
            P[4 * r + 2] = -P[4 * r + 2];
        }
        const int r = tid >> 2, c = tid & 3;
        double s = 0.0;
        for (int k = 0; k < 4; k++) s += (double)P[4 * r + k] * (double)tc_jac[4 * k + c];  // Tc = tc_jac[0:16]: the pose this step rendered
        A[tid] = s;
    }
    const int j = tid & 31, sub = tid >> 5;
    mine = j < J && free_j[j] != 0;  // (out: thread tid < J is joint tid's, and the caller's Adam wants to know)
    const int jk = j < J ? joint_kind[j] : 0;
    double acc = 0.0;
    const int BL = B * L;
    for (int base = 0; base < BL; base += EHR_JOINT_TILE) {
        __syncthreads();  // (A is written; the previous tile's wrenches have been read)
        const int i = base + tid;
        if (i < BL) {
            float g[16], lp[12];
#pragma unroll
            for (int k = 0; k < 16; k++) g[k] = grad_mvp[(size_t)i * 16 + k];
#pragma unroll
            for (int k = 0; k < 12; k++) lp[k] = link_poses[(size_t)i * 16 + k];
            double G[3][4];  // rows 0..2 of (PF @ Tc)^T @ g: D's last row is zero
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 4; c++)
                    G[r][c] = ((A[r] * (double)g[c] + A[4 + r] * (double)g[4 + c]) + A[8 + r] * (double)g[8 + c]) +
                              A[12 + r] * (double)g[12 + c];
            double Mx[3][3];  // G3 @ R_l^T
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int k = 0; k < 3; k++)
                    Mx[r][k] = (G[r][0] * (double)lp[4 * k] + G[r][1] * (double)lp[4 * k + 1]) + G[r][2] * (double)lp[4 * k + 2];
            Wr[tid][0] = Mx[2][1] - Mx[1][2];
            Wr[tid][1] = Mx[0][2] - Mx[2][0];
            Wr[tid][2] = Mx[1][0] - Mx[0][1];
            Wr[tid][3] = G[0][3];
            Wr[tid][4] = G[1][3];
            Wr[tid][5] = G[2][3];
            Wr[tid][6] = (double)lp[3];
            Wr[tid][7] = (double)lp[7];
            Wr[tid][8] = (double)lp[11];
        }
        __syncthreads();
        if (mine) {
            const int cnt = min(EHR_JOINT_TILE, BL - base);
            for (int k = sub; k < cnt; k += 8) {
                const int p = base + k;
                const int bb = p / L, l = p - bb * L;
                if (!((upstream[l] >> j) & 1u)) continue;
                const float* jf = joint_frames + ((size_t)bb * J + j) * 6;
                const double a0 = jf[0], a1 = jf[1], a2 = jf[2];
                const double* w = Wr[k];
                double t0 = w[3], t1 = w[4], t2 = w[5];  // prismatic: a . f
                if (jk == 1) {                          // revolute: a . (tau + (t_l - p) x f)
                    const double d0 = w[6] - (double)jf[3], d1 = w[7] - (double)jf[4], d2 = w[8] - (double)jf[5];
                    t0 = w[0] + (d1 * w[5] - d2 * w[4]);
                    t1 = w[1] + (d2 * w[3] - d0 * w[5]);
                    t2 = w[2] + (d0 * w[4] - d1 * w[3]);
                }
                if (jk == 1 || jk == 2) acc += (a0 * t0 + a1 * t1) + a2 * t2;
            }
        }
    }
    acc += wave_xor<32>(acc);
    if ((tid & 63) < 32) S[tid >> 6][j] = acc;
    __syncthreads();
}

// Single workgroup of 256 threads: one camera's sum (joint_offset_sums), then the offsets' Adam.
__global__ void __launch_bounds__(256) joint_backward_adam_kernel(
    const float* __restrict__ grad_mvp, const float* __restrict__ tc_jac, const float* __restrict__ K, int B, int L, int J,
    int H, int W, float n, float f, const float* __restrict__ link_poses, const float* __restrict__ joint_frames,
    const unsigned* __restrict__ upstream, const int* __restrict__ joint_kind, const float* __restrict__ red,
    const int* __restrict__ free_j, float* __restrict__ offset, float* __restrict__ m, float* __restrict__ v,
    int* __restrict__ step_j, float lr, float b1, float b2, float eps, float wd, float* __restrict__ grad_out) {
    __shared__ double A[16];                        // PF @ Tc
    __shared__ double Wr[EHR_JOINT_TILE][9];        // tau (3), f (3), t_l (3) of the tile's pairs
    __shared__ double S[4][EHR_JOINT_MAX_JOINTS];
    const int tid = threadIdx.x;
    bool mine;
    joint_offset_sums(grad_mvp, tc_jac, K, B, L, J, H, W, n, f, link_poses, joint_frames, upstream, joint_kind, free_j, mine,
                      A, Wr, S);
    // a reported step (any of red[0..7] not finite) touches nothing
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; k++) ok = ok && (fabsf(red[k]) < 3.0e38f);
    const int t = step_j[0] + 1;
    if (tid < J)
        group_adam(
            tid, mine, ok, [&]() { return ((S[0][tid] + S[1][tid]) + S[2][tid]) + S[3][tid]; }, red[7], t, offset, m, v, lr, b1,
            b2, eps, wd, grad_out);
    __syncthreads();
    if (tid == 0 && ok) step_j[0] = t;
}

// The rig's finish stage: C cameras watch one arm and share its joint offsets (easyhec_amd/rig_calib.py).  Single workgroup
// of 256 threads.  Per camera in order, joint_offset_sums on what that camera's chain left behind; thread tid < J keeps
// T = S_0 + S_1 + ... in ONE float64 register, n = red_0[7] + red_1[7] + ... in float32.  Then, for the rig as a whole: ok =
// every red_c[0..7] of every camera is finite (and every camera's B is in range) -> pose_adam_apply per camera on its own
// red_c and the offsets' Adam on T / n; otherwise nothing moves and every report is NaN.  A camera's struct is read from the
// device array with uniform loads where it is used: nothing is indexed at run time in a per-thread array.
__global__ void __launch_bounds__(256) rig_backward_adam_kernel(
    const ehr_rig_camera* __restrict__ cams, int C, int L, int J, const unsigned* __restrict__ upstream,
    const int* __restrict__ joint_kind, const int* __restrict__ free_j, float* __restrict__ offset, float* __restrict__ m,
    float* __restrict__ v, int* __restrict__ step_j, float pose_lr, float offset_lr, float b1, float b2, float eps,
    float pose_wd, float offset_wd, float* __restrict__ grad_out) {
    __shared__ double A[16];
    __shared__ double Wr[EHR_JOINT_TILE][9];
    __shared__ double S[4][EHR_JOINT_MAX_JOINTS];
    __shared__ float red_s[8];  // the red that pose_adam_apply judges: camera c's own, or poisoned where the RIG's step is reported
    const int tid = threadIdx.x;
    const int j = tid & 31;
    bool mine = j < J && free_j[j] != 0;
    bool ok = true;
    double T = 0.0;
    float nfr = 0.f;
    for (int c = 0; c < C; c++) {
        const ehr_rig_camera* cam = cams + c;
        const float* red = cam->red;
#pragma unroll
        for (int k = 0; k < 8; k++) ok = ok && (fabsf(red[k]) < 3.0e38f);
        const int B = cam->B;
        // (the array is device memory, so the host cannot judge B: a camera out of range is read nowhere and reports the step)
        const bool sized = B >= 1 && (long long)B * L <= 0x7fffffffll / 16;
        ok = ok && sized;
        if (sized)
            joint_offset_sums(cam->grad_mvp, cam->tc_jac, cam->K, B, L, J, cam->H, cam->W, cam->near_plane, cam->far_plane,
                              cam->link_poses, cam->joint_frames, upstream, joint_kind, free_j, mine, A, Wr, S);
        if (sized && tid < J) {
            const double s = ((S[0][tid] + S[1][tid]) + S[2][tid]) + S[3][tid];
            T = c == 0 ? s : T + s;  // (not 0.0 + s: that would turn a sum of -0.0 into +0.0)
        }
        nfr = c == 0 ? red[7] : nfr + red[7];
    }
    // every camera's pose: ehr_pose_adam on its own red, or nothing at all
    for (int c = 0; c < C; c++) {
        const ehr_rig_camera* cam = cams + c;
        __syncthreads();  // (the previous camera's red_s has been read)
        if (tid < 8) red_s[tid] = (ok || tid != 0) ? cam->red[tid] : __int_as_float(0x7fc00000);
        const AdamState st = pose_adam_fetch(cam->dof, cam->adam_m, cam->adam_v, cam->step);
        __syncthreads();
        pose_adam_apply(st, cam->dof, cam->adam_m, cam->adam_v, cam->step, red_s, pose_lr, b1, b2, eps, pose_wd, cam->loss_out,
                        cam->grad_out);
    }
    // the shared offsets: their own counter, offset_lr and offset_wd
    const int t = step_j[0] + 1;
    if (tid < J)
        group_adam(tid, mine, ok, [&]() { return T; }, nfr, t, offset, m, v, offset_lr, b1, b2, eps, offset_wd, grad_out);
    __syncthreads();
    if (tid == 0 && ok) step_j[0] = t;
}

}  // namespace ehr

using namespace ehr;

extern "C" {

int ehr_joint_forward(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                      const int32_t* qidx, const int32_t* use, int N, int J, int L, const double* qpos, const float* offset,
                      int B, float* link_poses, float* joint_frames, void* stream) {
    if (!parent || !origin || !kind || !axis || !qidx || !use || !qpos || !offset || !link_poses || !joint_frames)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward: NULL tensor");
    if (N < 1 || N > EHR_JOINT_MAX_LINKS || J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || B < 1)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward: bad sizes (N %d <= 64 links, J %d <= 32 joints, L %d, B %d)", N, J, L, B);
    joint_forward_kernel<<<B, 64, 0, (hipStream_t)stream>>>(parent, origin, kind, axis, qidx, use, N, J, L, qpos, offset,
                                                           link_poses, joint_frames);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_joint_forward_multi(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                            const int32_t* qidx, const int32_t* use, int N, int J, int L, const double* qpos,
                            const float* offset, int P, int Bv, float* link_poses, float* joint_frames, void* stream) {
    if (!parent || !origin || !kind || !axis || !qidx || !use || !qpos || !offset || !link_poses || !joint_frames)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward_multi: NULL tensor");
    if (N < 1 || N > EHR_JOINT_MAX_LINKS || J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || P < 1 || Bv < 1 ||
        (long long)P * Bv * L > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID,
                    "ehr_joint_forward_multi: bad sizes (N %d <= 64 links, J %d <= 32 joints, L %d, P %d, Bv %d)", N, J, L, P, Bv);
    joint_forward_multi_kernel<<<(unsigned)(P * Bv), 64, 0, (hipStream_t)stream>>>(parent, origin, kind, axis, qidx, use, N, J, L,
                                                                                 qpos, offset, Bv, link_poses, joint_frames);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_joint_forward_mounted(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                              const int32_t* qidx, const int32_t* use, int N, int J, int L, int mount, uint32_t mount_upstream,
                              const double* qpos, const float* offset, int B, float* link_poses, float* joint_frames,
                              void* stream) {
    if (!parent || !origin || !kind || !axis || !qidx || !use || !qpos || !offset || !link_poses || !joint_frames)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward_mounted: NULL tensor");
    if (N < 1 || N > EHR_JOINT_MAX_LINKS || J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || B < 1)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward_mounted: bad sizes (N %d <= 64 links, J %d <= 32 joints, L %d, B %d)", N,
                    J, L, B);
    if (mount < 0 || mount >= N)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward_mounted: mount %d is not a node of the table (N %d)", mount, N);
    joint_forward_mounted_kernel<<<B, 64, 0, (hipStream_t)stream>>>(parent, origin, kind, axis, qidx, use, N, J, L, mount,
                                                                   mount_upstream, qpos, offset, 0, link_poses, joint_frames);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_joint_forward_multi_mounted(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                                    const int32_t* qidx, const int32_t* use, int N, int J, int L, int mount,
                                    uint32_t mount_upstream, const double* qpos, const float* offset, int P, int Bv,
                                    float* link_poses, float* joint_frames, void* stream) {
    if (!parent || !origin || !kind || !axis || !qidx || !use || !qpos || !offset || !link_poses || !joint_frames)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward_multi_mounted: NULL tensor");
    if (N < 1 || N > EHR_JOINT_MAX_LINKS || J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || P < 1 || Bv < 1 ||
        (long long)P * Bv * L > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID,
                    "ehr_joint_forward_multi_mounted: bad sizes (N %d <= 64 links, J %d <= 32 joints, L %d, P %d, Bv %d)", N, J, L,
                    P, Bv);
    if (mount < 0 || mount >= N)
        return fail(EHR_ERR_INVALID, "ehr_joint_forward_multi_mounted: mount %d is not a node of the table (N %d)", mount, N);
    joint_forward_mounted_kernel<<<(unsigned)(P * Bv), 64, 0, (hipStream_t)stream>>>(
        parent, origin, kind, axis, qidx, use, N, J, L, mount, mount_upstream, qpos, offset, Bv, link_poses, joint_frames);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_joint_backward_adam(const float* grad_mvp, const float* tc_jac, const float* K, int B, int L, int J, int H, int W,
                            float near_plane, float far_plane, const float* link_poses, const float* joint_frames,
                            const uint32_t* upstream, const int32_t* joint_kind, const float* red, const int32_t* free_joints,
                            float* offset, float* adam_m, float* adam_v, int32_t* step_j, float lr, float beta1, float beta2,
                            float eps, float weight_decay, float* grad_out, void* stream) {
    if (!grad_mvp || !tc_jac || !K || !link_poses || !joint_frames || !upstream || !joint_kind || !red || !free_joints ||
        !offset || !adam_m || !adam_v || !step_j)
        return fail(EHR_ERR_INVALID, "ehr_joint_backward_adam: NULL tensor");
    if (J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || B < 1 || (long long)B * L > 0x7fffffffll / 16)
        return fail(EHR_ERR_INVALID, "ehr_joint_backward_adam: bad sizes (J %d <= 32 joints, L %d, B %d)", J, L, B);
    joint_backward_adam_kernel<<<1, 256, 0, (hipStream_t)stream>>>(
        grad_mvp, tc_jac, K, B, L, J, H, W, near_plane, far_plane, link_poses, joint_frames, upstream, joint_kind, red,
        free_joints, offset, adam_m, adam_v, step_j, lr, beta1, beta2, eps, weight_decay, grad_out);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_rig_backward_adam(const ehr_rig_camera* cams, int C, int L, int J, const uint32_t* upstream, const int32_t* joint_kind,
                          const int32_t* free_joints, float* offset, float* adam_m, float* adam_v, int32_t* step_j,
                          float pose_lr, float offset_lr, float beta1, float beta2, float eps, float pose_wd, float offset_wd,
                          float* offset_grad_out, void* stream) {
    if (!cams || !upstream || !joint_kind || !free_joints || !offset || !adam_m || !adam_v || !step_j)
        return fail(EHR_ERR_INVALID, "ehr_rig_backward_adam: NULL tensor");
    if (C < 1 || C > EHR_RIG_MAX_CAMERAS || J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || L > 0x7fffffff / 16)
        return fail(EHR_ERR_INVALID, "ehr_rig_backward_adam: bad sizes (C %d <= 16 cameras, J %d <= 32 joints, L %d)", C, J, L);
    rig_backward_adam_kernel<<<1, 256, 0, (hipStream_t)stream>>>(cams, C, L, J, upstream, joint_kind, free_joints, offset, adam_m,
                                                                 adam_v, step_j, pose_lr, offset_lr, beta1, beta2, eps, pose_wd,
                                                                 offset_wd, offset_grad_out);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
