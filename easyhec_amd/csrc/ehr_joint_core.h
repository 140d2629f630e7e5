// ehr_joint_core.h -- the forward kinematics of the flat joint table (include/ehr.h: ehr_joint_forward), as a device function
// that every kernel which walks the table calls: ehr_joint.hip (one wave per view) and ehr_segment_clearance.hip (a workgroup of
// 256 threads per candidate).  Written once, so that all of them give the same bits.
#pragma once
#include "ehr_host.h"

#define EHR_JOINT_MAX_LINKS 64
#define EHR_JOINT_MAX_JOINTS 32

namespace ehr {

// The workgroup's THREADS threads take part (all of them call: there are barriers inside); ehr_joint.hip runs one wave per
// view.  OM[i] = origin_i @ motion_i(q) has no dependency between links and is formed by all lanes; the walk
// F[i] = F[parent_i] @ OM[i] is serial in i and takes 16 lanes, one per entry.  Frames live in LDS (2 x 8 KB), never in a
// per-thread array.  Malformed tables (a parent that does not precede its child, an index out of range) are the caller's
// to refuse; here they only ever read inside the arrays and give NaN.
// The body is joint_forward_view, for ONE view: qpos [J] and offset [J] are the rows it walks, link_poses [L,16] and
// joint_frames [J,6] the view's own output (global memory or LDS).  Every entry is one thread's own arithmetic: the bits do not
// depend on THREADS.  The last writes are followed by no barrier, and a second call needs one before it.
//
// MOUNTED (eye-in-hand: the camera is bolted to table node `mount`): the walk is the same, and the
// outputs are expressed in the mount's frame, formed in float64 from the LDS frames F (R_m, t_m: the mount's) and rounded once:
//     link_poses  : Rel_R[r][c] = (R_m[0][r] R_u[0][c] + R_m[1][r] R_u[1][c]) + R_m[2][r] R_u[2][c]
//                   Rel_t[r]    = (R_m[0][r] d[0] + R_m[1][r] d[1]) + R_m[2][r] d[2],  d = t_u - t_m (subtracted first);
//                   the last row is F_u's
//     joint_frames: a'[k] = sigma_j ((R_m[0][k] a[0] + R_m[1][k] a[1]) + R_m[2][k] a[2]),  a[r] = the unmounted axis before
//                   its rounding, sigma_j = -1 where bit j of mount_upstream is set (joint j moves the mount) and +1 otherwise
//                   p'[k] = (R_m[0][k] e[0] + R_m[1][k] e[1]) + R_m[2][k] e[2],  e = t_i - t_m
// so that the unchanged D = [[a']x Rel_R | a' x (Rel_t - p')] with the mask upstream[l] XOR mount_upstream is the derivative
// of inv(F_m) F_l.  mount must be in [0, N): the caller refuses any other.  With MOUNTED == false (the default) the two
// arguments are ignored and the function is, instruction for instruction, what it was without them.
template <int THREADS, bool MOUNTED = false>
__device__ __forceinline__ void joint_forward_view(const int* __restrict__ parent, const double* __restrict__ origin,
                                                   const int* __restrict__ kind, const double* __restrict__ axis,
                                                   const int* __restrict__ qidx, const int* __restrict__ use, int N, int J,
                                                   int L, const double* __restrict__ qpos, const float* __restrict__ offset,
                                                   float* __restrict__ link_poses, float* __restrict__ joint_frames,
                                                   int mount = -1, unsigned mount_upstream = 0u) {
    __shared__ double OM[EHR_JOINT_MAX_LINKS][16];
    __shared__ double F[EHR_JOINT_MAX_LINKS][16];
    __shared__ double sc[EHR_JOINT_MAX_LINKS][3];  // sin, cos, q of the link's joint
    __shared__ int jlink[EHR_JOINT_MAX_JOINTS];    // the link active joint j moves
    const int lane = threadIdx.x;
    if (lane < EHR_JOINT_MAX_JOINTS) jlink[lane] = -1;
    __syncthreads();
    if (lane < N) {
        const int c = qidx[lane];
        double q = 0.0;
        if (c >= 0 && c < J) {
            q = qpos[c] + (double)offset[c];
            jlink[c] = lane;  // (one writer per joint: the host refuses a table in which two links share an active joint)
        }
        sc[lane][0] = sin(q);
        sc[lane][1] = cos(q);
        sc[lane][2] = q;
    }
    __syncthreads();
    for (int e = lane; e < N * 16; e += THREADS) {
        const int i = e >> 4, r = (e >> 2) & 3, c = e & 3;
        const double ax = axis[3 * i], ay = axis[3 * i + 1], az = axis[3 * i + 2];
        const int k = (qidx[i] >= 0 && qidx[i] < J) ? kind[i] : 0;
        // column c of the motion: I + sin(q) [a]x + (1 - cos q) [a]x^2 (revolute), a translation by q a (prismatic)
        double M[4] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, c == 3 ? 1.0 : 0.0};
        if (k == 1 && c < 3) {
            // (entries picked with selects, never by a run-time index into a per-thread array: that would be scratch)
            const double s = sc[i][0], v = 1.0 - sc[i][1], aa = (ax * ax + ay * ay) + az * az;
            const double ac = c == 0 ? ax : (c == 1 ? ay : az);
#pragma unroll
            for (int m = 0; m < 3; m++) {
                const double am = m == 0 ? ax : (m == 1 ? ay : az);
                const int o = 3 - m - c;  // [a]x[m][c] = -+ a[3 - m - c] off the diagonal, minus where c follows m cyclically
                const double ao = o == 0 ? ax : (o == 1 ? ay : az);
                const double kx = m == c ? 0.0 : (((c - m + 3) % 3 == 1) ? -ao : ao);
                const double k2 = am * ac - (m == c ? aa : 0.0);  // ([a]x^2)[m][c] = a_m a_c - delta_mc |a|^2
                M[m] = ((m == c ? 1.0 : 0.0) + s * kx) + v * k2;
            }
        } else if (k == 2 && c == 3) {
            M[0] = ax * sc[i][2];
            M[1] = ay * sc[i][2];
            M[2] = az * sc[i][2];
        }
        const double* O = origin + (size_t)i * 16 + 4 * r;
        OM[i][4 * r + c] = ((O[0] * M[0] + O[1] * M[1]) + O[2] * M[2]) + O[3] * M[3];
    }
    __syncthreads();
    for (int i = 0; i < N; i++) {  // (uniform trip count: every lane meets every barrier)
        if (lane < 16) {
            const int r = lane >> 2, c = lane & 3;
            const int p = parent[i];
            double t;
            if (p < 0) {
                t = OM[i][lane];
            } else if (p < i) {
                const double* A = F[p] + 4 * r;
                t = ((A[0] * OM[i][c] + A[1] * OM[i][4 + c]) + A[2] * OM[i][8 + c]) + A[3] * OM[i][12 + c];
            } else {
                t = __longlong_as_double(0x7ff8000000000000ll);
            }
            F[i][lane] = t;
        }
        __syncthreads();
    }
    // one rounding, at the end
    if (!MOUNTED) {
        for (int e = lane; e < L * 16; e += THREADS) {
            const int u = use[e >> 4];
            link_poses[e] = (u >= 0 && u < N) ? (float)F[u][e & 15] : __int_as_float(0x7fc00000);
        }
        for (int e = lane; e < J * 6; e += THREADS) {
            const int j = e / 6, k = e - 6 * j;
            const int i = jlink[j];
            float out = __int_as_float(0x7fc00000);
            if (i >= 0) {
                if (k < 3)  // a = R_i @ axis_i (the joint's own motion leaves its axis where it is)
                    out = (float)((F[i][4 * k] * axis[3 * i] + F[i][4 * k + 1] * axis[3 * i + 1]) + F[i][4 * k + 2] * axis[3 * i + 2]);
                else        // p = the moved link's origin: on the axis of a revolute joint (unused for a prismatic one)
                    out = (float)F[i][4 * (k - 3) + 3];
            }
            joint_frames[e] = out;
        }
    } else {
        const double* Fm = F[mount];
        for (int e = lane; e < L * 16; e += THREADS) {
            const int u = use[e >> 4], r = (e >> 2) & 3, c = e & 3;
            float out = __int_as_float(0x7fc00000);
            if (u >= 0 && u < N) {
                const double* Fu = F[u];
                double t;
                if (r == 3) {
                    t = Fu[12 + c];
                } else if (c < 3) {
                    t = (Fm[r] * Fu[c] + Fm[4 + r] * Fu[4 + c]) + Fm[8 + r] * Fu[8 + c];
                } else {
                    const double d0 = Fu[3] - Fm[3], d1 = Fu[7] - Fm[7], d2 = Fu[11] - Fm[11];
                    t = (Fm[r] * d0 + Fm[4 + r] * d1) + Fm[8 + r] * d2;
                }
                out = (float)t;
            }
            link_poses[e] = out;
        }
        for (int e = lane; e < J * 6; e += THREADS) {
            const int j = e / 6, k = e - 6 * j;
            const int i = jlink[j];
            float out = __int_as_float(0x7fc00000);
            if (i >= 0) {
                const double* Fi = F[i];
                double v0, v1, v2;
                if (k < 3) {  // the base-frame axis a = R_i @ axis_i, as above but not yet rounded
                    const double ax = axis[3 * i], ay = axis[3 * i + 1], az = axis[3 * i + 2];
                    v0 = (Fi[0] * ax + Fi[1] * ay) + Fi[2] * az;
                    v1 = (Fi[4] * ax + Fi[5] * ay) + Fi[6] * az;
                    v2 = (Fi[8] * ax + Fi[9] * ay) + Fi[10] * az;
                } else {
                    v0 = Fi[3] - Fm[3];
                    v1 = Fi[7] - Fm[7];
                    v2 = Fi[11] - Fm[11];
                }
                const int r = k < 3 ? k : k - 3;
                const double t = (Fm[r] * v0 + Fm[4 + r] * v1) + Fm[8 + r] * v2;
                out = (float)((k < 3 && ((mount_upstream >> j) & 1u)) ? -t : t);
            }
            joint_frames[e] = out;
        }
    }
}

}  // namespace ehr
