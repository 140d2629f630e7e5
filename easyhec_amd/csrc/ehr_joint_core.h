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
template <int THREADS>
__device__ __forceinline__ void joint_forward_view(const int* __restrict__ parent, const double* __restrict__ origin,
                                                   const int* __restrict__ kind, const double* __restrict__ axis,
                                                   const int* __restrict__ qidx, const int* __restrict__ use, int N, int J,
                                                   int L, const double* __restrict__ qpos, const float* __restrict__ offset,
                                                   float* __restrict__ link_poses, float* __restrict__ joint_frames) {
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
}

}  // namespace ehr
