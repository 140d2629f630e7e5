// ehr_segment_core.h -- what the kernels of ehr_segment_clearance.hip share beside the search itself (include/ehr.h states the
// mathematics expression by expression): the LDS layout, the argument block and the contract's expressions.  The search -- the
// statements of a kernel's body -- is ehr_segment_body.h, which both kernels include: segment_clearance_kernel (every
// candidate from one start) and edge_clearance_kernel (every edge of a roadmap between its own two nodes).
#pragma once
#include "ehr_device.h"      // wave_xor
#include "ehr_feas_core.h"   // FeasOffsets, FEAS_CULL_SLACK, feas_*, feas_to_base
#include "ehr_joint_core.h"  // joint_forward_view

#define SEG_THREADS 256

namespace ehr {

// LDS of one workgroup.  Dynamic: X | Y | Z | r | E of the Sp = S rounded up to even spheres (40 bytes each), then the fixed tail
// below; static: joint_forward_view's frames (SEG_STATIC_BYTES).  EHR_SEG_MAX_SPHERES of include/ehr.h is the largest S for
// which the sum stays inside the 160 KiB of a gfx950 compute unit.
#define SEG_TAIL_DOUBLES (EHR_FEAS_MAX_LINKS * 4 + 24 + 32 * 32 + 4 * 32)  // bounds | 4 waves' six minima | G [J][32] | |d|, d, q0, q(c)
#define SEG_TAIL_FLOATS (EHR_FEAS_MAX_LINKS * 16 + EHR_JOINT_MAX_JOINTS * 6)  // link_poses | joint_frames of the evaluation
#define SEG_TAIL_INTS (4 + 36 + 32 + 32 + 32 + 8)  // 4 waves' pair codes | offsets | joint kinds | upstream | joint_below | decision
#define SEG_TAIL_BYTES (SEG_TAIL_DOUBLES * 8 + SEG_TAIL_FLOATS * 4 + SEG_TAIL_INTS * 4 + EHR_FEAS_MAX_OBSTACLES)
#define SEG_STATIC_BYTES (18 * 1024)  // OM, F, sc, jlink: 18048 bytes, 18304 as the compiler lays them out
static inline size_t seg_lds_bytes(int Sp) { return (size_t)Sp * 40 + SEG_TAIL_BYTES; }
static_assert((size_t)EHR_SEG_MAX_SPHERES * 40 + SEG_TAIL_BYTES + SEG_STATIC_BYTES <= 160 * 1024, "EHR_SEG_MAX_SPHERES");

struct SegArgs {  // by value in the kernel's arguments; q0, q1: the tables a segment's two end points are rows of
    const int *parent, *kind, *qidx, *use;
    const double *origin, *axis;
    int N, J, L;
    const double *q0, *q1;
    const float* offset;
    const double* spheres;
    FeasOffsets offs;
    const double* link_bounds;
    const unsigned* pair_enable;
    const double* planes;
    int Np;
    const double* obstacles;
    int No;
    unsigned env_links;
    const double* reach;
    double cutoff;
    const unsigned *upstream, *joint_below;
    const double* reach_radius;
    double margin;
    int min_depth, max_depth, max_evals, S, Sp;
    int *status, *evals, *stop_pair;
    double *t_free, *cert_self, *cert_env, *cert_reach, *stop_self, *stop_env, *stop_reach, *trace_t, *trace_val;
};

__device__ __forceinline__ bool seg_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (NaN: false)
__device__ __forceinline__ double seg_pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }  // 2^e, exact

// ---- the contract's expressions ---------------------------------------------------------------------------------------------
// sum_{j in M} |d_j| rho[j,s], j ascending from 0.0: rho = |(c - p_j) x a_j| + r for a revolute joint, 1 otherwise
__device__ __forceinline__ double seg_rate(unsigned M, int J, const int* __restrict__ jkind, const float* __restrict__ JF,
                                           const double* __restrict__ dabs, double cx, double cy, double cz, double r) {
    double acc = 0.0;
    for (int j = 0; j < J; j++) {
        if (!((M >> j) & 1u)) continue;
        double rho = 1.0;
        if (jkind[j] == 1) {
            const double ax = (double)JF[6 * j], ay = (double)JF[6 * j + 1], az = (double)JF[6 * j + 2];
            const double vx = cx - (double)JF[6 * j + 3], vy = cy - (double)JF[6 * j + 4], vz = cz - (double)JF[6 * j + 5];
            rho = sqrt(feas_norm2(vy * az - vz * ay, vz * ax - vx * az, vx * ay - vy * ax)) + r;
        }
        acc = acc + dabs[j] * rho;
    }
    return acc;
}
// sum_{j in M} |d_j| T[j * stride + l], j ascending from 0.0: C(l,M) on G, the first-order part of Ebar(l,M) on W
__device__ __forceinline__ double seg_sum(unsigned M, int J, const double* __restrict__ dabs, const double* __restrict__ T,
                                          int stride, int l) {
    double acc = 0.0;
    for (int j = 0; j < J; j++)
        if ((M >> j) & 1u) acc = acc + dabs[j] * T[j * stride + l];
    return acc;
}
// E = h * first + (0.5 * h * h) * C
__device__ __forceinline__ double seg_inflate(double h, double first, double C) { return h * first + ((0.5 * h) * h) * C; }

// The interval after (k, i) in the depth-first walk, left to right, whose roots are the 2^min_depth intervals of depth min_depth:
// a finished right child finishes its parent.  False: none is left.
__device__ __forceinline__ bool seg_next(int min_depth, int& k, unsigned& i) {
    while (k > min_depth && (i & 1u)) {
        i >>= 1;
        k--;
    }
    i++;
    return !(k == min_depth && i == (1u << min_depth));
}

#define SEG_MIN_STEP(K)                                                      \
    {                                                                        \
        const double o = wave_xor<K>(v[0]);                                  \
        const int op = wave_xor<K>(sp);                                      \
        if (o < v[0] || (o == v[0] && op < sp && op >= 0)) {                 \
            v[0] = o;                                                        \
            sp = op;                                                         \
        }                                                                    \
        _Pragma("unroll") for (int q = 1; q < 6; q++) {                      \
            const double u = wave_xor<K>(v[q]);                              \
            if (u < v[q]) v[q] = u;                                          \
        }                                                                    \
    }

}  // namespace ehr
