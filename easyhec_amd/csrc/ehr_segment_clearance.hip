// ehr_segment_clearance.hip -- certified clearance of the sphere proxies along WHOLE straight joint-space segments
// (easyhec_amd/feasibility.py, DESIGN.md sections 6u and 6v): ehr_segment_clearance and ehr_edge_clearance of include/ehr.h, which
// states the mathematics expression by expression.  The search itself is the text of ehr_segment_body.h, which each kernel
// includes with its own two end points (SEG_Q0, SEG_Q1).
//
//   segment_clearance_kernel : one workgroup of 256 threads per candidate; every segment starts at the launch's one q0.
//   edge_clearance_kernel    : one workgroup of 256 threads per edge of a roadmap; the segment runs from node edge_a[e] to node
//                              edge_b[e].  An index outside 0..V-1 ends the workgroup before it reads a node or meets a barrier
//                              (the indices are uniform over the workgroup); thread 0 adds the edge's length.
//
// Float64 throughout, built with -ffp-contract=off.  No atomics, no allocation, no synchronisation with the host.
#include "ehr_segment_core.h"

namespace ehr {

__global__ void __launch_bounds__(SEG_THREADS) segment_clearance_kernel(const SegArgs A) {
#define SEG_Q0(j) A.q0[j]
#define SEG_Q1(j) A.q1[b * (size_t)J + j]  // (b, J: the body's own blockIdx.x and A.J)
#include "ehr_segment_body.h"
#undef SEG_Q0
#undef SEG_Q1
}

struct EdgeArgs {  // by value in the kernel's arguments
    SegArgs seg;   // (q0 = q1 = nodes)
    const int *edge_a, *edge_b;
    int V;
    double* length;
};

__global__ void __launch_bounds__(SEG_THREADS) edge_clearance_kernel(const EdgeArgs P) {
    const SegArgs& A = P.seg;
    const size_t edge = blockIdx.x;
    const int na = P.edge_a[edge], nb = P.edge_b[edge];
    if (na < 0 || na >= P.V || nb < 0 || nb >= P.V) {  // skipped: no node row is read, the trace stays as it is
        if (threadIdx.x == 0) {
            A.status[edge] = 3;
            A.t_free[edge] = 0.0;
            A.evals[edge] = 0;
            A.cert_self[edge] = A.cutoff;
            A.cert_env[edge] = A.cutoff;
            A.cert_reach[edge] = A.cutoff;
            A.stop_self[edge] = feas_nan();
            A.stop_env[edge] = feas_nan();
            A.stop_reach[edge] = feas_nan();
            A.stop_pair[edge] = -1;
            P.length[edge] = feas_nan();
        }
        return;
    }
    {
#define SEG_Q0(j) A.q0[(size_t)na * J + j]
#define SEG_Q1(j) A.q1[(size_t)nb * J + j]
#include "ehr_segment_body.h"
#undef SEG_Q0
#undef SEG_Q1
    }
    if (threadIdx.x == 0) {  // sqrt(sum_j d_j d_j), j ascending from 0.0, d_j the search's
        const double* __restrict__ q0 = A.q0 + (size_t)na * A.J;
        const double* __restrict__ q1 = A.q0 + (size_t)nb * A.J;
        double acc = 0.0;
        bool bad = false;
        for (int j = 0; j < A.J; j++) {
            const double a = q0[j], c = q1[j], d = c - a;
            bad |= !seg_finite(a) || !seg_finite(c);
            acc = acc + d * d;
        }
        P.length[edge] = bad ? feas_nan() : sqrt(acc);
    }
}

}  // namespace ehr

using namespace ehr;

// The checks and the argument block the two entry points share; q0, q1 stay the caller's.
static int seg_fill(const char* who, SegArgs& A, const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                    const int32_t* qidx, const int32_t* use, int N, int J, int L, const float* offset, int n, const double* spheres,
                    const int32_t* sphere_offsets, const double* link_bounds, const uint32_t* pair_enable, const double* planes,
                    int n_planes, const double* obstacles, int n_obstacles, uint32_t env_links, const double* reach, double cutoff,
                    const uint32_t* upstream, const uint32_t* joint_below, const double* reach_radius, double margin, int min_depth,
                    int max_depth, int max_evals, int32_t* status, double* t_free, int32_t* evals, double* cert_self,
                    double* cert_env, double* cert_reach, double* stop_self, double* stop_env, double* stop_reach,
                    int32_t* stop_pair, double* trace_t, double* trace_val) {
    if (N < 1 || N > EHR_JOINT_MAX_LINKS || J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || L > EHR_FEAS_MAX_LINKS || n < 1)
        return fail(EHR_ERR_INVALID, "%s: bad sizes (N %d <= %d links, J %d <= %d joints, L %d: 1 <= L <= %d, n %d >= 1)", who,
                    N, EHR_JOINT_MAX_LINKS, J, EHR_JOINT_MAX_JOINTS, L, EHR_FEAS_MAX_LINKS, n);
    if (n_planes < 0 || n_planes > EHR_FEAS_MAX_PLANES || n_obstacles < 0 || n_obstacles > EHR_FEAS_MAX_OBSTACLES)
        return fail(EHR_ERR_INVALID, "%s: bad sizes (%d planes <= %d, %d obstacles <= %d)", who, n_planes, EHR_FEAS_MAX_PLANES,
                    n_obstacles, EHR_FEAS_MAX_OBSTACLES);
    if (min_depth < 0 || min_depth > max_depth || max_depth > EHR_SEG_MAX_DEPTH || max_evals < 1 || max_evals > EHR_SEG_MAX_EVALS)
        return fail(EHR_ERR_INVALID, "%s: bad budget (0 <= min_depth %d <= max_depth %d <= %d, 1 <= max_evals %d <= %d)", who,
                    min_depth, max_depth, EHR_SEG_MAX_DEPTH, max_evals, EHR_SEG_MAX_EVALS);
    if (!(cutoff > 0.0) || !(cutoff <= 1.7976931348623157e308) || !(margin >= 0.0) || !(margin < cutoff))
        return fail(EHR_ERR_INVALID, "%s: need 0 <= margin %g < cutoff %g, finite", who, margin, cutoff);
    if (!parent || !origin || !kind || !axis || !qidx || !use || !offset || !sphere_offsets || !link_bounds || !pair_enable ||
        !upstream || !joint_below || !reach_radius || !status || !t_free || !evals || !cert_self || !cert_env || !cert_reach ||
        !stop_self || !stop_env || !stop_reach || !stop_pair || (n_planes > 0 && !planes) || (n_obstacles > 0 && !obstacles) ||
        (!trace_t != !trace_val))
        return fail(EHR_ERR_INVALID, "%s: NULL tensor", who);
    for (int l = 0; l <= L; l++) {
        A.offs.v[l] = sphere_offsets[l];
        if ((l == 0 && A.offs.v[0] != 0) || (l > 0 && A.offs.v[l] < A.offs.v[l - 1]))
            return fail(EHR_ERR_INVALID, "%s: sphere_offsets must ascend from 0 (entry %d is %d)", who, l, A.offs.v[l]);
    }
    const int S = A.offs.v[L];
    if (S > EHR_SEG_MAX_SPHERES) return fail(EHR_ERR_INVALID, "%s: bad sizes (S %d <= %d spheres)", who, S, EHR_SEG_MAX_SPHERES);
    if (S > 0 && !spheres) return fail(EHR_ERR_INVALID, "%s: NULL tensor", who);
    A.parent = parent, A.kind = kind, A.qidx = qidx, A.use = use, A.origin = origin, A.axis = axis;
    A.N = N, A.J = J, A.L = L, A.offset = offset, A.spheres = spheres, A.link_bounds = link_bounds;
    A.pair_enable = pair_enable, A.planes = planes, A.Np = n_planes, A.obstacles = obstacles, A.No = n_obstacles;
    A.env_links = env_links, A.reach = reach, A.cutoff = cutoff, A.upstream = upstream, A.joint_below = joint_below;
    A.reach_radius = reach_radius, A.margin = margin, A.min_depth = min_depth, A.max_depth = max_depth, A.max_evals = max_evals;
    A.S = S, A.Sp = (S + 1) & ~1;
    A.status = status, A.evals = evals, A.stop_pair = stop_pair, A.t_free = t_free, A.cert_self = cert_self, A.cert_env = cert_env;
    A.cert_reach = cert_reach, A.stop_self = stop_self, A.stop_env = stop_env, A.stop_reach = stop_reach;
    A.trace_t = trace_t, A.trace_val = trace_val;
    return EHR_OK;
}

// More than the default limit of a launch's LDS: ask for it (a runtime that needs no asking may refuse the question; the launch is
// what decides, and it fails cleanly where the device has less LDS than this).
static void seg_ask_lds(const void* kernel, size_t lds) {
    if (lds > 64 * 1024 - SEG_STATIC_BYTES && hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        (void)hipGetLastError();
}

extern "C" {

int ehr_segment_clearance(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis,
                          const int32_t* qidx, const int32_t* use, int N, int J, int L, const double* q0, const double* q1,
                          const float* offset, int n, const double* spheres, const int32_t* sphere_offsets,
                          const double* link_bounds, const uint32_t* pair_enable, const double* planes, int n_planes,
                          const double* obstacles, int n_obstacles, uint32_t env_links, const double* reach, double cutoff,
                          const uint32_t* upstream, const uint32_t* joint_below, const double* reach_radius, double margin,
                          int min_depth, int max_depth, int max_evals, int32_t* status, double* t_free, int32_t* evals,
                          double* cert_self, double* cert_env, double* cert_reach, double* stop_self, double* stop_env,
                          double* stop_reach, int32_t* stop_pair, double* trace_t, double* trace_val, void* stream) {
    SegArgs A = {};
    const int rc = seg_fill("ehr_segment_clearance", A, parent, origin, kind, axis, qidx, use, N, J, L, offset, n, spheres,
                            sphere_offsets, link_bounds, pair_enable, planes, n_planes, obstacles, n_obstacles, env_links, reach,
                            cutoff, upstream, joint_below, reach_radius, margin, min_depth, max_depth, max_evals, status, t_free,
                            evals, cert_self, cert_env, cert_reach, stop_self, stop_env, stop_reach, stop_pair, trace_t, trace_val);
    if (rc != EHR_OK) return rc;
    if (!q0 || !q1) return fail(EHR_ERR_INVALID, "ehr_segment_clearance: NULL tensor");
    A.q0 = q0, A.q1 = q1;
    const size_t lds = seg_lds_bytes(A.Sp);
    seg_ask_lds((const void*)segment_clearance_kernel, lds);
    segment_clearance_kernel<<<(unsigned)n, SEG_THREADS, lds, (hipStream_t)stream>>>(A);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_edge_clearance(const int32_t* parent, const double* origin, const int32_t* kind, const double* axis, const int32_t* qidx,
                       const int32_t* use, int N, int J, int L, const double* nodes, int V, const int32_t* edge_a,
                       const int32_t* edge_b, const float* offset, int n, const double* spheres, const int32_t* sphere_offsets,
                       const double* link_bounds, const uint32_t* pair_enable, const double* planes, int n_planes,
                       const double* obstacles, int n_obstacles, uint32_t env_links, const double* reach, double cutoff,
                       const uint32_t* upstream, const uint32_t* joint_below, const double* reach_radius, double margin,
                       int min_depth, int max_depth, int max_evals, int32_t* status, double* t_free, int32_t* evals,
                       double* cert_self, double* cert_env, double* cert_reach, double* stop_self, double* stop_env,
                       double* stop_reach, int32_t* stop_pair, double* length, double* trace_t, double* trace_val, void* stream) {
    EdgeArgs P = {};
    const int rc = seg_fill("ehr_edge_clearance", P.seg, parent, origin, kind, axis, qidx, use, N, J, L, offset, n, spheres,
                            sphere_offsets, link_bounds, pair_enable, planes, n_planes, obstacles, n_obstacles, env_links, reach,
                            cutoff, upstream, joint_below, reach_radius, margin, min_depth, max_depth, max_evals, status, t_free,
                            evals, cert_self, cert_env, cert_reach, stop_self, stop_env, stop_reach, stop_pair, trace_t, trace_val);
    if (rc != EHR_OK) return rc;
    if (V < 1) return fail(EHR_ERR_INVALID, "ehr_edge_clearance: bad sizes (V %d >= 1 nodes)", V);
    if (!nodes || !edge_a || !edge_b || !length) return fail(EHR_ERR_INVALID, "ehr_edge_clearance: NULL tensor");
    P.seg.q0 = P.seg.q1 = nodes, P.edge_a = edge_a, P.edge_b = edge_b, P.V = V, P.length = length;
    const size_t lds = seg_lds_bytes(P.seg.Sp);
    seg_ask_lds((const void*)edge_clearance_kernel, lds);
    edge_clearance_kernel<<<(unsigned)n, SEG_THREADS, lds, (hipStream_t)stream>>>(P);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
