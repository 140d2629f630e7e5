// ehr_segment_clearance.hip -- certified clearance of the sphere proxies along the WHOLE straight joint-space segment from the
// current configuration to a candidate (easyhec_amd/feasibility.py): ehr_segment_clearance of
// include/ehr.h, which states the mathematics expression by expression.
//
//   segment_clearance_kernel : one workgroup of 256 threads per candidate.  Depth-first bisection over the dyadic intervals of
//                              [0,1]; per interval ONE evaluation at its centre: the kinematics (joint_forward_view, the bits of
//                              ehr_joint_forward), the proxies to the base frame in LDS (feas_to_base, the bits of
//                              ehr_config_clearance), then every clearance twice, side by side: raw, and lowered by how far the
//                              spheres involved can travel within the interval's half-width (rates from each sphere's distance
//                              to each joint axis AT the centre, second order from the chain lengths).  Thread 0 decides (hit /
//                              certified / split / out of budget) and the decision is broadcast through LDS.
//
// The search needs no stack of its own: the pending intervals of a left-to-right depth-first walk are the right siblings of the
// current interval's ancestors, so (depth, index) of the current interval is the whole state -- see seg_next.
// Float64 throughout, built with -ffp-contract=off; every condition around a barrier is uniform over the workgroup; the loop runs
// at most max_evals times.  No atomics, no allocation, no synchronisation with the host.
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

struct SegArgs {  // by value in the kernel's arguments
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

__global__ void __launch_bounds__(SEG_THREADS) segment_clearance_kernel(const SegArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = A.S, Sp = A.Sp, L = A.L, J = A.J, Np = A.Np, No = A.No;
    double* X = (double*)smem;
    double* Y = X + Sp;
    double* Z = Y + Sp;
    double* Rr = Z + Sp;
    double* E = Rr + Sp;                        // the spheres' inflation under the current pair's masks
    double* BW = E + Sp;                        // [L][4] bounding spheres, base frame
    double* red = BW + EHR_FEAS_MAX_LINKS * 4;  // [4 waves][6]
    double* G = red + 24;                       // [J][32]
    double* dabs = G + 32 * 32;                 // |d_j|
    double* dd = dabs + 32;                     // d_j
    double* qa = dd + 32;                       // q0_j
    double* qc = qa + 32;                       // q(c)_j
    float* LP = (float*)(qc + 32);              // [L][16]
    float* JF = LP + EHR_FEAS_MAX_LINKS * 16;   // [J][6]
    int* redp = (int*)(JF + EHR_JOINT_MAX_JOINTS * 6);
    int* off = redp + 4;                        // [L + 1]
    int* jkind = off + 36;                      // the kind of the link each active joint moves
    int* ups = jkind + 32;                      // upstream [L]
    int* jbel = ups + 32;                       // joint_below [J]
    int* dec = jbel + 32;                       // thread 0's decision
    unsigned char* skip = (unsigned char*)(dec + 8);  // [No]: the current link's bound clears this obstacle
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t b = blockIdx.x;
    const double cutoff = A.cutoff, margin = A.margin, cull = cutoff + FEAS_CULL_SLACK;
    const double* __restrict__ W = A.reach_radius;
    const double* __restrict__ planes = A.planes;
    const double* __restrict__ obstacles = A.obstacles;

    // the candidate's tables
    int bad = 0;
    if (tid <= L) off[tid] = A.offs.v[tid];
    if (tid < L) ups[tid] = (int)A.upstream[tid];
    if (tid < 32) jkind[tid] = 0;
    if (tid < J) {
        const double a = A.q0[tid], c = A.q1[b * (size_t)J + tid];
        bad = !seg_finite(a) || !seg_finite(c);
        qa[tid] = a;
        dd[tid] = c - a;
        dabs[tid] = fabs(c - a);
        jbel[tid] = (int)A.joint_below[tid];
    }
    __syncthreads();
    if (tid < A.N) {
        const int c = A.qidx[tid];
        if (c >= 0 && c < J) jkind[c] = A.kind[tid];
    }
    bad = __syncthreads_or(bad);

    // thread 0's record of the search
    int status = bad ? 3 : -1, ev = 0, k = A.min_depth, stop_pair = -1;
    unsigned i = 0;
    double t_free = 0.0, cmin_s = cutoff, cmin_e = cutoff, cmin_r = cutoff;
    double stop_s = feas_nan(), stop_e = feas_nan(), stop_r = feas_nan();

    if (!bad) {
        // G[j,l] = sum_{k in up(l), k below j} |d_k| W[k,l], k ascending
        for (int e = tid; e < J * L; e += SEG_THREADS) {
            const int j = e / L, l = e - j * L;
            G[j * 32 + l] = seg_sum((unsigned)ups[l] & (unsigned)jbel[j], J, dabs, W, L, l);
        }
        __syncthreads();
    }

    while (status < 0) {
        const double h = seg_pow2(-(k + 1));  // the half-width; the interval is [a, a + 2 h]
        const double a = (double)(2u * i) * h, c = (double)(2u * i + 1u) * h;
        t_free = a;
        if (ev >= A.max_evals) {  // out of budget between two intervals: no evaluation stopped the search
            status = 2;
            break;
        }
        if (tid < J) qc[tid] = qa[tid] + c * dd[tid];
        __syncthreads();
        joint_forward_view<SEG_THREADS>(A.parent, A.origin, A.kind, A.axis, A.qidx, A.use, A.N, J, L, qc, A.offset, LP, JF);
        __syncthreads();
        bad = 0;
        for (int e = tid; e < L * 16; e += SEG_THREADS) bad |= !feas_finite(LP[e]);
        bad = __syncthreads_or(bad);
        if (bad) {  // a pose that cannot be judged
            if (tid == 0 && A.trace_t) {
                A.trace_t[b * (size_t)A.max_evals + ev] = c;
                for (int q = 0; q < 6; q++) A.trace_val[(b * (size_t)A.max_evals + ev) * 6 + q] = feas_nan();
            }
            ev++;
            status = 3;
            break;
        }
        feas_to_base<SEG_THREADS>(LP, A.spheres, off, A.link_bounds, L, S, X, Y, Z, Rr, BW);
        __syncthreads();

        // v: raw self, env, reach | certified self, env, reach of this thread
        double v[6] = {cutoff, cutoff, cutoff, cutoff, cutoff, cutoff};
        int sp = -1;

        // reach and the environment, per link, the inflation under up(l)
        for (int l = 0; l < L; l++) {
            const int s0 = off[l], s1 = off[l + 1];
            if (s0 == s1) continue;
            const bool env = (Np > 0 || No > 0) && ((A.env_links >> l) & 1u);
            if (!env && !A.reach) continue;
            const unsigned M = (unsigned)ups[l];
            const double C = seg_sum(M, J, dabs, G, 32, l);
            const double far = cutoff - seg_inflate(h, seg_sum(M, J, dabs, W, L, l), C);  // stands for what lies beyond cutoff
            if (A.reach && far < v[5]) v[5] = far;
            unsigned pmask = 0;  // the planes the link's bound does not clear
            if (env) {
                if (far < v[4]) v[4] = far;
                const double bx = BW[4 * l], by = BW[4 * l + 1], bz = BW[4 * l + 2], bR = BW[4 * l + 3];
                for (int p = 0; p < Np; p++)
                    if (!(feas_plane(planes[4 * p], planes[4 * p + 1], planes[4 * p + 2], planes[4 * p + 3], bx, by, bz, bR) > cull))
                        pmask |= 1u << p;
                if (No > 0) {
                    __syncthreads();  // (the previous link's flags have been read)
                    for (int o = tid; o < No; o += SEG_THREADS)
                        skip[o] = feas_gap(bx - obstacles[4 * o], by - obstacles[4 * o + 1], bz - obstacles[4 * o + 2], bR,
                                           obstacles[4 * o + 3]) > cull;
                    __syncthreads();
                }
            }
            for (int s = s0 + tid; s < s1; s += SEG_THREADS) {
                const double cx = X[s], cy = Y[s], cz = Z[s], r = Rr[s];
                const double e = seg_inflate(h, seg_rate(M, J, jkind, JF, dabs, cx, cy, cz, r), C);
                if (A.reach) {
                    const double d = feas_reach(A.reach[3], cx - A.reach[0], cy - A.reach[1], cz - A.reach[2], r);
                    if (d < v[2]) v[2] = d;
                    if (d < cutoff && d - e < v[5]) v[5] = d - e;
                }
                if (!env) continue;
                for (int p = 0; p < Np; p++) {
                    if (!((pmask >> p) & 1u)) continue;
                    const double d = feas_plane(planes[4 * p], planes[4 * p + 1], planes[4 * p + 2], planes[4 * p + 3], cx, cy, cz, r);
                    if (d < v[1]) v[1] = d;
                    if (d < cutoff && d - e < v[4]) v[4] = d - e;
                }
                for (int o = 0; o < No; o++) {
                    if (skip[o]) continue;
                    const double d = feas_gap(cx - obstacles[4 * o], cy - obstacles[4 * o + 1], cz - obstacles[4 * o + 2], r,
                                              obstacles[4 * o + 3]);
                    if (d < v[1]) v[1] = d;
                    if (d < cutoff && d - e < v[4]) v[4] = d - e;
                }
            }
        }

        // the arm against itself: link pairs in the order of their code 32 i + j, as config_clearance_kernel walks them
        const unsigned inL = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
        for (int li = 0; li + 1 < L; li++) {
            const unsigned m = A.pair_enable[li] & ~((2u << li) - 1u) & inL;  // j > i only
            const int oi = off[li], ni = off[li + 1] - oi;
            if (!m || ni <= 0) continue;
            for (int lj = li + 1; lj < L; lj++) {
                const int oj = off[lj], nj = off[lj + 1] - oj;
                if (!((m >> lj) & 1u) || nj <= 0) continue;
                // joints upstream of both links move them rigidly together
                const unsigned Mi = (unsigned)ups[li] & ~(unsigned)ups[lj], Mj = (unsigned)ups[lj] & ~(unsigned)ups[li];
                const double Ci = seg_sum(Mi, J, dabs, G, 32, li), Cj = seg_sum(Mj, J, dabs, G, 32, lj);
                // the pair's far value: every sphere pair at or beyond cutoff, a culled link pair's included, stays above it
                const double far = cutoff - (seg_inflate(h, seg_sum(Mi, J, dabs, W, L, li), Ci) +
                                             seg_inflate(h, seg_sum(Mj, J, dabs, W, L, lj), Cj));
                if (far < v[3]) v[3] = far;
                if (feas_bound_gap(BW, li, lj) > cull) continue;
                __syncthreads();  // (the previous pair's E has been read)
                for (int s = oi + tid; s < oi + ni; s += SEG_THREADS)
                    E[s] = seg_inflate(h, seg_rate(Mi, J, jkind, JF, dabs, X[s], Y[s], Z[s], Rr[s]), Ci);
                for (int s = oj + tid; s < oj + nj; s += SEG_THREADS)
                    E[s] = seg_inflate(h, seg_rate(Mj, J, jkind, JF, dabs, X[s], Y[s], Z[s], Rr[s]), Cj);
                __syncthreads();
                const int code = 32 * li + lj;
                const bool swap = nj < ni;
                const int a0 = swap ? oj : oi, na = swap ? nj : ni, b0 = swap ? oi : oj, nb = swap ? ni : nj;
                for (int sa = wave; sa < na; sa += SEG_THREADS / 64) {
                    const double ax = X[a0 + sa], ay = Y[a0 + sa], az = Z[a0 + sa], ar = Rr[a0 + sa], ae = E[a0 + sa];
                    for (int sb = b0 + lane; sb < b0 + nb; sb += 64) {
                        const double dx = ax - X[sb], dy = ay - Y[sb], dz = az - Z[sb], rs = ar + Rr[sb];
                        // no square root for a pair beyond cutoff: with t = cutoff + rs > 0, d2 > t^2 (1 + 1e-12) puts the
                        // rounded root above t (1 + 4e-13), that is above cutoff + rs by far more than t's own rounding, and
                        // rounding is monotonic: the gap comes out >= cutoff.  Such a gap replaces no raw minimum (they start
                        // at cutoff) and does not pass the certified value's gate; the pair's far value stands for it.
                        const double t = cutoff + rs, d2 = feas_norm2(dx, dy, dz);
                        if (d2 > (t * t) * 1.000000000001) continue;
                        const double d = sqrt(d2) - rs;  // == feas_gap(dx, dy, dz, ar, Rr[sb])
                        if (d < v[0]) {
                            v[0] = d;
                            sp = code;
                        }
                        if (d < cutoff) {
                            const double ci = d - (ae + E[sb]);
                            if (ci < v[3]) v[3] = ci;
                        }
                    }
                }
            }
        }

        // minima over the workgroup; among equal raw self clearances the lowest pair code
        SEG_MIN_STEP(32) SEG_MIN_STEP(16) SEG_MIN_STEP(8) SEG_MIN_STEP(4) SEG_MIN_STEP(2) SEG_MIN_STEP(1)
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; q++) red[6 * wave + q] = v[q];
            redp[wave] = sp;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < SEG_THREADS / 64; w++) {
                const double o = red[6 * w];
                const int op = redp[w];
                if (o < v[0] || (o == v[0] && op < sp && op >= 0)) {
                    v[0] = o;
                    sp = op;
                }
#pragma unroll
                for (int q = 1; q < 6; q++)
                    if (red[6 * w + q] < v[q]) v[q] = red[6 * w + q];
            }
            v[3] -= FEAS_CULL_SLACK;  // the float32 rounding of poses and axes
            v[4] -= FEAS_CULL_SLACK;
            v[5] -= FEAS_CULL_SLACK;
            if (A.trace_t) {
                A.trace_t[b * (size_t)A.max_evals + ev] = c;
#pragma unroll
                for (int q = 0; q < 6; q++) A.trace_val[(b * (size_t)A.max_evals + ev) * 6 + q] = v[q];
            }
            int act;
            if (!(v[0] > margin) || !(v[1] > margin) || !(v[2] >= 0.0)) {
                act = 1;  // hit
            } else if (v[3] > margin && v[4] > margin && v[5] >= 0.0) {
                act = 0;  // the whole interval is certified
                if (v[3] < cmin_s) cmin_s = v[3];
                if (v[4] < cmin_e) cmin_e = v[4];
                if (v[5] < cmin_r) cmin_r = v[5];
            } else if (k < A.max_depth && ev + 1 < A.max_evals) {
                act = 4;  // split, the left half first
            } else {
                act = 2;  // undecided
            }
            if (act == 1 || act == 2) {
                stop_s = v[0];
                stop_e = v[1];
                stop_r = v[2];
                stop_pair = sp;
            }
            dec[0] = act;
        }
        __syncthreads();  // (also: everybody has left the evaluation's LDS before the next one writes it)
        const int act = dec[0];
        ev++;
        if (act == 0) {
            if (!seg_next(A.min_depth, k, i)) {
                status = 0;
                t_free = 1.0;
            }
        } else if (act == 4) {
            k++;
            i *= 2u;
        } else {
            status = act;
        }
    }

    if (tid == 0) {
        A.status[b] = status;
        A.t_free[b] = t_free;
        A.evals[b] = ev;
        A.cert_self[b] = cmin_s;
        A.cert_env[b] = cmin_e;
        A.cert_reach[b] = cmin_r;
        A.stop_self[b] = stop_s;
        A.stop_env[b] = stop_e;
        A.stop_reach[b] = stop_r;
        A.stop_pair[b] = stop_pair;
    }
}

}  // namespace ehr

using namespace ehr;

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
    if (N < 1 || N > EHR_JOINT_MAX_LINKS || J < 1 || J > EHR_JOINT_MAX_JOINTS || L < 1 || L > EHR_FEAS_MAX_LINKS || n < 1)
        return fail(EHR_ERR_INVALID, "ehr_segment_clearance: bad sizes (N %d <= %d links, J %d <= %d joints, L %d: 1 <= L <= %d, n %d >= 1)",
                    N, EHR_JOINT_MAX_LINKS, J, EHR_JOINT_MAX_JOINTS, L, EHR_FEAS_MAX_LINKS, n);
    if (n_planes < 0 || n_planes > EHR_FEAS_MAX_PLANES || n_obstacles < 0 || n_obstacles > EHR_FEAS_MAX_OBSTACLES)
        return fail(EHR_ERR_INVALID, "ehr_segment_clearance: bad sizes (%d planes <= %d, %d obstacles <= %d)", n_planes,
                    EHR_FEAS_MAX_PLANES, n_obstacles, EHR_FEAS_MAX_OBSTACLES);
    if (min_depth < 0 || min_depth > max_depth || max_depth > EHR_SEG_MAX_DEPTH || max_evals < 1 || max_evals > EHR_SEG_MAX_EVALS)
        return fail(EHR_ERR_INVALID, "ehr_segment_clearance: bad budget (0 <= min_depth %d <= max_depth %d <= %d, 1 <= max_evals %d <= %d)",
                    min_depth, max_depth, EHR_SEG_MAX_DEPTH, max_evals, EHR_SEG_MAX_EVALS);
    if (!(cutoff > 0.0) || !(cutoff <= 1.7976931348623157e308) || !(margin >= 0.0) || !(margin < cutoff))
        return fail(EHR_ERR_INVALID, "ehr_segment_clearance: need 0 <= margin %g < cutoff %g, finite", margin, cutoff);
    if (!parent || !origin || !kind || !axis || !qidx || !use || !q0 || !q1 || !offset || !sphere_offsets || !link_bounds ||
        !pair_enable || !upstream || !joint_below || !reach_radius || !status || !t_free || !evals || !cert_self || !cert_env ||
        !cert_reach || !stop_self || !stop_env || !stop_reach || !stop_pair || (n_planes > 0 && !planes) ||
        (n_obstacles > 0 && !obstacles) || (!trace_t != !trace_val))
        return fail(EHR_ERR_INVALID, "ehr_segment_clearance: NULL tensor");
    SegArgs A = {};
    for (int l = 0; l <= L; l++) {
        A.offs.v[l] = sphere_offsets[l];
        if ((l == 0 && A.offs.v[0] != 0) || (l > 0 && A.offs.v[l] < A.offs.v[l - 1]))
            return fail(EHR_ERR_INVALID, "ehr_segment_clearance: sphere_offsets must ascend from 0 (entry %d is %d)", l, A.offs.v[l]);
    }
    const int S = A.offs.v[L];
    if (S > EHR_SEG_MAX_SPHERES)
        return fail(EHR_ERR_INVALID, "ehr_segment_clearance: bad sizes (S %d <= %d spheres)", S, EHR_SEG_MAX_SPHERES);
    if (S > 0 && !spheres) return fail(EHR_ERR_INVALID, "ehr_segment_clearance: NULL tensor");
    A.parent = parent, A.kind = kind, A.qidx = qidx, A.use = use, A.origin = origin, A.axis = axis;
    A.N = N, A.J = J, A.L = L, A.q0 = q0, A.q1 = q1, A.offset = offset, A.spheres = spheres, A.link_bounds = link_bounds;
    A.pair_enable = pair_enable, A.planes = planes, A.Np = n_planes, A.obstacles = obstacles, A.No = n_obstacles;
    A.env_links = env_links, A.reach = reach, A.cutoff = cutoff, A.upstream = upstream, A.joint_below = joint_below;
    A.reach_radius = reach_radius, A.margin = margin, A.min_depth = min_depth, A.max_depth = max_depth, A.max_evals = max_evals;
    A.S = S, A.Sp = (S + 1) & ~1;
    A.status = status, A.evals = evals, A.stop_pair = stop_pair, A.t_free = t_free, A.cert_self = cert_self, A.cert_env = cert_env;
    A.cert_reach = cert_reach, A.stop_self = stop_self, A.stop_env = stop_env, A.stop_reach = stop_reach;
    A.trace_t = trace_t, A.trace_val = trace_val;
    const size_t lds = seg_lds_bytes(A.Sp);
    if (lds > 64 * 1024 - SEG_STATIC_BYTES) {
        // more than the default limit of a launch's LDS: ask for it (a runtime that needs no asking may refuse the question; the
        // launch below is what decides, and it fails cleanly where the device has less LDS than this)
        if (hipFuncSetAttribute((const void*)segment_clearance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
            (void)hipGetLastError();
    }
    segment_clearance_kernel<<<(unsigned)n, SEG_THREADS, lds, (hipStream_t)stream>>>(A);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
