// ehr_feasible.hip -- feasibility of candidate joint configurations on sphere proxies (easyhec_amd/feasibility.py, DESIGN.md
// section 6s): ehr_config_clearance of include/ehr.h.
//
//   config_clearance_kernel : link_poses [n,L,16] (ehr_joint_forward's) + link-frame proxy spheres -> per configuration the
//                             clearance against itself (sphere pairs of the enabled link pairs), against planes and obstacle
//                             spheres, and inside the ball of allowed reach.  One workgroup of 256 threads per configuration: the
//                             S spheres are moved to the base frame ONCE, into LDS (structure of arrays: a wave reads consecutive
//                             doubles of the one link and a broadcast of the other), then the pairs run on them.
//
// Float64 throughout, every expression of the contract written once below (feas_* ; the library is built with
// -ffp-contract=off, so a product is rounded before it is added, as numpy evaluates tests/feasibility_reference.py).  A minimum
// is exact in any order: the result does not depend on how the pairs are dealt to the threads.  No atomics, no allocation, no
// synchronisation with the host.
#include "ehr_feas_core.h"  // FeasOffsets, FEAS_CULL_SLACK, the expressions (feas_*) and feas_to_base, shared with the siblings

#define FEAS_THREADS 256

namespace ehr {

// LDS of one workgroup, all of it in the dynamic region and every part a multiple of 16 bytes: x | y | z | r of the Sp = S
// rounded up to even spheres, then the fixed tail below
#define FEAS_TAIL_BOUNDS (EHR_FEAS_MAX_LINKS * 4)  // doubles: the links' bounding spheres in the base frame
#define FEAS_TAIL_RED (3 * FEAS_THREADS)           // doubles: the reduction's three minima
#define FEAS_TAIL_INTS (FEAS_THREADS + 36)         // ints: the reduction's pair codes | the offsets (33, padded)
#define FEAS_TAIL_BYTES ((FEAS_TAIL_BOUNDS + FEAS_TAIL_RED) * 8 + FEAS_TAIL_INTS * 4 + EHR_FEAS_MAX_OBSTACLES)
static inline size_t feas_lds_bytes(int Sp) { return (size_t)Sp * 32 + FEAS_TAIL_BYTES; }

__global__ void __launch_bounds__(FEAS_THREADS) config_clearance_kernel(
    const float* __restrict__ link_poses, const double* __restrict__ spheres, const FeasOffsets offs,
    const double* __restrict__ link_bounds, const unsigned* __restrict__ pair_enable, const double* __restrict__ planes, int Np,
    const double* __restrict__ obstacles, int No, unsigned env_links, const double* __restrict__ reach, double cutoff, int L,
    int S, int Sp, double* __restrict__ self_clear, int* __restrict__ self_pair, double* __restrict__ env_clear,
    double* __restrict__ reach_clear) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* X = (double*)smem;
    double* Y = X + Sp;
    double* Z = Y + Sp;
    double* Rr = Z + Sp;
    double* BW = Rr + Sp;                // [L][4] bounding spheres, base frame
    double* red = BW + FEAS_TAIL_BOUNDS;  // [3][256]
    int* redp = (int*)(red + FEAS_TAIL_RED);
    int* off = redp + FEAS_THREADS;      // [L + 1]
    unsigned char* skip = (unsigned char*)(off + 36);  // [No]: the current link's bound clears this obstacle
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t b = blockIdx.x;
    const float* P = link_poses + b * (size_t)L * 16;
    const double cull = cutoff + FEAS_CULL_SLACK;

    // a configuration that cannot be judged does not pass: NaN, and nothing else of it is read
    int bad = 0;
    for (int e = tid; e < L * 16; e += FEAS_THREADS) bad |= !feas_finite(P[e]);
    if (tid <= L) off[tid] = offs.v[tid];
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) {
            self_clear[b] = feas_nan();
            env_clear[b] = feas_nan();
            reach_clear[b] = feas_nan();
            self_pair[b] = -1;
        }
        return;
    }

    // every sphere to the base frame, once
    feas_to_base<FEAS_THREADS>(P, spheres, off, link_bounds, L, S, X, Y, Z, Rr, BW);
    __syncthreads();

    // reach: every sphere inside the allowed ball
    double rc = cutoff;
    if (reach) {
        const double ox = reach[0], oy = reach[1], oz = reach[2], R = reach[3];
        for (int s = tid; s < S; s += FEAS_THREADS) {
            const double d = feas_reach(R, X[s] - ox, Y[s] - oy, Z[s] - oz, Rr[s]);
            if (d < rc) rc = d;
        }
    }

    // the environment: a thread per sphere of the link; planes and obstacles the link's bound clears are not visited.  (Every
    // condition around a barrier is uniform over the workgroup.)
    double ec = cutoff;
    if (Np > 0 || No > 0) {
        for (int l = 0; l < L; l++) {
            const int s0 = off[l], s1 = off[l + 1];
            if (!((env_links >> l) & 1u) || s0 == s1) continue;
            const double bx = BW[4 * l], by = BW[4 * l + 1], bz = BW[4 * l + 2], bR = BW[4 * l + 3];
            for (int p = 0; p < Np; p++) {
                const double nx = planes[4 * p], ny = planes[4 * p + 1], nz = planes[4 * p + 2], pd = planes[4 * p + 3];
                if (feas_plane(nx, ny, nz, pd, bx, by, bz, bR) > cull) continue;
                for (int s = s0 + tid; s < s1; s += FEAS_THREADS) {
                    const double d = feas_plane(nx, ny, nz, pd, X[s], Y[s], Z[s], Rr[s]);
                    if (d < ec) ec = d;
                }
            }
            if (No > 0) {
                __syncthreads();  // (the previous link's flags have been read)
                for (int o = tid; o < No; o += FEAS_THREADS)
                    skip[o] = feas_gap(bx - obstacles[4 * o], by - obstacles[4 * o + 1], bz - obstacles[4 * o + 2], bR,
                                       obstacles[4 * o + 3]) > cull;
                __syncthreads();
                for (int s = s0 + tid; s < s1; s += FEAS_THREADS) {
                    const double cx = X[s], cy = Y[s], cz = Z[s], r = Rr[s];
                    for (int o = 0; o < No; o++) {
                        if (skip[o]) continue;
                        const double d = feas_gap(cx - obstacles[4 * o], cy - obstacles[4 * o + 1], cz - obstacles[4 * o + 2], r,
                                                  obstacles[4 * o + 3]);
                        if (d < ec) ec = d;
                    }
                }
            }
        }
    }

    // the arm against itself: link pairs in the order of their code 32 i + j, so that a thread's first pair at its minimum is
    // the lowest-numbered one.  The link with fewer spheres is dealt to the waves, the other's spheres to the lanes.
    double sc = cutoff;
    int sp = -1;
    const unsigned inL = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
    for (int i = 0; i + 1 < L; i++) {
        const unsigned m = pair_enable[i] & ~((2u << i) - 1u) & inL;  // j > i only
        const int oi = off[i], ni = off[i + 1] - oi;
        if (!m || ni <= 0) continue;
        for (int j = i + 1; j < L; j++) {
            const int oj = off[j], nj = off[j + 1] - oj;
            if (!((m >> j) & 1u) || nj <= 0) continue;
            if (feas_bound_gap(BW, i, j) > cull) continue;
            const int code = 32 * i + j;
            const bool swap = nj < ni;
            const int a0 = swap ? oj : oi, na = swap ? nj : ni, b0 = swap ? oi : oj, nb = swap ? ni : nj;
            for (int a = wave; a < na; a += FEAS_THREADS / 64) {
                const double ax = X[a0 + a], ay = Y[a0 + a], az = Z[a0 + a], ar = Rr[a0 + a];
                for (int k = b0 + lane; k < b0 + nb; k += 64) {
                    const double dx = ax - X[k], dy = ay - Y[k], dz = az - Z[k], rs = ar + Rr[k];
                    // no square root for a pair that cannot come below the thread's minimum: with t = sc + rs, a negative t
                    // means sc < -rs <= any gap, and d2 > t^2 (1 + 1e-12) puts sqrt(d2) - rs above sc by far more than the
                    // roundings of t, t^2, the root and the difference (a few 1e-16 each).  What is skipped would not have
                    // replaced sc, so the result has the bits of the plain evaluation.
                    const double t = sc + rs, d2 = feas_norm2(dx, dy, dz);
                    if (t < 0.0 || d2 > (t * t) * 1.000000000001) continue;
                    const double d = sqrt(d2) - rs;  // == feas_gap(dx, dy, dz, ar, Rr[k])
                    if (d < sc) {
                        sc = d;
                        sp = code;
                    }
                }
            }
        }
    }

    // minima over the workgroup; among equal self clearances the lowest pair code
    red[tid] = sc;
    red[FEAS_THREADS + tid] = ec;
    red[2 * FEAS_THREADS + tid] = rc;
    redp[tid] = sp;
    __syncthreads();
    for (int w = FEAS_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const double o = red[tid + w];
            const int op = redp[tid + w];
            if (o < red[tid] || (o == red[tid] && op < redp[tid] && op >= 0)) {
                red[tid] = o;
                redp[tid] = op;
            }
            if (red[FEAS_THREADS + tid + w] < red[FEAS_THREADS + tid]) red[FEAS_THREADS + tid] = red[FEAS_THREADS + tid + w];
            if (red[2 * FEAS_THREADS + tid + w] < red[2 * FEAS_THREADS + tid])
                red[2 * FEAS_THREADS + tid] = red[2 * FEAS_THREADS + tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        self_clear[b] = red[0];
        self_pair[b] = redp[0];
        env_clear[b] = red[FEAS_THREADS];
        reach_clear[b] = red[2 * FEAS_THREADS];
    }
}

}  // namespace ehr

using namespace ehr;

extern "C" {

int ehr_config_clearance(const float* link_poses, const double* spheres, const int32_t* sphere_offsets, const double* link_bounds,
                         const uint32_t* pair_enable, const double* planes, int n_planes, const double* obstacles,
                         int n_obstacles, uint32_t env_links, const double* reach, double cutoff, int n, int L,
                         double* self_clear, int32_t* self_pair, double* env_clear, double* reach_clear, void* stream) {
    if (L < 1 || L > EHR_FEAS_MAX_LINKS || n < 1)
        return fail(EHR_ERR_INVALID, "ehr_config_clearance: bad sizes (L %d: 1 <= L <= %d links, n %d >= 1)", L,
                    EHR_FEAS_MAX_LINKS, n);
    if (n_planes < 0 || n_planes > EHR_FEAS_MAX_PLANES || n_obstacles < 0 || n_obstacles > EHR_FEAS_MAX_OBSTACLES)
        return fail(EHR_ERR_INVALID, "ehr_config_clearance: bad sizes (%d planes <= %d, %d obstacles <= %d)", n_planes,
                    EHR_FEAS_MAX_PLANES, n_obstacles, EHR_FEAS_MAX_OBSTACLES);
    if (!(cutoff > 0.0) || !(cutoff <= 1.7976931348623157e308))
        return fail(EHR_ERR_INVALID, "ehr_config_clearance: cutoff %g must be finite and > 0", cutoff);
    if (!link_poses || !sphere_offsets || !link_bounds || !pair_enable || !self_clear || !self_pair || !env_clear ||
        !reach_clear || (n_planes > 0 && !planes) || (n_obstacles > 0 && !obstacles))
        return fail(EHR_ERR_INVALID, "ehr_config_clearance: NULL tensor");
    FeasOffsets offs = {};
    for (int l = 0; l <= L; l++) {
        offs.v[l] = sphere_offsets[l];
        if ((l == 0 && offs.v[0] != 0) || (l > 0 && offs.v[l] < offs.v[l - 1]))
            return fail(EHR_ERR_INVALID, "ehr_config_clearance: sphere_offsets must ascend from 0 (entry %d is %d)", l, offs.v[l]);
    }
    const int S = offs.v[L];
    if (S > EHR_FEAS_MAX_SPHERES)
        return fail(EHR_ERR_INVALID, "ehr_config_clearance: bad sizes (S %d <= %d spheres)", S, EHR_FEAS_MAX_SPHERES);
    if (S > 0 && !spheres) return fail(EHR_ERR_INVALID, "ehr_config_clearance: NULL tensor");
    const int Sp = (S + 1) & ~1;
    const size_t lds = feas_lds_bytes(Sp);
    if (lds > 64 * 1024) {
        // more than the default limit of a launch's dynamic LDS: ask for it (a runtime that needs no asking may refuse the
        // question; the launch below is what decides, and it fails cleanly where the device has less LDS than this)
        if (hipFuncSetAttribute((const void*)config_clearance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
            (void)hipGetLastError();
    }
    config_clearance_kernel<<<(unsigned)n, FEAS_THREADS, lds, (hipStream_t)stream>>>(
        link_poses, spheres, offs, link_bounds, pair_enable, planes, n_planes, obstacles, n_obstacles, env_links, reach, cutoff, L,
        S, Sp, self_clear, self_pair, env_clear, reach_clear);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
