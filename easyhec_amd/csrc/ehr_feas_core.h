// ehr_feas_core.h -- what the feasibility kernels share (ehr_feasible.hip: sphere proxies, ehr_mesh_clearance.hip: the
// meshes behind them, ehr_segment_clearance.hip: the proxies along a whole joint segment): the offsets' argument block, the
// culling slack, the contract's expressions of include/ehr.h and the proxies' move to the base frame, each written once.  The library is built with -ffp-contract=off: a product is rounded before it is added.
#pragma once
#include <math.h>

#include "ehr_host.h"

#define FEAS_CULL_SLACK 1e-6  // a bound must exceed cutoff by this much before it culls: its own rounding never decides

namespace ehr {

struct FeasOffsets {  // sphere_offsets, by value in the kernel's arguments
    int v[EHR_FEAS_MAX_LINKS + 1];
};

__device__ __forceinline__ bool feas_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // (NaN: false)
__device__ __forceinline__ double feas_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---- the contract's expressions ---------------------------------------------------------------------------------------------
// row k of a pose applied to a link-frame point: ((R_k0 x + R_k1 y) + R_k2 z) + t_k
__device__ __forceinline__ double feas_world(const float* __restrict__ row, double x, double y, double z) {
    return (((double)row[0] * x + (double)row[1] * y) + (double)row[2] * z) + (double)row[3];
}
__device__ __forceinline__ double feas_norm2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }
// sphere against sphere or obstacle
__device__ __forceinline__ double feas_gap(double dx, double dy, double dz, double ra, double rb) {
    return sqrt(feas_norm2(dx, dy, dz)) - (ra + rb);
}
__device__ __forceinline__ double feas_plane(double nx, double ny, double nz, double d, double cx, double cy, double cz, double r) {
    return (((nx * cx + ny * cy) + nz * cz) + d) - r;
}
__device__ __forceinline__ double feas_reach(double R, double dx, double dy, double dz, double r) {
    return R - (sqrt(feas_norm2(dx, dy, dz)) + r);
}

// ---- the proxies in the base frame ------------------------------------------------------------------------------------------
// Every sphere of the S (link l's are off[l] .. off[l + 1], off in LDS) and every link's bound to the base frame at the poses
// P [L,16]: X | Y | Z | Rr [S] and BW [L][4], the caller's LDS.  All THREADS threads of the workgroup call; the caller's barrier
// follows.
template <int THREADS>
__device__ __forceinline__ void feas_to_base(const float* __restrict__ P, const double* __restrict__ spheres,
                                             const int* __restrict__ off, const double* __restrict__ link_bounds, int L, int S,
                                             double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
                                             double* __restrict__ Rr, double* __restrict__ BW) {
    const int tid = threadIdx.x;
    for (int s = tid; s < S; s += THREADS) {
        int lo = 0, hi = L;  // off[lo] <= s < off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= s) lo = mid; else hi = mid;
        }
        const float* T = P + lo * 16;
        const double x = spheres[4 * (size_t)s], y = spheres[4 * (size_t)s + 1], z = spheres[4 * (size_t)s + 2];
        X[s] = feas_world(T, x, y, z);
        Y[s] = feas_world(T + 4, x, y, z);
        Z[s] = feas_world(T + 8, x, y, z);
        Rr[s] = spheres[4 * (size_t)s + 3];
    }
    if (tid < L) {
        const float* T = P + tid * 16;
        const double x = link_bounds[4 * tid], y = link_bounds[4 * tid + 1], z = link_bounds[4 * tid + 2];
        BW[4 * tid] = feas_world(T, x, y, z);
        BW[4 * tid + 1] = feas_world(T + 4, x, y, z);
        BW[4 * tid + 2] = feas_world(T + 8, x, y, z);
        BW[4 * tid + 3] = link_bounds[4 * tid + 3];
    }
}
// the gap of two links' bounds in BW
__device__ __forceinline__ double feas_bound_gap(const double* __restrict__ BW, int i, int j) {
    return feas_gap(BW[4 * i] - BW[4 * j], BW[4 * i + 1] - BW[4 * j + 1], BW[4 * i + 2] - BW[4 * j + 2], BW[4 * i + 3],
                    BW[4 * j + 3]);
}

}  // namespace ehr
