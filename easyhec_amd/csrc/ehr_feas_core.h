// ehr_feas_core.h -- what the two feasibility kernels share (ehr_feasible.hip: sphere proxies, ehr_mesh_clearance.hip: the
// meshes behind them): the offsets' argument block, the culling slack and the contract's expressions of include/ehr.h, each
// written once.  The library is built with -ffp-contract=off: a product is rounded before it is added.
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

}  // namespace ehr
