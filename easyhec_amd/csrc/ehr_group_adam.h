// ehr_group_adam.h -- Adam on a small parameter group that follows the chain (the joint offsets of ehr_joint.hip, the
// intrinsics' theta of ehr_intrinsics.hip), one element per thread.
#pragma once
#include <hip/hip_runtime.h>

namespace ehr {

// Element tid of the group: pose_adam_apply's expressions on g = (float)sum() / nfr.  An element that is not free (!mine)
// keeps everything and reports 0; a reported step (!ok: the caller's verdict) touches nothing and reports NaN for the free
// elements.  sum() returns the element's float64 sum and is called where the step counts only.  The caller advances the
// group's counter (t is the step this would be) behind a barrier.
template <class Sum>
__device__ __forceinline__ void group_adam(int tid, bool mine, bool ok, Sum sum, float nfr, int t, float* __restrict__ param,
                                           float* __restrict__ m, float* __restrict__ v, float lr, float b1, float b2,
                                           float eps, float wd, float* __restrict__ grad_out) {
    if (!mine) {
        if (grad_out) grad_out[tid] = 0.f;
    } else if (!ok) {
        if (grad_out) grad_out[tid] = __int_as_float(0x7fc00000);
    } else {
        const float gsum = (float)sum();
        float g = gsum / nfr;
        if (grad_out) grad_out[tid] = g;
        const float p = param[tid];
        g = g + wd * p;
        const float mi = b1 * m[tid] + (1.f - b1) * g;
        const float vi = b2 * v[tid] + (1.f - b2) * g * g;
        m[tid] = mi;
        v[tid] = vi;
        const float bc1 = 1.f - powf(b1, (float)t);
        const float bc2 = 1.f - powf(b2, (float)t);
        const float step_size = lr / bc1;
        const float rsq_bc2 = sqrtf(bc2);
        const float denom = sqrtf(vi) / rsq_bc2 + eps;
        param[tid] = p - step_size * (mi / denom);
    }
}

}  // namespace ehr
