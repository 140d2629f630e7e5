// ehr_distance.hip -- exact capped squared Euclidean distance transform of the observed masks (ehr_mask_distance), the
// per-call preparation of the pose search's soft-IoU score.
//
//   d2[s][y][x] = min(cap^2, min over foreground (x', y') of (x - x')^2 + (y - y')^2)
//
// in the separable form: pass one gives every pixel the distance g to the nearest foreground pixel of its own COLUMN
// (capped at cap: a column distance >= cap cannot give less than cap^2), pass two takes per row the minimum of
// (x - x')^2 + g[x']^2 over the columns x' within the cap.  Everything is an integer (g <= 4096 as u16, sums < 2^26),
// so the result is exact for every cap in [1, 4096] and does not depend on the launch geometry.
#include <algorithm>

#include "ehr_host.h"

namespace ehr {

constexpr int DIST_MAX_CAP = 4096;
constexpr int DIST_SEG = 256;       // pixels of a row a workgroup of pass two owns (one per thread)
constexpr int DIST_COL_BATCH = 8;   // rows pass one has in flight per column

// Pass one: a thread owns a column of a view (x fastest: a wave reads 256 contiguous bytes of an image row) and walks it
// down, then up, DIST_COL_BATCH independent loads at a time.  Foreground rule of ehr_mask_overlap: ref > 0.5f, NaN is background.
__global__ void __launch_bounds__(256)
dist_columns_kernel(const float* __restrict__ ref, int H, int W, int cap, unsigned short* __restrict__ g) {
    const int x = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (x >= W) return;
    const float* const img = ref + (size_t)s * H * W + x;
    unsigned short* const col = g + (size_t)s * H * W + x;
    int d = cap;  // rows since the last foreground pixel above, capped
    for (int y0 = 0; y0 < H; y0 += DIST_COL_BATCH) {
        float v[DIST_COL_BATCH];
#pragma unroll
        for (int j = 0; j < DIST_COL_BATCH; j++) v[j] = (y0 + j < H) ? img[(size_t)(y0 + j) * W] : 0.f;
#pragma unroll
        for (int j = 0; j < DIST_COL_BATCH; j++) {
            if (y0 + j >= H) break;
            d = (v[j] > 0.5f) ? 0 : min(d + 1, cap);
            col[(size_t)(y0 + j) * W] = (unsigned short)d;
        }
    }
    d = cap;      // ... below
    for (int y1 = H - 1; y1 >= 0; y1 -= DIST_COL_BATCH) {
        int v[DIST_COL_BATCH];
#pragma unroll
        for (int j = 0; j < DIST_COL_BATCH; j++) v[j] = (y1 - j >= 0) ? (int)col[(size_t)(y1 - j) * W] : 0;
#pragma unroll
        for (int j = 0; j < DIST_COL_BATCH; j++) {
            if (y1 - j < 0) break;
            d = (v[j] == 0) ? 0 : min(d + 1, cap);
            if (d < v[j]) col[(size_t)(y1 - j) * W] = (unsigned short)d;
        }
    }
}

// Pass two: a workgroup owns DIST_SEG pixels of one row and stages the columns within the cap of them in LDS (at most
// DIST_SEG + 2 (cap - 1) values of 16 bits: 16.5 KB at cap 4096).  A thread walks outwards from its own pixel, both sides
// per step, and stops as soon as the offset alone reaches the best it holds: dx^2 >= best, so it reads about as many
// columns as its distance is long (neighbouring lanes stop within a step or two of each other), never more than cap - 1
// a side.  A window that holds no column distance below the cap is cap^2 throughout, without a walk.
__global__ void __launch_bounds__(DIST_SEG)
dist_rows_kernel(const unsigned short* __restrict__ g, int W, int nseg, int cap, int32_t* __restrict__ d2) {
    __shared__ unsigned short win[DIST_SEG + 2 * (DIST_MAX_CAP - 1)];
    const size_t row = blockIdx.x / nseg;      // view * H + y
    const int x0 = (int)(blockIdx.x - row * nseg) * DIST_SEG;
    const int lo = max(x0 - (cap - 1), 0), hi = min(x0 + DIST_SEG - 1 + (cap - 1), W - 1);  // staged columns [lo, hi]
    const unsigned short* const gr = g + row * W;
    int any = 0;
    for (int i = lo + (int)threadIdx.x; i <= hi; i += DIST_SEG) {
        const unsigned short v = gr[i];
        win[i - lo] = v;
        any |= v < cap;
    }
    any = __syncthreads_or(any);
    const int x = x0 + (int)threadIdx.x;
    if (x >= W) return;
    int best = cap * cap;
    if (any) {
        const int gx = win[x - lo];
        best = min(best, gx * gx);
        for (int dx = 1; dx * dx < best; dx++) {
            const int l = x - dx, r = x + dx;
            if (l >= lo) {
                const int gl = win[l - lo];
                best = min(best, dx * dx + gl * gl);
            }
            if (r <= hi) {
                const int gr2 = win[r - lo];
                best = min(best, dx * dx + gr2 * gr2);
            }
        }
    }
    d2[row * W + x] = best;
}

}  // namespace ehr

using namespace ehr;

extern "C" int ehr_mask_distance(ehr_ctx* ctx, const float* ref, int S, int H, int W, int cap_px, int32_t* d2, void* stream_) {
    if (!ctx) return fail(EHR_ERR_INVALID, "ehr_mask_distance: ctx is NULL");
    if (!ref || !d2) return fail(EHR_ERR_INVALID, "ehr_mask_distance: NULL tensor");
    if (S <= 0 || H <= 0 || W <= 0) return fail(EHR_ERR_INVALID, "ehr_mask_distance: bad sizes");
    if (H > 32768 || W > 32768) return fail(EHR_ERR_INVALID, "ehr_mask_distance: resolution above 32768 is unsupported");
    const int nseg = (W + DIST_SEG - 1) / DIST_SEG;
    if ((long long)S * H * nseg > 0x7fffffffll || S > 65535) return fail(EHR_ERR_INVALID, "ehr_mask_distance: too many rows in one call: split the views");
    if (cap_px < 1 || cap_px > DIST_MAX_CAP) return fail(EHR_ERR_INVALID, "ehr_mask_distance: cap_px must be in [1, %d], got %d", DIST_MAX_CAP, cap_px);
    hipStream_t stream = (hipStream_t)stream_;
    {   // as for the drop-in ops: a call recorded into a stream capture pins its scratch where it is
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(stream, &cs);
        if (cs != hipStreamCaptureStatusNone) {
            if (ctx->sc_dist.cap < (size_t)S * H * W * sizeof(unsigned short))
                return fail(EHR_ERR_INVALID, "ehr_mask_distance: the scratch is not reserved yet: call once outside the capture");
            ctx->sc_dist.pinned = true;
        }
    }
    int rc;
    if ((rc = ctx->sc_dist.reserve((size_t)S * H * W * sizeof(unsigned short)))) return rc;
    unsigned short* g = (unsigned short*)ctx->sc_dist.ptr;
    dist_columns_kernel<<<dim3((W + 255) / 256, S), 256, 0, stream>>>(ref, H, W, cap_px, g);
    EHR_LAUNCH_CHECK();
    dist_rows_kernel<<<(unsigned)((size_t)S * H * nseg), DIST_SEG, 0, stream>>>(g, W, nseg, cap_px, d2);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}
