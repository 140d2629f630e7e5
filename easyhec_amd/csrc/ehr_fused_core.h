// ehr_fused_core.h -- pieces of the fused op's launch chain (ehr_vbuf.hip) that are not rasterization: fixed-point
// accumulators, the head / tail descriptors of a solver step and the finish stage (accumulators -> loss / grad_mvp ->
// pose backward -> Adam), which runs inside the composite kernel's finisher workgroup.
#pragma once
#include "ehr_host.h"
#include "ehr_pose_core.h"
#include "ehr_raster_core.h"

namespace ehr {

// Per-view sums (frame loss, 12 gradient numbers per link) are accumulated in 64-bit FIXED POINT with integer atomics:
// integer addition is associative, so the result does not depend on which workgroup adds first -- bit-reproducible like
// a fixed-order reduction, but without a reduction pass over all tiles.  Scale 2^32: addends are rounded to 2.3e-10
// (absolute), sums up to +-2.1e9 fit.  The guard below is PER ADDEND: an addend of 1e9 or more (or a NaN) raises the
// overflow flag (loss = NaN).  The total is not guarded: many addends below 1e9 can take it past 2^31 and wrap.  The
// contract is that a view's SSE (and each gradient sum) stays below 2^31, which any mask in a bounded range meets by orders
// of magnitude.  The flag is raised with an atomic: the finish stage reads it inside the same launch.
#define EHR_FIX_SCALE 4294967296.0
__device__ __forceinline__ long long fix_of(float v) { return __double2ll_rn((double)v * EHR_FIX_SCALE); }
__device__ __forceinline__ void fix_add(long long* acc, float v, int* meta) {
    if (!(fabsf(v) < 1.0e9f)) {  // also catches NaN
        atomicOr(&meta[EHR_META_OVERFLOW], 1);
        return;
    }
    if (v != 0.f) atomicAdd((unsigned long long*)acc, (unsigned long long)fix_of(v));
}
// acc += fix(v) - cached: the caller has bound a constant whose fixed-point value `cached` is already part of the
// view's total (the sum of ref^2 over a tile no link touches).  Integer arithmetic: the same bits as adding fix(v) to
// an accumulator that never held `cached`.
__device__ __forceinline__ void fix_add_delta(long long* acc, float v, long long cached, int* meta) {
    if (!(fabsf(v) < 1.0e9f)) {
        atomicOr(&meta[EHR_META_OVERFLOW], 1);
        return;
    }
    const long long d = ((v != 0.f) ? fix_of(v) : 0ll) - cached;
    if (d != 0) atomicAdd((unsigned long long*)acc, (unsigned long long)d);
}
__device__ __forceinline__ float fix_get(long long q) { return (float)((double)q * (1.0 / EHR_FIX_SCALE)); }
// accumulators are read inside the launch that adds to them (finish stage, once every arrival is counted): agent-scope
// loads, which are served by the memory side the atomics were performed on, never by this CU's L1
__device__ __forceinline__ long long acc_load(const long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Layout of the accumulators (ehr_ctx::vb_acc): per view 12 numbers per link (vb_acc_grad), then `nls` partial sums of the
// frame loss (from vb_acc_loss), VB_LOSS_STRIDE i64 apart (several slots, one 128-byte line each, so that thousands of
// tiles do not serialise on one address; integer sums, so the split does not change the result); behind the B views of a
// call, the meta block.  (Copies of the gradient block on lines of their own were measured and left out:
// profiles/atomic_spread.md.)
__host__ __device__ constexpr int vb_acc_grad(int l) { return 12 * l; }   // first gradient word of link l
__host__ __device__ constexpr int vb_acc_loss(int L) { return 12 * L; }   // first loss slot
__host__ __device__ constexpr int vb_acc_stride(int L, int nls = VB_LOSS_SLOTS) { return vb_acc_loss(L) + nls * VB_LOSS_STRIDE; }
__host__ __device__ __forceinline__ int* vb_acc_meta(long long* acc, int B, int L) { return (int*)(acc + (size_t)B * vb_acc_stride(L)); }

// Last stage, ONE workgroup: fixed-point accumulators -> loss[B] and grad_mvp[B,L,16]; with TAIL also the rest of a
// solver step (d sum(loss) / d dof = the 8 floats a data-parallel job all-reduces, then Adam unless deferred).
struct StepTail {  // what the solver-step form needs (all device pointers)
    const float* K;
    const float* link_poses;
    const float* tc_jac;
    float* red;
    float* dof;
    float* m;
    float* v;
    int* step;
    float* loss_out;
    float* grad_out;
    float n, f, lr, b1, b2, eps, wd;
    int defer_adam;
};

// The finish stage comes in two halves, both called by all 256 threads of ONE workgroup (the composite stage's finisher).
// finish_prefetch requests and prepares everything that does not depend on the accumulators or the overflow word: Adam's
// state and bias corrections, the Jacobian rows and the first 64 link poses (to LDS), PF and the first views' cached
// constants.  The finisher runs it while the other workgroups are still compositing.  finish_reduce runs once every other
// workgroup's atomics have been performed: it reads the accumulators, contracts, reduces and applies Adam.  Together
// they evaluate the expressions of the former single body in the same order: the split moves loads, not roundings.
struct FinishPre {
    AdamState st;
    PoseBwdPre pb;
    long long vt;  // nls == 32: vtot of the first view this thread publishes (view threadIdx.x / 32)
};

// vtot (optional): per view a constant that belongs to the frame loss (the bound reference mask's cached part).
template <bool TAIL>
__device__ __forceinline__ void finish_prefetch(FinishPre& pre, const BinGeom& g, int B, const long long* __restrict__ vtot,
                                                const StepTail& tail, int nls, float (*Js)[16] /* LDS [6][16] */,
                                                float* lp_lds /* LDS [1024] */) {
    const int tid = threadIdx.x;
    if (TAIL && !tail.defer_adam) pre.st = pose_adam_fetch(tail.dof, tail.m, tail.v, tail.step);
    pre.vt = (nls == 32 && vtot && (tid & 31) == 0 && (tid >> 5) < B) ? vtot[tid >> 5] : 0ll;
    if (TAIL) {
        pose_backward_prefetch(pre.pb, tail.K, tail.link_poses, tail.tc_jac, B, g.L, g.H, g.W, tail.n, tail.f, Js, lp_lds);
        // (Adam's bias corrections need the step count only)
        if (!tail.defer_adam) pose_adam_bias(pre.st, tail.lr, tail.b1, tail.b2);
    }
}

// facc: see vb_acc_stride (lstride = VB_LOSS_STRIDE).
template <bool TAIL>
__device__ __forceinline__ void finish_reduce(const FinishPre& pre, const BinGeom& g, int B, const long long* __restrict__ facc,
                                              const long long* __restrict__ vtot, float* __restrict__ loss,
                                              float* __restrict__ grad_mvp, int* __restrict__ meta, const StepTail& tail,
                                              int nls, int lstride, double (*S)[17] /* LDS [4][17] */,
                                              float* red_lds /* LDS [8] */, float (*Js)[16] /* LDS [6][16] */,
                                              const float* lp_lds /* LDS [1024] */) {
    const int tid = threadIdx.x, L = g.L;
    const int acc_stride = vb_acc_stride(L, nls);
    auto view_loss_slow = [&](int b) {
        long long s = vtot ? vtot[b] : 0ll;
        for (int k = 0; k < nls; k++) s += acc_load(&facc[(size_t)b * acc_stride + vb_acc_loss(L) + k * lstride]);
        return fix_get(s);
    };
    // Frame losses.  nls == 32: one slot per lane, half a wave per view -- a single round trip instead of 32 dependent
    // adds -- and the lane that ends up with a view's sum stores loss[b] and keeps it as ITS share of sum_b loss_b: no
    // hand-over through LDS, no barrier, so the reads below (gradient accumulators) travel with these instead of after
    // them.
    const bool bad = __hip_atomic_load(&meta[EHR_META_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    const float nanv = __int_as_float(0x7fc00000);  // overflow => NaN, never a silently wrong loss
    double la_mine = 0.0;
    if (nls == 32) {
        const int k = tid & 31;
        for (int base = 0; base < B; base += 32) {  // four groups of 8 views per round trip
            long long s4[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int b = base + 8 * j + (tid >> 5);
                s4[j] = (b < B) ? acc_load(&facc[(size_t)b * acc_stride + vb_acc_loss(L) + k * lstride]) : 0;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int b = base + 8 * j + (tid >> 5);
                if (base + 8 * j >= B) break;  // (workgroup-uniform)
                long long s = s4[j];
                s += wave_xor<16>(s);  // (the 32 slots of a view: half a wave)
                s += wave_xor<8>(s);
                s += wave_xor<4>(s);
                s += wave_xor<2>(s);
                s += wave_xor<1>(s);
                if (k == 0 && b < B) {
                    const float lv = bad ? nanv : fix_get(s + (vtot ? (base + j == 0 ? pre.vt : vtot[b]) : 0ll));
                    loss[b] = lv;
                    la_mine += (double)lv;
                }
            }
        }
    } else {
        for (int b = tid; b < B; b += 256) {
            const float lv = bad ? nanv : view_loss_slow(b);
            loss[b] = lv;
            la_mine += (double)lv;
        }
    }
    // Called by the four lanes of a quad (tid / 4 names the pair) with the same (view, link).  Lane c of the quad reads
    // COLUMN c of the pair's three rows -- 3 loads instead of 12 a lane, one round trip --, converts them, and the quad
    // hands the floats round: every lane ends up with all twelve, the values it would have loaded and converted itself.
    // PRECONDITION for every caller: the four lanes of a quad pass the same `bl` and all four are active (quad_lane reads
    // its neighbours); both callers below index pairs by tid / 4 in a workgroup of 256.
    auto grad16 = [&](int bl, float* G) {
        // rows x, y, w of the 4x4 gradient; the z row never receives gradient on this path
        const int b = bl / L, l = bl - b * L;
        const long long* a = facc + (size_t)b * acc_stride + vb_acc_grad(l) + (tid & 3);
        long long q[3];
#pragma unroll
        for (int r = 0; r < 3; r++) q[r] = acc_load(a + 4 * r);
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float v = bad ? nanv : fix_get(q[r]);
            float* const row = G + 4 * (r == 2 ? 3 : r);
            row[0] = quad_lane<0>(v);
            row[1] = quad_lane<1>(v);
            row[2] = quad_lane<2>(v);
            row[3] = quad_lane<3>(v);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) G[8 + c] = bad ? nanv : 0.f;
    };
    if (!TAIL) {
        if (grad_mvp)
            for (int i = tid >> 2; i < B * L; i += 64) {  // (a quad per pair, as pose_backward_reduce_t calls it below)
                float G[16];
                grad16(i, G);
                if ((tid & 3) == 0)
#pragma unroll
                    for (int e = 0; e < 16; e++) grad_mvp[(size_t)i * 16 + e] = G[e];
            }
        return;
    }
    // The gradients come straight from the accumulators, and Adam reads the 8 reduced floats back from LDS.
    pose_backward_reduce_t(
        [&](int i, float* G) {
            grad16(i, G);
            if (grad_mvp)
#pragma unroll
                for (int e = 0; e < 16; e++) grad_mvp[(size_t)i * 16 + e] = G[e];
        },
        [&](int) { return 0.f; }, pre.pb, tail.link_poses, B, L, tail.red, S, red_lds, &la_mine, nls == 32, Js, lp_lds);
    __syncthreads();
    if (!tail.defer_adam)
        pose_adam_apply(pre.st, tail.dof, tail.m, tail.v, tail.step, red_lds, tail.lr, tail.b1, tail.b2, tail.eps, tail.wd,
                        tail.loss_out, tail.grad_out);
}


static inline BinGeom make_geom(int H, int W, int L) {
    BinGeom g;
    g.W = W;
    g.H = H;
    g.ntx = (W + EHR_TILE_W - 1) / EHR_TILE_W;
    g.nty = (H + EHR_TILE_H - 1) / EHR_TILE_H;
    g.nt = g.ntx * g.nty;
    g.L = L;
    return g;
}

struct StepHead {  // inputs of the merged first stage (pose forward inside the vertex kernel)
    const float* dof;
    const float* K;
    const float* link_poses;
    float* tc_jac;
    int* hist_row;  // [1] row of `history` this step's pose goes to; advanced here (its own counter, not Adam's)
    float* history;
    int history_rows;
    float n, f;
    // A REPORTED step (overflow: loss NaN, pose and optimiser untouched -- on every rank of a data-parallel job, the NaN
    // travels with the exchanged sum) has written the unchanged pose to a row; the next step's head sees that Adam's
    // counter has not moved since the previous head and takes the same row again: the history keeps one row per EFFECTIVE
    // step with no host-side rewind (which had to guess which rows to give back).
    const int* adam_step;  // [1] the optimiser's step counter
    int* hstate;           // [2] ctx->vb_hstate
    // Multi-start form only (ehr_solver_step_multi; vb_vertex_kernel<true, true>): the launch's view b is virtual view
    // view0 + b = p * nviews + j, hypothesis p looking at real view j.  dof, tc_jac, hist_row, history, adam_step and
    // hstate (VB_HSTATE_INTS apart) are then arrays over p; link_poses holds the nviews real views.
    int view0, nviews;
};
constexpr int VB_HSTATE_INTS = 4;  // ints of head state per hypothesis: the three of StepHead::hstate, padded

// What one workgroup per hypothesis needs to finish a multi-start step (vb_finish_multi_kernel): the per-hypothesis
// arrays are those of StepTail, strided by hypothesis; the accumulators, loss_b and grad_mvp by virtual view.
struct MultiFinish {
    const long long* facc_all;  // accumulators of all P * Bv virtual views
    const long long* vtot_all;  // bound reference: the cached totals, tiled per virtual view (or NULL)
    const int* ref_flag;
    float* loss;                // [P * Bv]
    float* grad_mvp;            // [P * Bv][L][16]
    int* meta;
    int* lbox_all;              // the link boxes of all virtual views, re-armed here
    int P, Bv, nls;
    BinGeom g;
};


}  // namespace ehr
