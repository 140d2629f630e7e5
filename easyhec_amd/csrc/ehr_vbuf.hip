// ehr_vbuf.hip -- the fused hot path: the kernels and the launch chain behind ehr_render_mask_loss / ehr_solver_step
// (host entry points: ehr_fused.hip) and the coverage-only chain of ehr_mask_variance / ehr_mask_overlap (vb_cov_chain).  Restates
//   /root/reference/easyhec/modeling/models/rb_solve/rb_solver.py:60-72   (per-link render, sum, clamp, SSE)
//   /root/reference/easyhec/structures/nvdiffrast_renderer.py:33-47        (rasterize -> interpolate -> antialias -> flip)
//   /root/reference/easyhec/utils/nvdiffrast_utils.py:14-18                (transform_pos)
// without per-step triangle binning: no (tile, link) queues are built, counted, allocated or filled.  The meshes
// project to micro-triangles (median bounding box 8 px, a fifth of the non-empty boxes cover no pixel centre at all), for
// which building and draining per-tile queues cost more than the coverage tests themselves.  Instead ehr_fused_plan
// groups every link's triangles ONCE into clusters of 64 spatially close ones (recursive median split of the centroids
// in object space, valid for every pose), and a step is three launches per chunk of views (a fourth only after a step
// has met a triangle for the general path; the stateless render call always makes all four):
//
//   vb_vertex_kernel    [pose forward] + clip-space vertices (posc) + one wave per cluster: transforms the cluster's
//                       triangles, snaps them, tests small boxes exactly (a triangle that covers no pixel centre is
//                       dropped here, once) and publishes per triangle its pixel box (tbox) and its raster record
//                       (integer edge functions with the tie rule folded in, depth-range class; trec); per cluster and
//                       per link the union of the boxes (cbox; lbox through integer atomics).
//   vb_job_kernel       one WAVE per job = (view, link, 32x8 tile the link's box touches), persistent waves over a job
//                       list that is never materialised.  A job culls cluster boxes, then triangle boxes, and rasterizes
//                       the survivors COVERAGE FIRST: a wave-wide balanced walker (units of 4 pixels for narrow boxes,
//                       exactly solved row spans for wide ones) ORs coverage into an LDS bitmap and defers the covered
//                       units; at the job's end only the units that hold a covered pixel with an uncovered neighbour
//                       are depth tested (ds_min_u64 on ordered(z/w) << 32 | triangle: order independent, hence the
//                       oracle's z-buffer bit for bit wherever anyone will look).  Last step's heaviest jobs go first
//                       on whole workgroups, its long ones as the waves' static first jobs.
//   vb_slow_kernel      jobs that met a triangle for the general path: near-plane clipping, 64-bit edges (normally none; the
//                       solver step launches it only once a step has needed it, see vb_put_aside).
//   (resolve stage)     covered/uncovered pixel pairs by bit arithmetic on the coverage bitmap, silhouette analysis of the
//                       hits, the link's 256 antialiased values + the blended pairs -> job slot: no launch of its own, the
//                       wave that drew a job (in either of the two kernels above) resolves it from LDS
//                       (vb_resolve_from_lds).
//   vb_composite_kernel one wave per tile that holds a job (every tile without a bound reference mask): sums the links'
//                       values in link order, clamps, frame loss, mask write, back-propagates the tile's blended pairs
//                       to 12 numbers per link in the view's fixed-point accumulators; its finisher workgroup runs
//                       the finish stage (accumulators -> loss / grad_mvp [-> pose backward -> Adam]).  (Run at the end of
//                       the job kernel's launch instead, behind a grid-wide barrier, it was no faster: DESIGN.md section 6,
//                       profiles/experiments/r06_merged_job_composite.patch.)
//
// What runs once per rasterizer round or once per candidate cluster inside vb_job_kernel is kept free of LDS shuffles,
// integer divisions and searches: wave scans and reductions by DPP / v_permlane*_swap,
// a lane's first triangle by a scatter and a max-scan, packed hint ids, 24-bit multiplies.
//
// An earlier form kept the depth/id image in HBM and resolved visibility with one 64-bit global atomic-min per covered
// pixel; global atomics execute memory-side on this part (4.6 G/s with raster locality: 272 us for the 1.26 M fragments
// of the 8-view workload), see DESIGN.md section 6.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ehr_arrive.h"
#include "ehr_fused_core.h"

namespace ehr {

constexpr int VB_RW = EHR_TILE_W + 2;  // tile + 1-pixel halo
constexpr int VB_RH = EHR_TILE_H + 2;
constexpr int VB_RN = VB_RW * VB_RH;   // 340
constexpr int VB_WORDS = (VB_RN + 63) / 64;  // 6 coverage words
constexpr int VB_LBOX_STRIDE = 16;     // ints per (view, link) box: min x, min y, max x, max y, padding to a 64-byte line
constexpr int VB_HEAVY_T_DEFAULT = 3000;  // cost (4-pixel units walked + 256 per rasterizer round) from which a job counts
                                          // as heavy: next step a whole workgroup takes it.  Units, not triangles: a tile of
                                          // 130 long thin triangles (7000 units) keeps a wave busy for 60 us, one of 380 small
                                          // ones for 25
constexpr int VB_HEAVY_CAP = 4096;    // heavy jobs remembered per step
constexpr int VB_MED_CAP = 2048;      // long single-wave jobs remembered per step (they are started first)
constexpr int VB_MED_T_DEFAULT = 1250;    // cost from which a single-wave job counts as long (1500 until the box trim took a
                                          // third off the long jobs' costs; 1000 starts too many together: profiles/box_trim.md)
// Issue priority (s_setprio) of the waves on the jobs the kernel ends on: a long job started first runs beside three
// siblings per SIMD for most of its life (41 us instead of 30); with priority 48.5 instead of 50.0 us at 8 views.
constexpr int VB_PRIO_LONG = 3;
constexpr int VB_PRIO_HEAVY = 2;
constexpr int VB_JOB_ITEMS = 64;       // blended pairs kept in LDS per tile; the rest spills to a global pool
constexpr int VB_SPILL_BLOCK = 2048;   // items per spill allocation (one per overflowing tile)
constexpr u64 VB_EMPTY = ~0ull;
// Launch shapes: workgroups per CU of the chain's kernels, as many as stay resident together
constexpr int VB_VERTEX_GRID = 5;      // (VB_VERTEX_WAVES)
constexpr int VB_JOB_GRID = 4;         // (VB_JOB_WAVES: four workgroups' LDS fit a CU)
constexpr int VB_COMPOSITE_GRID = 6;
constexpr int VB_SCORE_COUNT_GRID = 4; // the scoring op's count kernel
constexpr int VB_SLOW_GRID = 32;       // in total: the general-triangle kernel (normally idle)
constexpr bool VB_XCD_SPLIT = true;    // vertex kernel: a chunk of VB_XCDS x k views gives every XCD the views its jobs go to (L2)
constexpr int VB_FAST_EXTENT = 8192;   // snapped extent (1/16 px) up to which 32-bit edge functions are exact

// (the part's XCDs, VB_XCDS, and what follows from them: ehr_arrive.h)

// Counters that many waves hit with atomics each get a 128-byte line of their own behind the meta block (atomics on
// one line serialise memory-side at ~12 ns each).
enum VbLine {
    VB_LINE_JOB_CURSOR = 0,                               // + xcd: job cursor of that XCD
    VB_LINE_COMP_ARRIVE = VB_LINE_JOB_CURSOR + VB_XCDS,   // + xcd: composite workgroups of that XCD that have arrived
    VB_LINE_SLOW_COUNT = VB_LINE_COMP_ARRIVE + VB_XCDS,   // jobs put aside for vb_slow_kernel
    VB_LINES
};
static_assert(VB_LINES <= 256, "one workgroup of the vertex kernel zeroes the lines, a thread each");
__host__ __device__ __forceinline__ int* vb_line(int* meta, int k) {
    return (int*)((((uintptr_t)(meta + EHR_META_INTS)) + 127) & ~(uintptr_t)127) + 32 * k;
}
// bytes of a meta block: the meta words, then the lines vb_line finds behind them (one more for its alignment)
constexpr size_t VB_META_BYTES = EHR_META_INTS * sizeof(int) + (VB_LINES + 1) * 128;

#define VB_WAVE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

struct VbItem {
    int packed;  // bits 0-9 q (region index of pixel0) | 10 d | 11-12 di | 13 tri1 | 14 (c1 - c0 > 0)
    int v1, v2;  // the two vertices of the crossing silhouette edge (global ids)
    float alpha;
};

// Scratch layouts.  Every scratch buffer of the chain is described ONCE, by a host function that carves its arrays, in
// order, from a base pointer (vb_recs, vb_heavy, vb_slots, vb_score_misc, vb_overlap_misc below); over a null base the end of the last
// array is the byte size the plan reserves.  (The bases come from hipMalloc: aligned beyond anything asked for here.)
struct VbCarve {
    uintptr_t at;
    template <class T>
    T* take(size_t n, size_t align = alignof(T)) {
        at = (at + align - 1) & ~(uintptr_t)(align - 1);
        T* const p = (T*)at;
        at += n * sizeof(T);
        return p;
    }
};

// Job slots of a chunk of views, compact (numbered like the jobs: a (view, link, tile) slot is found from the link's first
// job), and the tables that go with them.
struct VbSlots {
    float* jval;       // [jcap][256] the link's antialiased values of the tile
    VbItem* jitems;    // [jcap][VB_JOB_ITEMS] blended pairs for the backward pass
    int* jn;           // [jcap] number of blended pairs (-1: the link contributes nothing to the tile)
    int* jspill;       // [jcap] the job's first item in the spill pool
    int* jbase;        // [units + 1] first job of every (view, link) of the chunk
    unsigned* jutile;  // [units] its tile range
    int4* slow_list;   // [jcap] jobs put aside for vb_slow_kernel (NULL: that kernel is not launched, see vb_put_aside)
    int jcap;
};
constexpr size_t VB_SLOT_BYTES = 256 * sizeof(float) + VB_JOB_ITEMS * sizeof(VbItem) + 2 * sizeof(int) + sizeof(int4);  // the [jcap] arrays of vb_slots
static_assert(VB_SLOT_BYTES == 1024 + 1024 + 8 + 16, "job slot: 2072 bytes");
static VbSlots vb_slots(void* base, size_t jcap, size_t units, size_t* bytes = nullptr) {
    VbCarve c{(uintptr_t)base};
    VbSlots s;
    s.jval = c.take<float>(jcap * 256);
    s.jitems = c.take<VbItem>(jcap * VB_JOB_ITEMS);
    s.jn = c.take<int>(jcap);
    s.jspill = c.take<int>(jcap);
    s.jbase = c.take<int>(units + 1);
    s.jutile = c.take<unsigned>(units);
    s.slow_list = c.take<int4>(jcap, 16);
    s.jcap = (int)jcap;
    if (bytes) *bytes = c.at - (uintptr_t)base;
    return s;
}

// ---- compile-time bitmaps over the 34x10 region (bit i = region pixel i, row-major) ------------------------------
constexpr bool vb_interior(int i) {
    return (i % VB_RW) >= 1 && (i % VB_RW) <= EHR_TILE_W && (i / VB_RW) >= 1 && (i / VB_RW) <= EHR_TILE_H;
}
constexpr u64 vb_word_h(int k) {  // horizontal pair (i, i+1): same row, at least one pixel interior
    u64 w = 0;
    for (int j = 0; j < 64; j++) {
        const int i = 64 * k + j;
        if (i + 1 < VB_RN && (i % VB_RW) != VB_RW - 1 && (vb_interior(i) || vb_interior(i + 1))) w |= 1ull << j;
    }
    return w;
}
constexpr u64 vb_word_v(int k) {  // vertical pair (i, i+RW)
    u64 w = 0;
    for (int j = 0; j < 64; j++) {
        const int i = 64 * k + j;
        if (i + VB_RW < VB_RN && (vb_interior(i) || vb_interior(i + VB_RW))) w |= 1ull << j;
    }
    return w;
}

template <int S>
__device__ __forceinline__ void vb_shr(const u64 in[VB_WORDS], u64 out[VB_WORDS]) {
#pragma unroll
    for (int k = 0; k < VB_WORDS; k++) out[k] = (in[k] >> S) | (k + 1 < VB_WORDS ? in[k + 1] << (64 - S) : 0ull);
}

__device__ __forceinline__ int vb_readlane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float vb_readlane(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float4 vb_readlane(const float4& v, int lane) {
    return make_float4(vb_readlane(v.x, lane), vb_readlane(v.y, lane), vb_readlane(v.z, lane), vb_readlane(v.w, lane));
}
__device__ __forceinline__ int vb_mbcnt(u64 m) {  // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// ---- stage 1: vertices, screen boxes of triangles / clusters / links ---------------------------------------------

// Jobs that turned out heavy in the PREVIOUS step (poses move little between optimisation steps): remembered by their
// dense (view, link, tile) id, stamped into a table at the start of the step so that the single-wave enumeration skips
// them, and processed first, each by a whole workgroup.  Purely a scheduling hint: results do not depend on it.
struct VbHeavy {
    int* gen;     // [0] generation (one per call), [1..2] entries in list 0 / 1, [4..5] entries in mlist 0 / 1
    int* list;    // [2][VB_HEAVY_CAP] dense ids; list (gen & 1) is being written, the other one is being consumed
    int* mlist;   // [2][VB_MED_CAP] likewise: jobs below the heavy threshold that were long all the same
    int* stamp;   // [B * L * nt]  == generation: handled by a heavy workgroup this step; == -generation: a long job, dealt
                  // out as some wave's first job
    int mcap;     // long jobs consumed per step: min(VB_MED_CAP, 2 x workgroups of the job kernel) -- every one of them
                  // must find a wave with a static first job, and at least half the workgroups have those
    int heavy_base;  // the cost from which a job counts as heavy (gen[6] holds the value in force, never below this one)
    int heavy_max;   // heavy jobs a step can use (half the job kernel's workgroups): when a step records more, the value in
                     // force rises by an eighth, so that the heaviest jobs keep their workgroups instead of the whole phase
                     // being switched off (the Franka meshes at 1080p: 3000 jobs above 2500 in 8100; 112 instead of 124 us
                     // with the ~500 heaviest shared); it sinks back when fewer than half as many are recorded
};

// gen | list | mlist | stamp [nstamp]; the scheduling fields are the caller's (zero: the hint is off)
static VbHeavy vb_heavy(void* base, size_t nstamp, size_t* bytes = nullptr) {
    VbCarve c{(uintptr_t)base};
    VbHeavy hv = {};
    hv.gen = c.take<int>(8);
    hv.list = c.take<int>(2 * VB_HEAVY_CAP);
    hv.mlist = c.take<int>(2 * VB_MED_CAP);
    hv.stamp = c.take<int>(nstamp);
    if (bytes) *bytes = c.at - (uintptr_t)base;
    return hv;
}

// A remembered job in the hint lists: tile column | tile row << 10 | (view, link) << 22 -- no division on the way from a
// list entry to the first cluster box (the long jobs the kernel ends on start from these).
__device__ __forceinline__ int vb_hint_pack(int u, int tx, int ty) { return tx | (ty << 10) | (u << 22); }
__device__ __forceinline__ int vb_hint_dense(int id, int nt, int ntx) {
    return (int)((unsigned)id >> 22) * nt + ((id >> 10) & 4095) * ntx + (id & 1023);
}
static_assert(VB_MAX_UNITS <= 1024, "vb_hint_pack");
struct VbClusters {          // static acceleration index built by ehr_fused_plan (host): triangles grouped into
    const int32_t* ctri;     // [NC * 64] clusters of <= 64 spatially close triangles of one link (-1 = padding)
    const int32_t* clink;    // [NC] link of every cluster
    const int32_t* coff;     // [L + 1] first cluster of every link
    const float* laabb;      // [L][6] object-space bounding box of every link (min xyz, max xyz)
    const float4* cvert;     // [3][NC * 64] object-space corners of every cluster slot, packed (x0 y0 z0 x1 | y1 z1 x2 y2 |
                             // z2 valid - -): one coalesced round trip instead of the chain ctri -> tris -> verts
    int NC;
};

__device__ __forceinline__ uint2 vb_pack_box(int x0, int y0, int x1, int y1) {
    return make_uint2((unsigned)x0 | ((unsigned)y0 << 16), (unsigned)x1 | ((unsigned)y1 << 16));
}
#define VB_BOX_EMPTY make_uint2(0xffffffffu, 0u)  // x0 = y0 = 65535 > any pixel, x1 = y1 = 0: overlaps nothing

// grid = (nvb + ceil(NC / 4), B): the first nvb workgroups of a view transform its vertices (posc), the others take
// four clusters each -- one wave per cluster, one lane per triangle -- and publish the pixel bounding box of every
// triangle (tbox, empty for triangles that cover no pixel centre column/row), of every cluster (cbox) and, through a
// handful of integer atomics, of every link (lbox; reset by the finish kernel).  The cluster path transforms its own
// vertices with the same fma chain, so it does not wait for posc.  HEAD: the solver-step form (pose forward from dof,
// writes mvp / tc_jac / history row); otherwise mvp is an input.
// 32-bit edge functions of a triangle whose snapped extent is <= VB_FAST_EXTENT, relative to the centre of pixel
// (bx0, by0), which lies inside the triangle's bounding box: |coordinates| <= 2^13, products < 2^27.
struct VbEdges {
    int e0, e1, e2, sx0, sx1, sx2, sy0, sy1, sy2;
};
__device__ __forceinline__ VbEdges vb_edges(int X0, int Y0, int X1, int Y1, int X2, int Y2, int bx0, int by0, int W,
                                            int H) {
    VbEdges r;
    const int ox = 16 * bx0 + 8 - 8 * W, oy = 16 * by0 + 8 - 8 * H;
    X0 -= ox; X1 -= ox; X2 -= ox;
    Y0 -= oy; Y1 -= oy; Y2 -= oy;
    // (every factor is below 2^14 in magnitude: v_mul_i32_i24 is exact here and runs at full rate, v_mul_lo_u32 at a quarter)
    {
        const int dX = X1 - X0, dY = Y1 - Y0;
        r.e0 = __mul24(dX, 0 - Y0) - __mul24(dY, 0 - X0) - (((dY < 0) || (dY == 0 && dX < 0)) ? 0 : 1);
        r.sx0 = -16 * dY;
        r.sy0 = 16 * dX;
    }
    {
        const int dX = X2 - X1, dY = Y2 - Y1;
        r.e1 = __mul24(dX, 0 - Y1) - __mul24(dY, 0 - X1) - (((dY < 0) || (dY == 0 && dX < 0)) ? 0 : 1);
        r.sx1 = -16 * dY;
        r.sy1 = 16 * dX;
    }
    {
        const int dX = X0 - X2, dY = Y0 - Y2;
        r.e2 = __mul24(dX, 0 - Y2) - __mul24(dY, 0 - X2) - (((dY < 0) || (dY == 0 && dX < 0)) ? 0 : 1);
        r.sx2 = -16 * dY;
        r.sy2 = 16 * dX;
    }
    return r;
}

// Per-triangle raster record written by the cluster pass, read by the job waves (so a triangle is set up once per
// step, not once per tile it touches):
//   trec[2 i]     = { e0, e1, e2, dX0 | dY0 << 16 }   edge functions (tie rule folded in) at the centre of the box's
//   trec[2 i + 1] = { dX1 | dY1 << 16, dX2 | dY2 << 16, triangle id, kind }   first pixel; kind 0 = 32-bit fast path and
//                   every coverable pixel passes the depth-range test, 2 = fast path but the depth range must be tested
//                   per pixel, 1 = needs clipping / 64-bit (handled from the vertices)
// Depth is evaluated from the clip-space vertices (posc) of the few units that need it.
struct VbRecs {
    uint2* tbox;   // [B][NC][64] pixel box, VB_BOX_EMPTY if the triangle cannot cover a pixel centre
    uint2* cbox;   // [B][NC] union over the cluster
    int4* trec;    // [B][NC][64][2]: the two halves of a record side by side
    size_t n;      // B * NC * 64 (component stride)
};
constexpr size_t VB_REC_BYTES = sizeof(int4) * 2 + sizeof(uint2);              // a cluster slot: raster record + pixel box
constexpr size_t VB_CLUSTER_REC_BYTES = 64 * VB_REC_BYTES + sizeof(uint2);     // a (view, cluster): its 64 slots + its box
static_assert(VB_CLUSTER_REC_BYTES == 2568, "raster records: 64 x (32 + 8) + 8 bytes per (view, cluster)");
// trec | tbox | cbox of `views` views x NC clusters
static VbRecs vb_recs(void* base, size_t views, size_t NC, size_t* bytes = nullptr) {
    VbCarve c{(uintptr_t)base};
    VbRecs r;
    r.n = views * NC * 64;
    r.trec = c.take<int4>(r.n * 2);
    r.tbox = c.take<uint2>(r.n);
    r.cbox = c.take<uint2>(views * NC);
    if (bytes) *bytes = c.at - (uintptr_t)base;
    return r;
}

// True if every pixel centre the triangle's SNAPPED outline can cover evaluates to a depth z/w inside [-1, 1] in
// vb_depth_test's arithmetic, so that coverage = the integer edge test alone.  All w > 0 (no near-plane crossing).
// z/w is affine over the screen; a covered pixel centre lies within 1/32 pixel (per axis) of the unsnapped triangle, and
// the float evaluation perturbs the barycentric weights by at most ~5e-5 pixel / thickness.  Hence: depth of the
// vertices, widened by the depth gradient over 0.6 sixteenth-pixels and by a quarter of the depth range, must stay
// 1e-5 inside the planes; thickness (2 area / longest edge) at least 0.05 sixteenth-pixels; w within a factor 4.
// Everything else -- NaNs included -- is "unsafe" and gets the exact per-pixel test.  For a robot in front of the
// camera (z/w = 0.998 at 1 m with near 1 mm, far 10 m; depth range of a triangle ~1e-5) only edge-on slivers fail.
// pos: the stricter class of the scoring op (mask = z/w of the nearest fragment > 0): every coverable pixel centre has
// a depth in (0, 1], so that coverage alone decides the mask.
__device__ __forceinline__ bool vb_depth_safe(const float4& p0, const float4& p1, const float4& p2, int W, int H, bool pos = false) {
    // (a classification, not a result: where it says "safe" the per-pixel depth-range test is skipped, and both ways draw the
    //  same pixels as long as "safe" is never said wrongly -- so the ten quotients are products with hardware reciprocals
    //  (1 ulp: 1e-7 of a depth near 1, absorbed by the margins below, which are a tenth wider than the bound they come from)
    //  instead of ten IEEE divisions of ~10 instructions each in the busiest loop of the vertex kernel)
    const float r0 = __builtin_amdgcn_rcpf(p0.w), r1 = __builtin_amdgcn_rcpf(p1.w), r2 = __builtin_amdgcn_rcpf(p2.w);
    const float z0 = p0.z * r0, z1 = p1.z * r1, z2 = p2.z * r2;
    const float sx = (float)(8 * W), sy = (float)(8 * H);
    const float x0 = p0.x * r0 * sx, y0 = p0.y * r0 * sy;
    const float d1x = p1.x * r1 * sx - x0, d1y = p1.y * r1 * sy - y0;
    const float d2x = p2.x * r2 * sx - x0, d2y = p2.y * r2 * sy - y0;
    const float q1 = fabsf(z1 - z0), q2 = fabsf(z2 - z0);
    const float A = fabsf(d1x * d2y - d2x * d1y);
    const float l1 = fabsf(d1x) + fabsf(d1y), l2 = fabsf(d2x) + fabsf(d2y);
    const float delta = 0.66f * (q1 * l2 + q2 * l1) * __builtin_amdgcn_rcpf(A) + 0.275f * (q1 + q2);
    const float zmax = fmaxf(z0, fmaxf(z1, z2)), zmin = fminf(z0, fminf(z1, z2));
    const float wmax = fmaxf(p0.w, fmaxf(p1.w, p2.w)), wmin = fminf(p0.w, fminf(p1.w, p2.w));
    return (A >= 0.055f * (l1 + l2) + 1.1e-3f) && (wmax <= 4.f * wmin) && (zmax + delta <= 1.f - 1.1e-5f) &&
           (zmin - delta >= (pos ? 1.1e-5f : -1.f + 1.1e-5f));
}

// two 16-bit unsigned minima / maxima in one instruction (v_pk_min_u16 / v_pk_max_u16)
typedef unsigned short vb_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned vb_pk_min_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(vb_u16x2, a), __builtin_bit_cast(vb_u16x2, b)));
}
__device__ __forceinline__ unsigned vb_pk_max_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(vb_u16x2, a), __builtin_bit_cast(vb_u16x2, b)));
}

constexpr int VB_SMALL_BOX = 3;  // boxes of up to this many pixel centres a side are tested exactly by the vertex kernel (4: the
                                 // fourth row and column cost the VALU-bound kernel 7 % at Franka 16 x 1080p and drop nothing the
                                 // job kernel notices; 2: the job kernel pays 2.3 us at 8 views for the 3 x 3 boxes that cover nothing)
constexpr int VB_VERTEX_WAVES = 5;  // (five workgroups per CU stay resident: the launch deals the work accordingly)
// vb_vertex_kernel's chunk_role.  The views of a step go through the chain in chunks (one, unless views x links exceeds
// what a job kernel handles):
enum VbRole {
    VB_ROLE_FIRST_CHUNK = 1,  // the per-step housekeeping happens here
    VB_ROLE_LATER_CHUNK = 2,  // only the per-chunk counters are re-armed
    VB_ROLE_CHUNK_MASK = 3,
    VB_ROLE_POS_ONLY = 4,     // flag: the scoring op's chain (depth class "coverage decides")
};
// MULTI (with HEAD): the multi-start step -- view b of the launch is virtual view head.view0 + b = p * head.nviews + j:
// hypothesis p's pose (dof[p]) on real view j's link poses; the first workgroup of every hypothesis's first view writes
// that hypothesis's tc_jac, history row and head state.  The step-wide housekeeping stays with the call's first workgroup.
template <bool HEAD, bool MULTI = false>
__global__ void __launch_bounds__(256, VB_VERTEX_WAVES)
vb_vertex_kernel(const float* __restrict__ verts, const int32_t* __restrict__ vert_link,
                 const int32_t* __restrict__ tris, VbClusters cl, StepHead head, float* __restrict__ mvp, int V, int nvb,
                 BinGeom g, float4* __restrict__ posc, VbRecs rc, int* __restrict__ lbox, int* __restrict__ zacc,
                 int nzacc, int* __restrict__ meta, int B, int gx, int xcd_views, VbHeavy hv, int chunk_role) {
    __shared__ float Tc[16];
    __shared__ float M[32][16];
    // 1-D grid of B * gx workgroups.  xcd_views > 0 (B a multiple of VB_XCDS): workgroup w runs on XCD w % VB_XCDS and
    // that XCD takes views [xcd * xcd_views, (xcd + 1) * xcd_views) -- the same views whose jobs stage 2 gives to that XCD,
    // so the records it reads were written through the same L2.
    int b, bx;
    if (xcd_views > 0) {
        const int xcd = blockIdx.x & (VB_XCDS - 1), k = blockIdx.x >> VB_XCD_BITS;
        b = xcd * xcd_views + k / gx;
        bx = k - (k / gx) * gx;
    } else {
        b = blockIdx.x / gx;
        bx = blockIdx.x - b * gx;
    }
    const int tid = threadIdx.x, L = g.L, H = g.H, W = g.W;
    const bool pos_only = (chunk_role & VB_ROLE_POS_ONLY) != 0;
    chunk_role &= VB_ROLE_CHUNK_MASK;
    const bool first = bx == 0 && b == 0 && chunk_role == VB_ROLE_FIRST_CHUNK;
    const bool rearm = bx == 0 && b == 0 && chunk_role == VB_ROLE_LATER_CHUNK;
    int hyp = 0, bview = b;  // MULTI: the hypothesis of this view and the real view it looks at
    if (MULTI) {
        const int bg = head.view0 + b;
        hyp = bg / head.nviews;
        bview = bg - hyp * head.nviews;
        head.dof += 6 * hyp;
    }
    const bool first_head = MULTI ? (bx == 0 && bview == 0) : first;  // writes tc_jac, the history row and the head state
    // A view's work items: [0, nvb) blocks of 256 vertices (-> posc; nvb = 0 where the plan computes clip-space vertices on
    // demand, see VbLazy), then groups of four clusters (one wave per cluster, one lane per triangle).  The workgroup takes items bx, bx + gx, ...: the pose head above every item (exponential,
    // matrices: ~3 us of dependent arithmetic) is paid once per workgroup, not once per 256 vertices -- with one item per
    // workgroup the Franka scene (375 k vertices x 16 views) needed 32 k workgroups and 125 us.
    const int nitems = nvb + (cl.NC + 3) / 4;
    const int lane = tid & 63;
    int item = bx;
    int l = -1, t = -1;
    float vx[3] = {0.f, 0.f, 0.f}, vy[3] = {0.f, 0.f, 0.f}, vz[3] = {0.f, 0.f, 0.f};
    bool have = false;
    // geometry loads first: they do not depend on the pose, so their latency hides under the pose arithmetic below
    auto load_geometry = [&](int it) {
        l = -1;
        t = -1;
        have = false;
        if (it < nvb) {
            const int v = it * 256 + tid;
            if (v < V) {
                l = vert_link[v];
                vx[0] = verts[3 * v];
                vy[0] = verts[3 * v + 1];
                vz[0] = verts[3 * v + 2];
                have = true;
            }
        } else {
            const int c = (it - nvb) * 4 + (tid >> 6);
            if (c < cl.NC) {
                const size_t cs = (size_t)c * 64 + lane, cn = (size_t)cl.NC * 64;
                t = cl.ctri[cs];
                l = cl.clink[c];
                const float4 q0 = cl.cvert[cs], q1 = cl.cvert[cn + cs], q2 = cl.cvert[2 * cn + cs];
                vx[0] = q0.x; vy[0] = q0.y; vz[0] = q0.z;
                vx[1] = q0.w; vy[1] = q1.x; vz[1] = q1.y;
                vx[2] = q1.z; vy[2] = q1.w; vz[2] = q2.x;
                have = t >= 0 && q2.y != 0.f;  // padding slots and triangles with a vertex index out of range draw nothing
            }
        }
    };
    if (item < nitems) load_geometry(item);
    __shared__ int lacc[32][4];  // pixel box of every link as far as this workgroup's clusters go
    if (tid < 128) lacc[tid >> 2][tid & 3] = (tid & 2) ? -1 : INT_MAX;
    // HEAD: the view's link poses and the intrinsics are requested NOW, together with dof, and parked in LDS: behind the
    // barrier below they were a second cold round trip on every workgroup's chain (dof -> exponential -> barrier -> link
    // poses -> matrices)
    __shared__ float LP[32][16];
    __shared__ float Kc[9];
    float dofv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (HEAD) {
        // (uniform: scalar loads into scalar registers, requested first; the exponential below waits for these alone)
#pragma unroll
        for (int k = 0; k < 6; k++) dofv[k] = head.dof[k];
        float lpv[2] = {0.f, 0.f};
        float kv = 0.f;
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (tid + 256 * j < L * 16) lpv[j] = head.link_poses[(size_t)bview * L * 16 + tid + 256 * j];
        if (tid >= 64 && tid < 73) kv = head.K[tid - 64];
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (tid + 256 * j < L * 16) LP[(tid + 256 * j) >> 4][(tid + 256 * j) & 15] = lpv[j];
        if (tid >= 64 && tid < 73) Kc[tid - 64] = kv;
    }
    if (HEAD && tid < 6) {
        Dual<1> T6[16];
        se3_exp_dual<1>(dofv, 1e-4f, T6, tid);
        if (tid == 0)
            for (int i = 0; i < 16; i++) Tc[i] = T6[i].v;
        if (first_head) {
            if (MULTI) {
                head.tc_jac += 7 * 16 * hyp;
                if (head.history && head.hist_row) {
                    head.hist_row += hyp;
                    head.history += (size_t)hyp * head.history_rows * 6;
                }
                head.adam_step += hyp;
                head.hstate += VB_HSTATE_INTS * hyp;
            }
            for (int i = 0; i < 16; i++) {
                if (tid == 0) head.tc_jac[i] = T6[i].v;
                head.tc_jac[16 * (tid + 1) + i] = T6[i].d[0];
            }
            if (tid == 0 && head.history && head.hist_row) {  // rb_solver.py:50-51: the pose goes to the next free row
                int row = head.hist_row[0];
                if (head.hstate && head.adam_step) {
                    // no Adam step since the previous head: that step was reported, its row (the same pose) is this step's
                    // (and nobody has moved the cursor either -- a state loaded from outside sets both)
                    const int t1 = head.adam_step[0] + 1;
                    if (head.hstate[0] == t1 && head.hstate[1] && head.hstate[2] == row && row > 0) row -= 1;
                    head.hstate[0] = t1;
                }
                const bool adv = row >= 0 && row < head.history_rows;
                if (adv) {
                    for (int k = 0; k < 6; k++) head.history[6 * row + k] = dofv[k];
                    head.hist_row[0] = row + 1;
                }
                if (head.hstate) {
                    head.hstate[1] = adv ? 1 : 0;
                    head.hstate[2] = adv ? row + 1 : row;
                }
            }
        }
    }
    if (first) {
        // new generation of the heavy-job hint: stamp last step's heavy jobs, start this step's list empty
        __shared__ int s_gen;
        if (tid == 0) {
            s_gen = hv.gen[0] + 1;
            hv.gen[0] = s_gen;
            hv.gen[1 + (s_gen & 1)] = 0;
            hv.gen[4 + (s_gen & 1)] = 0;
            {   // the heavy threshold in force follows the number of heavy jobs the last step recorded
                const int nprev = hv.gen[1 + ((s_gen - 1) & 1)];
                int thr = max(hv.gen[6], hv.heavy_base);
                if (nprev > hv.heavy_max)
                    thr = min(thr + (thr >> 3), 1 << 24);
                else if (2 * nprev < hv.heavy_max)
                    thr = max(hv.heavy_base, thr - (thr >> 4));
                hv.gen[6] = thr;
            }
        }
        __syncthreads();
        {
            const int gen = s_gen, cur = (gen - 1) & 1;
            const int n = min(hv.gen[1 + cur], VB_HEAVY_CAP);
            for (int i = tid; i < n; i += 256) hv.stamp[min(vb_hint_dense(hv.list[cur * VB_HEAVY_CAP + i], g.nt, g.ntx), B * L * g.nt - 1)] = gen;
            const int n2 = min(hv.gen[4 + cur], hv.mcap);
            for (int i = tid; i < n2; i += 256) hv.stamp[min(vb_hint_dense(hv.mlist[cur * VB_MED_CAP + i], g.nt, g.ntx), B * L * g.nt - 1)] = -gen;
        }
        if (tid < 8) meta[tid] = 0;                          // overflow flag, spill cursor
        if (tid < VB_LINES) *vb_line(meta, tid) = 0;         // job cursors of the XCDs, arrival counters, slow-job count
    }
    if (rearm) {  // a later chunk of the same step: cursors and arrival counters again, the overflow flag stays
        if (tid < 8 && tid != EHR_META_OVERFLOW) meta[tid] = 0;
        if (tid < VB_LINES) *vb_line(meta, tid) = 0;
    }
    if (bx == 0) {  // fixed-point accumulators of this view (a few KB)
        const int nzv = nzacc / B;
        for (int i = tid; i < nzv; i += 256) zacc[(size_t)b * nzv + i] = 0;
    }
    __syncthreads();
    if (HEAD) {
        if (tid < L) {
            float P[16], C[16];
            projection(Kc, H, W, head.n, head.f, P);
            mvp_from_pose(Tc, P, LP[tid], C);
            for (int k = 0; k < 16; k++) M[tid][k] = C[k];
            if (bx == 0)
                for (int k = 0; k < 16; k++) mvp[((size_t)b * L + tid) * 16 + k] = C[k];
        }
    } else {
        for (int i = tid; i < L * 16; i += 256) M[i >> 4][i & 15] = mvp[(size_t)b * L * 16 + i];
    }
    __syncthreads();
    for (; item < nitems;) {
    const bool lv = (unsigned)l < (unsigned)L;
    if (item < nvb) {
        const int v = item * 256 + tid;
        if (v < V) {
            float4 o = make_float4(0.f, 0.f, 0.f, -1.f);  // invalid link -> behind the camera, never drawn
            if (lv) o = transform_vertex(M[l], vx[0], vy[0], vz[0]);
            posc[(size_t)b * V + v] = o;
        }
    } else {
    const int c = (item - nvb) * 4 + (tid >> 6);
    const bool cvalid = c < cl.NC;
    int x0 = 0xffff, y0 = 0xffff, x1 = 0, y1 = 0;  // empty (overlaps nothing)
    int4 r0 = make_int4(-1, -1, -1, 0), r1 = make_int4(0, 0, t, 0);
    if (have && lv) {
        const float4 p0 = transform_vertex(M[l], vx[0], vy[0], vz[0]);
        const float4 p1 = transform_vertex(M[l], vx[1], vy[1], vz[1]);
        const float4 p2 = transform_vertex(M[l], vx[2], vy[2], vz[2]);
        const bool simple = (p0.w > 0.f) && (p1.w > 0.f) && (p2.w > 0.f) && (p0.z + p0.w >= 0.f) &&
                            (p1.z + p1.w >= 0.f) && (p2.z + p2.w >= 0.f);
        if (!simple) {  // crosses the near plane: the pixel box of its clipped pieces (the whole-wave path draws it)
            const float4 pp[3] = {p0, p1, p2};
            const ClipPoly cp = clip_near_poly(pp);
            for (int sidx = 0; sidx + 2 < cp.n; sidx++) {
                const Coverage cv = (sidx == 0) ? setup_coverage(cp.q0, cp.q1, cp.q2, W, H) : setup_coverage(cp.q0, cp.q2, cp.q3, W, H);
                if (!cv.valid) continue;
                const int ax = max(cv.ix0, 0), ay = max(cv.iy0, 0), bx1 = min(cv.ix1, W - 1), by1 = min(cv.iy1, H - 1);
                if (ax > bx1 || ay > by1) continue;
                x0 = min(x0, ax);
                y0 = min(y0, ay);
                x1 = max(x1, bx1);
                y1 = max(y1, by1);
            }
            r1.w = 1;
        } else {
            const Coverage cv = setup_coverage(p0, p1, p2, W, H);
            if (cv.valid) {
                x0 = cv.ix0; y0 = cv.iy0; x1 = cv.ix1; y1 = cv.iy1;
                // (snapped coordinates lie within +-2^30: the extent fits 32 unsigned bits)
                const unsigned ex = (unsigned)max(cv.X[0], max(cv.X[1], cv.X[2])) - (unsigned)min(cv.X[0], min(cv.X[1], cv.X[2]));
                const unsigned ey = (unsigned)max(cv.Y[0], max(cv.Y[1], cv.Y[2])) - (unsigned)min(cv.Y[0], min(cv.Y[1], cv.Y[2]));
                if (ex > VB_FAST_EXTENT || ey > VB_FAST_EXTENT) {
                    r1.w = 1;
                } else {
                    const VbEdges ed = vb_edges(cv.X[0], cv.Y[0], cv.X[1], cv.Y[1], cv.X[2], cv.Y[2], x0, y0, W, H);
                    // A small box (<= VB_SMALL_BOX pixel centres a side: nearly half of all triangles) is tested exactly, once, here: a fifth of
                    // the triangles with a non-empty box cover no pixel centre at all (70 % of the 1 x 1 boxes), and would
                    // otherwise be fetched, staged and walked by every job whose region their box touches.  The same
                    // integer edge functions as the rasterizer's walk, so nothing that could be drawn is dropped.
                    if (x1 - x0 < VB_SMALL_BOX && y1 - y0 < VB_SMALL_BOX) {
                        const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
                        bool any = false;
                        int q0 = ed.e0, q1 = ed.e1, q2 = ed.e2;
#pragma unroll
                        for (int j = 0; j < VB_SMALL_BOX; j++) {
                            int a0 = q0, a1 = q1, a2 = q2;
#pragma unroll
                            for (int i = 0; i < VB_SMALL_BOX; i++) {
                                any = any || (i < bw && j < bh && (a0 | a1 | a2) >= 0);
                                a0 += ed.sx0;
                                a1 += ed.sx1;
                                a2 += ed.sx2;
                            }
                            q0 += ed.sy0;
                            q1 += ed.sy1;
                            q2 += ed.sy2;
                        }
                        if (!any) {
                            x0 = 0xffff; y0 = 0xffff; x1 = 0; y1 = 0;
                        }
                    }
                    r0 = make_int4(ed.e0, ed.e1, ed.e2, (int)(((unsigned)(ed.sy0 / 16) & 0xffffu) | ((unsigned)(-ed.sx0 / 16) << 16)));
                    r1.x = (int)(((unsigned)(ed.sy1 / 16) & 0xffffu) | ((unsigned)(-ed.sx1 / 16) << 16));
                    r1.y = (int)(((unsigned)(ed.sy2 / 16) & 0xffffu) | ((unsigned)(-ed.sx2 / 16) << 16));
                    r1.w = vb_depth_safe(p0, p1, p2, W, H, pos_only) ? 0 : 2;
                }
            }
        }
    }
    const size_t slot = ((size_t)b * cl.NC + (cvalid ? c : 0)) * 64 + lane;
    if (cvalid) rc.tbox[slot] = vb_pack_box(x0, y0, x1, y1);
    if (cvalid && x0 <= x1) {
        rc.trec[2 * slot] = r0;  // (the two halves side by side: one 32-byte piece of a cache line per triangle)
        rc.trec[2 * slot + 1] = r1;
    }
    // the cluster's box: a DPP reduction (four shifts inside the rows of 16 lanes, then the rows' results upwards: lane 63
    // ends up with everything; integers, so the order is free), no LDS.  The two words of the packed box ARE the operands: two
    // 16-bit minima / maxima per instruction (an empty box is (65535, 65535)-(0, 0): neutral both ways).
    const uint2 pbox = vb_pack_box(x0, y0, x1, y1);
    unsigned bmin = pbox.x, bmax = pbox.y;
#define VB_BOX_STEP(ctrl, rows)                                                                       \
    bmin = vb_pk_min_u16(bmin, (unsigned)__builtin_amdgcn_update_dpp((int)bmin, (int)bmin, ctrl, rows, 0xf, false)); \
    bmax = vb_pk_max_u16(bmax, (unsigned)__builtin_amdgcn_update_dpp((int)bmax, (int)bmax, ctrl, rows, 0xf, false));
    VB_BOX_STEP(0x111, 0xf) VB_BOX_STEP(0x112, 0xf) VB_BOX_STEP(0x114, 0xf) VB_BOX_STEP(0x118, 0xf)
    VB_BOX_STEP(0x142, 0xa) VB_BOX_STEP(0x143, 0xc)
#undef VB_BOX_STEP
    const int a = (int)(bmin & 0xffffu), bq = (int)(bmin >> 16), cc = (int)(bmax & 0xffffu), d = (int)(bmax >> 16);
    if (lane == 63) {
        const bool cne = cvalid && a <= cc;
        if (cvalid) rc.cbox[(size_t)b * cl.NC + c] = cne ? vb_pack_box(a, bq, cc, d) : VB_BOX_EMPTY;
        if (cne && lv) {  // link box: merged over everything this workgroup sees (LDS), published once at the end
            atomicMin(&lacc[l][0], a);
            atomicMin(&lacc[l][1], bq);
            atomicMax(&lacc[l][2], cc);
            atomicMax(&lacc[l][3], d);
        }
    }
    }
    item += gx;
    if (item < nitems) load_geometry(item);
    }
    // link boxes: integer atomics, one 64-byte line per (view, link): a workgroup's clusters belong to one or two links,
    // ~6 k atomics per step spread over B * L lines
    __syncthreads();
    if (tid < 4 * L && lacc[tid >> 2][0] != INT_MAX) {
        int* const lb = lbox + VB_LBOX_STRIDE * ((size_t)b * L + (tid >> 2));
        if (tid & 2)
            atomicMax(lb + (tid & 3), lacc[tid >> 2][tid & 3]);
        else
            atomicMin(lb + (tid & 3), lacc[tid >> 2][tid & 3]);
    }
}

// ---- stage 2: one wave per job: cull, coverage into LDS, depth only where the silhouette analysis will look ---------

// i / VB_RW for 0 <= i < 4096 by one full-rate 24-bit multiply (1928 = ceil(2^16 / 34), 1928 * 34 - 2^16 = 16)
__device__ __forceinline__ int vb_div_rw(int i) { return (int)(__umul24((unsigned)i, 1928u) >> 16); }
static_assert(VB_RW == 34, "vb_div_rw");
// ---- wave scans without LDS (DPP): four shifts inside the rows of 16 lanes, then the rows' totals into the rows above
#define VB_DPP_(v, ctrl, rows) __builtin_amdgcn_update_dpp(0, (v), (ctrl), (rows), 0xf, false)
__device__ __forceinline__ int vb_scan_add(int v) {  // inclusive sum
    v += VB_DPP_(v, 0x111, 0xf);  // row_shr:1
    v += VB_DPP_(v, 0x112, 0xf);  // row_shr:2
    v += VB_DPP_(v, 0x114, 0xf);  // row_shr:4
    v += VB_DPP_(v, 0x118, 0xf);  // row_shr:8
    v += VB_DPP_(v, 0x142, 0xa);  // row_bcast:15 -> rows 1 and 3
    v += VB_DPP_(v, 0x143, 0xc);  // row_bcast:31 -> rows 2 and 3
    return v;
}
__device__ __forceinline__ int vb_scan_max(int v) {  // inclusive maximum of values >= 0
    v = max(v, VB_DPP_(v, 0x111, 0xf));
    v = max(v, VB_DPP_(v, 0x112, 0xf));
    v = max(v, VB_DPP_(v, 0x114, 0xf));
    v = max(v, VB_DPP_(v, 0x118, 0xf));
    v = max(v, VB_DPP_(v, 0x142, 0xa));
    v = max(v, VB_DPP_(v, 0x143, 0xc));
    return v;
}
// x / d for 0 <= x < 2^16, 1 <= d <= 128 (inv = 1 / d to an ulp): (x + 0.5) / d is at least 0.5 / d away from the next
// integer, the float product at most 2^16 * 2^-22 -- exact
__device__ __forceinline__ int vb_div_small(int x, float inv) { return (int)(((float)x + 0.5f) * inv); }
// the next set bit of m above position j (there is one)
__device__ __forceinline__ int vb_next_set(u64 m, int j) { return j + __ffsll((unsigned long long)(m >> (j + 1))); }
// The steps j of [0, n) at which all three m[k] + j s[k] can be >= 0, as a range [lo, hi] (lo > hi: none).  m[k] is the
// edge's largest value across the box's other axis, so a step outside the range holds no covered pixel.  The values are
// integers: m + j s >= 0 is m + 0.5 + j s > 0, a bound -(m + 0.5) / s that is never an integer and never 0 / 0 (s = 0: the
// quotient is an infinity of the right sign).  The float quotient is within 1e-5 of the true one wherever it lies inside
// the box (|j| <= 34), and is pushed outwards by 1/256 before it is rounded: the range is never too small, and one step
// too large only where a bound comes that close to an integer.
__device__ __forceinline__ void vb_trim_range(const int m[3], const int s[3], int n, int& lo, int& hi) {
    float fl = 0.f, fh = (float)(n - 1);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float t = -((float)m[k] + 0.5f) * __builtin_amdgcn_rcpf((float)s[k]);
        if (s[k] >= 0)
            fl = fmaxf(fl, t);  // rising along the axis: a lower bound
        else
            fh = fminf(fh, t);
    }
    lo = (int)ceilf(fminf(fl, 64.f) - 0x1p-8f);
    hi = (int)floorf(fmaxf(fh, -1.f) + 0x1p-8f);
}

struct VbRegion {
    int x0, y0, x1, y1;  // pixels of the region inside the image (inclusive); region origin = (rx0, ry0) below
};

// Clip-space vertices ON DEMAND (round 6).  Until round 5 the vertex kernel wrote every vertex's clip-space position per view
// (posc [B][V] float4) for the few thousand the depth tests, the silhouette analysis and the backward pass look up per step --
// at Franka 16 x 1080p (unshared vertices: V = 3 T) 168 MB of a 286 MB, bandwidth-bound launch.  The consumers now
// transform the object-space vertex themselves: the same fma chain (transform_vertex) on the same matrix (mvp[b][l], which
// the vertex kernel publishes) gives the same bits.  VbLazy is what travels (two pointers); VbVerts holds the matrix in
// scalar registers for the short stretch in which vertices are looked up.
struct VbLazy {
    const float* verts;  // [V][3] object-space vertices
    const float* M;      // mvp[b][l], 16 floats: the job's (view, link) -- wave-uniform
    const float4* pc;    // the view's clip-space vertices (posc + b V) where the plan keeps them (LAZY = false), else NULL
};
// LAZY = true: the matrix in scalar registers, a vertex = three loads + twelve fmas; false: a vertex = one 16-byte load.
// A template, not a run-time switch: the sixteen scalars of the lazy form cost the job kernel -- which has six registers to
// spare -- 19 more spilled VGPRs (8 views: 41.3 -> 44.8 us) whether they are used or not, so the plan picks the instantiation:
// lazy where vertices outnumber what is looked up by far (unshared vertices, V > 1.5 T: Franka 16 x 1080p, vertex stage
// 64.8 -> 46.8 us, step 175.5 -> 163.1 us), eager otherwise.
template <bool LAZY>
struct VbVertsT;
template <>
struct VbVertsT<true> {
    const float* verts;
    float M[16];
    __device__ __forceinline__ float4 operator[](int v) const {
        const float* a = verts + 3 * (size_t)v;
        return transform_vertex(M, a[0], a[1], a[2]);
    }
};
template <>
struct VbVertsT<false> {
    const float4* pc;
    __device__ __forceinline__ float4 operator[](int v) const { return pc[v]; }
};
template <bool LAZY>
__device__ __forceinline__ VbVertsT<LAZY> vb_verts(const VbLazy& z);
template <>
__device__ __forceinline__ VbVertsT<true> vb_verts<true>(const VbLazy& z) {
    VbVertsT<true> r;
    r.verts = z.verts;
#pragma unroll
    for (int k = 0; k < 16; k++) r.M[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(z.M[k])));
    return r;
}
template <>
__device__ __forceinline__ VbVertsT<false> vb_verts<false>(const VbLazy& z) {
    VbVertsT<false> r;
    r.pc = z.pc;
    return r;
}

// What stage 2 has to leave behind for a (view, link, region) is (a) which region pixels the link covers and (b) the
// nearest triangle at those covered pixels that have an uncovered 4-neighbour: only pairs of one covered and one
// uncovered pixel reach the silhouette analysis (with constant colour inside a link a blend between two covered pixels
// is alpha * (1 - 1) = 0 in value and in gradient), and the analysis looks at the covered pixel's triangle.  So the
// rasterizer works COVERAGE FIRST: the walker ORs 4-pixel coverage masks into a bitmap (one 64-bit word per region row)
// and appends the covered units to a deferred list; when the job's coverage is complete (or the list is full) the
// list is filtered against the pixels that can still matter and only the survivors -- typically a sixth of the
// fragments -- are depth tested (one IEEE division per pixel, a 64-bit LDS atomic min each).  Filtering against a PARTIAL
// coverage is conservative: a pixel that is interior to the partial coverage stays interior, so what a partial flush
// drops could never have been looked at.
//
// A covered pixel is only drawn if its depth z/w lies in [-1, 1] (depth_test_write in ehr_raster_core.h, the oracle's
// z-buffer loop): the vertex kernel marks a triangle SAFE (kind 0) when that holds for every pixel centre its snapped
// outline can cover -- vertex depths away from the planes by more than the plane's screen-space depth gradient over the
// snapping distance plus the evaluation's rounding (see vb_depth_safe) -- which is every triangle of a robot in front
// of the camera.  The others (kind 2: edge-on slivers, geometry at the far plane) take the same walker, but their
// units do not enter the bitmap: they are always depth tested, and a pixel that passes sets its coverage bit then.
#define VB_SPAN_GW 4                   // boxes from this many 4-pixel units per row are walked by rows (solved spans), not by units
constexpr int VB_DL = 640;             // deferred units per wave (LDS); a full list is flushed against the partial coverage
constexpr int VB_SQ = 256;             // ring of culling survivors per wave (LDS): a whole group of candidate clusters' worth
constexpr unsigned VB_ID_COVERED = 0xfffffffeu;  // id of a covered pixel whose triangle nobody will ask for
constexpr u64 VB_ROW_MASK = (1ull << VB_RW) - 1ull;

struct alignas(16) VbRaster {  // staging area of one rasterizer round (64 candidate triangles)
    int e[64][3];          // edge functions at the first pixel of the job's box inside the region
    unsigned dxy[64][3];   // dX | dY << 16 of the three edges
    unsigned box[64];      // box inside the region: x0 | y0 << 8 | w << 16 | h << 24 (region-relative)
    unsigned ent[64];      // deferred-list entry of this triangle without pixel and mask: flag << 13 | link-relative slot << 14
    int pre[65];           // exclusive prefix of the jobs' work units (+ total)
};
struct alignas(16) VbWaveLds {   // per wave of the job kernel
    u64 key[VB_RN];              // depth/id of the region's pixels: ordered(z/w) << 32 | triangle, all-ones = never tested
    u64 cov[VB_RH];              // coverage bitmap, one word per region row (bit x = region column x)
    u64 need[VB_RH];             // flush: covered pixels with an uncovered 4-neighbour
    u64 intr[VB_RH];             // rounds: covered pixels whose four neighbours are covered too (as of the round's start)
    u64 intr_and[3][VB_RH];      // ... AND-ed over the rows r .. r + 2^k - 1 (k = 1, 2, 3; past the last row: all ones)
    VbRaster R;
    unsigned dl[VB_DL];          // deferred units: pixel (9 bits) | 4-bit coverage << 9 | R.ent
    unsigned sq[VB_SQ];          // survivors of the box culling waiting for a full round: record slots (ring)
    int bad;                     // scoring op: a flagged unit's pixel was drawn with a depth <= 0 (coverage cannot decide)
};

// z/w at the centre of pixel (ix, iy) from the triangle's clip-space vertices, the oracle's arithmetic
// (depth_test_write); true if the pixel is drawn (depth inside [-1, 1]), and then the z-buffer is updated.
// (*nonpos, optional: set if a drawn pixel's depth is <= 0 -- the scoring op's mask is "depth of the nearest fragment > 0")
__device__ __forceinline__ bool vb_depth_test(const float4 p[3], int t, int ix, int iy, int W, int H, u64* slot,
                                              bool* nonpos = nullptr) {
    const float xs = 2.f / (float)W, xo = 1.f / (float)W - 1.f;
    const float ys = 2.f / (float)H, yo = 1.f / (float)H - 1.f;
    const float fx = (float)ix * xs + xo;
    const float fy = (float)iy * ys + yo;
    float a0, a1, a2;
    eval_pixel(p, fx, fy, a0, a1, a2);
    const float zw = eval_zw(p, a0, a1, a2);
    if (zw >= -1.f && zw <= 1.f) {
        if (nonpos) {
            if (!(zw > 0.f)) *nonpos = true;
        } else {
            atomicMin(slot, ((u64)ord_key(zw) << 32) | (unsigned)t);
        }
        return true;
    }
    return false;
}

// Static per-cluster-slot table (plan time): the three vertex ids and the triangle id of every cluster slot, so that a
// deferred unit finds its clip-space vertices (posc) with one 16-byte gather + three.
struct VbSlotIdx {
    const int4* cvidx;  // [NC * 64] {v0, v1, v2, triangle}; padding slots hold {0, 0, 0, -1}
};

// General path, whole wave per triangle, wave-uniform arguments: near-plane clipping, 64-bit edge functions, immediate
// depth test.  Rare (triangles crossing the near plane or spanning more than 512 pixels); only compiled into
// vb_job_slow, which redoes a job in which the lean code met such a triangle.
__device__ __forceinline__ void vb_raster_wide(float4 pa, float4 pb, float4 pc, int t, int W, int H, VbRegion rg, int rx0,
                                            int ry0, u64* key, u64* cov) {
    const int lane = lane_id();
    const float4 p[3] = {pa, pb, pc};
    const ClipPoly c = clip_near_poly(p);
    for (int s = 0; s + 2 < c.n; s++) {
        Coverage cv = (s == 0) ? setup_coverage(c.q0, c.q1, c.q2, W, H) : setup_coverage(c.q0, c.q2, c.q3, W, H);
        if (!cv.valid) continue;
        const int bx0 = max(cv.ix0, rg.x0), by0 = max(cv.iy0, rg.y0);
        const int bx1 = min(cv.ix1, rg.x1), by1 = min(cv.iy1, rg.y1);
        if (bx0 > bx1 || by0 > by1) continue;
        const int bw = bx1 - bx0 + 1, npx = bw * (by1 - by0 + 1);
        const EdgeEval ee = setup_edges(cv, bx0, by0, W, H);
        for (int i0 = 0; i0 < npx; i0 += 64) {
            const int i = i0 + lane;
            if (i < npx) {
                const int dy = i / bw, dx = i - dy * bw;
                const i64 e0 = ee.e[0] + dx * ee.sx[0] + dy * ee.sy[0];
                const i64 e1 = ee.e[1] + dx * ee.sx[1] + dy * ee.sy[1];
                const i64 e2 = ee.e[2] + dx * ee.sx[2] + dy * ee.sy[2];
                if ((e0 | e1 | e2) >= 0) {
                    const int ix = bx0 + dx, iy = by0 + dy;
                    if (vb_depth_test(p, t, ix, iy, W, H, &key[(iy - ry0) * VB_RW + (ix - rx0)]))
                        atomicOr((unsigned long long*)&cov[iy - ry0], 1ull << (ix - rx0));
                }
            }
        }
    }
}

// Flush of the deferred list (n entries): the pixels that can still matter under the CURRENT coverage (`cov`, complete
// or partial; shared by the four waves of a workgroup in the heavy-job phase) are the covered ones with an uncovered
// 4-neighbour inside the region; entries that touch none of them are dropped, the others are depth tested at exactly
// those pixels.  Units of unsafe triangles (flag) are always tested, at all their pixels, and set their coverage bits.
// COVER (scoring op): the list holds flagged units only; a pixel that passes the depth-range test is covered, and one whose
// depth is not positive raises *bad (the coverage-only chain cannot decide that pixel: the caller falls back).
template <bool COVER = false, bool LAZY = false>
__device__ __forceinline__ void vb_flush(VbWaveLds& S, u64* key, u64* cov, int n, const VbLazy& pvz,
                                      const int4* __restrict__ cvidx_link, int W, int H, int rx0, int ry0) {
    const int lane = lane_id();
    VB_WAVE_SYNC();
    if (lane < VB_RH) {
        const u64 c = cov[lane];
        const u64 up = (lane + 1 < VB_RH) ? cov[lane + 1] : VB_ROW_MASK;
        const u64 dn = (lane > 0) ? cov[lane - 1] : VB_ROW_MASK;
        // neighbour x + 1 is bit x of c >> 1, neighbour x - 1 bit x of c << 1; past the region's edge counts as covered
        const u64 inner = ((c >> 1) | (1ull << (VB_RW - 1))) & ((c << 1) | 1ull) & up & dn;
        S.need[lane] = c & ~inner & VB_ROW_MASK;
    }
    VB_WAVE_SYNC();
    int nk = 0;  // wave-uniform
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        unsigned e = 0;
        bool keep = false;
        if (i < n) {
            e = S.dl[i];
            const int pix = e & 511u, row = vb_div_rw(pix), col = pix - row * VB_RW;
            const unsigned m4 = (e >> 9) & 15u;
            const unsigned m = (e & (1u << 13)) ? m4 : (m4 & (unsigned)(S.need[row] >> col));
            keep = m != 0;
            e = (e & ~(15u << 9)) | (m << 9);
        }
        const u64 km = __ballot(keep);
        if (keep) S.dl[nk + vb_mbcnt(km)] = e;  // in place: nk <= base, and this round's reads are done
        nk += __popcll(km);
    }
    VB_WAVE_SYNC();
    const VbVertsT<LAZY> pv = vb_verts<LAZY>(pvz);  // (lazy: the matrix in scalar registers for the tests below)
    for (int base = 0; base < nk; base += 64) {
        const int i = base + lane;
        if (i < nk) {
            const unsigned e = S.dl[i];
            const int4 vi = cvidx_link[e >> 14];
            const float4 p[3] = {pv[vi.x], pv[vi.y], pv[vi.z]};
            const int pix = e & 511u, row = vb_div_rw(pix), col = pix - row * VB_RW;
            const unsigned m = (e >> 9) & 15u;
            const bool flag = (e >> 13) & 1u;
            // (one pass per set bit of the fullest mask in the wave: after the filter a unit has one or two pixels left)
            unsigned drawn = 0, mm = m;
            while (mm) {
                const int k = __ffs(mm) - 1;
                mm &= mm - 1;
                bool nonpos = false;
                if (vb_depth_test(p, vi.w, rx0 + col + k, ry0 + row, W, H, &key[pix + k], COVER ? &nonpos : nullptr)) drawn |= 1u << k;
                if (COVER && nonpos) S.bad = 1;
            }
            if (flag && drawn) atomicOr((unsigned long long*)&cov[row], (u64)drawn << col);
        }
    }
    VB_WAVE_SYNC();
}

// One round of the wave-level rasterizer: up to 64 candidate triangles (lane `sv` holds one: record slot `slot` of the
// view, `srel` the same relative to the link's first cluster slot) are rasterized into the job's coverage bitmap and
// their covered 4-pixel units appended to the wave's deferred list (n entries on entry; returns the new count).  The
// triangles' boxes (clamped to the region) are cut into units of 4 horizontally adjacent pixels; a wave-wide prefix sum
// splits the concatenated unit sequence EVENLY over the 64 lanes (a third of the candidates have boxes above 16
// pixels, so one lane per triangle would leave most lanes idle) and each lane walks its contiguous run stepping 32-bit
// edge functions.  Fed by the per-triangle records of the vertex kernel; nothing but LDS is touched inside the walk.
// COVER: the coverage-only form of the scoring op's chain -- no deferred units, no depth anywhere: every triangle must be
// of the class "coverage decides" (kind 0 under the positive-depth test), anything else aborts the job (-1); what is
// already covered (not just interior) hides a box.
template <bool WIDE, bool COVER = false, bool LAZY = false>
__device__ __forceinline__ int vb_raster_round(bool sv, size_t slot, unsigned srel, const VbRecs& rc, const VbRegion& rg,
                                               int rx0, int ry0, int W, int H, VbWaveLds& S, u64* key, u64* cov, int n,
                                               const VbLazy& pv, const int4* __restrict__ cvidx_link, bool& full,
                                               int& cost, int qh) {
    VbRaster& R = S.R;
    const int lane = lane_id();
    int units = 0, srows = 0;
    bool wide = false;
    uint2 bx = VB_BOX_EMPTY;
    int4 r0 = make_int4(0, 0, 0, 0), r1 = r0;
    if (sv) {
        bx = rc.tbox[slot];
        r0 = rc.trec[2 * slot];
        r1 = rc.trec[2 * slot + 1];
    }
    // Interior of the coverage so far: covered pixels whose four neighbours (inside the region) are covered too.  Nobody
    // will ever ask which triangle is visible there, and coverage cannot change there: a triangle whose box lies inside
    // the interior is skipped, units inside it are not deferred, and a region that is all interior ends the job (the
    // inner tiles of a link seen from close by: a few large triangles cover everything, the other layers add nothing).
    bool has_in = false;
    {
        u64 in = 0;
        if (lane < VB_RH) {
            const u64 c = cov[lane];
            const u64 up = (lane + 1 < VB_RH) ? cov[lane + 1] : VB_ROW_MASK;
            const u64 dn = (lane > 0) ? cov[lane - 1] : VB_ROW_MASK;
            in = COVER ? (c & VB_ROW_MASK) : (c & ((c >> 1) | (1ull << (VB_RW - 1))) & ((c << 1) | 1ull) & up & dn & VB_ROW_MASK);
            S.intr[lane] = in;
        }
        {
            // a sparse table over the rows (lanes 0-9 hold the rows; lanes 10-15 the identity): "is this box inside the
            // interior" is then two reads and an AND per triangle instead of a pass over all ten rows
            unsigned lo = (lane < VB_RH) ? (unsigned)in : 0xffffffffu, hi = (lane < VB_RH) ? (unsigned)(in >> 32) : 0xffffffffu;
#define VB_ROWS_AND(k, ctrl)                                                                              \
    lo &= (unsigned)__builtin_amdgcn_update_dpp(-1, (int)lo, ctrl, 0xf, 0xf, false);                      \
    hi &= (unsigned)__builtin_amdgcn_update_dpp(-1, (int)hi, ctrl, 0xf, 0xf, false);                      \
    if (lane < VB_RH) S.intr_and[k][lane] = (u64)lo | ((u64)hi << 32);
            VB_ROWS_AND(0, 0x101)  // row_shl:1: lane i <- lane i + 1
            VB_ROWS_AND(1, 0x102)  // row_shl:2
            VB_ROWS_AND(2, 0x104)  // row_shl:4
#undef VB_ROWS_AND
        }
        if (__ballot(lane < VB_RH && in != VB_ROW_MASK) == 0) {
            full = true;
            return n;
        }
        has_in = __ballot(lane < VB_RH && in != 0ull) != 0;  // (no interior yet -- most first rounds --: nothing can be hidden)
        VB_WAVE_SYNC();
    }
    if (sv) {
        if (r1.w == 1) {
            wide = true;
        } else if (LAZY) {
            // (the lazy instantiation has no register to spare while the records are live: it stages the clamped box as it
            // is and trims it from the staged values, below)
            const int ix0 = bx.x & 0xffffu, iy0 = bx.x >> 16, ix1 = bx.y & 0xffffu, iy1 = bx.y >> 16;
            const int cx0 = max(ix0, rg.x0), cy0 = max(iy0, rg.y0);
            const int bw = min(ix1, rg.x1) - cx0 + 1, bh = min(iy1, rg.y1) - cy0 + 1;  // > 0: the boxes overlap
            const unsigned w[3] = {(unsigned)r0.w, (unsigned)r1.x, (unsigned)r1.y};
            const int ev[3] = {r0.x, r0.y, r0.z};
            const int ox = cx0 - ix0, oy = cy0 - iy0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int dX = (int)(short)(w[k] & 0xffffu), dY = (int)(short)(w[k] >> 16);
                R.e[lane][k] = ev[k] - 16 * __mul24(dY, ox) + 16 * __mul24(dX, oy);  // (24-bit operands: full-rate multiplies)
                R.dxy[lane][k] = w[k];
            }
            R.box[lane] = (unsigned)(cx0 - rx0) | ((unsigned)(cy0 - ry0) << 8) | ((unsigned)bw << 16) | ((unsigned)bh << 24);
            R.ent[lane] = (srel << 14) | ((r1.w == 2) ? (1u << 13) : 0u);
        } else {
            R.ent[lane] = (srel << 14) | ((r1.w == 2) ? (1u << 13) : 0u);
            const int ix0 = bx.x & 0xffffu, iy0 = bx.x >> 16, ix1 = bx.y & 0xffffu, iy1 = bx.y >> 16;
            int cx0 = max(ix0, rg.x0), cy0 = max(iy0, rg.y0);
            int bw = min(ix1, rg.x1) - cx0 + 1, bh = min(iy1, rg.y1) - cy0 + 1;  // > 0: the boxes overlap
            const unsigned w[3] = {(unsigned)r0.w, (unsigned)r1.x, (unsigned)r1.y};
            const int ev[3] = {r0.x, r0.y, r0.z};
            const int ox = cx0 - ix0, oy = cy0 - iy0;
            int e[3], sx[3], sy[3], m[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                sx[k] = -16 * (int)(short)(w[k] >> 16);
                sy[k] = 16 * (int)(short)(w[k] & 0xffffu);
                e[k] = ev[k] + __mul24(sx[k], ox) + __mul24(sy[k], oy);  // (24-bit operands: full-rate multiplies)
                R.dxy[lane][k] = w[k];
            }
            // Box trim: the clamped box is often a corner of the triangle's own box which the triangle barely reaches, or
            // misses (a quarter of the triangles that get here cover no pixel of the region, two thirds of the units hold no
            // covered pixel).  Cut it down to the rows, then to the columns of those rows, on which all three edges can
            // still be >= 0 (m[k]: edge k's largest value across the other axis), and move the edge values to its new
            // first pixel.  The walkers test the same integers on fewer pixels, none of them covered: same bits.
            int t0, t1;
#pragma unroll
            for (int k = 0; k < 3; k++) m[k] = e[k] + max(0, __mul24(sx[k], bw - 1));
            vb_trim_range(m, sy, bh, t0, t1);
            cy0 += t0;
            bh = t1 - t0 + 1;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                e[k] += __mul24(sy[k], t0);
                m[k] = e[k] + max(0, __mul24(sy[k], bh - 1));
            }
            vb_trim_range(m, sx, bw, t0, t1);
            cx0 += t0;
            bw = t1 - t0 + 1;
            const bool empty = bh <= 0 || bw <= 0;  // the triangle misses the region: as good as hidden
#pragma unroll
            for (int k = 0; k < 3; k++) R.e[lane][k] = e[k] + __mul24(sx[k], t0);
            R.box[lane] = (unsigned)(cx0 - rx0) | ((unsigned)(cy0 - ry0) << 8) | ((unsigned)bw << 16) | ((unsigned)bh << 24);
            const u64 bm = ((1ull << bw) - 1ull) << (cx0 - rx0);
            bool hidden = has_in || empty;
            if (has_in && !empty) {
                // rows y0 .. y0 + bh - 1 = the 2^k rows from y0 and the 2^k rows up to the last, k = floor(log2(bh))
                const int y0r = cy0 - ry0, k = 31 - __clz(bh);
                const u64* const tab = (k == 0) ? S.intr : S.intr_and[k - 1];
                const u64 all = tab[y0r] & tab[y0r + bh - (1 << k)];
                hidden = (all & bm) == bm;
            }
            // a box of VB_SPAN_GW or more units per row goes to the span walker: work = its rows
            if (!hidden) {
                if (((bw + 3) >> 2) >= VB_SPAN_GW && !(COVER && r1.w == 2))  // (coverage-only form: flagged boxes stay with the units)
                    srows = bh;
                else
                    units = ((bw + 3) >> 2) * bh;
            }
        }
    }
    if ((!WIDE || COVER) && __ballot(wide)) return -1;  // the lean instantiation hands the whole job to vb_job_slow
    if (LAZY && sv && !wide) {
        // the box trim of the eager form above, on the staged values: the records' registers are dead here (this way round
        // the lazy instantiation spills 21 VGPRs, the other way round 33; the eager one 6 against 8)
        const unsigned b4 = R.box[lane];
        int x0r = b4 & 255, y0r = (b4 >> 8) & 255, bw = (b4 >> 16) & 255, bh = b4 >> 24;
        int e[3], sx[3], sy[3], m[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const unsigned w = R.dxy[lane][k];
            sx[k] = -16 * (int)(short)(w >> 16);
            sy[k] = 16 * (int)(short)(w & 0xffffu);
            e[k] = R.e[lane][k];
            m[k] = e[k] + max(0, __mul24(sx[k], bw - 1));
        }
        int t0, t1;
        vb_trim_range(m, sy, bh, t0, t1);
        y0r += t0;
        bh = t1 - t0 + 1;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            e[k] += __mul24(sy[k], t0);
            m[k] = e[k] + max(0, __mul24(sy[k], bh - 1));
        }
        vb_trim_range(m, sx, bw, t0, t1);
        x0r += t0;
        bw = t1 - t0 + 1;
#pragma unroll
        for (int k = 0; k < 3; k++) R.e[lane][k] = e[k] + __mul24(sx[k], t0);
        R.box[lane] = (unsigned)x0r | ((unsigned)y0r << 8) | ((unsigned)bw << 16) | ((unsigned)bh << 24);
        bool hidden = bh <= 0 || bw <= 0;  // the triangle misses the region: as good as hidden
        if (has_in && !hidden) {
            // rows y0 .. y0 + bh - 1 = the 2^k rows from y0 and the 2^k rows up to the last, k = floor(log2(bh))
            const u64 bm = ((1ull << bw) - 1ull) << x0r;
            const int k = 31 - __clz(bh);
            const u64* const tab = (k == 0) ? S.intr : S.intr_and[k - 1];
            const u64 all = tab[y0r] & tab[y0r + bh - (1 << k)];
            hidden = (all & bm) == bm;
        }
        // a box of VB_SPAN_GW or more units per row goes to the span walker: work = its rows
        if (!hidden) {
            if (((bw + 3) >> 2) >= VB_SPAN_GW && !(COVER && (R.ent[lane] & (1u << 13))))  // (coverage-only form: flagged boxes stay with the units)
                srows = bh;
            else
                units = ((bw + 3) >> 2) * bh;
        }
    }
    // one scan for both walkers: units in the low half (<= 64 x 90), span rows in the high half (<= 64 x 10)
    const int packed = units | (srows << 16);
    const int incl = vb_scan_add(packed);
    const int Ptot = vb_readlane(incl, 63);
    const int Stot = Ptot & 0xffff, Wtot = Ptot >> 16;
    const u64 nzu = __ballot(units > 0), nzs = __ballot(srows > 0);  // triangles with units / with span rows
    cost += Stot + 3 * Wtot + 256;  // what the job costs a wave: a step per 64 units, three per 64 span rows, about four per round
    if (Ptot > 0) {
        R.pre[lane] = incl - packed;
        if (lane == 63) R.pre[64] = Ptot;
        VB_WAVE_SYNC();
        const int K = (Stot + 63) >> 6;
        const int start = __mul24(lane, K), end = min(start + K, Stot);
        int j = 0, bw = 1, bh = 1, gw = 1, gx = 0, dy = 0, crow = 0, ccol0 = 0;
        unsigned eb = 0, lastm = 15u;  // lastm: the pixels of a row's last unit that lie inside the box
        int e0 = -1, e1 = -1, e2 = -1, sx0 = 0, sx1 = 0, sx2 = 0, sy0 = 0, sy1 = 0, sy2 = 0, er0 = 0, er1 = 0, er2 = 0;
        // Which triangle does a lane start in?  Asked the other way round: triangle j's units begin at pre[j]; the first
        // lane to start at or after that is ceil(pre[j] / K), and if that start still lies inside the triangle, j puts its
        // number there.  A lane's triangle is the last number at or below its own place: a max-scan.  (One LDS round
        // trip instead of the six of a binary search over pre[] -- in every round of every job.  The table is the half of
        // the survivor ring this round has just emptied.)
        unsigned* const own = S.sq + qh;
        {
            const float invK = __builtin_amdgcn_rcpf((float)K);
            const int pj = (incl - packed) & 0xffff, uj = packed & 0xffff;
            const int wf = vb_div_small(pj + K - 1, invK);
            own[lane] = 0u;
            if (uj > 0 && __mul24(wf, K) < pj + uj) own[wf] = (unsigned)lane + 1u;
            VB_WAVE_SYNC();
            j = vb_scan_max((int)own[lane]) - 1;
        }
        if (start < end) {
            const unsigned b4 = R.box[j];
            ccol0 = b4 & 255;
            const int y0r = (b4 >> 8) & 255;
            bw = (b4 >> 16) & 255;
            bh = b4 >> 24;
            gw = (bw + 3) >> 2;
            lastm = (1u << (bw - 4 * (gw - 1))) - 1u;
            eb = R.ent[j];
            const unsigned w0 = R.dxy[j][0], w1 = R.dxy[j][1], w2 = R.dxy[j][2];
            sx0 = -16 * (int)(short)(w0 >> 16); sy0 = 16 * (int)(short)(w0 & 0xffffu);
            sx1 = -16 * (int)(short)(w1 >> 16); sy1 = 16 * (int)(short)(w1 & 0xffffu);
            sx2 = -16 * (int)(short)(w2 >> 16); sy2 = 16 * (int)(short)(w2 & 0xffffu);
            const int o = start - (R.pre[j] & 0xffff);
            dy = vb_div_small(o, __builtin_amdgcn_rcpf((float)gw));
            gx = o - __mul24(dy, gw);  // (|s*| < 2^20, dy < 2^7, gx < 4: 24-bit operands, full-rate multiplies)
            er0 = R.e[j][0] + __mul24(dy, sy0);
            er1 = R.e[j][1] + __mul24(dy, sy1);
            er2 = R.e[j][2] + __mul24(dy, sy2);
            e0 = er0 + __mul24(4 * gx, sx0);
            e1 = er1 + __mul24(4 * gx, sx1);
            e2 = er2 + __mul24(4 * gx, sx2);
            crow = y0r + dy;
        }
        for (int it0 = 0; it0 < K;) {
            // the deferred list takes at most 64 entries per step: walk as many steps as it has room for
            const int room = (VB_DL - n) >> 6;
            if (room == 0) {
                vb_flush<COVER, LAZY>(S, key, cov, n, pv, cvidx_link, W, H, rx0, ry0);
                n = 0;
                continue;
            }
            const int it1 = min(K, it0 + room);
#pragma nounroll
            for (int it = it0; it < it1; it++) {
                const bool act = start + it < end;
                unsigned m4 = 0;
                if (act) {
                    const int a1 = e0 + sx0, a2 = a1 + sx0, a3 = a2 + sx0;
                    const int b1 = e1 + sx1, b2 = b1 + sx1, b3 = b2 + sx1;
                    const int c1 = e2 + sx2, c2 = c1 + sx2, c3 = c2 + sx2;
                    // a pixel is inside if none of its three edge values is negative: the four sign bits, funnelled into
                    // one word by three double-word shifts
                    unsigned sg = (unsigned)(a3 | b3 | c3) >> 31;
                    sg = __builtin_amdgcn_alignbit(sg, (unsigned)(a2 | b2 | c2), 31);
                    sg = __builtin_amdgcn_alignbit(sg, (unsigned)(a1 | b1 | c1), 31);
                    sg = __builtin_amdgcn_alignbit(sg, (unsigned)(e0 | e1 | e2), 31);
                    m4 = ~sg & ((gx == gw - 1) ? lastm : 15u);  // (the row's last unit: only its pixels inside the box)
                }
                const bool inside = m4 != 0;
                const u64 m = __ballot(inside);
                if (COVER && !(__ballot(inside && (eb & (1u << 13))))) {
                    if (inside) atomicOr((unsigned long long*)&cov[crow], (u64)m4 << (ccol0 + 4 * gx));
                } else if (m) {
                    // deferred for a depth test: the unit's covered pixels outside the interior (as of the round's start)
                    unsigned md = 0;
                    if (inside) {
                        const int ccol = ccol0 + 4 * gx;
                        if (!(eb & (1u << 13))) atomicOr((unsigned long long*)&cov[crow], (u64)m4 << ccol);
                        md = COVER ? ((eb & (1u << 13)) ? m4 : 0u) : (m4 & ~(unsigned)(S.intr[crow] >> ccol));
                    }
                    const u64 ma = __ballot(md != 0);
                    if (md) S.dl[n + vb_mbcnt(ma)] = eb | (unsigned)(__mul24(crow, VB_RW) + ccol0 + 4 * gx) | (md << 9);
                    n += __popcll(ma);
                }
                if (act && start + it + 1 < end) {
                    gx++;
                    e0 += 4 * sx0;
                    e1 += 4 * sx1;
                    e2 += 4 * sx2;
                    if (gx == gw) {
                        gx = 0;
                        dy++;
                        crow++;
                        er0 += sy0;
                        er1 += sy1;
                        er2 += sy2;
                        e0 = er0;
                        e1 = er1;
                        e2 = er2;
                        if (dy == bh) {  // next job with a non-empty box
                            j = vb_next_set(nzu, j);
                            const unsigned b4 = R.box[j];
                            ccol0 = b4 & 255;
                            crow = (b4 >> 8) & 255;
                            bw = (b4 >> 16) & 255;
                            bh = b4 >> 24;
                            gw = (bw + 3) >> 2;
                            lastm = (1u << (bw - 4 * (gw - 1))) - 1u;
                            eb = R.ent[j];
                            const unsigned w0 = R.dxy[j][0], w1 = R.dxy[j][1], w2 = R.dxy[j][2];
                            sx0 = -16 * (int)(short)(w0 >> 16); sy0 = 16 * (int)(short)(w0 & 0xffffu);
                            sx1 = -16 * (int)(short)(w1 >> 16); sy1 = 16 * (int)(short)(w1 & 0xffffu);
                            sx2 = -16 * (int)(short)(w2 >> 16); sy2 = 16 * (int)(short)(w2 & 0xffffu);
                            er0 = e0 = R.e[j][0];
                            er1 = e1 = R.e[j][1];
                            er2 = e2 = R.e[j][2];
                            dy = 0;
                        }
                    }
                }
            }
            it0 = it1;
        }
        // ---- span walker: the triangles whose box is VB_SPAN_GW or more units wide (long thin ones mostly: 17 % of the rows
        //      but 45 % of the units, and most of those units empty).  A lane takes rows instead of units and solves each
        //      row's covered span [lo, hi] from the three edge functions: floor(E / |sx|) from a float estimate, made exact by
        //      one integer step (the estimate is within 1e-5 of the quotient wherever the result matters, |q| <= 40).  The
        //      span goes into the bitmap with one OR; its 4-pixel units that are not interior are deferred as usual.
        if (Wtot > 0) {
            const int K2 = (Wtot + 63) >> 6;
            const int s2 = __mul24(lane, K2), e2 = min(s2 + K2, Wtot);
            int j = 0, bw = 1, bh = 1, dy = 0, crow = 0, ccol0 = 0;
            unsigned eb = 0;
            int sx0 = 0, sx1 = 0, sx2 = 0, sy0 = 0, sy1 = 0, sy2 = 0, er0 = 0, er1 = 0, er2 = 0;
            float iv0 = 0.f, iv1 = 0.f, iv2 = 0.f;
            auto load_tri = [&](int jj) {
                const unsigned b4 = R.box[jj];
                ccol0 = b4 & 255;
                crow = (b4 >> 8) & 255;
                bw = (b4 >> 16) & 255;
                bh = b4 >> 24;
                eb = R.ent[jj];
                const unsigned w0 = R.dxy[jj][0], w1 = R.dxy[jj][1], w2 = R.dxy[jj][2];
                sx0 = -16 * (int)(short)(w0 >> 16); sy0 = 16 * (int)(short)(w0 & 0xffffu);
                sx1 = -16 * (int)(short)(w1 >> 16); sy1 = 16 * (int)(short)(w1 & 0xffffu);
                sx2 = -16 * (int)(short)(w2 >> 16); sy2 = 16 * (int)(short)(w2 & 0xffffu);
                iv0 = __builtin_amdgcn_rcpf((float)abs(sx0));
                iv1 = __builtin_amdgcn_rcpf((float)abs(sx1));
                iv2 = __builtin_amdgcn_rcpf((float)abs(sx2));
                er0 = R.e[jj][0];
                er1 = R.e[jj][1];
                er2 = R.e[jj][2];
                dy = 0;
            };
            {
                const float invK = __builtin_amdgcn_rcpf((float)K2);
                const int pj = (incl - packed) >> 16, uj = packed >> 16;
                const int wf = vb_div_small(pj + K2 - 1, invK);
                VB_WAVE_SYNC();  // (the unit walker's reads of the table are complete)
                own[lane] = 0u;
                if (uj > 0 && __mul24(wf, K2) < pj + uj) own[wf] = (unsigned)lane + 1u;
                VB_WAVE_SYNC();
                j = vb_scan_max((int)own[lane]) - 1;
            }
            if (s2 < e2) {
                load_tri(j);
                dy = s2 - (R.pre[j] >> 16);
                er0 += __mul24(dy, sy0);
                er1 += __mul24(dy, sy1);
                er2 += __mul24(dy, sy2);
                crow += dy;
            }
#pragma nounroll
            for (int it = 0; it < K2;) {
                const bool act = s2 + it < e2;
                int lo = 0, hi = -1;
                if (act) {
                    hi = bw - 1;
#define VB_SPAN_EDGE(E, SX, IV)                                                                    \
    if ((SX) == 0) {                                                                               \
        if ((E) < 0) hi = -1;                                                                      \
    } else {                                                                                       \
        const int asx = abs(SX);                                                                   \
        const float qf = fminf(fmaxf(floorf((float)(E) * (IV)), -40.f), 40.f);                     \
        int u = (int)qf;                                                                           \
        const int t = (E) - __mul24(u, asx);                                                       \
        u += (t < 0) ? -1 : ((t >= asx) ? 1 : 0);                                                  \
        if ((SX) > 0)                                                                              \
            lo = max(lo, -u);                                                                      \
        else                                                                                       \
            hi = min(hi, u);                                                                       \
    }
                    VB_SPAN_EDGE(er0, sx0, iv0)
                    VB_SPAN_EDGE(er1, sx1, iv1)
                    VB_SPAN_EDGE(er2, sx2, iv2)
#undef VB_SPAN_EDGE
                }
                u64 rm = 0;
                int c0 = 0;
                if (lo <= hi) {
                    c0 = ccol0 + lo;
                    rm = ((1ull << (hi - lo + 1)) - 1ull) << c0;
                }
                if (COVER) {
                    if (rm) atomicOr((unsigned long long*)&cov[crow], rm);
                    if (act && s2 + it + 1 < e2) {
                        dy++;
                        crow++;
                        er0 += sy0;
                        er1 += sy1;
                        er2 += sy2;
                        if (dy == bh) {
                            j = vb_next_set(nzs, j);
                            load_tri(j);
                        }
                    }
                    it++;
                    continue;
                }
                // deferred: the span's units (aligned to the span's first pixel) with a pixel outside the interior
                const u64 md = rm ? ((rm & ~S.intr[crow]) >> c0) : 0ull;
                u64 nz = (md | (md >> 1) | (md >> 2) | (md >> 3)) & 0x1111111111111111ull;
                const int cnt = __popcll(nz);
                const int inc = vb_scan_add(cnt);
                const int T = vb_readlane(inc, 63);
                if (n + T > VB_DL) {  // no room for this step's entries: flush, then take the step again
                    vb_flush<COVER, LAZY>(S, key, cov, n, pv, cvidx_link, W, H, rx0, ry0);
                    n = 0;
                    continue;
                }
                if (rm && !(eb & (1u << 13))) atomicOr((unsigned long long*)&cov[crow], rm);
                int pos = n + inc - cnt;
                while (nz) {
                    const int bpos = __ffsll((unsigned long long)nz) - 1;
                    nz &= nz - 1;
                    S.dl[pos++] = eb | (unsigned)(crow * VB_RW + c0 + bpos) | ((unsigned)((md >> bpos) & 15ull) << 9);
                }
                n += T;
                if (act && s2 + it + 1 < e2) {
                    dy++;
                    crow++;
                    er0 += sy0;
                    er1 += sy1;
                    er2 += sy2;
                    if (dy == bh) {  // next triangle of this class
                        j = vb_next_set(nzs, j);
                        load_tri(j);
                    }
                }
                it++;
            }
        }
        VB_WAVE_SYNC();  // the staging area is rewritten by the next round
    }
    if (WIDE) {  // rare: near-plane clipping / very large extents, one triangle at a time, depth tested at once
        u64 wm = __ballot(wide);
        while (wm) {
            const int s = __ffsll((unsigned long long)wm) - 1;
            wm &= wm - 1;
            const int4 vi = cvidx_link[vb_readlane((int)srel, s)];
            const VbVertsT<LAZY> pvv = vb_verts<LAZY>(pv);
            vb_raster_wide(pvv[vi.x], pvv[vi.y], pvv[vi.z], vi.w, W, H, rg, rx0, ry0, key, cov);
        }
    }
    return n;
}

// tiles (+ 1-pixel halo) a link's pixel box touches: the jobs of that (view, link)
// (halo = 0: the scoring op's coverage-only jobs, which look at their tile alone)
__device__ __forceinline__ bool vb_unit_tiles(const int* __restrict__ bx, int W, int H, int& tx0, int& ty0, int& nx, int& ny,
                                              int halo = 1) {
    const int x0 = bx[0], y0 = bx[1], x1 = bx[2], y1 = bx[3];
    if (x0 > x1 || y0 > y1) return false;
    tx0 = max(x0 - halo, 0) / EHR_TILE_W;
    ty0 = max(y0 - halo, 0) / EHR_TILE_H;
    nx = min(x1 + halo, W - 1) / EHR_TILE_W - tx0 + 1;
    ny = min(y1 + halo, H - 1) / EHR_TILE_H - ty0 + 1;
    return true;
}

constexpr int VB_CULL_BATCHES = 2;  // batches of 64 cluster boxes requested together
constexpr int VB_CULL_GROUP = 8;    // candidate clusters whose triangle boxes are requested together
// Kernel-wide arguments of a job's rasterizer (what vb_job_raster needs besides the job itself); both kernels that draw jobs
// assemble it from their own parameters.
struct VbJobArgs {
    const float* verts;   // [V][3] object-space vertices
    const float* mvp;     // [B][L][16] the chunk's (view, link) matrices: clip-space vertices are computed on demand (VbLazy) ...
    VbRecs rc;
    int NC, V, W, H, L;
    const int4* cvidx;    // [NC * 64] {v0, v1, v2, triangle} of every cluster slot
    const float4* posc;   // ... or read from here ([B][V]) where the plan keeps them (NULL: lazy)
    const int* lcoff;     // first cluster of every link (the job kernel: its copy in LDS)
};

// Culls the link's clusters and triangles against the job's region and rasterizes this wave's share of them into the
// job's coverage bitmap `cov_` / depth-id buffer `key_` (LDS, initialised by the caller).  share / nshare: the wave takes
// every nshare-th candidate cluster -- 0 / 1 for a job of its own, wave / 4 when the whole workgroup works on one heavy
// job.  The survivors' covered units are left in the wave's deferred list (dln entries on return): the caller flushes it
// once the job's coverage is complete.  Returns 1 if anything survived the culling, 0 if not, and -1 (lean
// instantiation only) if a survivor needs the general path: the caller then redoes the job with vb_job_slow.
template <bool WIDE, bool COVER = false, bool LAZY = false>
__device__ __forceinline__ int vb_job_raster(const VbJobArgs& A, VbWaveLds& W_, u64* key_, u64* cov_, int b, int l,
                                             const VbRegion& rg, int rx0, int ry0, int share, int nshare, int& nsurv,
                                             int& dln) {
    const int lane = lane_id();
    const int c0 = A.lcoff[l], c1 = A.lcoff[l + 1];
    const uint2* const cb = A.rc.cbox + (size_t)b * A.NC;
    const unsigned rlo = (unsigned)rg.x0 | ((unsigned)rg.y0 << 16), rhi = (unsigned)rg.x1 | ((unsigned)rg.y1 << 16);
    // Survivors of the triangle-box test are queued (record slots) until 64 are waiting, so that every round of
    // the rasterizer is full; the triangle boxes of up to VB_CULL_GROUP candidate clusters are fetched per round trip.
    const size_t vbase = (size_t)b * A.NC * 64;
    const VbLazy pv = {A.verts, A.mvp + ((size_t)b * A.L + l) * 16, A.posc ? A.posc + (size_t)b * A.V : nullptr};
    const int4* const cvl = A.cvidx + (size_t)c0 * 64;  // the link's first cluster slot
    const unsigned srel0 = (unsigned)c0 * 64u;
    bool full = false;   // set by a round that finds the whole region interior
    int qh = 0, qn = 0;  // wave-uniform ring state
    int cord = 0;        // running ordinal of the candidate clusters
    bool drawn = false;
    // The cluster boxes of VB_CULL_BATCHES x 64 clusters are requested together (one round trip under load is ~1-2 us, and
    // all but one of the xArm7's links have between 65 and 128 clusters), then the batches are worked off one by one.
    for (int cb0 = c0; cb0 < c1; cb0 += 64 * VB_CULL_BATCHES) {
        u64 cmk[VB_CULL_BATCHES];
        {
            uint2 bxk[VB_CULL_BATCHES];
#pragma unroll
            for (int k = 0; k < VB_CULL_BATCHES; k++) {
                const int c = cb0 + 64 * k + lane;
                bxk[k] = VB_BOX_EMPTY;
                if (c < c1) bxk[k] = cb[c];
            }
#pragma unroll
            for (int k = 0; k < VB_CULL_BATCHES; k++)
                cmk[k] = __ballot((bxk[k].x & 0xffffu) <= (rhi & 0xffffu) && (bxk[k].y & 0xffffu) >= (rlo & 0xffffu) &&
                                  (bxk[k].x >> 16) <= (rhi >> 16) && (bxk[k].y >> 16) >= (rlo >> 16));
        }
#pragma nounroll
        for (int kb = 0; kb < VB_CULL_BATCHES; kb++) {
            const int cbase = cb0 + 64 * kb;
            u64 cm = cmk[0];
#pragma unroll
            for (int kk = 1; kk < VB_CULL_BATCHES; kk++)
                if (kb == kk) cm = cmk[kk];
            if (!cm) continue;
            if (nshare > 1) {  // cooperative job: this wave takes every nshare-th candidate cluster
                u64 mine = 0;
                u64 all = cm;
                while (all) {
                    const u64 low = all & (~all + 1);
                    if ((cord++ % nshare) == share) mine |= low;
                    all ^= low;
                }
                cm = mine;
            }
            while (cm) {  // wave-uniform
                // A group of up to VB_CULL_GROUP candidate clusters: their triangle boxes in one round trip, the survivors
                // of ALL of them pushed in one unrolled pass when the ring has room for them (the rule: the ring holds 256),
                // then as many rounds as are full.  Masks and cluster numbers are scalar registers that die before the
                // first round starts.  (Per cluster -- read the mask back, test, push, count, test for a round -- the loop
                // was ~30 instructions x 33 k candidates a step, and 25 of the 94 kcycles of the jobs the kernel ends on.)
                // Only when the ring cannot take the whole group do they wait in the LANES of three vector registers
                // (lane k: entry k) and go in one by one, a round whenever 64 are waiting.
                int ccv = 0, ng = 0, knext = 0;
                unsigned mlo = 0, mhi = 0;
                {
                    int cks[VB_CULL_GROUP];
                    uint2 tb[VB_CULL_GROUP];
#pragma unroll
                    for (int k = 0; k < VB_CULL_GROUP; k++) {
                        tb[k] = VB_BOX_EMPTY;
                        cks[k] = 0;
                        if (cm) {
                            cks[k] = cbase + __ffsll((unsigned long long)cm) - 1;
                            cm &= cm - 1;
                            tb[k] = A.rc.tbox[vbase + (size_t)cks[k] * 64 + lane];
                            ng = k + 1;
                        }
                    }
                    u64 mk[VB_CULL_GROUP];
                    int total = 0;
#pragma unroll
                    for (int k = 0; k < VB_CULL_GROUP; k++) {
                        mk[k] = 0;
                        if (k < ng) {
                            mk[k] = __ballot((tb[k].x & 0xffffu) <= (rhi & 0xffffu) && (tb[k].y & 0xffffu) >= (rlo & 0xffffu) &&
                                             (tb[k].x >> 16) <= (rhi >> 16) && (tb[k].y >> 16) >= (rlo >> 16));
                            total += __popcll(mk[k]);
                        }
                    }
                    if (total == 0) continue;
                    drawn = true;
                    if (qn + total <= VB_SQ) {
#pragma unroll
                        for (int k = 0; k < VB_CULL_GROUP; k++) {
                            if (mk[k]) {
                                if ((mk[k] >> lane) & 1) W_.sq[(qh + qn + vb_mbcnt(mk[k])) & (VB_SQ - 1)] = (unsigned)(cks[k] * 64 + lane);
                                qn += __popcll(mk[k]);
                            }
                        }
                        knext = ng;
                    } else {
#pragma unroll
                        for (int k = 0; k < VB_CULL_GROUP; k++) {
                            ccv = (lane == k) ? cks[k] : ccv;
                            mlo = (lane == k) ? (unsigned)mk[k] : mlo;
                            mhi = (lane == k) ? (unsigned)(mk[k] >> 32) : mhi;
                        }
                    }
                }
                for (;;) {
                    // not unrolled, one call site: one copy of the rasterizer round (the kernel was 69 KB of code, more
                    // than the instruction cache two CUs share)
                    while (qn >= 64) {
                        VB_WAVE_SYNC();
                        const unsigned sl = W_.sq[(qh + lane) & (VB_SQ - 1)];
                        dln = vb_raster_round<WIDE, COVER, LAZY>(true, vbase + sl, sl - srel0, A.rc, rg, rx0, ry0, A.W, A.H, W_, key_, cov_, dln, pv, cvl, full, nsurv, qh);
                        if (dln < 0) return -1;
                        if (full) return 1;  // every pixel of the region is interior: nothing can change any more
                        qh = (qh + 64) & (VB_SQ - 1);
                        qn -= 64;
                    }
                    if (knext >= ng) break;
                    const u64 sm = (u64)(unsigned)__builtin_amdgcn_readlane((int)mlo, knext) | ((u64)(unsigned)__builtin_amdgcn_readlane((int)mhi, knext) << 32);
                    const int ck = __builtin_amdgcn_readlane(ccv, knext);
                    knext++;
                    if (sm) {
                        if ((sm >> lane) & 1) W_.sq[(qh + qn + vb_mbcnt(sm)) & (VB_SQ - 1)] = (unsigned)(ck * 64 + lane);
                        qn += __popcll(sm);
                    }
                }
            }
        }
    }
    if (qn) {
        VB_WAVE_SYNC();
        const bool sv = lane < qn;
        const unsigned sl = sv ? W_.sq[(qh + lane) & (VB_SQ - 1)] : srel0;
        dln = vb_raster_round<WIDE, COVER, LAZY>(sv, vbase + sl, sl - srel0, A.rc, rg, rx0, ry0, A.W, A.H, W_, key_, cov_, dln, pv, cvl, full, nsurv, qh);
        if (dln < 0) return -1;
    }
    return drawn ? 1 : 0;
}

// Stage 2: one WAVE per job = (view, link, 32x8 tile the link's screen box touches); persistent waves over the job list,
// which is never materialised (every workgroup derives it from the link boxes with a prefix sum over B * L counts).
// A job culls the link's cluster boxes, then the triangle boxes of the surviving clusters, and rasterizes the survivors
// into the wave's LDS depth/id buffer (tile + 1-pixel halo); the same wave then resolves the job from there
// (vb_resolve_from_lds), or marks the slot empty (jn = -1) when nothing was drawn.  No workgroup barriers after the prologue
// except in the heavy-job phase; thousands of independent waves hide each other's latency.
// A job that met a triangle for the general path goes on the list vb_slow_kernel works off.  The solver-step form of the
// chain does not launch that kernel until a step has needed it (slow_list == NULL: an empty launch costs the step 1.7 us
// and a robot in front of the camera never has such a triangle): then the job is marked empty and the step REPORTS it --
// VB_FLAG_NEED_SLOW among the overflow bits, so loss and gradient come out NaN and the optimiser state stays as it was; ehr_fused_status() returns
// EHR_ERR_RETRY and switches the pass on for the context's later calls.
__device__ __forceinline__ void vb_put_aside(int4* __restrict__ slow_list, int* __restrict__ meta, int* __restrict__ jn,
                                             int job, int u, int tx, int ty) {
    if (slow_list) {
        int* const nslow = vb_line(meta, VB_LINE_SLOW_COUNT);
        slow_list[atomicAdd(nslow, 1)] = make_int4(job, u, tx, ty);
    } else {
        atomicOr(&meta[EHR_META_OVERFLOW], VB_FLAG_NEED_SLOW);
        jn[job] = -1;
    }
}

// Kernel-wide arguments of the resolve stage (what vb_resolve_job needs besides the job itself).
struct VbResolveArgs {
    const float* verts;   // [V][3] object-space vertices
    const float* mvp;     // [B][L][16] (clip-space vertices on demand: VbLazy) ...
    const float4* posc;   // ... or kept: [B][V] (NULL: lazy)
    int L;
    const int4* tri4;     // [T] padded index table
    const int4* opp4;     // [T] opposite vertices (edge topology)
    VbSlots sl;
    VbItem* spill;        // pool of blended pairs for jobs that exceed their slot
    int* meta;
    int V, T, W, H, spill_cap, want_grad;
};

// The resolve stage of ONE drawn job, by one wave, from LDS: `ids` = triangle id of every region pixel (all-ones =
// uncovered, VB_ID_COVERED = covered but never depth tested: no uncovered neighbour), C = the region's coverage bitmap
// (bit i = region pixel i; wave-uniform).  Covered/uncovered pixel pairs by wave-uniform bit arithmetic, silhouette
// analysis of the compacted hits (restates nvdiffrast's antialias mesh kernel), gather of the link's antialiased value per
// pixel in the oracle's order.  Leaves in the job's slot the 256 values (jval), the blended pairs the backward pass needs
// (jitems) and their number (jn; -1 = the link contributes nothing here).  pairA [2 * VB_RN] and hits [2 * VB_RN] are the
// wave's LDS work areas.  Called right after a job's depth tests, by the wave that ran them (vb_resolve_from_lds: the ids
// never leave LDS).
template <bool LAZY = false>
__device__ __forceinline__ void vb_resolve_job(const VbResolveArgs& Q, const unsigned* ids, float* pairA,
                                               unsigned short* hits, const u64 (&C)[VB_WORDS], size_t slot, int b,
                                               int l, int rx0, int ry0) {
    const int lane = lane_id();
    const int4* const tri4 = Q.tri4;
    const int4* const opp4 = Q.opp4;
    int *const jn = Q.sl.jn, *const jspill = Q.sl.jspill, *const meta = Q.meta;
    float* const jval = Q.sl.jval;
    VbItem *const jitems = Q.sl.jitems, *const spill = Q.spill;
    const int V = Q.V, T = Q.T, W = Q.W, H = Q.H, spill_cap = Q.spill_cap, want_grad = Q.want_grad;
#define KT(i) (ids[i])
    const int r = lane >> 3, c4 = (lane & 7) * 4;
    const int myq = (r + 1) * VB_RW + (c4 + 1);
    const VbLazy pvz = {Q.verts, Q.mvp + ((size_t)b * Q.L + l) * 16, Q.posc ? Q.posc + (size_t)b * V : nullptr};
    int nitems = 0;       // wave-uniform
    int spill_base = -1;  // wave-uniform: first item of this job's spill block, once one was needed
    VB_WAVE_SYNC();
    for (int i = lane; i < 2 * VB_RN; i += 64) pairA[i] = 0.f;
    // region pixels inside the image (wave-uniform bitmap) and the pair-validity bitmaps derived from it
    u64 Iw[VB_WORDS];
#pragma unroll
    for (int k = 0; k < VB_WORDS; k++) {
        const unsigned i = 64u * k + lane;
        const int qy = vb_div_rw((int)i), qx = (int)i - qy * VB_RW;
        const int x = rx0 + qx, y = ry0 + qy;
        Iw[k] = __ballot(i < (unsigned)VB_RN && x >= 0 && x < W && y >= 0 && y < H);
    }
    u64 Vh[VB_WORDS], Vv[VB_WORDS];
    {
        // compile-time bitmaps (forced: a constexpr call with a loop index is otherwise evaluated at run time)
        constexpr u64 KH[VB_WORDS] = {vb_word_h(0), vb_word_h(1), vb_word_h(2), vb_word_h(3), vb_word_h(4), vb_word_h(5)};
        constexpr u64 KV[VB_WORDS] = {vb_word_v(0), vb_word_v(1), vb_word_v(2), vb_word_v(3), vb_word_v(4), vb_word_v(5)};
        static_assert(VB_WORDS == 6, "tables above");
        u64 s1[VB_WORDS], s34[VB_WORDS];
        vb_shr<1>(Iw, s1);
        vb_shr<VB_RW>(Iw, s34);
#pragma unroll
        for (int k = 0; k < VB_WORDS; k++) {
            Vh[k] = Iw[k] & s1[k] & KH[k];
            Vv[k] = Iw[k] & s34[k] & KV[k];
        }
    }
    // ---- pairs with exactly one covered pixel.  Only those can change the result: with constant colour inside a
    //      link a blend between two covered pixels is alpha * (1 - 1) = 0 in value and in gradient.
    u64 Hw[2 * VB_WORDS];
    int nh = 0;
    {
        u64 s1[VB_WORDS], s34[VB_WORDS];
        vb_shr<1>(C, s1);
        vb_shr<VB_RW>(C, s34);
#pragma unroll
        for (int k = 0; k < VB_WORDS; k++) {
            Hw[k] = (C[k] ^ s1[k]) & Vh[k];
            Hw[VB_WORDS + k] = (C[k] ^ s34[k]) & Vv[k];
            nh += __popcll(Hw[k]) + __popcll(Hw[VB_WORDS + k]);
        }
    }
    VB_WAVE_SYNC();
    float val[4];
#pragma unroll
    for (int j = 0; j < 4; j++) val[j] = (KT(myq + j) != 0xffffffffu) ? 1.f : 0.f;
    if (nh != 0) {
        // ---- dense hit list, ordered by (direction, region index)
        {
            int base = 0;
#pragma unroll
            for (int s = 0; s < 2 * VB_WORDS; s++) {
                const u64 w = Hw[s];
                if (w) {
                    if ((w >> lane) & 1)
                        hits[base + vb_mbcnt(w)] = (unsigned short)(((s % VB_WORDS) * 64 + lane) | ((s / VB_WORDS) << 15));
                    base += __popcll(w);
                }
            }
        }
        VB_WAVE_SYNC();
        // ---- silhouette analysis of the hits (restates nvdiffrast's antialias mesh kernel), 64 per round
        const VbVertsT<LAZY> pv = vb_verts<LAZY>(pvz);
        for (int hbase = 0; hbase < nh; hbase += 64) {
            const int h = hbase + lane;
            bool keep = false;
            VbItem it;
            it.packed = 0;
            it.v1 = 0;
            it.v2 = 0;
            it.alpha = 0.f;
            if (h < nh) {
                const int hq = hits[h];
                const int d = hq >> 15, q = hq & 0x7fff;
                const int qy = vb_div_rw(q), qx = q - qy * VB_RW;
                const int nq = q + (d ? VB_RW : 1);
                const unsigned k0 = KT(q), k1 = KT(nq);
                const bool chose0 = k0 != 0xffffffffu;  // exactly one of the two is covered
                const int t = min((int)(chose0 ? k0 : k1) & 0x7fffffff, T - 1);  // (always a triangle id: the pixel has an uncovered neighbour)
                int px = rx0 + qx, py = ry0 + qy;
                if (!chose0) {
                    px += 1 - d;
                    py += d;
                }
                float4 p[3], o[3];
                const int4 ti = tri4[t], oi = opp4[t];  // one aligned 16-byte gather each
                const int vi[3] = {ti.x, ti.y, ti.z}, ov[3] = {oi.x, oi.y, oi.z};
#pragma unroll
                for (int k = 0; k < 3; k++) p[k] = pv[vi[k]];
#pragma unroll
                for (int k = 0; k < 3; k++) o[k] = ((unsigned)ov[k] < (unsigned)V) ? pv[ov[k]] : p[k];
                const AAPair a = aa_analyze(p, o, px, py, d, chose0, W, H);
                if (a.found) {
                    pairA[d * VB_RN + q] = a.alpha;
                    // keep for the backward pass if the destination pixel is interior to this tile
                    const int oq = (a.alpha > 0.f) ? q : nq;
                    const int oy = vb_div_rw(oq), ox = oq - oy * VB_RW;
                    const bool oi = ox >= 1 && ox <= EHR_TILE_W && oy >= 1 && oy <= EHR_TILE_H;
                    if (oi && a.alpha != 0.f) {
                        it.packed = q | (d << 10) | (a.di << 11) | (a.tri1 << 13) | ((chose0 ? 0 : 1) << 14);
                        it.v1 = (a.di == 0) ? vi[1] : (a.di == 1 ? vi[2] : vi[0]);  // edge di: v1-v2, v2-v0, v0-v1
                        it.v2 = (a.di == 0) ? vi[2] : (a.di == 1 ? vi[0] : vi[1]);
                        it.alpha = a.alpha;
                        keep = want_grad != 0;
                    }
                }
            }
            const u64 km = __ballot(keep);
            if (km) {
                const int at = nitems + vb_mbcnt(km);
                const int nnew = nitems + __popcll(km);
                if (nnew > VB_JOB_ITEMS && spill_base < 0) {  // wave-uniform: first overflow of this job
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&meta[EHR_META_SPILL], VB_SPILL_BLOCK);
                    spill_base = __builtin_amdgcn_readfirstlane(base);
                }
                // items this job can keep: its slot, then its block of the spill pool as far as the pool reaches
                int room = VB_JOB_ITEMS;
                if (spill_base >= 0 && spill_base < spill_cap) room += min(VB_SPILL_BLOCK, spill_cap - spill_base);
                if (keep) {
                    if (at < VB_JOB_ITEMS)
                        jitems[slot * VB_JOB_ITEMS + at] = it;
                    else if (at < room)
                        spill[spill_base + (at - VB_JOB_ITEMS)] = it;
                    else
                        meta[EHR_META_OVERFLOW] = 1;  // reported through loss = NaN, never silent
                }
                nitems = min(nnew, room);  // never more than were stored: the composite kernel reads exactly these
            }
        }
        VB_WAVE_SYNC();
        // ---- gather the antialiased value of this link at my pixels (fixed order: down, left, right, up pair)
        {
            float cn[6], cd[4], cu[4];
#pragma unroll
            for (int j = 0; j < 6; j++) cn[j] = (KT(myq - 1 + j) != 0xffffffffu) ? 1.f : 0.f;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                cd[j] = (KT(myq - VB_RW + j) != 0xffffffffu) ? 1.f : 0.f;
                cu[j] = (KT(myq + VB_RW + j) != 0xffffffffu) ? 1.f : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float c = cn[j + 1];
                float v = c;
                float a;
                a = pairA[VB_RN + myq + j - VB_RW];
                if (a < 0.f) v += a * (c - cd[j]);
                a = pairA[myq + j - 1];
                if (a < 0.f) v += a * (c - cn[j]);
                a = pairA[myq + j];
                if (a > 0.f) v += a * (cn[j + 2] - c);
                a = pairA[VB_RN + myq + j];
                if (a > 0.f) v += a * (cu[j] - c);
                val[j] = v;
            }
        }
    }
    // ---- publish: the link's value at the tile's pixels (tile-local row-major), the number of blended pairs
    const bool nz = __ballot(val[0] != 0.f || val[1] != 0.f || val[2] != 0.f || val[3] != 0.f) != 0;
    if (nz) *reinterpret_cast<float4*>(jval + slot * 256 + r * EHR_TILE_W + c4) = make_float4(val[0], val[1], val[2], val[3]);
    if (lane == 0) {
        int* const n_out = &jn[slot];
        *n_out = nz ? nitems : -1;
        if (nitems > VB_JOB_ITEMS) jspill[slot] = spill_base;
    }
#undef KT
}

// The call of a wave that has drawn a job (vb_job_kernel, vb_job_slow): the job's coverage rows (cov) and depth/id buffer
// (key) are complete in LDS; the ids move to the (now idle) deferred list, the key buffer becomes the pair table, and the
// wave resolves the job it has just drawn.
// Nothing of the job's region goes through global memory, and the resolve stage needs no launch of its own: it was a
// 10 us kernel of one dependent chain per job behind a boundary; here the chain runs while other waves still rasterize.
// (Resolve and rasterizer never overlap inside a wave: the live ranges of the two are disjoint, unlike round 2's fusion.)
template <bool LAZY = false>
__device__ __forceinline__ void vb_resolve_from_lds(const VbResolveArgs& Q, VbWaveLds& S, u64* key, const u64* cov, size_t slot,
                                                    int b, int l, int rx0, int ry0) {
    const int lane = lane_id();
    static_assert(VB_RN <= VB_DL && 2 * VB_RN * sizeof(unsigned short) <= sizeof(VbRaster), "ids live in the deferred list's storage, the hit list in the rounds' staging area");
    VB_WAVE_SYNC();
    u64 C[VB_WORDS];
    unsigned idw[VB_WORDS];
#pragma unroll
    for (int k = 0; k < VB_WORDS; k++) {
        const unsigned i = 64u * k + lane;
        const unsigned row = (unsigned)vb_div_rw((int)i), col = i - row * VB_RW;
        const bool in = i < (unsigned)VB_RN;
        const bool cv = in && ((cov[in ? row : 0] >> col) & 1ull);
        const unsigned id = in ? (unsigned)key[i] : 0xffffffffu;  // low word = triangle id; all-ones stays all-ones
        C[k] = __ballot(cv);
        // covered pixels whose triangle was never asked for (no uncovered neighbour) carry a marker instead of an id
        idw[k] = (id != 0xffffffffu) ? id : (cv ? VB_ID_COVERED : 0xffffffffu);
    }
    VB_WAVE_SYNC();  // every lane has read its keys: the buffer is free
    unsigned* const ids = S.dl;
#pragma unroll
    for (int k = 0; k < VB_WORDS; k++) {
        const unsigned i = 64u * k + lane;
        if (i < (unsigned)VB_RN) ids[i] = idw[k];
    }
    vb_resolve_job<LAZY>(Q, ids, reinterpret_cast<float*>(key), reinterpret_cast<unsigned short*>(&S.R), C, slot, b, l, rx0, ry0);
    VB_WAVE_SYNC();
}

// a lane's four pixels of a mask tile row := 0 (the composite kernel's layout: lane -> row lane / 8, columns 4 (lane % 8)..+3)
__device__ __forceinline__ void vb_zero_tile_row(float* __restrict__ mask, size_t im, bool row_in, int ix, int W, int vec_ok) {
    if (!row_in) return;
    if (vec_ok) {
        if (ix < W) *reinterpret_cast<float4*>(mask + im) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (ix + j < W) mask[im + j] = 0.f;
    }
}

// What the composite stage needs besides its LDS tables.  vb_composite_kernel takes the struct by value, and the ORDER of the
// fields (with StepTail behind the struct) is what the register allocator's result depends on: this order was found by
// trying random ones and, when VbSlots changed size, every position of `sl` (spilled scalar registers <TAIL,FILL> 21,
// <TAIL> 20, <FILL> 20, <> 18; `sl` elsewhere 20-24).  Adding or moving a field moves those figures: compare tools/kres.py
// before and after (profiles/r07_scratch_layout_refactor.md and r10_slow_pass_resolves_itself.md hold the tables).
// (Read in place through the kernarg pointer instead, the fields are fetched again in the tile loop: 16-19 spilled, and
// 0.5-1 % of the step slower.)
struct VbCompArgs {
    const long long* tsum;
    int nls, want_grad, vec_ok;
    float* loss;         // (loss .. lbox_all, ref_flag: for the finish stage, run by the finisher workgroup of the call's
    int B;               //  last chunk of views -- do_finish -- over ALL views of the call)
    long long* facc;     // the chunk's accumulators
    int do_finish, B_all;
    const float* mvp;    // [B][L][16] (clip-space vertices on demand: VbLazy)
    int spill_cap;
    int* lbox_all;
    VbSlots sl;          // (read only here)
    float* mask;
    const float* verts;
    const float* ref;
    const long long* vtot_all;
    int* meta;
    float* grad_mvp;
    const VbItem* spill;
    int V;
    const long long* facc_all;
    const int* ref_flag;
    BinGeom g;
};

// The composite stage's work items of ONE wave (slot `wslot` of the `nslots` wave slots its XCD has; `nwg` workgroups in
// all): see vb_composite_kernel.  s_jbase / s_utile: the (view, link) tables in LDS; gpix: 256 floats of LDS of this wave.
// SHARED (the multi-start step): the chunk's view b is virtual view sh.view0 + b and compares with real view
// (sh.view0 + b) % sh.nviews of `ref` (which then holds sh.nviews images, passed whole); masks, sums and the bound
// reference's cached sums stay per virtual view.
struct VbSharedRef {
    int view0, nviews;
};
// The bound per-pixel weights of the loss (ehr_fused_bind_weight): `nviews` images [H][W], row 0 = top; the
// chunk's view b is view view0 + b of the call and reads image (view0 + b) % nviews -- the reference's sharing rule with the
// weights' own count.  The kernels' LAST parameter, behind StepTail / VbSharedRef, and never copied into VbCompArgs (see
// there): the WEIGHTED instantiations read it in place, through the kernarg pointer, where a tile needs it; the others
// never look at it.
struct VbWeight {
    const float* w;
    int view0, nviews;
};
struct VbCompParamsW;  // (the composite kernel's kernarg segment down to the weights: below, with VbCompParams)
typedef const VbCompParamsW __attribute__((address_space(4)))* VbCompParamsWPtr;
__device__ __forceinline__ VbCompParamsWPtr vb_comp_params_w();
__device__ __forceinline__ VbWeight vb_comp_weight(VbCompParamsWPtr p);
// a lane's four weights of a tile row (the reference's read: one float4 where vec_ok, which then also vouches for `w`)
__device__ __forceinline__ void vb_read_weights(const VbWeight& wt, int b, int H, int W, int row, int ix, const bool* pin, int vec_ok, float* wf) {
    const size_t imw = ((size_t)((wt.view0 + b) % wt.nviews) * H + row) * W + ix;
    if (vec_ok) {
        if (pin[0]) {
            const float4 w4 = *reinterpret_cast<const float4*>(wt.w + imw);
            wf[0] = w4.x; wf[1] = w4.y; wf[2] = w4.z; wf[3] = w4.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (pin[j]) wf[j] = wt.w[imw + j];
    }
}
// In-range links of a tile whose slot values the composite stage asks for in the item's first round trip, beside `jn`, the
// reference and the cached sum; the links beyond take a round trip each.  Four VGPRs a link, dead once the sum is formed.
// Chosen by measurement among 1, 2, 4 (profiles/composite_requests.md: at the headline views 52 % of the owned tiles have one
// link in range, 42 % two, 5 % three).  The pairs of those links were asked for there too and left out again: no faster, and
// the four registers a link they hold across the whole tile cost the multi-start forms a spilled VGPR.
constexpr int VB_COMP_PRE = 2;
// Wave-uniform reads of memory that nobody writes during the launch, as SCALAR loads: no vector register, no place in the
// vector memory queue, and the value is in scalar registers where a matrix is wanted anyway.  The index is made provably
// uniform (it derives from the wave's number, which the compiler cannot see is).
typedef const float __attribute__((address_space(4)))* VbScalarF;
typedef const long long __attribute__((address_space(4)))* VbScalarLL;
__device__ __forceinline__ void vb_scalar_matrix(const float* mvp, int unit, float* M) {  // mvp[unit][16]
    const VbScalarF p = (VbScalarF)mvp + (size_t)__builtin_amdgcn_readfirstlane(unit) * 16;
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = p[k];
}
__device__ __forceinline__ long long vb_scalar_ll(const long long* a, int i) {
    return ((VbScalarLL)a)[(size_t)__builtin_amdgcn_readfirstlane(i)];
}
// WEIGHTED: loss = sum w (mask - ref)^2 with the bound weights; per pixel  e = m - r; we = w * e; e2 += we * e;
// gv = gate ? 2 we : 0  (w == 1.0f: the unweighted expression bit for bit).  The unweighted instantiations are the code
// they were before the weights existed.
template <bool FILL, bool SHARED = false, bool WEIGHTED = false>
__device__ __forceinline__ void vb_composite_items(const VbCompArgs& C, const int* s_jbase, const unsigned* s_utile, float* gpix,
                                                   int xcd, int wslot, int nslots, int nwg, VbSharedRef sh = {0, 1}) {
    const BinGeom& g = C.g;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int W = g.W, H = g.H, L = g.L, B = C.B, U = B * L;
    const bool sparse = C.tsum != nullptr;
    const int jcap = C.sl.jcap, nls = C.nls, want_grad = C.want_grad, vec_ok = C.vec_ok, V = C.V, spill_cap = C.spill_cap;
    const float *const mvpc = C.mvp, *const verts = C.verts, *const jval = C.sl.jval, *const ref = C.ref;
    const int *const jn = C.sl.jn, *const jspill = C.sl.jspill;
    const VbItem *const jitems = C.sl.jitems, *const spill = C.spill;
    float* const mask = C.mask;
    long long* const facc = C.facc;
    int* const meta = C.meta;
    const long long* const tsum = C.tsum;
    // work items: every tile of every view, or (bound reference) the JOBS -- a job stands for its tile if no link before
    // its own has a job there, so that every tile with a job comes up exactly once and the others never
    const int nitems = sparse ? min(s_jbase[U], jcap) : B * g.nt;
    // XCD-aware order (locality only): every XCD takes a contiguous run of items
    const int per_xcd = vb_xcd_share(nitems);
    const int ibeg = xcd * per_xcd, iend = min(ibeg + per_xcd, nitems);
    const int istep = nslots;
    const int acc_stride = vb_acc_stride(L, nls);
    const int r = lane >> 3, c4 = (lane & 7) * 4;
    const float invL = __builtin_amdgcn_rcpf((float)L);  // (u / L by vb_div_small)
    const VbCompParamsWPtr wparams = vb_comp_params_w();  // (WEIGHTED: where the weights' descriptor is read from)
    for (int item = ibeg + wslot; item < iend; item += istep) {
    int b, tx, ty;
    if (sparse) {
        int lo = 0;
        if (U <= 64) {  // the last (view, link) whose first job is <= item: one LDS read per lane and a ballot
            lo = __popcll(__ballot(lane < U && s_jbase[lane] <= item)) - 1;
        } else {
            int hi = U - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (s_jbase[mid] <= item)
                    lo = mid;
                else
                    hi = mid - 1;
            }
        }
        b = vb_div_small(lo, invL);
        const unsigned ut = s_utile[lo];
        const int nx = (int)(ut >> 22), k = item - s_jbase[lo];
        const int kr = vb_div_small(k, __builtin_amdgcn_rcpf((float)nx));  // (k < 2^16 tiles, nx <= 128: exact)
        ty = (int)((ut >> 10) & 4095u) + kr;
        tx = (int)(ut & 1023u) + k - kr * nx;
        // owner of the tile = the job of the first link that has one there
        bool prior = false;
        if (lane < lo - b * L) {
            const int u2 = b * L + lane;
            const unsigned u2t = s_utile[u2];
            const int n2 = s_jbase[u2 + 1] - s_jbase[u2];
            const int ax0 = u2t & 1023u, ay0 = (u2t >> 10) & 4095u, anx = u2t >> 22;
            prior = n2 > 0 && tx >= ax0 && tx < ax0 + anx && ty >= ay0 && (ty - ay0) * anx < n2;  // (n2 = anx x the rows)
        }
        if (__ballot(prior)) continue;
    } else {
        b = item / g.nt;
        const int tile = item - b * g.nt;
        tx = tile % g.ntx;
        ty = tile / g.ntx;
    }
    const int tile = ty * g.ntx + tx;
    long long* const vacc = facc + (size_t)b * acc_stride;
    long long* const lacc = vacc + vb_acc_loss(L) + (tile % nls) * VB_LOSS_STRIDE;
    const int rx0 = tx * EHR_TILE_W - 1, ry0 = ty * EHR_TILE_H - 1;
    // ---- the item's FIRST ROUND TRIP: what the forward half needs is asked for here, before anything is waited for --
    //      the links' `jn`, the reference (and weights), the tile's cached sum and the slot values of the first
    //      VB_COMP_PRE in-range links: their addresses follow from (b, tx, ty) and the tables in LDS.  `jn` only decides
    //      whether a value is USED, not where it lives: what was asked for a link that turns out to hold nothing
    //      (jn < 0) is a read inside jval[jcap][256] that nobody looks at.
    // links whose tile range (the tiles + halo their screen box touches: the jobs stage 2 ran) contains this tile (lane l
    // tests link l, from the tables in LDS)
    int myn = -1, myslot = 0;
    bool inr = false;
    if (lane < L) {
        const int u = b * L + lane;
        const unsigned ut = s_utile[u];
        const int j0 = s_jbase[u], n = s_jbase[u + 1] - j0;
        const int tx0 = ut & 1023u, ty0 = (ut >> 10) & 4095u, nx = ut >> 22;
        if (n > 0 && tx >= tx0 && tx < tx0 + nx && ty >= ty0 && (ty - ty0) * nx < n) {
            const int slot = j0 + (ty - ty0) * nx + (tx - tx0);
            inr = slot < jcap;
            if (inr) {
                myslot = slot;
                myn = jn[slot];
            }
        }
    }
    unsigned rest = (unsigned)__ballot(inr);  // links in range (known at once), in link order
    const int ix = tx * EHR_TILE_W + c4, iy = ty * EHR_TILE_H + r;  // first of my 4 pixels (GL rows: y up)
    const bool row_in = iy < H;
    const size_t im = ((size_t)b * H + (H - 1 - (row_in ? iy : 0))) * W + ix;  // image convention: row 0 = top
    const size_t imr = SHARED ? ((size_t)((sh.view0 + b) % sh.nviews) * H + (H - 1 - (row_in ? iy : 0))) * W + ix : im;
    float rf[4] = {0.f, 0.f, 0.f, 0.f};
    bool pin[4];
#pragma unroll
    for (int j = 0; j < 4; j++) pin[j] = row_in && (ix + j) < W;
    if (vec_ok) {
        if (pin[0]) {
            const float4 r4 = *reinterpret_cast<const float4*>(ref + imr);
            rf[0] = r4.x; rf[1] = r4.y; rf[2] = r4.z; rf[3] = r4.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (pin[j]) rf[j] = ref[imr + j];
    }
    float wf[4] = {0.f, 0.f, 0.f, 0.f};
    if (WEIGHTED) vb_read_weights(vb_comp_weight(wparams), b, H, W, H - 1 - (row_in ? iy : 0), ix, pin, vec_ok, wf);
    const long long cached = sparse ? vb_scalar_ll(tsum, b * g.nt + tile) : 0ll;  // (constant of the solve, wave-uniform)
    // (No branch around these requests -- a conditional request makes the compiler wait for it where the branches join:
    //  where fewer links are in range, lane 0's slot is read again -- `myslot` is 0 where lane 0's link is not in range --
    //  and ignored.)
    int pl[VB_COMP_PRE];       // the link (-1: fewer in range)
    float4 pval[VB_COMP_PRE];  // my four values of its slot
#pragma unroll
    for (int k = 0; k < VB_COMP_PRE; k++) {
        const int l = rest ? __ffs(rest) - 1 : 0;
        pl[k] = rest ? l : -1;
        rest &= rest - 1;
        const size_t slot = (size_t)vb_readlane(myslot, l);  // (< jcap)
        pval[k] = *reinterpret_cast<const float4*>(jval + slot * 256 + r * EHR_TILE_W + c4);
    }
    // ---- one wait, then the decisions.  (The empty statements make what was asked for above a value that is complete
    //      HERE: without them the compiler moves each request down to its use, behind the wait for `jn`, and the chain is
    //      the one it was.)
#pragma unroll
    for (int k = 0; k < VB_COMP_PRE; k++) asm volatile("" : "+v"(pval[k].x), "+v"(pval[k].y), "+v"(pval[k].z), "+v"(pval[k].w));
    const unsigned tmask = (unsigned)__ballot(myn >= 0);  // links that contribute a value here
    if (sparse && tmask == 0) {  // nothing drawn here: the tile's cached sum(ref^2) is part of vtot already
        if (FILL) vb_zero_tile_row(mask, im, row_in, ix, W, vec_ok);
        continue;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < VB_COMP_PRE; k++)  // sum in link order: the links asked for above are the first ones in range ...
        if (pl[k] >= 0 && ((tmask >> pl[k]) & 1u)) {
            acc[0] += pval[k].x;
            acc[1] += pval[k].y;
            acc[2] += pval[k].z;
            acc[3] += pval[k].w;
        }
    unsigned todo = tmask & rest;
    while (todo) {  // ... then the others, a request and a wait each
        const int l = __ffs(todo) - 1;
        todo &= todo - 1;
        const size_t slot = (size_t)vb_readlane(myslot, l);
        const float4 v4 = *reinterpret_cast<const float4*>(jval + slot * 256 + r * EHR_TILE_W + c4);
        acc[0] += v4.x;
        acc[1] += v4.y;
        acc[2] += v4.z;
        acc[3] += v4.w;
    }
    // ---- composite, loss, mask write (image convention: row 0 = top)
    float e2 = 0.f, gv[4];
    float mv[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        gv[j] = 0.f;
        mv[j] = 0.f;
        if (pin[j]) {
            const float m = acc[j] > 1.f ? 1.f : acc[j];
            const float e = m - rf[j];
            if (WEIGHTED) {
                const float we = wf[j] * e;
                e2 += we * e;
                gv[j] = (acc[j] <= 1.f) ? 2.f * we : 0.f;
            } else {
                e2 += e * e;
                gv[j] = (acc[j] <= 1.f) ? 2.f * e : 0.f;
            }
            mv[j] = m;
        }
    }
    if (mask) {
        if (vec_ok) {
            if (pin[0]) *reinterpret_cast<float4*>(mask + im) = make_float4(mv[0], mv[1], mv[2], mv[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (pin[j]) mask[im + j] = mv[j];
        }
    }
    {
        const float s = wave_sum(e2);
        if (lane == 0) {
            if (sparse)
                fix_add_delta(lacc, s, cached, meta);
            else
                fix_add(lacc, s, meta);
        }
    }
    const unsigned bmask = (unsigned)__ballot(myn > 0);  // links with blended pairs to back-propagate
    if (!want_grad || bmask == 0) continue;

    // ---- backward: blended pairs -> rows (x, y, w) of d loss / d MVP, per link
    VB_WAVE_SYNC();  // the previous tile's reads of gpix are complete
#pragma unroll
    for (int j = 0; j < 4; j++) gpix[r * EHR_TILE_W + c4 + j] = gv[j];
    VB_WAVE_SYNC();
    unsigned links = bmask;
    while (links) {
        const int l = __ffs(links) - 1;
        links &= links - 1;
        const size_t slot = (size_t)vb_readlane(myslot, l);
        int n = vb_readlane(myn, l);
        int sbase = 0;
        if (n > VB_JOB_ITEMS) {  // the rest of the list lives in the spill pool; never read outside it
            sbase = jspill[slot];
            if (sbase < 0 || sbase >= spill_cap) n = VB_JOB_ITEMS;
            else n = min(n, VB_JOB_ITEMS + (spill_cap - sbase));
        }
        float M[16];  // the link's matrix (clip space on demand; wave-uniform: a scalar load, no vector request behind `jn`)
        vb_scalar_matrix(mvpc, b * L + l, M);
        float G[12];
#pragma unroll
        for (int k = 0; k < 12; k++) G[k] = 0.f;
        for (int i = lane; i < n; i += 64) {
            const VbItem itm = *((i < VB_JOB_ITEMS) ? &jitems[slot * VB_JOB_ITEMS + i] : &spill[sbase + (i - VB_JOB_ITEMS)]);
            const int q = itm.packed & 1023, d = (itm.packed >> 10) & 1;
            const int tri1 = (itm.packed >> 13) & 1;
            const float dc = ((itm.packed >> 14) & 1) ? 1.f : -1.f;
            const int nq = q + (d ? VB_RW : 1);
            const int oq = (itm.alpha > 0.f) ? q : nq;
            const int oy = vb_div_rw(oq), ox = oq - oy * VB_RW;
            const float gi = gpix[(oy - 1) * EHR_TILE_W + (ox - 1)];
            const float dd = gi * dc;
            if (gi == 0.f || dd == 0.f) continue;
            const int qy = vb_div_rw(q), qx = q - qy * VB_RW;
            int px = rx0 + qx, py = ry0 + qy;
            if (tri1) {
                px += 1 - d;
                py += d;
            }
            float g1[3], g2[3];
            const float* a1 = verts + 3 * (size_t)itm.v1;
            const float* a2 = verts + 3 * (size_t)itm.v2;
            const float h1[4] = {a1[0], a1[1], a1[2], 1.f}, h2[4] = {a2[0], a2[1], a2[2], 1.f};
            // (the object-space vertices are needed for the matrix gradient anyway: their clip-space positions come from them)
            aa_pos_grad(transform_vertex(M, h1[0], h1[1], h1[2]), transform_vertex(M, h2[0], h2[1], h2[2]), px, py, d,
                        itm.alpha, dd, W, H, g1, g2);
#pragma unroll
            for (int rr = 0; rr < 3; rr++)
#pragma unroll
                for (int c = 0; c < 4; c++) G[4 * rr + c] += g1[rr] * h1[c] + g2[rr] * h2[c];
        }
        // the twelve sums in 14 shuffles (bit-equal to twelve wave_sum calls); one lane per element adds its sum
        const float mine = wave_sum12(G, lane);
        if ((lane & 3) == 0 && (lane & 12) != 12) fix_add(&vacc[vb_acc_grad(l) + wave_sum12_element(lane)], mine, meta);
    }
    }
    // ---- bound reference AND a mask output: the tiles that hold a job were written by their owners above; every other
    //      tile of the images is zero.  The waves share them out (most have no item, or one): a wave tests a tile against
    //      the links' tile ranges -- the predicate that decides whether the tile HAS an owner -- and stores 1 KB of zeros if
    //      it has none.  Stores only: nothing here is waited for before the arrival's vmcnt.
    if (FILL) {
        const int total = B * g.nt;
        for (int t = (int)blockIdx.x * 4 + wave; t < total; t += nwg * 4) {
            const int b = t / g.nt, tile = t - b * g.nt;
            const int ty = tile / g.ntx, tx = tile - ty * g.ntx;
            bool owned = false;
            if (lane < L) {
                const int u = b * L + lane;
                const unsigned ut = s_utile[u];
                const int n = s_jbase[u + 1] - s_jbase[u];
                const int tx0 = ut & 1023u, ty0 = (ut >> 10) & 4095u, nx = ut >> 22;
                owned = n > 0 && tx >= tx0 && tx < tx0 + nx && ty >= ty0 && (ty - ty0) * nx < n;
            }
            if (__ballot(owned)) continue;
            const int ix = tx * EHR_TILE_W + c4, iy = ty * EHR_TILE_H + r;
            const bool row_in = iy < H;
            vb_zero_tile_row(mask, ((size_t)b * H + (H - 1 - (row_in ? iy : 0))) * W + ix, row_in, ix, W, vec_ok);
        }
    }
}

constexpr int VB_JOB_WAVES = 4;
// What the coverage-only form of the job kernel (COVER, the scoring op) writes instead of job slots; the buffers are
// described by vb_score_misc.
struct VbCoverOut {
    u64* tcov;    // [candidate][tile][pose][4] coverage words the jobs OR their tile's interior into
    int* sticky;  // [0]: raised by a job that met a triangle whose depth class does not let coverage decide
    int S;        // poses per candidate
};
// The job kernel's parameters, ONE struct in the kernarg segment.  The kernel does not name its parameter; it reads the
// fields through the kernarg segment pointer, made opaque to the optimiser at every use (vb_job_params), so that a field
// is a scalar load where it is needed instead of one of ~60 scalar registers filled at kernel entry and kept -- i.e.
// spilled to vector-register lanes and reloaded -- across the whole job loop (by-value use, round 4: 237 spilled SGPRs
// in this kernel).
struct VbJobParams {
    BinGeom g;
    int B;
    VbClusters cl;
    VbRecs rc;
    const int* lbox;
    int use_hint;  // 1: deal the previous step's heavy and long jobs (the hint names jobs by their dense id in a chunk)
    VbHeavy hv;
    VbSlotIdx si;
    int heavy_t, med_t0;
    VbResolveArgs rq;  // the scene, the job slots and the meta block: the resolve stage runs on the wave that drew the job
    VbCoverOut co;     // COVER only (rq then holds the scene and the meta block, no slots)
};
typedef const VbJobParams __attribute__((address_space(4)))* VbJobParamsPtr;
__device__ __forceinline__ VbJobParamsPtr vb_job_params() {
    VbJobParamsPtr p = (VbJobParamsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));  // (what the optimiser cannot see through it cannot hoist to the kernel's entry)
    return p;
}
// a whole sub-struct of the parameters, copied through a generic pointer: address-space inference turns the copy back into
// scalar loads of the kernarg segment (checked in the ISA: the job kernels hold no flat_load at all)
template <class T>
__device__ __forceinline__ T vb_prm_copy(const T __attribute__((address_space(4)))* p) {
    return *(const T*)p;
}
// COVER (the scoring op): no slots, no lists; the jobs' outputs are those of VbCoverOut.
template <bool COVER, bool LAZY = false>
__global__ void __launch_bounds__(256, VB_JOB_WAVES)
vb_job_kernel(VbJobParams) {
    __shared__ VbWaveLds lds_all[4];
    // PRM(field): a kernel parameter, read where it is used (see VbJobParams)
#define PRM(f) (vb_job_params()->f)
    const int W = PRM(g.W), H = PRM(g.H), L = PRM(g.L), gnt = PRM(g.nt), gntx = PRM(g.ntx);
    const int B = PRM(B), V = PRM(rq.V);
    int heavy_t = max(PRM(heavy_t), PRM(hv.gen)[6]);  // (the value in force: the vertex kernel adapts it, see VbHeavy)
    const float* const pverts = PRM(rq.verts);
    const float* const pmvp = PRM(rq.mvp);
    const float4* const posc = LAZY ? nullptr : PRM(rq.posc);
    // the scheduling hint of the previous step is requested before anything else, in ONE round trip: which of the two
    // lists is the one to consume follows from the generation, so both lists' counts and this workgroup's entry of either are
    // requested together with it (they were a second, dependent round trip on every wave's way to its first job)
    const int* const hgen = PRM(hv.gen);
    const int gen = hgen[0], hc1 = hgen[1], hc2 = hgen[2], hm4 = hgen[4], hm5 = hgen[5];
    const int hida = PRM(hv.list)[min((int)blockIdx.x, VB_HEAVY_CAP - 1)];
    const int hidb = PRM(hv.list)[VB_HEAVY_CAP + min((int)blockIdx.x, VB_HEAVY_CAP - 1)];
    // (Not the long job a wave starts with: its index depends on the number of heavy workgroups.  Dealing the long jobs to
    //  the XCD's LAST workgroups instead, counted from the end, makes the index known here -- measured: 84.7 vs 83.1 us, the
    //  last workgroups of a 1024-workgroup grid start last.)
    const int hcur = (gen - 1) & 1, hnxt = gen & 1;
    const int nheavy_prev = hcur ? hc2 : hc1;
    const int hid_first = hcur ? hidb : hida;
    __shared__ int upre[VB_MAX_UNITS + 1];   // first job of every (view, link)
    __shared__ unsigned utile[VB_MAX_UNITS];  // its tile range: tx0 | ty0 << 10 | nx << 22
    __shared__ int lcoff[33];                 // first cluster of every link
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    VbWaveLds& S = lds_all[wave];
    const int U = B * L;
    const float invL = __builtin_amdgcn_rcpf((float)L);  // (u / L by vb_div_small)
    // ---- prologue (every workgroup, redundantly): tile range and job count of every (view, link), prefix sum
    int total;
    if (U <= 64) {
        // At most one (view, link) per lane: EVERY WAVE builds the tables by itself -- its own read of the link boxes, a wave
        // scan, the same values to the same LDS words as its three siblings -- and goes on without a barrier: the two
        // workgroup barriers and the LDS hand-over of the cooperative form below stood between every wave and its first job
        // (3.0-3.4 us into the kernel; the long jobs the kernel ends on are first jobs).
        if (lane <= L) lcoff[lane] = PRM(cl.coff)[lane];
        int cnt = 0;
        if (lane < U) {
            int tx0 = 0, ty0 = 0, nx = 0, ny = 0;
            const bool ne = vb_unit_tiles(PRM(lbox) + VB_LBOX_STRIDE * (size_t)lane, W, H, tx0, ty0, nx, ny, COVER ? 0 : 1);
            cnt = ne ? nx * ny : 0;
            utile[lane] = (unsigned)tx0 | ((unsigned)ty0 << 10) | ((unsigned)(ne ? nx : 1) << 22);
        }
        const int incl = vb_scan_add(cnt);
        if (lane < U) upre[lane + 1] = incl;
        if (lane == 0) upre[0] = 0;
        total = vb_readlane(incl, 63);
        VB_WAVE_SYNC();
    } else {
    if (tid <= L) lcoff[tid] = PRM(cl.coff)[tid];
    for (int u = tid; u < U; u += 256) {
        int tx0 = 0, ty0 = 0, nx = 0, ny = 0;
        const bool ne = vb_unit_tiles(PRM(lbox) + VB_LBOX_STRIDE * (size_t)u, W, H, tx0, ty0, nx, ny, COVER ? 0 : 1);
        upre[u + 1] = ne ? nx * ny : 0;
        utile[u] = (unsigned)tx0 | ((unsigned)ty0 << 10) | ((unsigned)(ne ? nx : 1) << 22);
    }
    if (tid == 0) upre[0] = 0;
    __syncthreads();
    if (wave == 0) {
        int run = 0;
        for (int base = 0; base < U; base += 64) {
            const int i = base + lane;
            int incl = (i < U) ? upre[i + 1] : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            if (i < U) upre[i + 1] = run + incl;
            run += vb_readlane(incl, 63);
        }
    }
    __syncthreads();
    total = upre[U];
    }
    if (!COVER && blockIdx.x == 0) {
        // job slots are numbered like the jobs: stage 3 finds a (view, link, tile) slot from the link's first job
        // (every entry this wave may read here it has written itself, or a barrier lies in between: see above)
        for (int u = tid; u <= U; u += 256) PRM(rq.sl.jbase)[u] = upre[u];
        for (int u = tid; u < U; u += 256) PRM(rq.sl.jutile)[u] = utile[u];
        if (tid == 0 && total > PRM(rq.sl.jcap)) PRM(rq.meta)[EHR_META_OVERFLOW] = 1;  // cannot happen with one slot per (view, link, tile)
    }
    if (!COVER) total = min(total, PRM(rq.sl.jcap));
    // XCD-aware order (workgroup w runs on XCD w % VB_XCDS; used for L2 locality only): every XCD takes a contiguous
    // eighth of the job list, so that a view's vertices, boxes and records stay in one L2.  Inside that eighth every wave
    // takes one job statically; the jobs beyond that are claimed (one returning atomic on the XCD's cursor) by whichever
    // wave finishes first.  Jobs differ by two orders of magnitude in cost: dealt statically, the kernel waits for a wave
    // that got a heavy SECOND job; claimed from the start, 500 waves hit each cursor at once (~12 ns per same-address
    // atomic) and the kernel is 20 % slower.
    const int per_xcd = vb_xcd_share(total), xcd = blockIdx.x & (VB_XCDS - 1);
    const int jbeg = xcd * per_xcd, jend = min(jbeg + per_xcd, total);
    int* const cursor = vb_line(PRM(rq.meta), VB_LINE_JOB_CURSOR + xcd);
    VbJobArgs A;
    A.rc = vb_prm_copy(&PRM(rc));
    A.verts = pverts;
    A.mvp = pmvp;
    A.posc = posc;
    A.cvidx = PRM(si.cvidx);
    A.lcoff = lcoff;
    A.NC = PRM(cl.NC);
    A.V = V;
    A.W = W;
    A.H = H;
    A.L = L;
    // ---- heavy jobs first, one workgroup each: the four waves share the job's depth/id buffer (wave 0's) and split the
    //      candidate clusters; wave 0 resolves it.  A job alone costs up to ~80 us on one wave (a thousand candidate
    //      triangles in one tile), which used to be the duration of this kernel at small batch sizes.
    __shared__ int s_heavy[2];  // drawn flag, survivors
    // Only when the machine is short of jobs (at most ~2 per wave): with many views per GPU the kernel is bound by the
    // sum of the jobs, not by the longest, and four waves on one job are less efficient than four jobs (measured: 64
    // views 8 % slower with the heavy phase, 8 views 10 % faster, 1 view 40 % faster).
    // Likewise when heavy jobs are the rule rather than the exception (more than one per two workgroups: the Franka
    // meshes at 1080p have ~3000 of them in 8100 jobs and run 17 % slower with the heavy phase; the 8-view xArm7
    // workload has ~220 in 5000).
    const int use_hint = PRM(use_hint);
    const int nheavy = (!use_hint || total > 2 * 4 * (int)gridDim.x || nheavy_prev > (int)gridDim.x / 2) ? 0 : min(nheavy_prev, min(VB_HEAVY_CAP, (int)gridDim.x));  // (<= one heavy job per workgroup)
    // ... and when there are fewer jobs than waves (one view, small images) most workgroups are idle anyway: jobs count as
    // heavy from a proportionally lower cost (down to an eighth: a few rounds), so that the longest ones are shared
    {
        const float f = fminf(1.f, fmaxf(0.125f, (float)total / (float)(2 * (int)gridDim.x)));
        heavy_t = (int)((float)heavy_t * f);
    }
    auto remember_heavy = [&](int id) {
        const int at = atomicAdd(&PRM(hv.gen)[1 + hnxt], 1);
        if (at < VB_HEAVY_CAP) PRM(hv.list)[hnxt * VB_HEAVY_CAP + at] = id;
    };
    // Long jobs below the heavy threshold: a wave that claims one late (after two or three others) is what the kernel
    // ends on -- 30 us on one wave whenever it starts -- so they are remembered as well and dealt out as static FIRST jobs,
    // one per wave, in the next step.  Only when the machine is short of jobs (at most 1.5 per wave): with more, claiming
    // balances the waves anyway and the jobs are better off in their own XCD's eighth of the list (L2).
    const int med_t = max(PRM(med_t0), 1);
    const int nmed = (!use_hint || total > 6 * (int)gridDim.x) ? 0 : min(hcur ? hm5 : hm4, PRM(hv.mcap));
    auto remember_long = [&](int id) {
        const int at = atomicAdd(&PRM(hv.gen)[4 + hnxt], 1);
        if (at < VB_MED_CAP) PRM(hv.mlist)[hnxt * VB_MED_CAP + at] = id;
    };
    if ((int)blockIdx.x < nheavy) {  // (workgroup-uniform: the others go straight on, without a barrier)
        if (tid < 2) s_heavy[tid] = 0;
        __syncthreads();
    }
    if ((int)blockIdx.x < nheavy) __builtin_amdgcn_s_setprio(VB_PRIO_HEAVY);
    int hres_job = -1, hres_b = 0, hres_l = 0, hres_rx0 = 0, hres_ry0 = 0;  // the heavy job wave 0 resolves once the workgroup has split up again
    for (int hj = blockIdx.x; hj < nheavy; hj += gridDim.x) {  // workgroup-uniform (at most one turn: nheavy <= gridDim.x)
        const int id = (hj == (int)blockIdx.x) ? hid_first : PRM(hv.list)[hcur * VB_HEAVY_CAP + hj];
        const int u = min((int)((unsigned)id >> 22), U - 1), tx = id & 1023, ty = (id >> 10) & 4095;
        const unsigned ut = utile[u];
        const int tx0 = ut & 1023u, ty0 = (ut >> 10) & 4095u, nx = ut >> 22, n = upre[u + 1] - upre[u];
        const int job = upre[u] + (ty - ty0) * nx + (tx - tx0);
        // (n is nx times the rows: ty inside the rows <=> the tile's job number inside the link's jobs)
        if (n <= 0 || tx < tx0 || tx >= tx0 + nx || ty < ty0 || (ty - ty0) * nx >= n || job >= total) continue;  // the link moved away
        const int b = vb_div_small(u, invL), l = u - b * L;
        const int rx0 = tx * EHR_TILE_W - 1, ry0 = ty * EHR_TILE_H - 1;
        VbRegion rg;
        rg.x0 = max(rx0, 0);
        rg.y0 = max(ry0, 0);
        rg.x1 = min(rx0 + VB_RW - 1, W - 1);
        rg.y1 = min(ry0 + VB_RH - 1, H - 1);
        VbWaveLds& S0 = lds_all[0];
        for (int i = tid; i < VB_RN; i += 256) S0.key[i] = VB_EMPTY;
        if (tid < VB_RH) S0.cov[tid] = 0ull;
        __syncthreads();
        int nsurv = 0, dln = 0;
        const int drawn = vb_job_raster<false, false, LAZY>(A, S, S0.key, S0.cov, b, l, rg, rx0, ry0, wave, 4, nsurv, dln);
        if (lane == 0) {
            if (drawn > 0) atomicOr(&s_heavy[0], 1);
            if (drawn < 0) atomicOr(&s_heavy[0], 2);  // a triangle for the general path: wave 0 redoes the job alone
            atomicAdd(&s_heavy[1], nsurv);
        }
        __syncthreads();  // the job's coverage is complete: every wave filters its own deferred units against it
        const int any_drawn = s_heavy[0];
        int tot_surv = s_heavy[1];
        if (!(any_drawn & 2) && dln > 0)
            vb_flush<false, LAZY>(S, S0.key, S0.cov, dln, VbLazy{pverts, pmvp + ((size_t)b * L + l) * 16, LAZY ? nullptr : posc + (size_t)b * V}, PRM(si.cvidx) + (size_t)lcoff[l] * 64, W, H, rx0, ry0);
        __syncthreads();
        if (!COVER && any_drawn == 1) {
            hres_job = job;
            hres_b = b;
            hres_l = l;
            hres_rx0 = rx0;
            hres_ry0 = ry0;
        }
        if (wave == 0) {
            if (any_drawn & 2) {  // put aside for vb_slow_kernel
                if (lane == 0) vb_put_aside(PRM(rq.sl.slow_list), PRM(rq.meta), PRM(rq.sl.jn), job, u, tx, ty);
            } else if (any_drawn) {
            } else if (lane == 0) {
                PRM(rq.sl.jn)[job] = -1;
            }
            if (lane == 0) {
                s_heavy[0] = 0;
                s_heavy[1] = 0;
                if (tot_surv >= heavy_t)
                    remember_heavy(id);
                else if (tot_surv >= med_t)
                    remember_long(id);
            }
        }
        __syncthreads();
    }

    // (the loop's last barrier is behind us: waves 1-3 go on to their own jobs, nobody touches wave 0's LDS but wave 0)
    if (!COVER && wave == 0 && hres_job >= 0) vb_resolve_from_lds<LAZY>(vb_prm_copy(&PRM(rq)), S, S.key, S.cov, (size_t)hres_job, hres_b, hres_l, hres_rx0, hres_ry0);
    __builtin_amdgcn_s_setprio(0);
    // workgroups that just spent their time on a heavy job take no static job: the first hk of this XCD's workgroups
    const int nhw = min(nheavy, (int)gridDim.x);
    const int hk = (nhw > xcd) ? vb_xcd_share(nhw - xcd) : 0;
    const int kx = blockIdx.x >> VB_XCD_BITS;            // this workgroup's index inside its XCD
    const int G8 = (int)gridDim.x >> VB_XCD_BITS;        // workgroups per XCD
    // static first jobs: wave rx of this XCD's static waves (global rank VB_XCDS rx + xcd) takes long job number <rank> of the
    // previous step if there is one, else the (rx - nmx)-th job of the XCD's eighth; the rest of the eighth is claimed
    const int nmx = (nmed > xcd) ? vb_xcd_share(nmed - xcd) : 0;  // long jobs that go to this XCD's waves (<= the static waves, see mcap)
    // (the long jobs one per WORKGROUP first -- rank wave * (G8 - hk) + (kx - hk) -- instead of four to a workgroup: measured in
    //  round 6, no difference: 41.1 / 33.9 / 90.4 us job stage either way at 8 views / 1 view / Franka)
    const int rx = (kx - hk) * 4 + wave;
    bool list_first = kx >= hk && rx < nmx;
    bool first_job = kx >= hk && !list_first;
    const int nsn = (G8 - hk) * 4 - nmx;                       // static jobs of the eighth itself
    int sjob = jbeg + rx - nmx;
    for (;;) {
        int job = 0, u = -1, tx = 0, ty = 0;
        if (list_first) {
            list_first = false;
            __builtin_amdgcn_s_setprio(VB_PRIO_LONG);
            const int id = PRM(hv.mlist)[hcur * VB_MED_CAP + VB_XCDS * rx + xcd];
            u = min((int)((unsigned)id >> 22), U - 1);
            tx = id & 1023;
            ty = (id >> 10) & 4095;
            const unsigned ut = utile[u];
            const int tx0 = ut & 1023u, ty0 = (ut >> 10) & 4095u, nx = ut >> 22, n = upre[u + 1] - upre[u];
            job = upre[u] + (ty - ty0) * nx + (tx - tx0);
            if (n <= 0 || tx < tx0 || tx >= tx0 + nx || ty < ty0 || (ty - ty0) * nx >= n || job >= total) continue;  // the link moved away
        } else {
            __builtin_amdgcn_s_setprio(0);
            if (first_job) {
                job = sjob;
                sjob += max(nsn, 1);
                first_job = false;
                if (job >= jbeg + nsn) job = jend;  // (more static waves than jobs)
            } else {  // whoever is done first takes the next one: the waves stuck with a heavy first job take no second
                if (lane == 0) job = jbeg + nsn + atomicAdd(cursor, 1);
                job = __builtin_amdgcn_readfirstlane(job);
            }
            if (job >= jend) {
                break;
            }
            if (U <= 64) {  // the last (view, link) whose first job is <= job: one LDS read per lane and a ballot
                u = __popcll(__ballot(lane < U && upre[lane] <= job)) - 1;
            } else {
                int lo = 0, hi = U - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (upre[mid] <= job)
                        lo = mid;
                    else
                        hi = mid - 1;
                }
                u = lo;
            }
            {
                const unsigned ut = utile[u];
                const int nx = (int)(ut >> 22), k = job - upre[u];
                const int kr = vb_div_small(k, __builtin_amdgcn_rcpf((float)nx));  // (k < 2^16 tiles, nx <= 128: exact)
                ty = (int)((ut >> 10) & 4095u) + kr;
                tx = (int)(ut & 1023u) + k - kr * nx;
            }
            const int st = (nheavy > 0 || nmed > 0) ? PRM(hv.stamp)[u * gnt + ty * gntx + tx] : 0;
            // a workgroup took this one in the heavy phase / it is some wave's first job
            if ((nheavy > 0 && st == gen) || (nmed > 0 && st == -gen)) continue;
        }
        const int b = vb_div_small(u, invL), l = u - b * L;
        const size_t slot = (size_t)job;
        const int hint_id = vb_hint_pack(u, tx, ty);
        const int rx0 = tx * EHR_TILE_W - 1, ry0 = ty * EHR_TILE_H - 1;
        VbRegion rg;  // tile + 1-pixel halo, inside the image (coverage-only form: the tile alone, same origin)
        rg.x0 = COVER ? rx0 + 1 : max(rx0, 0);
        rg.y0 = COVER ? ry0 + 1 : max(ry0, 0);
        rg.x1 = min(rx0 + VB_RW - 1 - (COVER ? 1 : 0), W - 1);
        rg.y1 = min(ry0 + VB_RH - 1 - (COVER ? 1 : 0), H - 1);
        VB_WAVE_SYNC();
        if (!COVER) {
#pragma unroll
            for (int k = 0; k < VB_WORDS; k++) {
                const unsigned i = 64u * k + lane;
                if (i < (unsigned)VB_RN) S.key[i] = VB_EMPTY;
            }
        }
        if (lane < VB_RH) S.cov[lane] = 0ull;
        if (COVER && lane == 0) S.bad = 0;
        VB_WAVE_SYNC();
        int nsurv = 0, dln = 0;
        const int drawn = vb_job_raster<false, COVER, LAZY>(A, S, S.key, S.cov, b, l, rg, rx0, ry0, 0, 1, nsurv, dln);
        if (COVER) {
            // flagged units (their depth range must be tested per pixel: edge-on slivers mostly) are the only deferred ones
            if (drawn >= 0 && dln > 0)
                vb_flush<true, LAZY>(S, S.key, S.cov, dln, VbLazy{pverts, pmvp + ((size_t)b * L + l) * 16, LAZY ? nullptr : posc + (size_t)b * V}, PRM(si.cvidx) + (size_t)lcoff[l] * 64, W, H, rx0, ry0);
            VB_WAVE_SYNC();
            if (drawn < 0 || S.bad) {  // a triangle for the general path, or a drawn pixel with a depth <= 0: coverage cannot
                if (lane == 0) PRM(co.sticky)[0] = 1;  // decide here and the caller falls back for the whole call
                continue;
            }
            if (drawn > 0) {
                // the tile's 32 x 8 interior of the coverage rows, OR-ed into the (view, tile) words (all links of a view)
                VB_WAVE_SYNC();
                if (lane < 4) {
                    const u64 w = ((S.cov[2 * lane + 1] >> 1) & 0xffffffffull) | (((S.cov[2 * lane + 2] >> 1) & 0xffffffffull) << 32);
                    // (layout [candidate][tile][pose][4]: the count kernel reads a candidate's words of a tile in one piece)
                    if (w) atomicOr((unsigned long long*)&PRM(co.tcov)[((((size_t)(b / PRM(co.S)) * gnt + (size_t)ty * gntx + tx) * PRM(co.S) + (b % PRM(co.S))) * 4 + lane)], w);
                }
            }
            continue;
        }
        if (drawn < 0) {  // a triangle for the general path (near-plane clipping, huge extent): put the job aside
            if (lane == 0) vb_put_aside(PRM(rq.sl.slow_list), PRM(rq.meta), PRM(rq.sl.jn), job, u, tx, ty);
            continue;
        }
        if (dln > 0) vb_flush<false, LAZY>(S, S.key, S.cov, dln, VbLazy{pverts, pmvp + ((size_t)b * L + l) * 16, LAZY ? nullptr : posc + (size_t)b * V}, PRM(si.cvidx) + (size_t)lcoff[l] * 64, W, H, rx0, ry0);
        if (lane == 0) {
            if (nsurv >= heavy_t)
                remember_heavy(hint_id);
            else if (nsurv >= med_t)
                remember_long(hint_id);
        }
        if (drawn == 0) {  // the link's box touches this tile, its triangles do not
            if (lane == 0) PRM(rq.sl.jn)[slot] = -1;
            continue;
        }
        vb_resolve_from_lds<LAZY>(vb_prm_copy(&PRM(rq)), S, S.key, S.cov, slot, b, l, rx0, ry0);
    }
}
#undef PRM

// A whole job on one wave with the general triangle path compiled in (near-plane clipping, 64-bit edge functions): what a
// job falls back to when the lean code meets such a triangle; the wave resolves the job it has redrawn like the job kernel's
// waves do.  Runs in a kernel of its own (vb_slow_kernel) over the list of such jobs: compiled into the job kernel --
// inline or as a call, in the rounds or at the job loop's end -- the general path cost the lean code 50-70 spilled
// registers and 13 us at 8 views.
template <bool LAZY>
__device__ __forceinline__ void vb_job_slow(const VbJobArgs& A, const VbResolveArgs& Q, VbWaveLds& S, int job, int u, int tx,
                                            int ty) {
    const int lane = lane_id();
    const int b = u / A.L, l = u - b * A.L;
    const int rx0 = tx * EHR_TILE_W - 1, ry0 = ty * EHR_TILE_H - 1;
    VbRegion rg;
    rg.x0 = max(rx0, 0);
    rg.y0 = max(ry0, 0);
    rg.x1 = min(rx0 + VB_RW - 1, A.W - 1);
    rg.y1 = min(ry0 + VB_RH - 1, A.H - 1);
    VB_WAVE_SYNC();
#pragma unroll
    for (int k = 0; k < VB_WORDS; k++) {
        const unsigned i = 64u * k + lane;
        if (i < (unsigned)VB_RN) S.key[i] = VB_EMPTY;
    }
    if (lane < VB_RH) S.cov[lane] = 0ull;
    VB_WAVE_SYNC();
    int nsurv = 0, dln = 0;
    const int drawn = vb_job_raster<true, false, LAZY>(A, S, S.key, S.cov, b, l, rg, rx0, ry0, 0, 1, nsurv, dln);
    if (dln > 0) vb_flush<false, LAZY>(S, S.key, S.cov, dln, VbLazy{A.verts, A.mvp + ((size_t)b * A.L + l) * 16, A.posc ? A.posc + (size_t)b * A.V : nullptr}, A.cvidx + (size_t)A.lcoff[l] * 64, A.W, A.H, rx0, ry0);
    if (drawn > 0)
        vb_resolve_from_lds<LAZY>(Q, S, S.key, S.cov, (size_t)job, b, l, rx0, ry0);
    else if (lane == 0)
        Q.sl.jn[job] = -1;
}

// Stage 2a (normally empty): the jobs the lean code put aside, one wave each, with the general triangle path.  Takes the
// resolve stage's arguments and what the rasterizer needs beyond them.  (Not a hot kernel: its scalar spills do not matter,
// and both forms of the vertex look-up are compiled in, chosen per launch.)
__global__ void __launch_bounds__(256)
vb_slow_kernel(VbResolveArgs Q, VbRecs rc, int NC, const int4* __restrict__ cvidx, const int* __restrict__ lcoff) {
    const int n = *vb_line(Q.meta, VB_LINE_SLOW_COUNT);  // jobs put aside (vb_put_aside)
    if (n == 0) return;
    __shared__ VbWaveLds lds_all[4];
    const int wave = threadIdx.x >> 6;
    const VbJobArgs A = {Q.verts, Q.mvp, rc, NC, Q.V, Q.W, Q.H, Q.L, cvidx, Q.posc, lcoff};
    for (int i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
        const int4 e = Q.sl.slow_list[i];
        if (e.x >= Q.sl.jcap) continue;  // (no slot of that number: nothing of it may be written)
        if (Q.posc)
            vb_job_slow<false>(A, Q, lds_all[wave], e.x, e.y, e.z, e.w);
        else
            vb_job_slow<true>(A, Q, lds_all[wave], e.x, e.y, e.z, e.w);
    }
}

// Per (view, tile) of a BOUND reference mask: the fixed-point value the composite kernel would add to the view's frame
// loss for a tile no link touches (mask = 0, so the tile contributes sum(ref^2), summed exactly like vb_composite_kernel
// sums it: four pixels per lane, then the shuffle tree), and per view the total over all tiles.  The reference mask does
// not change during a solve, so these are constants of the solve (ehr_fused_bind_ref); with them the composite kernel only
// visits tiles inside the view's link boxes and adds fix(new) - cached there.  Integer sums are associative: bit-identical
// to streaming every tile.
// WEIGHTED (weights bound, ehr_fused_bind_weight): the cached value is sum(w ref^2), with the composite's own expression
// (e = 0 - r; we = w * e; e2 += we * e); view b of this launch is view wt.view0 + b of the plan.
template <bool WEIGHTED>
__global__ void __launch_bounds__(256)
vb_refsum_kernel(BinGeom g, int B, const float* __restrict__ ref, int vec_ok, long long* __restrict__ tsum,
                 long long* __restrict__ vtot, int* __restrict__ flag, VbWeight wt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gw = blockIdx.x * 4 + wave;
    if (gw >= B * g.nt) return;
    const int W = g.W, H = g.H;
    const int b = gw / g.nt, tile = gw - b * g.nt;
    const int tx = tile % g.ntx, ty = tile / g.ntx;
    const int r = lane >> 3, c4 = (lane & 7) * 4;
    const int ix = tx * EHR_TILE_W + c4, iy = ty * EHR_TILE_H + r;
    const bool row_in = iy < H;
    const size_t im = ((size_t)b * H + (H - 1 - (row_in ? iy : 0))) * W + ix;
    float rf[4] = {0.f, 0.f, 0.f, 0.f};
    bool pin[4];
#pragma unroll
    for (int j = 0; j < 4; j++) pin[j] = row_in && (ix + j) < W;
    if (vec_ok) {
        if (pin[0]) {
            const float4 r4 = *reinterpret_cast<const float4*>(ref + im);
            rf[0] = r4.x; rf[1] = r4.y; rf[2] = r4.z; rf[3] = r4.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (pin[j]) rf[j] = ref[im + j];
    }
    float wf[4] = {0.f, 0.f, 0.f, 0.f};
    if (WEIGHTED) vb_read_weights(wt, b, H, W, H - 1 - (row_in ? iy : 0), ix, pin, vec_ok, wf);
    float e2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (pin[j]) {
            const float e = 0.f - rf[j];
            if (WEIGHTED) {
                const float we = wf[j] * e;
                e2 += we * e;
            } else {
                e2 += e * e;
            }
        }
    const float s = wave_sum(e2);
    if (lane == 0) {
        long long q = 0;
        if (!(fabsf(s) < 1.0e9f))
            atomicOr(flag, 1);  // every step on this reference reports the overflow (loss = NaN)
        else if (s != 0.f)
            q = fix_of(s);
        tsum[gw] = q;
        if (q != 0) atomicAdd((unsigned long long*)&vtot[b], (unsigned long long)q);
    }
}

// The composite kernel's kernarg segment as its finish section reads it (see there and vb_job_params)
struct VbCompParams {
    VbCompArgs C;
    StepTail tail;
};
struct VbCompParamsW {  // ... and as a WEIGHTED instantiation reads its last parameter
    VbCompArgs C;
    StepTail tail;
    VbSharedRef sh;
    VbWeight wt;
};
__device__ __forceinline__ VbCompParamsWPtr vb_comp_params_w() {
    return (VbCompParamsWPtr)__builtin_amdgcn_kernarg_segment_ptr();
}
__device__ __forceinline__ VbWeight vb_comp_weight(VbCompParamsWPtr p) {
    VbWeight wt;
    wt.w = p->wt.w;
    wt.view0 = p->wt.view0;
    wt.nviews = p->wt.nviews;
    return wt;
}
typedef const VbCompParams __attribute__((address_space(4)))* VbCompParamsPtr;
__device__ __forceinline__ VbCompParamsPtr vb_comp_params() {
    VbCompParamsPtr p = (VbCompParamsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// (how many workgroups arrive on which XCD's counter: vb_comp_arrivals, vb_comp_expected in ehr_arrive.h)
constexpr int VB_FINISH_POLLS = 1 << 21;  // bound of the finisher's wait, ~0.5 us a poll

// Stage 3: one WAVE per 32x8 tile (4 pixels per lane, float4 image accesses, no workgroup barriers): sums the links'
// values in link order, clamps, accumulates the frame loss, writes the mask, and back-propagates the tile's blended
// pairs to 12 numbers per link which go to the view's fixed-point accumulators.  Persistent waves over
//   tsum == NULL: every tile of every view (tiles no link box touches just stream: mask = 0, loss += ref^2);
//   tsum != NULL (bound reference mask): the tiles of the views' link rectangles only; a tile that no link contributes
//                 to is skipped without reading the reference -- its cached sum is already in vtot.  With a mask output
//                 the tiles outside every rectangle are then filled with zeros (stores only, no reference read, no sums).
// One designated workgroup of the call's last launch (the finisher, see below) runs the finish stage: accumulators ->
// loss / grad_mvp [-> pose backward -> Adam]; the launch also re-arms the link boxes.  vec_ok: W % 4 == 0 and 16-byte aligned images
// (reference, mask output and, where bound, weights).
template <bool TAIL, bool FILL, bool SHARED = false, bool WEIGHTED = false>
__global__ void __launch_bounds__(256, FILL ? 5 : 6)
vb_composite_kernel(VbCompArgs C, StepTail tail, VbSharedRef sh, VbWeight wt) {
    __shared__ float gpix_all[4][EHR_TILE_W * EHR_TILE_H];
    extern __shared__ int s_dyn[];  // [U + 1] first job of every (view, link) | [U] its tile range
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const gpix = gpix_all[wave];
    const int U = C.B * C.g.L;
    int* const s_jbase = s_dyn;
    unsigned* const s_utile = reinterpret_cast<unsigned*>(s_dyn + U + 1);
    const bool sparse = C.tsum != nullptr;
    for (int i = tid; i <= U; i += 256) s_jbase[i] = C.sl.jbase[i];
    for (int i = tid; i < U; i += 256) s_utile[i] = C.sl.jutile[i];
    // The links' screen boxes start "empty" in the next step.  Nobody reads them after the job kernel's prologue, so the
    // call's last composite launch re-arms them here, a store per thread of its first workgroups, instead of in the
    // finish stage at its end (where it was 32 stores per thread on the step's critical path).
    if (C.do_finish && C.lbox_all)
        for (int i = (int)blockIdx.x * 256 + tid; i < VB_LBOX_STRIDE * C.B_all * C.g.L; i += (int)gridDim.x * 256)
            C.lbox_all[i] = (i & 2) ? INT_MIN : INT_MAX;  // one line per box: min x, min y, max x, max y, padding
    __syncthreads();
    const int nwg = gridDim.x, xcd = blockIdx.x & (VB_XCDS - 1);
    vb_composite_items<FILL, SHARED, WEIGHTED>(C, s_jbase, s_utile, gpix, xcd, (int)(blockIdx.x >> VB_XCD_BITS) * 4 + wave, (nwg >> VB_XCD_BITS) * 4, nwg, sh);
    // ---- the finish stage: ONE designated workgroup, the finisher, runs it once every other workgroup's atomics have
    //      been performed.  A workgroup that had work waits for its own atomics (vmcnt covers them), then one lane adds 1
    //      to its XCD's arrival counter -- no value comes back, nobody waits for one -- and the workgroup is done.  A
    //      workgroup without work does not arrive at all: how many of an XCD's workgroups have work follows from the
    //      tables every workgroup holds (vb_comp_arrivals), so the finisher knows each counter's final value.  It requests
    //      what the finish needs besides the accumulators (finish_prefetch) while the others composite, polls the eight
    //      counters, then reduces.  One line per XCD counter: arrivals on one address serialise at ~12 ns each.
    //      Nobody resets the counters here (the stores' round trip was on the step's chain): the vertex kernel's first
    //      workgroup zeroes every counter line at the start of every step and of every later chunk, and every launch of
    //      this kernel has a vertex launch of its chain (vbuf_chain, replayed whole by a graph) in front of it.
    //      Forward progress does not depend on co-residency: only the finisher waits, and only for workgroups that wait
    //      for nobody.  Dispatched early it holds one of a CU's slots while the others run; dispatched last it finds the
    //      counters complete.  The accumulators are only ever touched by agent-scope atomics and read back with
    //      agent-scope loads (acc_load), so no cache maintenance is needed between the two.
    if (!vb_comp_params()->C.do_finish) return;  // (not the last chunk of views: the kernel boundary orders its sums before the last chunk's finish)
    // (What follows reads its parameters where it needs them, through the kernarg pointer (vb_comp_params): taken from
    //  the by-value struct they would be scalar registers kept -- spilled -- across the whole tile loop above.)
    const VbCompParamsPtr Q = vb_comp_params();
    const int per = nwg >> VB_XCD_BITS;  // workgroups per XCD (nwg is a multiple of VB_XCDS)
    const int nitems = sparse ? min(s_jbase[U], Q->C.sl.jcap) : Q->C.B * Q->C.g.nt;
    const int nfill = FILL ? Q->C.B * Q->C.g.nt : 0, nlbox = Q->C.lbox_all ? VB_LBOX_STRIDE * Q->C.B_all * Q->C.g.L : 0;
    const int kblk = (int)(blockIdx.x >> VB_XCD_BITS);
    const bool finisher = (int)blockIdx.x == nwg - VB_XCDS;  // the highest workgroup of XCD 0: the last to get an item there
    const bool arrives = kblk < vb_comp_arrivals(xcd, per, nitems, nfill, nlbox);
    if (!finisher) {
        if (!arrives) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // (relaxed, behind the vmcnt and the barrier: what the finisher reads was written by agent-scope atomics that
        //  have been performed by now.  A release here makes every arriving workgroup write its L2 back first -- +12 us
        //  a step, profiles/r08_waiting_finisher.md.)
        if (tid == 0)
            (void)__hip_atomic_fetch_add(vb_line(Q->C.meta, VB_LINE_COMP_ARRIVE + xcd), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    __shared__ double S[4][17];
    __shared__ float red_lds[8];
    __shared__ float Js[6][16];
    const long long* const vtot = sparse ? Q->C.vtot_all : nullptr;
    const BinGeom g = ((const VbCompParams*)Q)->C.g;  // (struct copies: through a generic pointer, still scalar loads)
    const StepTail tl = ((const VbCompParams*)Q)->tail;
    FinishPre pre;
    __syncthreads();  // (every wave is done with its gpix: the link poses go there)
    finish_prefetch<TAIL>(pre, g, Q->C.B_all, vtot, tl, Q->C.nls, Js, gpix_all[0]);
    if (Q->C.ref_flag && tid == 0 && Q->C.ref_flag[0]) atomicOr(&Q->C.meta[EHR_META_OVERFLOW], 1);  // the bound reference's own sums overflowed
    if (wave == 0) {
        // lane x < 8 watches XCD x's counter (the finisher itself is not counted).  The wait is bounded: a count that
        // never completes (it cannot, short of a fault elsewhere) is reported as an overflow -- loss = NaN, pose
        // untouched -- after about a second instead of holding the device.
        int* const ctr = vb_line(Q->C.meta, VB_LINE_COMP_ARRIVE + (lane & (VB_XCDS - 1)));
        const int want = vb_comp_expected(lane & (VB_XCDS - 1), per, nitems, nfill, nlbox);
        bool done = false;
        for (int polls = 0; polls < VB_FINISH_POLLS; polls++) {
            const int have = (lane < VB_XCDS) ? __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
            done = __ballot(have < want) == 0;
            if (done) break;
            __builtin_amdgcn_s_sleep(2);
        }
        if (!done && lane == 0) atomicOr(&Q->C.meta[EHR_META_OVERFLOW], 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the finisher's own sums, if it had items)
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    finish_reduce<TAIL>(pre, g, Q->C.B_all, Q->C.facc_all, vtot, Q->C.loss, Q->C.grad_mvp, Q->C.meta, tl, Q->C.nls, VB_LOSS_STRIDE, S, red_lds, Js, gpix_all[0]);
}

// The finish stage of a multi-start step (ehr_solver_step_multi): ONE WORKGROUP PER HYPOTHESIS, a launch of its own behind
// the call's last composite launch (which then has no finisher).  Workgroup p runs finish_prefetch / finish_reduce<TAIL> --
// the bodies the single-pose finisher runs -- on hypothesis p's Bv views and state, so its sums are the expression tree of
// a solo step with B = Bv, bit for bit, and the P accumulate -> reduce -> Adam chains run side by side.  The overflow word
// is the step's: a reported step freezes every hypothesis.  Also re-arms the link boxes (the composite launch's job
// where it finishes).
__global__ void __launch_bounds__(256)
vb_finish_multi_kernel(MultiFinish A, StepTail tail) {
    __shared__ double S[4][17];
    __shared__ float red_lds[8];
    __shared__ float Js[6][16];
    __shared__ float lp_lds[1024];
    const int p = blockIdx.x, tid = threadIdx.x, L = A.g.L;
    for (int i = p * 256 + tid; i < VB_LBOX_STRIDE * A.P * A.Bv * L; i += (int)gridDim.x * 256)
        A.lbox_all[i] = (i & 2) ? INT_MIN : INT_MAX;
    tail.tc_jac += 7 * 16 * p;
    tail.red += 8 * p;
    tail.dof += 6 * p;
    tail.m += 6 * p;
    tail.v += 6 * p;
    tail.step += p;
    if (tail.loss_out) tail.loss_out += p;
    if (tail.grad_out) tail.grad_out += 6 * p;
    const size_t v0 = (size_t)p * A.Bv;
    const long long* const vtot = A.vtot_all ? A.vtot_all + v0 : nullptr;
    FinishPre pre;
    finish_prefetch<true>(pre, A.g, A.Bv, vtot, tail, A.nls, Js, lp_lds);
    if (A.ref_flag && tid == 0 && A.ref_flag[0]) atomicOr(&A.meta[EHR_META_OVERFLOW], 1);  // the bound reference's own sums overflowed
    __syncthreads();
    finish_reduce<true>(pre, A.g, A.Bv, A.facc_all + v0 * vb_acc_stride(L, A.nls), vtot, A.loss + v0,
                        A.grad_mvp + v0 * L * 16, A.meta, tail, A.nls, VB_LOSS_STRIDE, S, red_lds, Js, lp_lds);
}

// Content hash of the scoring op's mesh arrays: the cluster index holds copies of the vertex positions, so a mesh edited
// in place under the same pointers must rebuild it.  Every (word, position) pair goes through a 64-bit finaliser
// (murmur3's fmix64) before it is summed: a sum of the raw words, however weighted, is linear, and two compensating
// edits would cancel; the sum of the mixed values is still order independent.
__global__ void __launch_bounds__(256)
vb_hash_kernel(const unsigned* __restrict__ a, size_t na, const unsigned* __restrict__ b, size_t nb, const unsigned* __restrict__ c,
               size_t nc, unsigned long long* __restrict__ out) {
    unsigned long long h = 0;
    const size_t n = na + nb + nc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned w = i < na ? a[i] : (i < na + nb ? b[i - na] : c[i - na - nb]);
        unsigned long long x = (unsigned long long)w + 0x9e3779b97f4a7c15ull * ((unsigned long long)i + 1ull);
        x ^= x >> 33;
        x *= 0xff51afd7ed558ccdull;
        x ^= x >> 33;
        x *= 0xc4ceb9fe1a85ec53ull;
        x ^= x >> 33;
        h += x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, h);
}

// Scoring op, last stage: one wave per (candidate, tile), four pixels per lane: c = number of the candidate's S views
// whose coverage word has the pixel's bit, score[q] += sum c (S - c) (space_explorer.py:152-165: the summed unbiased
// variance of S binary masks is that integer over S (S - 1)); optionally the count image (row 0 = top).  Also re-arms
// the link boxes for the next chunk of views.
__global__ void __launch_bounds__(256)
vb_score_count_kernel(BinGeom g, int nq, int S, const u64* __restrict__ tcov, unsigned long long* __restrict__ sacc,
                      unsigned char* __restrict__ count_img, int* __restrict__ lbox, int nlbox,
                      unsigned long long* __restrict__ prev_sacc, long long* __restrict__ prev_score, int prev_nq) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nlbox; i += gridDim.x * 256) lbox[i] = (i & 2) ? INT_MIN : INT_MAX;
    // The sums of a chunk are collected in scratch, one 128-byte line per candidate (a few hundred atomics per candidate:
    // on the caller's packed int64 array they would all hit one line and serialise at ~25 ns each), and stored to the
    // caller's array by the NEXT launch of this kernel (the last one has nq = 0).
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < prev_nq; i += 256) {
            prev_score[i] = (long long)prev_sacc[16 * i];
            prev_sacc[16 * i] = 0ull;
        }
    const int r = lane >> 3, c4 = (lane & 7) * 4;
    const int sh = (r & 1) * 32 + c4;
    // persistent waves (a workgroup per four items would be bound by the rate workgroups are dispatched at)
    for (int item = blockIdx.x * 4 + wave; item < nq * g.nt; item += gridDim.x * 4) {
    const int q = item / g.nt, tile = item - q * g.nt;
    int c[4] = {0, 0, 0, 0};
    // one round trip per 16 views: lane 4 s + k requests word k of view s, the words then go round by readlane
    for (int s0 = 0; s0 < S; s0 += 16) {
        const int ls = s0 + (lane >> 2);
        const u64 mine = (ls < S) ? tcov[(((size_t)q * g.nt + tile) * S + ls) * 4 + (lane & 3)] : 0ull;
        if (__ballot(mine != 0ull) == 0) continue;  // (most tiles hold nothing)

        const int ns = min(16, S - s0);
        for (int k = 0; k < ns; k++) {
            const int src = 4 * k + (r >> 1);
            const unsigned lo = (unsigned)__shfl((int)(unsigned)mine, src, 64), hi = (unsigned)__shfl((int)(unsigned)(mine >> 32), src, 64);
            const unsigned bits = (unsigned)(((((u64)hi) << 32) | lo) >> sh) & 15u;
#pragma unroll
            for (int j = 0; j < 4; j++) c[j] += (bits >> j) & 1u;
        }
    }
    int v = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) v += c[j] * (S - c[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0 && v) atomicAdd(&sacc[16 * q], (unsigned long long)v);
    if (count_img) {
        const int tx = tile % g.ntx, ty = tile / g.ntx;
        const int ix = tx * EHR_TILE_W + c4, iy = ty * EHR_TILE_H + r;
        if (iy < g.H)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ix + j < g.W && c[j]) count_img[((size_t)q * g.H + (g.H - 1 - iy)) * g.W + ix + j] = (unsigned char)c[j];
    }
    }
}

static_assert(EHR_TILE_W == 32 && EHR_TILE_H == 8, "coverage words: four u64 per tile, word r >> 1 holds row r at bit (r & 1) * 32 + col");

// Pose search (ehr_mask_overlap), once per call: the observed masks ref [S][H][W] (row 0 = top; foreground iff > 0.5f, so
// NaN is background) in the bit layout of the coverage words, rbits [S][nt][4], and their areas.  One wave per tile, lane
// = (tile row, four columns) as in the count kernel above: eight lanes read 128 contiguous bytes of an image row, the 16
// lanes of a word OR their shifted nibbles together.  Pixels beyond W / H pack as 0.  blockIdx.y = view; a wave adds
// its tiles' popcounts up and issues one atomic.
__global__ void __launch_bounds__(256)
vb_overlap_pack_ref_kernel(BinGeom g, const float* __restrict__ ref, u64* __restrict__ rbits,
                           unsigned long long* __restrict__ ref_area) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = blockIdx.y;
    const int r = lane >> 3, c4 = (lane & 7) * 4;
    const int sh = (r & 1) * 32 + c4;
    const float* const img = ref + (size_t)s * g.H * g.W;
    unsigned n = 0;
    for (int tile = blockIdx.x * 4 + wave; tile < g.nt; tile += gridDim.x * 4) {
        const int tx = tile % g.ntx, ty = tile / g.ntx;
        const int ix = tx * EHR_TILE_W + c4, iy = ty * EHR_TILE_H + r;
        unsigned bits = 0;
        if (iy < g.H) {
            const float* const row = img + (size_t)(g.H - 1 - iy) * g.W;  // tile rows count from the image's bottom
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ix + j < g.W && row[ix + j] > 0.5f) bits |= 1u << j;
        }
        u64 w = (u64)bits << sh;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) w |= __shfl_xor(w, o, 64);
        if ((lane & 15) == 0) {
            rbits[((size_t)s * g.nt + tile) * 4 + (lane >> 4)] = w;
            n += __popcll(w);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0 && n) atomicAdd(&ref_area[s], (unsigned long long)n);
}

// Pose search, last stage of a chunk: per (candidate, view) the integers |render| and |render & ref|.  Persistent waves;
// a wave owns `per_wave` CONSECUTIVE (candidate, tile) items, lane 4 s + k fetches coverage word k of view s (16 views per
// round trip, four tiles in flight) and, where the tile holds anything at all, the matching word of rbits (L2 resident,
// shared by every candidate).  Each lane keeps the popcounts of its own word in two registers across the tiles of a
// candidate; only when the candidate changes or the range ends are the four lanes of a view summed and flushed with ONE
// 64-bit integer atomic, area << 32 | inter (both <= H W <= 2^30, so the halves never carry into each other), on a
// 128-byte line of the (candidate, view)'s own -- the serialisation the comment in vb_score_count_kernel records, divided
// by per_wave.  S > 16: the range is walked once per block of 16 views, so the registers do not grow with S.  Like
// vb_score_count_kernel it re-arms the link boxes and hands the PREVIOUS chunk's sums to the caller's packed [.,S,2] array
// with plain stores (the last launch has nq = 0).
__global__ void __launch_bounds__(256)
vb_overlap_count_kernel(BinGeom g, int nq, int S, int per_wave, const u64* __restrict__ tcov, const u64* __restrict__ rbits,
                        unsigned long long* __restrict__ oacc, int* __restrict__ lbox, int nlbox,
                        unsigned long long* __restrict__ prev_oacc, long long* __restrict__ prev_out, int prev_n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nlbox; i += gridDim.x * 256) lbox[i] = (i & 2) ? INT_MIN : INT_MAX;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < prev_n; i += 256) {
            const unsigned long long v = prev_oacc[16 * (size_t)i];
            prev_out[2 * (size_t)i] = (long long)(v & 0xffffffffull);
            prev_out[2 * (size_t)i + 1] = (long long)(v >> 32);
            prev_oacc[16 * (size_t)i] = 0ull;
        }
    const long long total = (long long)nq * g.nt;
    const long long first = (long long)(blockIdx.x * 4 + wave) * per_wave;
    if (first >= total) return;
    const int i0 = (int)first, i1 = (int)min(total, first + per_wave);
    const int k = lane & 3;
    for (int s0 = 0; s0 < S; s0 += 16) {
        const int ls = s0 + (lane >> 2);
        const bool on = ls < S;
        const u64* const cov = tcov + (size_t)(on ? ls : 0) * 4 + k;            // + item * S * 4
        const u64* const rb = rbits + (size_t)(on ? ls : 0) * g.nt * 4 + k;     // + tile * 4
        unsigned inter = 0, area = 0;
        int q = i0 / g.nt, tile = i0 - q * g.nt;
        auto flush = [&]() {
            inter += __shfl_xor(inter, 1, 64);
            inter += __shfl_xor(inter, 2, 64);
            area += __shfl_xor(area, 1, 64);
            area += __shfl_xor(area, 2, 64);
            if (k == 0 && area) atomicAdd(&oacc[16 * ((size_t)q * S + ls)], ((unsigned long long)area << 32) | inter);
            inter = area = 0;
        };
        for (int i = i0; i < i1; i += 4) {
            u64 m[4];
#pragma unroll
            for (int j = 0; j < 4; j++) m[j] = (on && i + j < i1) ? cov[(size_t)(i + j) * S * 4] : 0ull;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (i + j >= i1) break;                       // (wave-uniform)
                if (__ballot(m[j] != 0ull) != 0) {            // (most tiles hold nothing)
                    const u64 rw = on ? rb[(size_t)tile * 4] : 0ull;
                    area += __popcll(m[j]);
                    inter += __popcll(m[j] & rw);
                }
                if (++tile == g.nt) {                         // the candidate changes
                    flush();
                    tile = 0;
                    q++;
                }
            }
        }
        if (tile != 0) flush();
    }
}

// Pose search, soft score (ehr_mask_cost), once per call: the cost images cost [C][S][H][W] (int32, row 0 = top) in a
// tile-major layout that follows the coverage words' bit order, cpack [S][nt][C][256]: value 32 r + col of a tile is the
// pixel of coverage bit (r & 1) * 32 + col of word r >> 1, so the four pixels under nibble n of word w are the int4 at
// 16 w + n -- lane = (tile row, four columns) as in vb_overlap_pack_ref_kernel, and a wave stores a channel's tile as one
// contiguous KB.  Pixels beyond W / H cost 0.  blockIdx.y = view, blockIdx.z = channel.
__global__ void __launch_bounds__(256)
vb_cost_pack_kernel(BinGeom g, const int32_t* __restrict__ cost, int S, int C, int32_t* __restrict__ cpack) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = blockIdx.y, c = blockIdx.z;
    const int r = lane >> 3, c4 = (lane & 7) * 4;
    const int32_t* const img = cost + ((size_t)c * S + s) * g.H * g.W;
    for (int tile = blockIdx.x * 4 + wave; tile < g.nt; tile += gridDim.x * 4) {
        const int tx = tile % g.ntx, ty = tile / g.ntx;
        const int ix = tx * EHR_TILE_W + c4, iy = ty * EHR_TILE_H + r;
        int v[4] = {0, 0, 0, 0};
        if (iy < g.H) {
            const int32_t* const row = img + (size_t)(g.H - 1 - iy) * g.W;  // tile rows count from the image's bottom
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ix + j < g.W) v[j] = row[ix + j];
        }
        reinterpret_cast<int4*>(cpack + (((size_t)s * g.nt + tile) * C + c) * 256)[lane] = make_int4(v[0], v[1], v[2], v[3]);
    }
}

// Sums C per-lane values over the wave, all channels in one pass: the first two exchanges (xor 1, xor 2) halve the channels
// a lane carries, the other four are a plain butterfly.  Every lane ends with the wave's total of channel lane & 3 (C > 2),
// lane & 1 (C == 2) or the only one: 6 or 7 64-bit shuffles instead of 6 C.
template <int C>
__device__ __forceinline__ long long vb_cost_wave_sum(const long long (&t)[C], int lane) {
    long long x = t[0];
    if constexpr (C >= 2) {
        const bool odd = lane & 1;
        x = (odd ? t[1] : t[0]) + __shfl_xor(odd ? t[0] : t[1], 1, 64);                 // channel lane & 1
        if constexpr (C > 2) {
            const long long t3 = (C > 3) ? t[C - 1] : 0ll;
            const long long y = (odd ? t3 : t[2]) + __shfl_xor(odd ? t[2] : t3, 1, 64);  // channel 2 + (lane & 1)
            const bool up = lane & 2;
            x = (up ? y : x) + __shfl_xor(up ? x : y, 2, 64);                           // channel lane & 3
        } else {
            x += __shfl_xor(x, 2, 64);
        }
    } else {
        x += __shfl_xor(x, 1, 64);
        x += __shfl_xor(x, 2, 64);
    }
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// Pose search, soft score, last stage of a chunk: per (candidate, view) the integers |render| and, per channel, the sum
// of the cost under the render.  A wave owns `per_wave` tiles of ONE candidate, a stride of nt / per_wave apart: the covered
// tiles, where all the fetching is, lie together, and a strided range hands every wave of a candidate about the same
// number of them (consecutive ranges left a tenth of the waves with all the work).  As in vb_overlap_count_kernel lane
// 4 s + k fetches coverage word k of view s, 16 views per round trip, four tiles in flight.  Only where a (candidate, view, tile) holds a set bit at all are its cost values fetched, U views a turn so that
// their loads are in flight together: the wave takes a view's four words by shuffle, lane l looks at nibble l & 15 of word
// l >> 4 and, if it is not empty, loads the int4 under it per channel (a KB per channel when every lane does); the picked
// values are summed over the wave in 64 bits (vb_cost_wave_sum) and lane 4 s + c of the view keeps channel c's total next to
// its word's popcount.  Flushed once per wave and block of 16 views: one 64-bit integer atomic per value on the
// (candidate, view)'s own 128-byte line {area, sum_0 .. sum_{C-1}} (two's complement: a sum of negative costs wraps to the
// right int64).  Re-arms the link boxes and hands the PREVIOUS chunk's lines to the caller's packed [.,S,C+1] array with
// plain stores, like the overlap kernel (the last launch has nq = 0).
template <int C>
__global__ void __launch_bounds__(256)
vb_cost_count_kernel(BinGeom g, int nq, int S, int per_wave, const u64* __restrict__ tcov, const int32_t* __restrict__ cpack,
                     unsigned long long* __restrict__ cacc, int* __restrict__ lbox, int nlbox,
                     unsigned long long* __restrict__ prev_cacc, long long* __restrict__ prev_out, int prev_n) {
    static_assert(C >= 1 && C <= 4, "a view's four lanes keep one channel each");
    constexpr int U = C <= 2 ? 4 : 2;  // views whose cost loads are in flight together (U C int4 per lane)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nlbox; i += gridDim.x * 256) lbox[i] = (i & 2) ? INT_MIN : INT_MAX;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < prev_n; i += 256)
#pragma unroll
            for (int c = 0; c <= C; c++) {
                prev_out[(C + 1) * (size_t)i + c] = (long long)prev_cacc[16 * (size_t)i + c];
                prev_cacc[16 * (size_t)i + c] = 0ull;
            }
    const int wq = (g.nt + per_wave - 1) / per_wave;       // waves per candidate
    const long long wid = (long long)blockIdx.x * 4 + wave;
    if (wid >= (long long)nq * wq) return;
    const int q = (int)(wid / wq), r = (int)(wid - (long long)q * wq);  // this wave: tiles r, r + wq, r + 2 wq, .. of candidate q
    const int k = lane & 3;
    const int sub = lane >> 4, nib = (lane & 15) * 4;
    for (int s0 = 0; s0 < S; s0 += 16) {
        const int ls = s0 + (lane >> 2);
        const bool on = ls < S;
        const u64* const cov = tcov + ((size_t)q * g.nt * S + (on ? ls : 0)) * 4 + k;   // + tile * S * 4
        unsigned area = 0;
        long long csum = 0;
        for (int t0 = r; t0 < g.nt; t0 += 4 * wq) {
            u64 m[4];
#pragma unroll
            for (int j = 0; j < 4; j++) m[j] = (on && t0 + j * wq < g.nt) ? cov[(size_t)(t0 + j * wq) * S * 4] : 0ull;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int tile = t0 + j * wq;
                if (tile >= g.nt) break;                      // (wave-uniform)
                const u64 nz = __ballot(m[j] != 0ull);
                if (nz == 0) continue;                        // (most tiles hold nothing)
                area += __popcll(m[j]);
                u64 vm = (nz | (nz >> 1) | (nz >> 2) | (nz >> 3)) & 0x1111111111111111ull;  // bit 4 v: view s0 + v holds something
                while (vm) {                                  // (wave-uniform) U views a turn: their loads are in flight together
                    int sl[U];
                    unsigned bits[U];
                    int4 v[U][C];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        sl[u] = vm ? __builtin_ctzll(vm) : -1;
                        vm &= vm - 1;
                        bits[u] = 0;
                        if (sl[u] >= 0) {
                            const unsigned lo = (unsigned)__shfl((int)(unsigned)m[j], sl[u] + sub, 64);
                            const unsigned hi = (unsigned)__shfl((int)(unsigned)(m[j] >> 32), sl[u] + sub, 64);
                            bits[u] = (unsigned)(((((u64)hi) << 32) | lo) >> nib) & 15u;
                        }
                        const int4* const p = reinterpret_cast<const int4*>(cpack + (((size_t)(s0 + (max(sl[u], 0) >> 2)) * g.nt + tile) * C) * 256) + lane;
#pragma unroll
                        for (int c = 0; c < C; c++) v[u][c] = bits[u] ? p[c * 64] : make_int4(0, 0, 0, 0);
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (sl[u] < 0) break;
                        long long t[C];
#pragma unroll
                        for (int c = 0; c < C; c++)
                            t[c] = (long long)((bits[u] & 1u) ? v[u][c].x : 0) + (long long)((bits[u] & 2u) ? v[u][c].y : 0) +
                                   (long long)((bits[u] & 4u) ? v[u][c].z : 0) + (long long)((bits[u] & 8u) ? v[u][c].w : 0);
                        const long long mine = vb_cost_wave_sum<C>(t, lane);
                        if ((lane & ~3) == sl[u] && k < C) csum += mine;
                    }
                }
            }
        }
        area += __shfl_xor(area, 1, 64);
        area += __shfl_xor(area, 2, 64);
        if (area) {  // (then the view exists; no coverage, no cost)
            unsigned long long* const line = cacc + 16 * ((size_t)q * S + ls);
            if (k == 0) atomicAdd(&line[0], (unsigned long long)area);
            if (k < C && csum) atomicAdd(&line[1 + k], (unsigned long long)csum);
        }
    }
}

// [T][3] int32 -> [T] int4 (one aligned 16-byte gather per triangle in the silhouette analysis)
__global__ void vb_pad_kernel(const int32_t* __restrict__ a, int T, int4* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T) out[t] = make_int4(a[3 * t], a[3 * t + 1], a[3 * t + 2], 0);
}

}  // namespace ehr
using namespace ehr;

// ---- host side ------------------------------------------------------------------------------------------------------

// Reorders idx[0..n) (indices into the centroid array) in place: median split along the longest axis, left part
// rounded to a multiple of 64, recursively.  Against a Morton curve of the centroids (first version) the clusters'
// screen boxes touch a third fewer tiles (xArm7 at 720p: 4.4 k instead of 6.5 k cluster-tile pairs per view), i.e. a third
// fewer candidate clusters per job.
static void vb_kd_order(const float* cen, int* idx, int n) {
    if (n <= 64) return;
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const float c = cen[3 * (size_t)idx[i] + k];
            lo[k] = std::min(lo[k], c);
            hi[k] = std::max(hi[k], c);
        }
    int ax = 0;
    if (hi[1] - lo[1] > hi[ax] - lo[ax]) ax = 1;
    if (hi[2] - lo[2] > hi[ax] - lo[ax]) ax = 2;
    const int half = std::min(std::max(((n / 2 + 63) / 64) * 64, 64), n - 1);
    std::nth_element(idx, idx + half, idx + n, [&](int a, int b) {
        const float ca = cen[3 * (size_t)a + ax], cb = cen[3 * (size_t)b + ax];
        return ca < cb || (ca == cb && a < b);  // index as tie-break: the same scene always gives the same clusters
    });
    vb_kd_order(cen, idx, half);
    vb_kd_order(cen, idx + half, n - half);
}

// Static acceleration index of a scene: per link, the triangles ordered by a median-split tree over their centroids (object
// space, so it holds for every pose) and cut into clusters of 64.  Triangle ids stay the caller's: depth ties and the
// antialias topology are unaffected.
// tri_link == NULL: the links come from vert_link (the scoring op's packed mesh): a triangle belongs to the link of its
// vertices; *mixed is set if a triangle's vertices disagree or the triangles are not grouped by link (the caller then
// keeps to the per-triangle path).
static int vb_build_clusters(Scratch& out, int& nc_out, int L, int V, int T, const float* verts, const int32_t* tris,
                             const int32_t* tri_link, const int32_t* vert_link = nullptr, bool* mixed = nullptr) {
    std::vector<float> hv((size_t)3 * std::max(V, 1));
    std::vector<int32_t> ht((size_t)3 * std::max(T, 1)), hl((size_t)std::max(T, 1));
    if (V > 0) EHR_HIP(hipMemcpy(hv.data(), verts, (size_t)3 * V * sizeof(float), hipMemcpyDeviceToHost));
    if (T > 0) {
        EHR_HIP(hipMemcpy(ht.data(), tris, (size_t)3 * T * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (tri_link) {
            EHR_HIP(hipMemcpy(hl.data(), tri_link, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost));
        } else {
            std::vector<int32_t> vl((size_t)std::max(V, 1), 0);
            if (V > 0) EHR_HIP(hipMemcpy(vl.data(), vert_link, (size_t)V * sizeof(int32_t), hipMemcpyDeviceToHost));
            int prev = 0;
            for (int t = 0; t < T; t++) {
                int lk[3];
                for (int j = 0; j < 3; j++) {
                    const int v = ht[3 * (size_t)t + j];
                    lk[j] = ((unsigned)v < (unsigned)V) ? vl[v] : -1;
                }
                if (lk[0] != lk[1] || lk[0] != lk[2] || (unsigned)lk[0] >= (unsigned)L || lk[0] < prev) {
                    *mixed = true;
                    return EHR_OK;
                }
                prev = lk[0];
                hl[t] = lk[0];
            }
        }
    }
    std::vector<int32_t> ctri, clink, coff((size_t)L + 1, 0);
    std::vector<float> aabb((size_t)6 * L);
    for (int l = 0; l < L; l++)
        for (int k = 0; k < 3; k++) {
            aabb[6 * (size_t)l + k] = 3.4e38f;
            aabb[6 * (size_t)l + 3 + k] = -3.4e38f;
        }
    int t = 0;
    for (int l = 0; l < L; l++) {
        coff[l] = (int32_t)clink.size();
        const int t0 = t;
        while (t < T && hl[t] == l) t++;
        if (t < T && hl[t] < l) return fail(EHR_ERR_INVALID, "ehr_fused_plan: tri_link must be sorted by link");
        const int n = t - t0;
        if (n == 0) continue;
        std::vector<float> cen((size_t)3 * n);
        float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
        for (int i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) {
                float c = 0.f;
                for (int j = 0; j < 3; j++) {
                    const int v = ht[3 * (size_t)(t0 + i) + j];
                    const float x = ((unsigned)v < (unsigned)V) ? hv[3 * (size_t)v + k] : 0.f;
                    c += x;
                    if ((unsigned)v < (unsigned)V) {
                        aabb[6 * (size_t)l + k] = std::min(aabb[6 * (size_t)l + k], x);
                        aabb[6 * (size_t)l + 3 + k] = std::max(aabb[6 * (size_t)l + 3 + k], x);
                    }
                }
                c *= (1.f / 3.f);
                if (!(c == c)) c = 0.f;
                cen[3 * (size_t)i + k] = c;
                lo[k] = std::min(lo[k], c);
                hi[k] = std::max(hi[k], c);
            }
        // order the link's triangles so that every run of 64 is spatially compact: recursive median split along the
        // longest axis of the centroids, the left part a multiple of 64 (so that clusters never straddle a split)
        std::vector<int> order((size_t)n);
        for (int i = 0; i < n; i++) order[i] = i;
        vb_kd_order(cen.data(), order.data(), n);
        for (int i = 0; i < n; i++) {
            if ((i & 63) == 0) clink.push_back(l);
            ctri.push_back(t0 + order[i]);
        }
        while (ctri.size() & 63) ctri.push_back(-1);
    }
    if (t != T) return fail(EHR_ERR_INVALID, "ehr_fused_plan: tri_link holds a link outside [0, %d) or is not sorted", L);
    coff[L] = (int32_t)clink.size();
    const int NC = (int)clink.size();
    nc_out = NC;
    int rc;
    const size_t n_ctri = (size_t)std::max(NC, 1) * 64;
    std::vector<float> cvert(12 * n_ctri, 0.f);  // three float4 planes
    for (size_t i = 0; i < ctri.size(); i++) {
        const int tt = ctri[i];
        if (tt < 0) continue;
        const int v0 = ht[3 * (size_t)tt], v1 = ht[3 * (size_t)tt + 1], v2 = ht[3 * (size_t)tt + 2];
        if ((unsigned)v0 >= (unsigned)V || (unsigned)v1 >= (unsigned)V || (unsigned)v2 >= (unsigned)V) continue;
        const float c9[9] = {hv[3 * (size_t)v0], hv[3 * (size_t)v0 + 1], hv[3 * (size_t)v0 + 2], hv[3 * (size_t)v1], hv[3 * (size_t)v1 + 1],
                             hv[3 * (size_t)v1 + 2], hv[3 * (size_t)v2], hv[3 * (size_t)v2 + 1], hv[3 * (size_t)v2 + 2]};
        for (int k = 0; k < 4; k++) cvert[4 * i + k] = c9[k];
        for (int k = 0; k < 4; k++) cvert[4 * (n_ctri + i) + k] = c9[4 + k];
        cvert[4 * (2 * n_ctri + i)] = c9[8];
        cvert[4 * (2 * n_ctri + i) + 1] = 1.f;
    }
    std::vector<int32_t> cvidx(4 * n_ctri, 0);  // {v0, v1, v2, triangle} of every cluster slot
    for (size_t i = 0; i < n_ctri; i++) {
        const int tt = i < ctri.size() ? ctri[i] : -1;
        cvidx[4 * i + 3] = tt;
        if (tt < 0) continue;
        for (int k = 0; k < 3; k++) {
            const int v = ht[3 * (size_t)tt + k];
            cvidx[4 * i + k] = ((unsigned)v < (unsigned)V) ? v : 0;  // (such a triangle draws nothing: never looked up)
        }
    }
    for (int l = 0; l < L; l++)  // a deferred unit names its triangle by an 18-bit slot relative to its link's first cluster
        if (coff[l + 1] - coff[l] > 4096)
            return fail(EHR_ERR_INVALID, "ehr_fused_plan: link %d has more than 262144 triangles", l);
    if ((rc = out.reserve((n_ctri + std::max(NC, 1) + L + 1 + 6 * (size_t)L) * sizeof(int32_t) + 32 + cvert.size() * sizeof(float) +
                          cvidx.size() * sizeof(int32_t)))) return rc;
    int32_t* d = (int32_t*)out.ptr;
    if (NC > 0) {
        EHR_HIP(hipMemcpy(d, ctri.data(), (size_t)NC * 64 * sizeof(int32_t), hipMemcpyHostToDevice));
        EHR_HIP(hipMemcpy(d + n_ctri, clink.data(), (size_t)NC * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    EHR_HIP(hipMemcpy(d + n_ctri + std::max(NC, 1), coff.data(), ((size_t)L + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    EHR_HIP(hipMemcpy(d + n_ctri + std::max(NC, 1) + L + 1, aabb.data(), aabb.size() * sizeof(float), hipMemcpyHostToDevice));
    {
        const uintptr_t at = ((uintptr_t)(d + n_ctri + std::max(NC, 1) + L + 1 + 6 * (size_t)L) + 15) & ~(uintptr_t)15;
        EHR_HIP(hipMemcpy((void*)at, cvert.data(), cvert.size() * sizeof(float), hipMemcpyHostToDevice));
        EHR_HIP(hipMemcpy((char*)at + cvert.size() * sizeof(float), cvidx.data(), cvidx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return EHR_OK;
}

// The device view of a cluster index vb_build_clusters wrote into `scratch` (NC clusters, L links; NC = 0: one padding
// cluster's room)
static std::pair<VbClusters, VbSlotIdx> vb_cluster_index(const Scratch& scratch, int NC, int L) {
    const int NC1 = std::max(NC, 1);
    VbClusters cl;
    cl.ctri = (const int32_t*)scratch.ptr;
    cl.clink = cl.ctri + (size_t)NC1 * 64;
    cl.coff = cl.clink + NC1;
    cl.laabb = (const float*)(cl.coff + L + 1);
    cl.cvert = (const float4*)(((uintptr_t)(cl.laabb + 6 * (size_t)L) + 15) & ~(uintptr_t)15);
    cl.NC = NC;
    VbSlotIdx si;
    si.cvidx = (const int4*)(cl.cvert + 3 * (size_t)NC1 * 64);
    return {cl, si};
}

// The vertex kernel's grid for Bk views of `nitems` work items: gx workgroups per view, as many as stay resident together,
// every one with the same number of work items; xcd_views as vb_vertex_kernel takes it
struct VbVertexGrid {
    int gx, xcd_views;
};
static VbVertexGrid vb_vertex_grid(int num_cus, int nitems, int Bk) {
    const int per_view_cap = std::max(8, (num_cus * VB_VERTEX_GRID) / std::max(Bk, 1));
    const int items_per_wg = (nitems + per_view_cap - 1) / per_view_cap;
    VbVertexGrid v;
    v.gx = std::max(1, (nitems + items_per_wg - 1) / std::max(items_per_wg, 1));
    v.xcd_views = (VB_XCD_SPLIT && (Bk % VB_XCDS) == 0) ? Bk / VB_XCDS : 0;
    return v;
}

int ehr::vbuf_plan(ehr_ctx* ctx, int B, int L, int V, int T, int H, int W, float slack, const float* verts,
                   const int32_t* tris, const int32_t* tri_link, const int32_t* opp) {
    if (H > 32760 || W > 32736)  // tile counts are packed into 10 (columns) and 12 (rows) bits
        return fail(EHR_ERR_INVALID, "ehr_fused_plan: resolution above 32736 x 32760 (W x H) is unsupported");
    if ((V > 0 && !verts) || (T > 0 && (!tris || !tri_link || !opp)))
        return fail(EHR_ERR_INVALID, "ehr_fused_plan: the scene arrays (verts, tris, tri_link, opp) are required");
    int rc;
    if ((rc = vb_build_clusters(ctx->vb_clus, ctx->vb_nc, L, V, T, verts, tris, tri_link))) return rc;
    const int NC = std::max(ctx->vb_nc, 1);
    // The views of a call go through the chain in CHUNKS of Bc views (one chunk in the common case): the job kernel
    // keeps its (view, link) tables in LDS (VB_MAX_UNITS entries), and the per-chunk scratch -- clip-space vertices,
    // raster records (vb_recs), job slots (vb_slots, 2 KB each) -- is bounded to 24 GB of the 288 (EHR_VB_SCRATCH_MB) however many views a
    // call brings: a chunk costs a pass of the chain with its own tails, so chunks are as large as they may be (the reference
    // batches all frames of a data set in one step, configs/xarm7/example.yaml: batch_size 100).  A job = a (link, tile)
    // pair whose boxes touch; by default (`slack` <= 0) one slot per (link, tile) is provided, so nothing can overflow;
    // `slack` > 0 provides `slack` jobs per view tile instead (a fraction is fine: a robot's links touch a twentieth of
    // the tiles of a typical frame; less scratch, larger chunks); a view that needs more (every pixel under more than
    // `slack` link boxes on average) is reported (loss = NaN, ehr_fused_status).
    BinGeom gp = make_geom(H, W, L);
    const double jobs_per_view = std::max(1.0, ((slack > 0.f) ? std::min((double)L, (double)slack) : (double)L) * gp.nt);
    const double view_bytes = jobs_per_view * VB_SLOT_BYTES + (double)NC * VB_CLUSTER_REC_BYTES + (double)std::max(V, 1) * sizeof(float4) +
                              (double)L * gp.nt * sizeof(int);
    static const double budget = getenv("EHR_VB_SCRATCH_MB") ? atof(getenv("EHR_VB_SCRATCH_MB")) * 1048576.0 : 24576.0 * 1048576.0;
    int Bc = std::min(B, std::max(1, VB_MAX_UNITS / L));
    Bc = std::max(1, std::min(Bc, (int)(budget / view_bytes)));
    if (jobs_per_view * Bc > 2.0e9) return fail(EHR_ERR_INVALID, "ehr_fused_plan: views x links x tiles of a chunk exceeds 2e9");
    ctx->vb_chunk = Bc;
    if ((rc = ctx->vb_acc.reserve((size_t)B * vb_acc_stride(L) * sizeof(long long) + VB_META_BYTES))) return rc;
    {   // Clip-space vertices: kept per view (posc, 16 B per vertex and view, written by the vertex kernel) or computed where
        // they are looked up (VbLazy).  Lazy pays where vertices outnumber the look-ups by far -- meshes with unshared
        // vertices (V ~ 3 T): Franka 16 x 1080p spends 168 of the vertex launch's 286 MB on them -- and costs the job kernel
        // registers it does not have (8 views xArm7: +3.5 us), hence a choice per plan.  EHR_VB_LAZY=0/1 overrides.
        const char* e = getenv("EHR_VB_LAZY");
        ctx->vb_lazy = e ? atoi(e) != 0 : (double)V > 1.5 * (double)std::max(T, 1);
        if (ctx->vb_lazy != (ctx->vb_posc.ptr == nullptr) && ctx->gexec) {  // (a captured chain has the form baked in)
            EHR_HIP(hipGraphExecDestroy(ctx->gexec));
            ctx->gexec = nullptr;
        }
        if (!ctx->vb_lazy && (rc = ctx->vb_posc.reserve((size_t)Bc * std::max(V, 1) * sizeof(float4)))) return rc;
    }
    size_t bytes;
    vb_recs(nullptr, Bc, NC, &bytes);
    if ((rc = ctx->vb_boxes.reserve(bytes))) return rc;
    {  // pool of blended pairs for jobs that exceed their slot (EHR_VB_SPILL_ITEMS: test hook for the overflow path)
        const char* e = getenv("EHR_VB_SPILL_ITEMS");
        ctx->vb_spill_cap = e ? std::max(0, atoi(e)) : VB_SPILL_ITEMS;
        // (the 1 MB floor: room for the per-wave records of the timeline build, profiles/experiments/job_kernel_instruments.patch)
        if ((rc = ctx->vb_spill.reserve(std::max((size_t)ctx->vb_spill_cap * sizeof(VbItem), (size_t)1 << 20)))) return rc;
    }
    if ((rc = ctx->vb_units.reserve((size_t)VB_LBOX_STRIDE * B * L * sizeof(int)))) return rc;  // link boxes (one 64-byte line each), all views
    {  // a bound reference mask's cached sums: tsum [B][nt] | vtot [B] | flag
        if ((rc = ctx->vb_refsum.reserve(((size_t)B * gp.nt + B + 1) * sizeof(long long)))) return rc;
        ctx->vb_ref = nullptr;  // a new plan forgets the binding
        ctx->vb_weight = nullptr;  // ... and the weights (ehr_fused_bind_weight)
        ctx->vb_weight_views = 0;
    }
    ctx->vb_jcap = (int)(jobs_per_view * Bc);
    vb_slots(nullptr, (size_t)ctx->vb_jcap, (size_t)Bc * L, &bytes);
    if ((rc = ctx->vb_jobs.reserve(bytes))) return rc;
    vb_heavy(nullptr, (size_t)Bc * L * gp.nt, &bytes);  // (the stamp table: dense ids of a chunk)
    if ((rc = ctx->vb_heavy.reserve(bytes))) return rc;
    EHR_HIP(hipMemset(ctx->vb_heavy.ptr, 0, bytes));
    if ((rc = ctx->vb_idx.reserve((size_t)2 * std::max(T, 1) * sizeof(int4)))) return rc;
    if (T > 0) {
        vb_pad_kernel<<<(T + 255) / 256, 256>>>(tris, T, (int4*)ctx->vb_idx.ptr);
        vb_pad_kernel<<<(T + 255) / 256, 256>>>(opp, T, (int4*)ctx->vb_idx.ptr + T);
        EHR_LAUNCH_CHECK();
    }
    if (!ctx->vb_hstate.ptr) {  // (once per context: a re-plan after a reported step must not forget that step)
        if ((rc = ctx->vb_hstate.reserve(16 * sizeof(int)))) return rc;
        EHR_HIP(hipMemset(ctx->vb_hstate.ptr, 0, 16 * sizeof(int)));
    }
    if (ctx->vb_hstate_m.cap < (size_t)VB_HSTATE_INTS * B * sizeof(int)) {  // (likewise: only a larger plan starts it afresh)
        if ((rc = ctx->vb_hstate_m.reserve((size_t)VB_HSTATE_INTS * B * sizeof(int)))) return rc;
        EHR_HIP(hipMemset(ctx->vb_hstate_m.ptr, 0, ctx->vb_hstate_m.cap));
    }
    ctx->vb_plan_tris = tris;
    ctx->vb_plan_opp = opp;
    ctx->vb_plan_verts = verts;
    EHR_HIP(hipMemset(ctx->vb_acc.ptr, 0, ctx->vb_acc.cap));
    std::vector<int> boxes((size_t)VB_LBOX_STRIDE * B * L);  // link boxes start "empty"; the finish kernel re-arms them
    for (size_t i = 0; i < boxes.size(); i++) boxes[i] = (i & 2) ? INT_MIN : INT_MAX;
    EHR_HIP(hipMemcpy(ctx->vb_units.ptr, boxes.data(), boxes.size() * sizeof(int), hipMemcpyHostToDevice));
    EHR_HIP(hipDeviceSynchronize());
    return EHR_OK;
}

int ehr::vbuf_meta_read(ehr_ctx* ctx, int* meta4) {
    EHR_HIP(hipMemcpy(meta4, vb_acc_meta((long long*)ctx->vb_acc.ptr, ctx->pB, ctx->pL), 4 * sizeof(int), hipMemcpyDeviceToHost));
    return EHR_OK;
}

// ---- information matrix of the mask loss (ehr_mask_information) ------------------------------
// After a chunk's composite launch every job slot still holds what the backward pass was built from.  vb_info_kernel
// reads them once more and forms, per tile that holds a job, the Gauss-Newton sums over the tile's pixels for N caller
// given tangents dmvp[k] = d MVP / d theta_k:
//     J_p[k] = gate_p sum_l sum_pairs <d si_l,p / d MVP[b,l], dmvp[k,b,l]>      float32, links in link order, pairs in list order
//     record = upper triangle of sum_p w_p J_p J_p^T | sum_p (2 w_p e_p) J_p | pixels with w_p > 0 and J_p != 0     float64
// One wave per tile, no atomics on values: pairs that land on the same pixel are added one after the other in list
// order (their rank among the batch's lanes), a lane owns whole entries of the record and walks the tile's active pixels
// in pixel order.  Two small kernels then add the records of a view in tile order, 64 tiles to a group, in float64.
// A record entry is a sum of squares of per-radian sensitivities (thousands squared, over thousands of pixels): float64,
// not the 2^32 fixed point of the loss.
constexpr int VB_INFO_MAX_N = 32;
constexpr int VB_INFO_GROUP = 64;  // tile records added per workgroup of the first reduction level
__host__ __device__ constexpr int vb_info_tri(int N) { return N * (N + 1) / 2; }
__host__ __device__ constexpr int vb_info_rec(int N) { return vb_info_tri(N) + N + 1; }  // doubles per record
constexpr int VB_INFO_LANE_ENTRIES = (vb_info_tri(VB_INFO_MAX_N) + VB_INFO_MAX_N + 63) / 64;  // entries a lane owns, at most (9)
constexpr int vb_info_wave_floats(int N) { return 256 * (N + 3); }  // LDS of a wave: J [256][N] | w | 2 w e | active list
// record entry e -> (ka, kb): info entry (ka <= kb), or gradient entry ka with kb = -1
__host__ __device__ __forceinline__ void vb_info_entry(int e, int N, int& ka, int& kb) {
    int k = 0;
    while (k < N && e >= N - k) {
        e -= N - k;
        k++;
    }
    if (k < N) {
        ka = k;
        kb = k + e;
    } else {
        ka = e;
        kb = -1;
    }
}

struct VbInfoArgs {
    VbSlots sl;           // (read only)
    const VbItem* spill;
    int spill_cap;
    const float* verts;
    int V;
    const float* mvp;     // [B][L][16] of the chunk
    const float* dmvp;    // [N][B_all][L][16] of the call
    const float* ref;     // [B][H][W] of the chunk
    VbWeight wt;          // (w == NULL: every weight is 1)
    int N, B, b0, B_all;  // tangents; views of the chunk, its first view, views of the call
    BinGeom g;
    double* rec;          // [B][nt][vb_info_rec(N)] tile records
    int* valid;           // [B][nt] a record was written (zero before the launch)
    int* meta;
};

__global__ void __launch_bounds__(256)
vb_info_kernel(VbInfoArgs A) {
    extern __shared__ int s_dyn[];  // [U + 1] first job of every (view, link) | [U] its tile range | per wave vb_info_wave_floats(N)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (int)(blockDim.x >> 6);
    const BinGeom g = A.g;
    const int W = g.W, H = g.H, L = g.L, B = A.B, U = B * L, N = A.N, V = A.V;
    const int jcap = A.sl.jcap, spill_cap = A.spill_cap;
    int* const s_jbase = s_dyn;
    unsigned* const s_utile = reinterpret_cast<unsigned*>(s_dyn + U + 1);
    float* const J = reinterpret_cast<float*>(s_dyn + 2 * U + 1) + (size_t)wave * vb_info_wave_floats(N);
    float* const wq = J + 256 * N;   // gate ? w : 0
    float* const gq = wq + 256;      // 2 w e
    int* const list = reinterpret_cast<int*>(gq + 256);
    for (int i = tid; i <= U; i += (int)blockDim.x) s_jbase[i] = A.sl.jbase[i];
    for (int i = tid; i < U; i += (int)blockDim.x) s_utile[i] = A.sl.jutile[i];
    __syncthreads();
    const int nitems = min(s_jbase[U], jcap);
    const int r = lane >> 3, c4 = (lane & 7) * 4;
    const float invL = __builtin_amdgcn_rcpf((float)L);
    const int nent = vb_info_tri(N) + N, R = vb_info_rec(N);
    int ea[VB_INFO_LANE_ENTRIES], eb[VB_INFO_LANE_ENTRIES];
#pragma unroll
    for (int j = 0; j < VB_INFO_LANE_ENTRIES; j++) {
        ea[j] = -1;
        eb[j] = -1;
        if (lane + 64 * j < nent) vb_info_entry(lane + 64 * j, N, ea[j], eb[j]);
    }
    for (int item = (int)blockIdx.x * nw + wave; item < nitems; item += (int)gridDim.x * nw) {
        // the job's (view, link) and tile, and whether it stands for its tile (vb_composite_items' sparse enumeration)
        int lo = 0, hi = U - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_jbase[mid] <= item)
                lo = mid;
            else
                hi = mid - 1;
        }
        const int b = vb_div_small(lo, invL);
        int tx, ty;
        {
            const unsigned ut = s_utile[lo];
            const int nx = (int)(ut >> 22), k = item - s_jbase[lo];
            const int kr = nx > 0 ? k / nx : 0;
            ty = (int)((ut >> 10) & 4095u) + kr;
            tx = (int)(ut & 1023u) + k - kr * nx;
        }
        unsigned tmask;
        int myn = -1, myslot = 0;
        bool beyond = false;
        {
            bool mine = false;
            if (lane < L) {
                const int u = b * L + lane;
                const unsigned ut = s_utile[u];
                const int j0 = s_jbase[u], n = s_jbase[u + 1] - j0;
                const int tx0 = ut & 1023u, ty0 = (ut >> 10) & 4095u, nx = ut >> 22;
                if (n > 0 && tx >= tx0 && tx < tx0 + nx && ty >= ty0 && (ty - ty0) * nx < n) {
                    mine = true;
                    myslot = j0 + (ty - ty0) * nx + (tx - tx0);
                    if (myslot < jcap)
                        myn = A.sl.jn[myslot];
                    else
                        beyond = true;
                }
            }
            const u64 have = __ballot(mine);
            if (have == 0 || (int)__ffsll((unsigned long long)have) - 1 != lo - b * L) continue;  // an earlier link owns the tile
            tmask = (unsigned)__ballot(myn >= 0);
        }
        if (__ballot(beyond) && lane == 0) atomicOr(&A.meta[EHR_META_OVERFLOW], 1);  // a slot beyond jcap: reported
        const unsigned bmask = (unsigned)__ballot(myn > 0);
        if (bmask == 0 || tx >= g.ntx || ty >= g.nty) continue;  // no blended pair: every J of the tile is zero
        const int tile = ty * g.ntx + tx;
        const int rx0 = tx * EHR_TILE_W - 1, ry0 = ty * EHR_TILE_H - 1;
        // ---- 1. the links' sum in link order, gate, e, w (the composite stage's float32 expressions)
        {
            const int ix = tx * EHR_TILE_W + c4, iy = ty * EHR_TILE_H + r;
            const bool row_in = iy < H;
            const int row = H - 1 - (row_in ? iy : 0);  // image convention: row 0 = top
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            unsigned todo = tmask;
            while (todo) {
                const int l = __ffs(todo) - 1;
                todo &= todo - 1;
                const size_t slot = (size_t)vb_readlane(myslot, l);
                const float4 v4 = *reinterpret_cast<const float4*>(A.sl.jval + slot * 256 + r * EHR_TILE_W + c4);
                acc[0] += v4.x;
                acc[1] += v4.y;
                acc[2] += v4.z;
                acc[3] += v4.w;
            }
            VB_WAVE_SYNC();  // the previous tile's reads of this wave's LDS are complete
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float wg = 0.f, ge = 0.f;
                if (row_in && ix + j < W) {
                    const float rf = A.ref[((size_t)b * H + row) * W + ix + j];
                    const float wv = A.wt.w ? A.wt.w[((size_t)((A.wt.view0 + b) % A.wt.nviews) * H + row) * W + ix + j] : 1.f;
                    const float m = acc[j] > 1.f ? 1.f : acc[j];
                    const float e = m - rf;
                    const float we = wv * e;
                    ge = 2.f * we;
                    wg = (acc[j] <= 1.f) ? wv : 0.f;
                }
                wq[r * EHR_TILE_W + c4 + j] = wg;
                gq[r * EHR_TILE_W + c4 + j] = ge;
            }
            for (int i = lane; i < 256 * N; i += 64) J[i] = 0.f;
            VB_WAVE_SYNC();
        }
        // ---- 2. every blended pair of every link -> J of the pixel it blends into
        unsigned links = bmask;
        while (links) {
            const int l = __ffs(links) - 1;
            links &= links - 1;
            const size_t slot = (size_t)vb_readlane(myslot, l);
            int n = vb_readlane(myn, l);
            int sbase = 0;
            if (n > VB_JOB_ITEMS) {  // the rest of the list lives in the spill pool; never read outside it
                sbase = A.sl.jspill[slot];
                if (sbase < 0 || sbase >= spill_cap) {
                    n = VB_JOB_ITEMS;
                    if (lane == 0) atomicOr(&A.meta[EHR_META_OVERFLOW], 1);
                } else if (n > VB_JOB_ITEMS + (spill_cap - sbase)) {
                    n = VB_JOB_ITEMS + (spill_cap - sbase);
                    if (lane == 0) atomicOr(&A.meta[EHR_META_OVERFLOW], 1);
                }
            }
            const float* const M = A.mvp + ((size_t)b * L + l) * 16;
            const float* const D0 = A.dmvp + (((size_t)(A.b0 + b)) * L + l) * 16;
            const size_t dstride = (size_t)A.B_all * L * 16;
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                bool on = i < n;
                int tp = -1;
                float g1[3] = {0.f, 0.f, 0.f}, g2[3] = {0.f, 0.f, 0.f};
                float h1[3] = {0.f, 0.f, 0.f}, h2[3] = {0.f, 0.f, 0.f};
                if (on) {
                    const VbItem itm = *((i < VB_JOB_ITEMS) ? &A.sl.jitems[slot * VB_JOB_ITEMS + i] : &A.spill[sbase + (i - VB_JOB_ITEMS)]);
                    const int q = itm.packed & 1023, d = (itm.packed >> 10) & 1;
                    const int tri1 = (itm.packed >> 13) & 1;
                    const float dc = ((itm.packed >> 14) & 1) ? 1.f : -1.f;
                    const int nq = q + (d ? VB_RW : 1);
                    const int oq = (itm.alpha > 0.f) ? q : nq;
                    const int oy = vb_div_rw(oq), ox = oq - oy * VB_RW;
                    on = ox >= 1 && ox <= EHR_TILE_W && oy >= 1 && oy <= EHR_TILE_H && (unsigned)itm.v1 < (unsigned)V &&
                         (unsigned)itm.v2 < (unsigned)V;
                    if (on) {
                        tp = (oy - 1) * EHR_TILE_W + (ox - 1);
                        on = wq[tp] != 0.f;  // gated, outside the image or without weight: contributes nothing
                    }
                    if (on) {
                        const int qy = vb_div_rw(q), qx = q - qy * VB_RW;
                        int px = rx0 + qx, py = ry0 + qy;
                        if (tri1) {
                            px += 1 - d;
                            py += d;
                        }
                        const float* a1 = A.verts + 3 * (size_t)itm.v1;
                        const float* a2 = A.verts + 3 * (size_t)itm.v2;
                        h1[0] = a1[0]; h1[1] = a1[1]; h1[2] = a1[2];
                        h2[0] = a2[0]; h2[1] = a2[1]; h2[2] = a2[2];
                        aa_pos_grad(transform_vertex(M, h1[0], h1[1], h1[2]), transform_vertex(M, h2[0], h2[1], h2[2]), px, py, d,
                                    itm.alpha, dc, W, H, g1, g2);
                    } else {
                        tp = -1;
                    }
                }
                // rank of this pair among the batch's pairs of the same pixel: they are added one after the other
                int rank = 0;
                for (int j = 0; j < 64; j++) {
                    const int tj = vb_readlane(tp, j);
                    rank += (j < lane && tj == tp) ? 1 : 0;
                }
                if (!on) rank = -1;
                const int nrank = vb_scan_max(rank + 1);
                const int rounds = vb_readlane(nrank, 63);
                for (int k = 0; k < N; k++) {
                    const float* const D = D0 + (size_t)k * dstride;
                    // d clip / d theta_k of the two vertices, then the pair's contribution: rows x, y, w
                    const float4 t1 = transform_vertex(D, h1[0], h1[1], h1[2]);
                    const float4 t2 = transform_vertex(D, h2[0], h2[1], h2[2]);
                    const float c = (g1[0] * t1.x + g1[1] * t1.y + g1[2] * t1.w) + (g2[0] * t2.x + g2[1] * t2.y + g2[2] * t2.w);
                    for (int rr = 0; rr < rounds; rr++) {
                        if (rank == rr) J[tp * N + k] += c;
                        VB_WAVE_SYNC();
                    }
                }
            }
        }
        VB_WAVE_SYNC();
        // ---- 3. the tile's active pixels in pixel order, then its record
        int npix = 0, cnt = 0;
        for (int c = 0; c < 4; c++) {
            const int p = c * 64 + lane;
            bool any = false;
            for (int k = 0; k < N; k++) any = any || (J[p * N + k] != 0.f);
            const u64 m = __ballot(any);
            if (any) list[npix + vb_mbcnt(m)] = p;
            npix += __popcll(m);
            cnt += __popcll(__ballot(any && wq[p] > 0.f));
        }
        if (npix == 0) continue;
        VB_WAVE_SYNC();
        double sum[VB_INFO_LANE_ENTRIES];
#pragma unroll
        for (int j = 0; j < VB_INFO_LANE_ENTRIES; j++) sum[j] = 0.0;
        for (int i = 0; i < npix; i++) {
            const int p = list[i];
            const double w = (double)wq[p], ge = (double)gq[p];
            const float* const Jp = J + p * N;
#pragma unroll
            for (int j = 0; j < VB_INFO_LANE_ENTRIES; j++) {
                if (ea[j] < 0) continue;
                const double a = (double)Jp[ea[j]];
                if (eb[j] >= 0)
                    sum[j] += w * (a * (double)Jp[eb[j]]);
                else
                    sum[j] += ge * a;
            }
        }
        double* const rec = A.rec + ((size_t)b * g.nt + tile) * R;
#pragma unroll
        for (int j = 0; j < VB_INFO_LANE_ENTRIES; j++)
            if (ea[j] >= 0) rec[lane + 64 * j] = sum[j];
        if (lane == 0) {
            rec[R - 1] = (double)cnt;
            A.valid[(size_t)b * g.nt + tile] = 1;
        }
    }
}

// out[b][grp][e] = sum in order of in[b][t][e] over the group's valid records t (valid == NULL: all of them)
__global__ void __launch_bounds__(256)
vb_info_group_kernel(const double* __restrict__ in, const int* __restrict__ valid, int n, int R, double* __restrict__ out) {
    const int b = blockIdx.y, grp = blockIdx.x, ngrp = gridDim.x;
    const int t0 = grp * VB_INFO_GROUP, t1 = min(n, t0 + VB_INFO_GROUP);
    for (int e = threadIdx.x; e < R; e += 256) {
        double s = 0.0;
        for (int t = t0; t < t1; t++)
            if (!valid || valid[(size_t)b * n + t]) s += in[((size_t)b * n + t) * R + e];
        out[((size_t)b * ngrp + grp) * R + e] = s;
    }
}

// grp [B][ngrp][R] -> info [B][N][N] (both triangles), grad [B][N], count [B] of the chunk's views; a non-finite sum is reported
__global__ void __launch_bounds__(256)
vb_info_finish_kernel(const double* __restrict__ grp, int ngrp, int N, double* __restrict__ info, double* __restrict__ grad,
                      long long* __restrict__ count, int* __restrict__ meta) {
    const int b = blockIdx.x, R = vb_info_rec(N);
    for (int e = threadIdx.x; e < R; e += 256) {
        double s = 0.0;
        for (int k = 0; k < ngrp; k++) s += grp[((size_t)b * ngrp + k) * R + e];
        if (!(fabs(s) <= 1.7e308)) atomicOr(&meta[EHR_META_OVERFLOW], 1);  // (also a NaN)
        if (e == R - 1) {
            count[b] = (long long)s;
        } else {
            int ka, kb;
            vb_info_entry(e, N, ka, kb);
            if (kb < 0) {
                grad[(size_t)b * N + ka] = s;
            } else {
                info[((size_t)b * N + ka) * N + kb] = s;
                info[((size_t)b * N + kb) * N + ka] = s;
            }
        }
    }
}

// A reported call (the chain's own overflow, or one of the above): every output is NaN, count -1
__global__ void __launch_bounds__(256)
vb_info_report_kernel(const int* __restrict__ meta, int B, int N, double* __restrict__ info, double* __restrict__ grad,
                      long long* __restrict__ count, float* __restrict__ loss) {
    if (__hip_atomic_load(&meta[EHR_META_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    const int b = blockIdx.x;
    for (int e = threadIdx.x; e < N * N; e += 256) info[(size_t)b * N * N + e] = nanv;
    for (int e = threadIdx.x; e < N; e += 256) grad[(size_t)b * N + e] = nanv;
    if (threadIdx.x == 0) {
        count[b] = -1;
        if (loss) loss[b] = __int_as_float(0x7fc00000);
    }
}

// scratch of ehr_mask_information (ehr_ctx::vb_info), for chunks of Bc views
struct VbInfoScratch {
    double* rec;    // [Bc][nt][R]
    double* grp;    // [Bc][ngrp][R]
    int* valid;     // [Bc][nt]
    int* hint;      // a copy of the heavy-job hint (ehr_ctx::vb_heavy), put back after the call
    float* loss;    // [B] where the caller wants no loss
    float* grad;    // [B][L][16] where the caller wants no grad_mvp
};
static VbInfoScratch vb_info_scratch(void* base, size_t Bc, size_t nt, size_t R, size_t hint_bytes, size_t B, size_t L, size_t* bytes = nullptr) {
    VbCarve c{(uintptr_t)base};
    VbInfoScratch s;
    const size_t ngrp = (nt + VB_INFO_GROUP - 1) / VB_INFO_GROUP;
    s.rec = c.take<double>(Bc * nt * R);
    s.grp = c.take<double>(Bc * ngrp * R);
    s.valid = c.take<int>(Bc * nt);
    s.hint = c.take<int>(hint_bytes / sizeof(int), 16);
    s.loss = c.take<float>(B, 16);
    s.grad = c.take<float>(B * L * 16, 16);
    if (bytes) *bytes = c.at - (uintptr_t)base;
    return s;
}

// The chunk's launches of ehr_mask_information, behind its composite launch
static int vb_info_launch(ehr_ctx* ctx, const InfoCall& ic, const VbSlots& sl, const VbItem* spill, const float* verts, int V,
                          const float* mvp_k, const float* ref_k, const VbWeight& wt, int Bk, int b0, int B, const BinGeom& g,
                          int* meta, hipStream_t stream) {
    const int N = ic.N, R = vb_info_rec(N);
    const int Bc = std::max(1, std::min(ctx->vb_chunk, B));
    const VbInfoScratch s = vb_info_scratch(ctx->vb_info.ptr, Bc, g.nt, R, ctx->vb_heavy.cap, B, g.L);
    int rc;
    if ((rc = zero_words(s.valid, (size_t)Bk * g.nt, stream))) return rc;
    VbInfoArgs a;
    a.sl = sl; a.spill = spill; a.spill_cap = ctx->vb_spill_cap; a.verts = verts; a.V = V; a.mvp = mvp_k; a.dmvp = ic.dmvp;
    a.ref = ref_k; a.wt = wt; a.N = N; a.B = Bk; a.b0 = b0; a.B_all = B; a.g = g; a.rec = s.rec; a.valid = s.valid; a.meta = meta;
    // waves per workgroup: as many of 4, 2, 1 as the default 64 KB of dynamic LDS hold
    const size_t tables = (2 * (size_t)Bk * g.L + 1) * sizeof(int), per_wave = (size_t)vb_info_wave_floats(N) * sizeof(float);
    int nw = 4;
    while (nw > 1 && tables + nw * per_wave > 65536) nw >>= 1;
    const int nwg = std::max(1, ctx->num_cus * 16 / nw);
    vb_info_kernel<<<nwg, 64 * nw, tables + nw * per_wave, stream>>>(a);
    EHR_LAUNCH_CHECK();
    const int ngrp = (g.nt + VB_INFO_GROUP - 1) / VB_INFO_GROUP;
    vb_info_group_kernel<<<dim3(ngrp, Bk), 256, 0, stream>>>(s.rec, s.valid, g.nt, R, s.grp);
    EHR_LAUNCH_CHECK();
    vb_info_finish_kernel<<<Bk, 256, 0, stream>>>(s.grp, ngrp, N, ic.info + (size_t)b0 * N * N, ic.grad + (size_t)b0 * N,
                                                  ic.count + b0, meta);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr::vbuf_information(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const int32_t* opp,
                          const float* mvp, const float* dmvp, int N, const float* ref, int B, int L, int V, int T, int H, int W,
                          double* info, double* grad, long long* count, float* loss, float* grad_mvp, hipStream_t stream) {
    if (N < 1 || N > VB_INFO_MAX_N)
        return fail(EHR_ERR_INVALID, "ehr_mask_information: N = %d tangents (1 <= N <= %d)", N, VB_INFO_MAX_N);
    if (ctx->capturing) return fail(EHR_ERR_INVALID, "ehr_mask_information: not inside a graph capture");
    const BinGeom g = make_geom(H, W, L);
    const int Bc = std::max(1, std::min(ctx->vb_chunk, B));
    size_t bytes;
    vb_info_scratch(nullptr, Bc, g.nt, vb_info_rec(N), ctx->vb_heavy.cap, B, L, &bytes);
    int rc;
    if ((rc = ctx->vb_info.reserve(bytes))) return rc;
    const VbInfoScratch s = vb_info_scratch(ctx->vb_info.ptr, Bc, g.nt, vb_info_rec(N), ctx->vb_heavy.cap, B, L);
    // the heavy-job hint is the solve's: the chain below advances it, so it is put back as it was
    if ((rc = copy_words(s.hint, ctx->vb_heavy.ptr, ctx->vb_heavy.cap / sizeof(int), stream))) return rc;
    InfoCall ic;
    ic.dmvp = dmvp; ic.N = N; ic.info = info; ic.grad = grad; ic.count = count;
    float* const loss_k = loss ? loss : s.loss;
    rc = vbuf_chain(ctx, verts, tris, vert_link, opp, const_cast<float*>(mvp), ref, B, L, V, T, H, W, nullptr, loss_k,
                    grad_mvp ? grad_mvp : s.grad, nullptr, nullptr, stream, 0, &ic);
    if (rc) return rc;
    if ((rc = copy_words(ctx->vb_heavy.ptr, s.hint, ctx->vb_heavy.cap / sizeof(int), stream))) return rc;
    vb_info_report_kernel<<<B, 256, 0, stream>>>(vb_acc_meta((long long*)ctx->vb_acc.ptr, B, L), B, N, info, grad, count, loss);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr::vbuf_chain(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const int32_t* opp, float* mvp, const float* ref, int B, int L, int V,
                    int T, int H, int W, float* mask, float* loss, float* grad_mvp, const StepHead* head,
                    const StepTail* tail, hipStream_t stream, int multi_views, const InfoCall* info) {
    const bool multi = multi_views > 0;  // B = P x multi_views virtual views; ref and head->link_poses hold multi_views real ones
    if (tris != ctx->vb_plan_tris || opp != ctx->vb_plan_opp || verts != ctx->vb_plan_verts)
        return fail(EHR_ERR_INVALID, "fused op: the scene arrays differ from the planned ones; call ehr_fused_plan again");
    BinGeom g = make_geom(H, W, L);
    long long* const facc_all = (long long*)ctx->vb_acc.ptr;
    const int acc_stride = vb_acc_stride(L);
    int* meta = vb_acc_meta(facc_all, B, L);
    int* const lbox_all = (int*)ctx->vb_units.ptr;
    VbItem* spill = (VbItem*)ctx->vb_spill.ptr;
    const int NC = ctx->vb_nc, NC1 = std::max(NC, 1);
    const auto [cl, si] = vb_cluster_index(ctx->vb_clus, NC, L);
    const int Bc = std::max(1, std::min(ctx->vb_chunk, B));
    VbHeavy hv = vb_heavy(ctx->vb_heavy.ptr, (size_t)Bc * L * g.nt);

    hipEvent_t* ev = nullptr;
    if (ctx->timing) {
        const size_t need = ctx->ev_used + EHR_FUSED_STAGES + 1;
        while (ctx->ev.size() < need) {
            hipEvent_t e;
            EHR_HIP(hipEventCreate(&e));
            ctx->ev.push_back(e);
        }
        ev = ctx->ev.data() + ctx->ev_used;
        ctx->ev_used = need;
        EHR_HIP(hipEventRecord(ev[0], stream));
    }
    const float* const weight = ctx->vb_weight;  // per-pixel weights of the loss (ehr_fused_bind_weight), or NULL
    const int vec_ok = ((W & 3) == 0) && (((uintptr_t)ref & 15) == 0) && (!mask || ((uintptr_t)mask & 15) == 0) &&
                       (((uintptr_t)weight & 15) == 0);
    const int job_wgs = vb_xcd_round_up(ctx->num_cus * VB_JOB_GRID);
    hv.mcap = std::min(VB_MED_CAP, 2 * job_wgs);
    hv.heavy_base = VB_HEAVY_T_DEFAULT;
    hv.heavy_max = job_wgs / 2;
    const bool sparse = ctx->vb_ref != nullptr && ctx->vb_ref == ref && ctx->vb_ref_views == (multi ? multi_views : B);
    const long long* const tsum_all = sparse ? (const long long*)ctx->vb_refsum.ptr : nullptr;
    const long long* const vtot_all = sparse ? tsum_all + (size_t)B * g.nt : nullptr;
    const int* const ref_flag = sparse ? (const int*)(vtot_all + B) : nullptr;
    // stage 1a (below) is launched by the stateless render call always, by the solver step only once a step needed it
    const bool with_slow = !tail || ctx->vb_slow_needed;
    VbSlots sl = vb_slots(ctx->vb_jobs.ptr, (size_t)ctx->vb_jcap, (size_t)Bc * L);
    if (!with_slow) sl.slow_list = nullptr;
    const bool lazy = ctx->vb_lazy;
    float4* const posc = lazy ? nullptr : (float4*)ctx->vb_posc.ptr;
    const int nvb = lazy ? 0 : (std::max(V, 1) + 255) / 256;  // (no per-vertex work items where clip-space vertices are computed on demand)
    const int nitems = nvb + (NC + 3) / 4;
    for (int b0 = 0; b0 < B; b0 += Bc) {  // chunks of views (one, unless views x links / scratch say otherwise)
        const int Bk = std::min(Bc, B - b0);
        const bool first_chunk = b0 == 0, last_chunk = b0 + Bk == B;
        const bool time_it = ev && last_chunk;  // (stage times of a multi-chunk call: those of its last chunk)
        long long* facc = facc_all + (size_t)b0 * acc_stride;
        int* lbox = lbox_all + (size_t)VB_LBOX_STRIDE * b0 * L;
        float* mvp_k = mvp + (size_t)b0 * L * 16;
        const float* ref_k = multi ? ref : ref + (size_t)b0 * H * W;  // (multi: the real views, indexed by VbSharedRef)
        float* mask_k = mask ? mask + (size_t)b0 * H * W : nullptr;
        const VbRecs recs = vb_recs(ctx->vb_boxes.ptr, Bk, NC1);
        // stage 0: [pose forward] + vertices + screen boxes
        const VbVertexGrid vg = vb_vertex_grid(ctx->num_cus, nitems, Bk);
        const dim3 vgrid(vg.gx * Bk);
        const int nacc_ints = 2 * Bk * acc_stride;
        const int role = first_chunk ? VB_ROLE_FIRST_CHUNK : VB_ROLE_LATER_CHUNK;
        if (head && multi) {
            StepHead hk = *head;
            hk.view0 = b0;
            hk.nviews = multi_views;
            vb_vertex_kernel<true, true><<<vgrid, 256, 0, stream>>>(verts, vert_link, tris, cl, hk, mvp_k, V, nvb, g, posc, recs, lbox,
                                                                   (int*)facc, nacc_ints, meta, Bk, vg.gx, vg.xcd_views, hv, role);
        } else if (head) {
            StepHead hk = *head;
            hk.link_poses = head->link_poses + (size_t)b0 * L * 16;
            vb_vertex_kernel<true><<<vgrid, 256, 0, stream>>>(verts, vert_link, tris, cl, hk, mvp_k, V, nvb, g, posc, recs, lbox,
                                                             (int*)facc, nacc_ints, meta, Bk, vg.gx, vg.xcd_views, hv, role);
        } else {
            StepHead none = {};
            vb_vertex_kernel<false><<<vgrid, 256, 0, stream>>>(verts, vert_link, tris, cl, none, mvp_k, V, nvb, g, posc, recs,
                                                              lbox, (int*)facc, nacc_ints, meta, Bk, vg.gx, vg.xcd_views, hv, role);
        }
        EHR_LAUNCH_CHECK();
        if (time_it) EHR_HIP(hipEventRecord(ev[1], stream));
        // stage 1: jobs = (view, link, tile) -> coverage, the triangle ids the silhouette analysis asks for, and the resolve
        // stage on the wave that drew the job -> per-link values and blended pairs in the job's slot
        VbResolveArgs rq;
        rq.verts = verts; rq.mvp = mvp_k; rq.posc = posc; rq.V = V; rq.L = L; rq.W = W; rq.H = H;
        rq.tri4 = (const int4*)ctx->vb_idx.ptr;
        rq.opp4 = (const int4*)ctx->vb_idx.ptr + T;
        rq.T = T;
        rq.sl = sl;
        rq.spill = spill;
        rq.spill_cap = ctx->vb_spill_cap;
        rq.meta = meta;
        rq.want_grad = grad_mvp ? 1 : 0;
        VbJobParams jp = {};
        jp.g = g; jp.B = Bk; jp.cl = cl; jp.si = si; jp.rc = recs; jp.lbox = lbox; jp.hv = hv;
        jp.use_hint = Bc == B;  // (the heavy-job hint names jobs by their dense id inside a chunk: off with more than one)
        jp.heavy_t = VB_HEAVY_T_DEFAULT;
        jp.med_t0 = VB_MED_T_DEFAULT;
        jp.rq = rq;
        if (lazy)
            vb_job_kernel<false, true><<<job_wgs, 256, 0, stream>>>(jp);
        else
            vb_job_kernel<false><<<job_wgs, 256, 0, stream>>>(jp);
        EHR_LAUNCH_CHECK();
        // stage 1a: jobs with a triangle that crosses the near plane or spans > 512 pixels (normally none: the kernel returns at once)
        if (with_slow) {
            vb_slow_kernel<<<VB_SLOW_GRID, 256, 0, stream>>>(rq, recs, cl.NC, si.cvidx, cl.coff);
            EHR_LAUNCH_CHECK();
        }
        if (time_it) {  // (ms[2] of the timing ABI, ev[2]..ev[3], is an empty pair: the resolve stage has no launch of its own)
            for (int k = 2; k <= 4; k++) EHR_HIP(hipEventRecord(ev[k], stream));
        }
        // stage 2: composite, loss, mask, backward.  In the call's last chunk its finisher workgroup runs the finish
        // stage over ALL views (accumulators -> loss / grad_mvp, + pose backward and Adam in the solver-step form; re-arms
        // the link boxes).  With a bound reference mask and no mask output only tiles that hold a job are visited.
        // (The finisher counts arrivals up from ZERO and does not reset the counters: it relies on this chunk's vertex launch
        //  above, whose first workgroup zeroes every counter line.  A composite launch with do_finish and no vertex launch in
        //  front of it would finish on stale counts.)
        int nwg = ctx->num_cus * VB_COMPOSITE_GRID;
        if (!sparse) nwg = std::min(nwg, (Bk * g.nt + 3) / 4);
        nwg = std::max(VB_XCDS, vb_xcd_round_up(nwg));  // a multiple of VB_XCDS: the XCD split and the per-XCD arrival counters rely on it
        const size_t dyn = (2 * (size_t)Bk * L + 1) * sizeof(int);  // link tables in LDS
        const bool fill = sparse && mask_k != nullptr;  // (FILL: the zero fill of the tiles no job owns, a variant of its own
                                                          //  so that the form without a mask output keeps its registers)
        VbCompArgs ca;
        ca.g = g; ca.B = Bk; ca.mvp = mvp_k; ca.V = V; ca.verts = verts; ca.sl = sl; ca.ref = ref_k; ca.mask = mask_k; ca.facc = facc;
        ca.nls = VB_LOSS_SLOTS; ca.want_grad = rq.want_grad; ca.vec_ok = vec_ok; ca.spill = spill; ca.spill_cap = ctx->vb_spill_cap;
        ca.meta = meta;
        ca.tsum = sparse ? tsum_all + (size_t)b0 * g.nt : nullptr;
        ca.ref_flag = ref_flag; ca.loss = loss; ca.grad_mvp = grad_mvp;
        ca.do_finish = (last_chunk && !multi) ? 1 : 0; ca.B_all = B; ca.facc_all = facc_all; ca.vtot_all = vtot_all; ca.lbox_all = lbox_all;
        const VbWeight wt = {weight, b0, weight ? ctx->vb_weight_views : 1};  // (the weighted instantiations alone read it)
#define VB_COMPOSITE_W(TAILV, FILLV, SHAREDV, tailarg, sharg)                                                      \
    do {                                                                                                             \
        if (weight)                                                                                                  \
            vb_composite_kernel<TAILV, FILLV, SHAREDV, true><<<nwg, 256, dyn, stream>>>(ca, tailarg, sharg, wt);     \
        else                                                                                                         \
            vb_composite_kernel<TAILV, FILLV, SHAREDV><<<nwg, 256, dyn, stream>>>(ca, tailarg, sharg, wt);           \
    } while (0)
#define VB_COMPOSITE(TAILV, FILLV, tailarg) VB_COMPOSITE_W(TAILV, FILLV, false, tailarg, (VbSharedRef{0, 1}))
        StepTail none = {};
        if (multi) {  // (no finisher: vb_finish_multi_kernel follows the last chunk)
            const VbSharedRef sh = {b0, multi_views};
            if (fill)
                VB_COMPOSITE_W(false, true, true, none, sh);
            else
                VB_COMPOSITE_W(false, false, true, none, sh);
        } else if (tail) {
            if (fill) VB_COMPOSITE(true, true, *tail); else VB_COMPOSITE(true, false, *tail);
        } else {
            if (fill) VB_COMPOSITE(false, true, none); else VB_COMPOSITE(false, false, none);
        }
#undef VB_COMPOSITE
#undef VB_COMPOSITE_W
        EHR_LAUNCH_CHECK();
        if (info) {  // ehr_mask_information: the chunk's slots are read once more before the next chunk overwrites them
            const int rc = vb_info_launch(ctx, *info, sl, spill, verts, V, mvp_k, ref_k, wt, Bk, b0, B, g, meta, stream);
            if (rc) return rc;
        }
    }
    if (ev) EHR_HIP(hipEventRecord(ev[5], stream));
    if (multi) {  // the finish stage, one workgroup per hypothesis (ms[5] of the timing ABI)
        MultiFinish mf;
        mf.facc_all = facc_all; mf.vtot_all = vtot_all; mf.ref_flag = ref_flag; mf.loss = loss; mf.grad_mvp = grad_mvp;
        mf.meta = meta; mf.lbox_all = lbox_all; mf.P = B / multi_views; mf.Bv = multi_views; mf.nls = VB_LOSS_SLOTS; mf.g = g;
        vb_finish_multi_kernel<<<mf.P, 256, 0, stream>>>(mf, *tail);
        EHR_LAUNCH_CHECK();
    }
    if (ev) {
        for (int k = 6; k <= 7; k++) EHR_HIP(hipEventRecord(ev[k], stream));
    }
    return EHR_OK;
}

// The coverage chain's small scratch (ehr_ctx::sc_misc), for a chunk of Qc candidates x S poses = Bc views
struct VbScoreMisc {
    int* lbox;                  // [Bc][L][VB_LBOX_STRIDE] link boxes
    int* meta;                  // a meta block (VB_META_BYTES)
    VbHeavy hv;                 // the heavy-job hint's counters and lists (no stamps: the hint is off)
    int* sticky;                // [16] [0]: a triangle needs the exact z-buffer
    size_t zero_bytes;          // hv .. sticky, cleared at the start of a call
    unsigned long long* sacc;   // [2][Qc][16] per-candidate sums of the variance op, double buffered
    u64* tcov;                  // [Bc][nt][4] coverage words of the (view, tile)s
    void* own;                  // `own_bytes` of the op's last stage (128-byte aligned; VbOverlapMisc)
};
static VbScoreMisc vb_score_misc(void* base, size_t Qc, size_t Bc, int L, int nt, size_t own_bytes, size_t* bytes = nullptr) {
    VbCarve c{(uintptr_t)base};
    VbScoreMisc m;
    m.lbox = c.take<int>((size_t)VB_LBOX_STRIDE * Bc * L);
    m.meta = (int*)c.take<char>(VB_META_BYTES, alignof(int));
    size_t hv_bytes;
    m.hv = vb_heavy((void*)c.at, 0, &hv_bytes);
    c.at += hv_bytes;
    m.hv.stamp = m.hv.gen;  // (never touched)
    m.sticky = c.take<int>(16);
    m.zero_bytes = c.at - (uintptr_t)m.hv.gen;
    m.sacc = c.take<unsigned long long>(2 * 16 * Qc, 128);
    m.tcov = c.take<u64>(Bc * nt * 4);
    m.own = c.take<char>(own_bytes, 128);
    if (bytes) *bytes = c.at - (uintptr_t)base;
    return m;
}

// The pose search's own part of that scratch
struct VbOverlapMisc {
    unsigned long long* oacc;   // [2][Bc][16] area << 32 | inter of a (candidate, view), one 128-byte line each, double buffered
    u64* rbits;                 // [S][nt][4] the observed masks in the coverage words' bit layout (32 B per (view, tile))
};
static VbOverlapMisc vb_overlap_misc(void* base, size_t Bc, int S, int nt, size_t* bytes = nullptr) {
    VbCarve c{(uintptr_t)base};
    VbOverlapMisc m;
    m.oacc = c.take<unsigned long long>(2 * 16 * Bc, 128);
    m.rbits = c.take<u64>((size_t)S * nt * 4, 128);
    if (bytes) *bytes = c.at - (uintptr_t)base;
    return m;
}

// What a chunk's last stage gets to see of the coverage chain
struct VbCovChunk {
    BinGeom g;
    int S, Qc, Bc, nlbox, num_cus;
    VbScoreMisc m;
};

// The coverage-only chain on the solver's machinery, shared by the scoring op (ehr_mask_variance) and the pose search
// (ehr_mask_overlap), both in csrc/ehr_score.hip: the static cluster index of the packed mesh, then per chunk of
// candidates the vertex kernel (records + link boxes; depth class "coverage decides": every coverable pixel of the
// triangle has z/w in (0, 1]), the job kernel in its coverage-only form (no deferred units, no depth, no slots: a job ORs
// its tile's coverage into the view's word) and the op's own last stage, which also re-arms the link boxes:
//   st.op                           the op's name, for messages
//   st.own_bytes(Bc, nt)            scratch of its own (VbScoreMisc::own)
//   st.begin(c, stream)             clears its outputs and sums, arms the link boxes
//   st.chunk(c, q0, nq, stream)     consumes the coverage words of candidates [q0, q0 + nq)
//   st.end(c, stream)               hands the last chunk's sums over
// *handled = 0 if the call cannot take this road (then nothing the caller sees was touched beyond the op's outputs, which
// it rewrites): links not grouped, too many views per candidate for one chunk, or -- known only afterwards -- a triangle
// whose depth class needs the exact z-buffer (geometry within two near-plane distances of the camera, or crossing the
// far plane).
template <class Stage>
static int vb_cov_chain(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const float* mvp, int Q,
                        int S, int L, int V, int T, int H, int W, hipStream_t stream, int* handled, Stage& st) {
    *handled = 0;
    // EHR_SCORE_PATH (tests, A/B): "tile" = always the per-triangle queue path of ehr_score.hip, "chain" = this one or an error
    const char* const want = getenv("EHR_SCORE_PATH");
    const bool must = want && !strcmp(want, "chain");
    if (want && !strcmp(want, "tile")) return EHR_OK;
    if (!vert_link || L > 32 || S * L > VB_MAX_UNITS || H > 32760 || W > 32736)
        return must ? fail(EHR_ERR_INVALID, "%s: EHR_SCORE_PATH=chain, but the call's sizes do not allow it", st.op) : EHR_OK;
    int rc;
    unsigned long long hash = 0;
    {
        if ((rc = ctx->sc_misc.reserve(4096))) return rc;
        unsigned long long* dh = (unsigned long long*)ctx->sc_misc.ptr;
        EHR_HIP(hipMemsetAsync(dh, 0, sizeof(unsigned long long), stream));
        vb_hash_kernel<<<64, 256, 0, stream>>>((const unsigned*)verts, (size_t)3 * V, (const unsigned*)tris, (size_t)3 * T,
                                                (const unsigned*)vert_link, (size_t)V, dh);
        EHR_LAUNCH_CHECK();
        EHR_HIP(hipMemcpyAsync(ctx->host_pinned, dh, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        EHR_HIP(hipStreamSynchronize(stream));
        hash = *(unsigned long long*)ctx->host_pinned;
    }
    if (ctx->sc_key[0] != verts || ctx->sc_key[1] != tris || ctx->sc_key[2] != vert_link || ctx->sc_key_n[0] != V ||
        ctx->sc_key_n[1] != T || ctx->sc_key_n[2] != L || ctx->sc_hash != hash) {
        bool mixed = false;
        ctx->sc_key[0] = nullptr;
        if ((rc = vb_build_clusters(ctx->sc_clus, ctx->sc_nc, L, V, T, verts, tris, nullptr, vert_link, &mixed))) {
            if (rc == EHR_ERR_INVALID) return EHR_OK;  // (a link with too many triangles for a slot id: the other path takes it)
            return rc;
        }
        ctx->sc_mixed = mixed;
        ctx->sc_key[0] = verts;
        ctx->sc_key[1] = tris;
        ctx->sc_key[2] = vert_link;
        ctx->sc_key_n[0] = V;
        ctx->sc_key_n[1] = T;
        ctx->sc_key_n[2] = L;
        ctx->sc_hash = hash;
    }
    if (ctx->sc_mixed || ctx->sc_nc <= 0)
        return must ? fail(EHR_ERR_INVALID, "%s: EHR_SCORE_PATH=chain, but the mesh's links are not grouped", st.op) : EHR_OK;
    VbCovChunk c;
    c.g = make_geom(H, W, L);
    const BinGeom& g = c.g;
    const int NC = ctx->sc_nc;
    const auto [cl, si] = vb_cluster_index(ctx->sc_clus, NC, L);
    // candidates per chunk: (view, link) units of a chunk fit the job kernel's LDS tables; scratch bounded like the solver's
    const double view_bytes = (double)NC * VB_CLUSTER_REC_BYTES + (double)V * sizeof(float4) + (double)g.nt * 4 * sizeof(u64);
    int Qc = std::max(1, (VB_MAX_UNITS / L) / S);
    Qc = std::max(1, std::min(Qc, (int)(8192.0 * 1048576.0 / (view_bytes * S))));
    Qc = std::min(Qc, Q);
    const int Bc = Qc * S;
    size_t bytes;
    if ((rc = ctx->sc_posc.reserve((size_t)Bc * V * sizeof(float4)))) return rc;
    vb_recs(nullptr, Bc, NC, &bytes);
    if ((rc = ctx->sc_entries.reserve(bytes))) return rc;
    const size_t own_bytes = st.own_bytes(Bc, g.nt);
    vb_score_misc(nullptr, Qc, Bc, L, g.nt, own_bytes, &bytes);
    if ((rc = ctx->sc_misc.reserve(bytes))) return rc;
    ctx->sc_entries_cap = 0;  // (the per-triangle path sizes its queues again if it runs after this)
    c.m = vb_score_misc(ctx->sc_misc.ptr, Qc, Bc, L, g.nt, own_bytes);
    c.S = S; c.Qc = Qc; c.Bc = Bc; c.nlbox = VB_LBOX_STRIDE * Bc * L; c.num_cus = ctx->num_cus;
    const VbScoreMisc& m = c.m;
    float4* posc = (float4*)ctx->sc_posc.ptr;
    EHR_HIP(hipMemsetAsync(m.hv.gen, 0, m.zero_bytes, stream));
    const int nvb = (std::max(V, 1) + 255) / 256;
    const int nitems = nvb + (NC + 3) / 4;
    const int job_wgs = vb_xcd_round_up(ctx->num_cus * VB_JOB_GRID);
    if ((rc = st.begin(c, stream))) return rc;  // (link boxes start empty; afterwards the last stage re-arms them)
    for (int q0 = 0; q0 < Q; q0 += Qc) {
        const int nq = std::min(Qc, Q - q0), Bk = nq * S;
        const VbRecs recs = vb_recs(ctx->sc_entries.ptr, Bk, NC);
        const VbVertexGrid vg = vb_vertex_grid(ctx->num_cus, nitems, Bk);
        StepHead none = {};
        vb_vertex_kernel<false><<<dim3(vg.gx * Bk), 256, 0, stream>>>(verts, vert_link, tris, cl, none, const_cast<float*>(mvp) + (size_t)q0 * S * L * 16,
                                                                   V, nvb, g, posc, recs, m.lbox, (int*)m.tcov, Bk * g.nt * 8, m.meta, Bk, vg.gx,
                                                                   vg.xcd_views, m.hv, VB_ROLE_FIRST_CHUNK | VB_ROLE_POS_ONLY);
        EHR_LAUNCH_CHECK();
        VbJobParams jp = {};
        jp.g = g; jp.B = Bk; jp.cl = cl; jp.si = si; jp.rc = recs; jp.lbox = m.lbox; jp.hv = m.hv;  // (use_hint = 0)
        jp.rq.verts = verts; jp.rq.posc = posc; jp.rq.V = V; jp.rq.meta = m.meta;
        jp.rq.mvp = mvp + (size_t)q0 * S * L * 16;
        jp.co = {m.tcov, m.sticky, S};
        jp.heavy_t = 0x7fffffff;
        jp.med_t0 = 0x7fffffff;
        vb_job_kernel<true><<<job_wgs, 256, 0, stream>>>(jp);
        EHR_LAUNCH_CHECK();
        if ((rc = st.chunk(c, q0, nq, stream))) return rc;
    }
    if ((rc = st.end(c, stream))) return rc;
    EHR_HIP(hipMemcpyAsync(ctx->host_pinned, m.sticky, sizeof(int), hipMemcpyDeviceToHost, stream));
    EHR_HIP(hipMemcpyAsync(ctx->host_pinned + 1, m.meta + EHR_META_OVERFLOW, sizeof(int), hipMemcpyDeviceToHost, stream));
    EHR_HIP(hipStreamSynchronize(stream));
    if (ctx->host_pinned[0] || ctx->host_pinned[1])  // a triangle needs the exact z-buffer: the other path redoes the call
        return must ? fail(EHR_ERR_INVALID, "%s: EHR_SCORE_PATH=chain, but a triangle needs the exact z-buffer", st.op) : EHR_OK;
    *handled = 1;
    return EHR_OK;
}

// Last stage of the scoring op: vb_score_count_kernel, sums collected per chunk in m.sacc and handed to `score` by the
// next launch.
struct VbVarianceStage {
    const char* op = "ehr_mask_variance";
    long long* score;
    unsigned char* count;
    int Q, H, W;
    unsigned long long* prev_sacc = nullptr;
    long long* prev_score = nullptr;
    int prev_nq = 0, flip = 0;
    size_t own_bytes(int, int) const { return 0; }
    int begin(const VbCovChunk& c, hipStream_t stream) {
        EHR_HIP(hipMemsetAsync(c.m.sacc, 0, 2 * 16 * (size_t)c.Qc * sizeof(unsigned long long), stream));
        EHR_HIP(hipMemsetAsync(score, 0, (size_t)Q * sizeof(long long), stream));
        if (count) EHR_HIP(hipMemsetAsync(count, 0, (size_t)Q * H * W, stream));
        vb_score_count_kernel<<<64, 256, 0, stream>>>(c.g, 0, c.S, c.m.tcov, c.m.sacc, nullptr, c.m.lbox, c.nlbox, c.m.sacc, score, 0);
        EHR_LAUNCH_CHECK();
        prev_sacc = c.m.sacc;
        prev_score = score;
        return EHR_OK;
    }
    int chunk(const VbCovChunk& c, int q0, int nq, hipStream_t stream) {
        unsigned long long* const sacc = c.m.sacc + (size_t)flip * 16 * c.Qc;
        vb_score_count_kernel<<<std::min((nq * c.g.nt + 3) / 4, VB_SCORE_COUNT_GRID * c.num_cus), 256, 0, stream>>>(
            c.g, nq, c.S, c.m.tcov, sacc, count ? count + (size_t)q0 * H * W : nullptr, c.m.lbox, c.nlbox, prev_sacc, prev_score, prev_nq);
        EHR_LAUNCH_CHECK();
        prev_sacc = sacc;
        prev_score = score + q0;
        prev_nq = nq;
        flip ^= 1;
        return EHR_OK;
    }
    int end(const VbCovChunk& c, hipStream_t stream) {
        vb_score_count_kernel<<<1, 256, 0, stream>>>(c.g, 0, c.S, c.m.tcov, c.m.sacc, nullptr, c.m.lbox, 0, prev_sacc, prev_score, prev_nq);
        EHR_LAUNCH_CHECK();
        return EHR_OK;
    }
};

int ehr::vbuf_score(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const float* mvp, int Q,
                    int S, int L, int V, int T, int H, int W, long long* score, unsigned char* count, hipStream_t stream,
                    int* handled) {
    VbVarianceStage st;
    st.score = score; st.count = count; st.Q = Q; st.H = H; st.W = W;
    return vb_cov_chain(ctx, verts, tris, vert_link, mvp, Q, S, L, V, T, H, W, stream, handled, st);
}

// Last stage of the pose search: the observed masks packed once per call (begin), then vb_overlap_count_kernel per chunk,
// sums collected in VbOverlapMisc::oacc and handed to `overlap` [Q][S][2] by the next launch.
constexpr int VB_OVERLAP_WAVE_ITEMS = 32;  // (candidate, tile) items a wave of the count kernel owns, at least: a candidate's
                                           // line then takes nt / 32 atomics (113 at 1280x720) instead of one per tile
struct VbOverlapStage {
    const char* op = "ehr_mask_overlap";
    const float* ref;
    long long* overlap;
    long long* ref_area;
    int Q, S;
    VbOverlapMisc o = {};
    unsigned long long* prev_oacc = nullptr;
    long long* prev_out = nullptr;
    int prev_n = 0, flip = 0;
    size_t own_bytes(int Bc, int nt) const {
        size_t bytes;
        vb_overlap_misc(nullptr, Bc, S, nt, &bytes);
        return bytes;
    }
    int begin(const VbCovChunk& c, hipStream_t stream) {
        o = vb_overlap_misc(c.m.own, c.Bc, c.S, c.g.nt);
        EHR_HIP(hipMemsetAsync(o.oacc, 0, 2 * 16 * (size_t)c.Bc * sizeof(unsigned long long), stream));
        EHR_HIP(hipMemsetAsync(overlap, 0, (size_t)Q * c.S * 2 * sizeof(long long), stream));
        EHR_HIP(hipMemsetAsync(ref_area, 0, (size_t)c.S * sizeof(long long), stream));
        vb_overlap_pack_ref_kernel<<<dim3(std::min((c.g.nt + 3) / 4, 16), c.S), 256, 0, stream>>>(c.g, ref, o.rbits,
                                                                                                  (unsigned long long*)ref_area);
        EHR_LAUNCH_CHECK();
        vb_overlap_count_kernel<<<64, 256, 0, stream>>>(c.g, 0, c.S, 1, c.m.tcov, o.rbits, o.oacc, c.m.lbox, c.nlbox, o.oacc, overlap, 0);
        EHR_LAUNCH_CHECK();
        prev_oacc = o.oacc;
        prev_out = overlap;
        return EHR_OK;
    }
    int chunk(const VbCovChunk& c, int q0, int nq, hipStream_t stream) {
        unsigned long long* const oacc = o.oacc + (size_t)flip * 16 * c.Bc;
        const long long total = (long long)nq * c.g.nt;
        const long long max_waves = 4ll * VB_SCORE_COUNT_GRID * c.num_cus;
        const int per_wave = (int)std::max<long long>(VB_OVERLAP_WAVE_ITEMS, (total + max_waves - 1) / max_waves);
        const int wgs = (int)((total + 4ll * per_wave - 1) / (4ll * per_wave));
        vb_overlap_count_kernel<<<wgs, 256, 0, stream>>>(c.g, nq, c.S, per_wave, c.m.tcov, o.rbits, oacc, c.m.lbox, c.nlbox, prev_oacc,
                                                         prev_out, prev_n);
        EHR_LAUNCH_CHECK();
        prev_oacc = oacc;
        prev_out = overlap + (size_t)q0 * c.S * 2;
        prev_n = nq * c.S;
        flip ^= 1;
        return EHR_OK;
    }
    int end(const VbCovChunk& c, hipStream_t stream) {
        vb_overlap_count_kernel<<<1, 256, 0, stream>>>(c.g, 0, c.S, 1, c.m.tcov, o.rbits, o.oacc, c.m.lbox, 0, prev_oacc, prev_out, prev_n);
        EHR_LAUNCH_CHECK();
        return EHR_OK;
    }
};

int ehr::vbuf_overlap(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const float* mvp,
                      const float* ref, int Q, int S, int L, int V, int T, int H, int W, long long* overlap, long long* ref_area,
                      hipStream_t stream, int* handled) {
    VbOverlapStage st;
    st.ref = ref; st.overlap = overlap; st.ref_area = ref_area; st.Q = Q; st.S = S;
    return vb_cov_chain(ctx, verts, tris, vert_link, mvp, Q, S, L, V, T, H, W, stream, handled, st);
}

// The soft score's own part of the coverage chain's scratch
struct VbCostMisc {
    unsigned long long* cacc;   // [2][Bc][16] {area, sum_0 .. sum_{C-1}} of a (candidate, view), one 128-byte line each, double buffered
    int32_t* cpack;             // [S][nt][C][256] the cost images, tile-major in the coverage words' bit order (1 KB per channel, view and tile)
};
static VbCostMisc vb_cost_misc(void* base, size_t Bc, int S, int nt, int C, size_t* bytes = nullptr) {
    VbCarve c{(uintptr_t)base};
    VbCostMisc m;
    m.cacc = c.take<unsigned long long>(2 * 16 * Bc, 128);
    m.cpack = c.take<int32_t>((size_t)S * nt * C * 256, 128);
    if (bytes) *bytes = c.at - (uintptr_t)base;
    return m;
}

// Last stage of the pose search's soft score: the cost images packed once per call (begin), then vb_cost_count_kernel per
// chunk, sums collected in VbCostMisc::cacc and handed to `sums` [Q][S][C+1] by the next launch.
constexpr int VB_COST_WAVE_ITEMS = 8;  // tiles of a candidate a wave of the count kernel owns, at least; only waves that met coverage
                                       // flush, so a line sees at most nt / 8 atomics per value and mostly far fewer
struct VbCostStage {
    const char* op = "ehr_mask_cost";
    const int32_t* cost;
    long long* sums;
    int Q, S, C;
    VbCostMisc o = {};
    unsigned long long* prev_cacc = nullptr;
    long long* prev_out = nullptr;
    int prev_n = 0, flip = 0;
    size_t own_bytes(int Bc, int nt) const {
        size_t bytes;
        vb_cost_misc(nullptr, Bc, S, nt, C, &bytes);
        return bytes;
    }
    void count(int wgs, const VbCovChunk& c, int nq, int per_wave, unsigned long long* cacc, int nlbox, hipStream_t stream) const {
        auto go = [&](auto kernel) {
            kernel<<<wgs, 256, 0, stream>>>(c.g, nq, c.S, per_wave, c.m.tcov, o.cpack, cacc, c.m.lbox, nlbox, prev_cacc, prev_out, prev_n);
        };
        switch (C) {
            case 1: go(vb_cost_count_kernel<1>); break;
            case 2: go(vb_cost_count_kernel<2>); break;
            case 3: go(vb_cost_count_kernel<3>); break;
            default: go(vb_cost_count_kernel<4>); break;
        }
    }
    int begin(const VbCovChunk& c, hipStream_t stream) {
        o = vb_cost_misc(c.m.own, c.Bc, c.S, c.g.nt, C);
        EHR_HIP(hipMemsetAsync(o.cacc, 0, 2 * 16 * (size_t)c.Bc * sizeof(unsigned long long), stream));
        EHR_HIP(hipMemsetAsync(sums, 0, (size_t)Q * c.S * (C + 1) * sizeof(long long), stream));
        vb_cost_pack_kernel<<<dim3(std::min((c.g.nt + 3) / 4, 256), c.S, C), 256, 0, stream>>>(c.g, cost, c.S, C, o.cpack);
        EHR_LAUNCH_CHECK();
        prev_cacc = o.cacc;
        prev_out = sums;
        count(64, c, 0, 1, o.cacc, c.nlbox, stream);
        EHR_LAUNCH_CHECK();
        return EHR_OK;
    }
    int chunk(const VbCovChunk& c, int q0, int nq, hipStream_t stream) {
        unsigned long long* const cacc = o.cacc + (size_t)flip * 16 * c.Bc;
        const long long total = (long long)nq * c.g.nt;
        const long long max_waves = 4ll * VB_SCORE_COUNT_GRID * c.num_cus;
        const int per_wave = (int)std::max<long long>(VB_COST_WAVE_ITEMS, (total + max_waves - 1) / max_waves);
        const long long waves = (long long)nq * ((c.g.nt + per_wave - 1) / per_wave);  // (the kernel forms the same quotient)
        count((int)((waves + 3) / 4), c, nq, per_wave, cacc, c.nlbox, stream);
        EHR_LAUNCH_CHECK();
        prev_cacc = cacc;
        prev_out = sums + (size_t)q0 * c.S * (C + 1);
        prev_n = nq * c.S;
        flip ^= 1;
        return EHR_OK;
    }
    int end(const VbCovChunk& c, hipStream_t stream) {
        count(1, c, 0, 1, o.cacc, 0, stream);
        EHR_LAUNCH_CHECK();
        return EHR_OK;
    }
};

int ehr::vbuf_cost(ehr_ctx* ctx, const float* verts, const int32_t* tris, const int32_t* vert_link, const float* mvp,
                   const int32_t* cost, int C, int Q, int S, int L, int V, int T, int H, int W, long long* sums,
                   hipStream_t stream, int* handled) {
    VbCostStage st;
    st.cost = cost; st.sums = sums; st.Q = Q; st.S = S; st.C = C;
    return vb_cov_chain(ctx, verts, tris, vert_link, mvp, Q, S, L, V, T, H, W, stream, handled, st);
}

// Binds a reference mask to the plan (ehr_fused_bind_ref): one pass stores per (view, tile) the fixed-point sum(ref^2)
// exactly as the composite kernel would add it for a tile no link touches, and per view the total.  ref == NULL unbinds.
// views < B (ehr_fused_bind_ref_shared): ref holds `views` images which the plan's B = P x views virtual views share; the
// sums are TILED -- computed once per hypothesis into the layout of a B-view reference -- so that every reader indexes
// them by virtual view like any others (9.6 KB per 640x480 view).
int ehr::vbuf_bind_ref(ehr_ctx* ctx, const float* ref, int views, hipStream_t stream) {
    ctx->vb_ref = nullptr;
    if (!ref) return EHR_OK;
    const int B = ctx->pB, H = ctx->pH, W = ctx->pW;
    if (views <= 0 || B % views != 0) return fail(EHR_ERR_INVALID, "ehr_fused_bind_ref: the plan's %d views are not a multiple of %d", B, views);
    BinGeom g = make_geom(H, W, ctx->pL);
    long long* tsum = (long long*)ctx->vb_refsum.ptr;
    long long* vtot = tsum + (size_t)B * g.nt;
    EHR_HIP(hipMemsetAsync(vtot, 0, ((size_t)B + 1) * sizeof(long long), stream));
    const float* const weight = ctx->vb_weight;  // bound weights: the cached sums are sum(w ref^2)
    const int vec_ok = ((W & 3) == 0) && (((uintptr_t)ref & 15) == 0) && (((uintptr_t)weight & 15) == 0);
    const int nw = views * g.nt;
    for (int b0 = 0; b0 < B; b0 += views) {
        const VbWeight wt = {weight, b0, weight ? ctx->vb_weight_views : 1};
        if (weight)
            vb_refsum_kernel<true><<<(nw + 3) / 4, 256, 0, stream>>>(g, views, ref, vec_ok, tsum + (size_t)b0 * g.nt, vtot + b0, (int*)(vtot + B), wt);
        else
            vb_refsum_kernel<false><<<(nw + 3) / 4, 256, 0, stream>>>(g, views, ref, vec_ok, tsum + (size_t)b0 * g.nt, vtot + b0, (int*)(vtot + B), wt);
        EHR_LAUNCH_CHECK();
    }
    ctx->vb_ref = ref;
    ctx->vb_ref_views = views;
    return EHR_OK;
}
