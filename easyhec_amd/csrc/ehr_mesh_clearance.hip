// ehr_mesh_clearance.hip -- the narrow phase behind the sphere proxies of the feasibility filter (easyhec_amd/feasibility.py,
// DESIGN.md section 6t): ehr_mesh_clearance of include/ehr.h.
//
//   mesh_clearance_kernel : link_poses [n,L,16] + the proxy spheres + the triangles each sphere stands for -> per configuration
//                           the exact distance between the meshes of the enabled link pairs (with a link pair and a triangle
//                           pair that attain it) and of the meshes to planes and obstacle spheres.  One workgroup of 256 threads
//                           per configuration.  The spheres go to the base frame once, into LDS, as in ehr_feasible.hip; they are
//                           the broad phase.  A wave takes a leaf (sphere) of the pair's first link and tests 64 leaves of the second
//                           per pass.  For every leaf pair that survives it stages the spheres around the first leaf's triangles
//                           in its own LDS slice, each lane holds the sphere of one triangle of the second, and the triangle
//                           pairs whose spheres allow it go to the wave's queue.  The long part -- the triangle-triangle
//                           distance -- runs on 64 queued pairs at a time, a lane each, so that no lane idles through it.
//
// Float64 throughout, -ffp-contract=off, every expression of the contract written once below (mesh_*; feas_* of ehr_feas_core.h)
// and restated operation by operation in tests/mesh_clearance_reference.py.  Division and square root are correctly rounded and
// a minimum is exact in any order, so the outputs do not depend on how the pairs are dealt out or on what was culled; the
// witnesses are SOME pair at the minimum.  The running minimum is shared through an LDS atomic; no atomics to global memory, no
// allocation, no synchronisation with the host, one launch.
#include "ehr_feas_core.h"

#define MESH_THREADS 256
#define MESH_WAVES (MESH_THREADS / 64)
#define MESH_STAGE 64   // triangles of the first leaf a wave stages at a time
#define MESH_REC 4      // doubles of a staged triangle: the centre and radius of the sphere around its world corners
#define MESH_QUEUE 128  // triangle pairs a wave's queue holds: fewer than 64 wait, a pass over one staged triangle adds up to 64
#define MESH_SLICE (MESH_REC * MESH_STAGE + MESH_QUEUE)  // doubles of a wave's LDS slice (a queued pair is two ints)

namespace ehr {

// LDS of one workgroup, all dynamic, every part a multiple of 16 bytes: x | y | z | r of the Sp spheres, the links' bounds, the
// waves' staging slices (the final reduction reuses them), the offsets, the shared minimum
#define MESH_TAIL_BOUNDS (EHR_FEAS_MAX_LINKS * 4)
#define MESH_TAIL_STAGE (MESH_WAVES * MESH_SLICE)
#define MESH_TAIL_BYTES ((MESH_TAIL_BOUNDS + MESH_TAIL_STAGE) * 8 + 36 * 4 + 16)
static_assert(MESH_TAIL_STAGE * 8 >= MESH_THREADS * (2 * 8 + 3 * 4), "the reduction fits into the staging slices");
static inline size_t mesh_lds_bytes(int Sp) { return (size_t)Sp * 32 + MESH_TAIL_BYTES; }

struct V3 {
    double x, y, z;
};

// ---- the contract's expressions (include/ehr.h spells them out) -------------------------------------------------------------
__device__ __forceinline__ V3 mesh_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double mesh_dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 mesh_cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double mesh_clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }
// num / den where den > 0, else 0: a zero-length edge or zero-area triangle never divides (an exact-zero test, no epsilon)
__device__ __forceinline__ double mesh_ratio(double num, double den) { return den > 0.0 ? num / den : 0.0; }
__device__ __forceinline__ double mesh_min(double a, double b) { return b < a ? b : a; }

// point against segment a..b: t = clamp(((p - a).(b - a)) / |b - a|^2), q = a + (b - a) t
__device__ __forceinline__ double mesh_point_segment(V3 p, V3 a, V3 b) {
    const V3 ab = mesh_sub(b, a), ap = mesh_sub(p, a);
    const double e = mesh_dot(ab, ab);
    const double t = e > 0.0 ? mesh_clamp01(mesh_dot(ap, ab) / e) : 0.0;
    const V3 q = {a.x + ab.x * t, a.y + ab.y * t, a.z + ab.z * t};
    const V3 d = mesh_sub(p, q);
    return feas_norm2(d.x, d.y, d.z);
}

// point against triangle: the closest point q = (a + ab v) + ac w by the Voronoi region p lies in; a triangle of zero area
// (|ab x ac|^2 == 0) is its three edges
__device__ __forceinline__ double mesh_point_triangle(V3 p, V3 a, V3 b, V3 c) {
    const V3 ab = mesh_sub(b, a), ac = mesh_sub(c, a);
    const V3 n = mesh_cross(ab, ac);
    if (!(mesh_dot(n, n) > 0.0))
        return mesh_min(mesh_min(mesh_point_segment(p, a, b), mesh_point_segment(p, b, c)), mesh_point_segment(p, c, a));
    const V3 ap = mesh_sub(p, a), bp = mesh_sub(p, b), cp = mesh_sub(p, c);
    const double d1 = mesh_dot(ab, ap), d2 = mesh_dot(ac, ap), d3 = mesh_dot(ab, bp), d4 = mesh_dot(ac, bp);
    const double d5 = mesh_dot(ab, cp), d6 = mesh_dot(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    double v, w;
    if (d1 <= 0.0 && d2 <= 0.0) {  // corner a
        v = 0.0, w = 0.0;
    } else if (d3 >= 0.0 && d4 <= d3) {  // corner b
        v = 1.0, w = 0.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {  // edge ab
        v = mesh_ratio(d1, d1 - d3), w = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {  // corner c
        v = 0.0, w = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {  // edge ac
        v = 0.0, w = mesh_ratio(d2, d2 - d6);
    } else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) {  // edge bc
        w = mesh_ratio(e43, e43 + e56), v = 1.0 - w;
    } else {  // the face
        const double s = (va + vb) + vc;
        v = mesh_ratio(vb, s), w = mesh_ratio(vc, s);
    }
    const V3 q = {(a.x + ab.x * v) + ac.x * w, (a.y + ab.y * v) + ac.y * w, (a.z + ab.z * v) + ac.z * w};
    const V3 d = mesh_sub(p, q);
    return feas_norm2(d.x, d.y, d.z);
}

// segment p1..q1 against segment p2..q2: the clamped closest parameters s, t
__device__ __forceinline__ double mesh_segment_segment(V3 p1, V3 q1, V3 p2, V3 q2) {
    const V3 d1 = mesh_sub(q1, p1), d2 = mesh_sub(q2, p2), r = mesh_sub(p1, p2);
    const double a = mesh_dot(d1, d1), e = mesh_dot(d2, d2), f = mesh_dot(d2, r), c = mesh_dot(d1, r), b = mesh_dot(d1, d2);
    double s, t;
    if (a > 0.0 && e > 0.0) {
        const double den = a * e - b * b;
        s = den > 0.0 ? mesh_clamp01((b * f - c * e) / den) : 0.0;  // (parallel: any s, the clamps below settle it)
        t = (b * s + f) / e;
        if (t < 0.0) {
            t = 0.0, s = mesh_clamp01(-c / a);
        } else if (t > 1.0) {
            t = 1.0, s = mesh_clamp01((b - c) / a);
        }
    } else if (a > 0.0) {  // the second is a point
        t = 0.0, s = mesh_clamp01(-c / a);
    } else if (e > 0.0) {  // the first is a point
        s = 0.0, t = mesh_clamp01(f / e);
    } else {
        s = 0.0, t = 0.0;
    }
    const V3 c1 = {p1.x + d1.x * s, p1.y + d1.y * s, p1.z + d1.z * s};
    const V3 c2 = {p2.x + d2.x * t, p2.y + d2.y * t, p2.z + d2.z * t};
    const V3 d = mesh_sub(c1, c2);
    return feas_norm2(d.x, d.y, d.z);
}

// does the open segment p..q pass through triangle a b c: its ends strictly on either side of the plane, and the three scalar
// triple products of its direction with the corners seen from p of one sign (zero counts with both).  A triangle of zero area
// has n = 0 and is never pierced; an end ON the plane is the vertex tests' business.
__device__ __forceinline__ bool mesh_pierces(V3 p, V3 q, V3 a, V3 b, V3 c) {
    const V3 n = mesh_cross(mesh_sub(b, a), mesh_sub(c, a));
    const double sp = mesh_dot(n, mesh_sub(p, a)), sq = mesh_dot(n, mesh_sub(q, a));
    if (!((sp > 0.0 && sq < 0.0) || (sp < 0.0 && sq > 0.0))) return false;
    const V3 d = mesh_sub(q, p), pa = mesh_sub(a, p), pb = mesh_sub(b, p), pc = mesh_sub(c, p);
    const double u = mesh_dot(d, mesh_cross(pa, pb)), v = mesh_dot(d, mesh_cross(pb, pc)), w = mesh_dot(d, mesh_cross(pc, pa));
    return (u >= 0.0 && v >= 0.0 && w >= 0.0) || (u <= 0.0 && v <= 0.0 && w <= 0.0);
}

// squared distance of triangle A to triangle B: 0 where an edge of one pierces the other, else the least of the six
// vertex-triangle and nine edge-edge squared distances
__device__ __forceinline__ double mesh_triangle_triangle(const V3* A, const V3* B) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (mesh_pierces(A[k], A[(k + 1) % 3], B[0], B[1], B[2])) return 0.0;
        if (mesh_pierces(B[k], B[(k + 1) % 3], A[0], A[1], A[2])) return 0.0;
    }
    double m = mesh_point_triangle(A[0], B[0], B[1], B[2]);
    m = mesh_min(m, mesh_point_triangle(A[1], B[0], B[1], B[2]));
    m = mesh_min(m, mesh_point_triangle(A[2], B[0], B[1], B[2]));
    m = mesh_min(m, mesh_point_triangle(B[0], A[0], A[1], A[2]));
    m = mesh_min(m, mesh_point_triangle(B[1], A[0], A[1], A[2]));
    m = mesh_min(m, mesh_point_triangle(B[2], A[0], A[1], A[2]));
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) m = mesh_min(m, mesh_segment_segment(A[i], A[(i + 1) % 3], B[j], B[(j + 1) % 3]));
    return m;
}

// ---- what is NOT part of the contract: bounds that only cull -----------------------------------------------------------------
// triangle t of link-frame `triangles` at pose T -> world corners W, and a sphere about their mean that contains them
__device__ __forceinline__ void mesh_load(const double* __restrict__ triangles, size_t t, const float* __restrict__ T, V3* W,
                                          V3& ctr, double& rad) {
    const double* q = triangles + 9 * t;
    for (int k = 0; k < 3; k++) {
        const double x = q[3 * k], y = q[3 * k + 1], z = q[3 * k + 2];
        W[k] = {feas_world(T, x, y, z), feas_world(T + 4, x, y, z), feas_world(T + 8, x, y, z)};
    }
    ctr = {((W[0].x + W[1].x) + W[2].x) * (1.0 / 3.0), ((W[0].y + W[1].y) + W[2].y) * (1.0 / 3.0),
           ((W[0].z + W[1].z) + W[2].z) * (1.0 / 3.0)};
    double r2 = 0.0;
    for (int k = 0; k < 3; k++) {
        const V3 d = mesh_sub(W[k], ctr);
        r2 = fmax(r2, feas_norm2(d.x, d.y, d.z));
    }
    rad = sqrt(r2);
}

// a wave's LDS writes are seen by its own later reads (the hardware keeps one wave's LDS operations in order); this keeps the
// compiler from moving them across
__device__ __forceinline__ void mesh_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double mesh_shared_min(const unsigned long long* p) {  // the same value in every lane of the wave
    const unsigned long long v = *(const volatile unsigned long long*)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_clearance_kernel(
    const float* __restrict__ link_poses, const double* __restrict__ spheres, const FeasOffsets offs,
    const double* __restrict__ link_bounds, const unsigned* __restrict__ pair_enable, const double* __restrict__ planes, int Np,
    const double* __restrict__ obstacles, int No, unsigned env_links, double cutoff, int L, int S, int Sp,
    const double* __restrict__ triangles, const int* __restrict__ tri_offsets, int T, double* __restrict__ mesh_clear,
    int* __restrict__ mesh_pair, int* __restrict__ mesh_tri, double* __restrict__ env_clear) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* X = (double*)smem;
    double* Y = X + Sp;
    double* Z = Y + Sp;
    double* Rr = Z + Sp;
    double* BW = Rr + Sp;                    // [L][4] bounding spheres, base frame
    double* stage = BW + MESH_TAIL_BOUNDS;   // [waves][MESH_SLICE]; the reduction's at the end
    int* off = (int*)(stage + MESH_TAIL_STAGE);  // [L + 1]
    unsigned long long* shared2 = (unsigned long long*)(off + 36);  // the least squared distance any thread has found (bits)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t b = blockIdx.x;
    const float* P = link_poses + b * (size_t)L * 16;
    const double cull = cutoff + FEAS_CULL_SLACK;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);

    // a configuration that cannot be judged does not pass: NaN, and nothing else of it is read
    int bad = 0;
    for (int e = tid; e < L * 16; e += MESH_THREADS) bad |= !feas_finite(P[e]);
    if (tid <= L) off[tid] = offs.v[tid];
    if (tid == 0) *shared2 = 0x7ff0000000000000ull;
    bad = __syncthreads_or(bad);
    if (bad) {
        if (tid == 0) {
            mesh_clear[b] = feas_nan();
            env_clear[b] = feas_nan();
            mesh_pair[b] = -1;
            mesh_tri[2 * b] = mesh_tri[2 * b + 1] = -1;
        }
        return;
    }

    // every sphere to the base frame, once
    for (int s = tid; s < S; s += MESH_THREADS) {
        int lo = 0, hi = L;  // off[lo] <= s < off[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (off[mid] <= s) lo = mid; else hi = mid;
        }
        const float* Tl = P + lo * 16;
        const double x = spheres[4 * (size_t)s], y = spheres[4 * (size_t)s + 1], z = spheres[4 * (size_t)s + 2];
        X[s] = feas_world(Tl, x, y, z);
        Y[s] = feas_world(Tl + 4, x, y, z);
        Z[s] = feas_world(Tl + 8, x, y, z);
        Rr[s] = spheres[4 * (size_t)s + 3];
    }
    if (tid < L) {
        const float* Tl = P + tid * 16;
        const double x = link_bounds[4 * tid], y = link_bounds[4 * tid + 1], z = link_bounds[4 * tid + 2];
        BW[4 * tid] = feas_world(Tl, x, y, z);
        BW[4 * tid + 1] = feas_world(Tl + 4, x, y, z);
        BW[4 * tid + 2] = feas_world(Tl + 8, x, y, z);
        BW[4 * tid + 3] = link_bounds[4 * tid + 3];
    }
    __syncthreads();

    // the triangles of sphere s: tri_offsets is device memory nobody has checked, so every range is clamped into 0..T
    auto tri_range = [&](int s, int& t0, int& t1) {
        t0 = min(max(tri_offsets[s], 0), T);
        t1 = min(max(tri_offsets[s + 1], t0), T);
    };

    // ---- the environment: a wave per leaf of the links in env_links, a lane per triangle.  A leaf's sphere contains its
    // triangles in the link frame; a float32 pose that is no exact rotation moves that by parts in 1e7 of the radius, which the
    // slack of 1e-6 m covers (as for the proxies themselves): a plane (unit normal) or an obstacle the sphere clears by more
    // than cutoff + slack holds no vertex or triangle below cutoff, and what is not visited would not have lowered the minimum.
    double ec = cutoff;
    if (Np > 0 || No > 0) {
        for (int l = 0; l < L; l++) {
            if (!((env_links >> l) & 1u)) continue;
            const float* Tl = P + l * 16;
            for (int s = off[l] + wave; s < off[l + 1]; s += MESH_WAVES) {
                const double cx = X[s], cy = Y[s], cz = Z[s], r = Rr[s];
                unsigned pm = 0;
                for (int p = 0; p < Np; p++)
                    if (!(feas_plane(planes[4 * p], planes[4 * p + 1], planes[4 * p + 2], planes[4 * p + 3], cx, cy, cz, r) > cull))
                        pm |= 1u << p;
                int t0, t1;
                tri_range(s, t0, t1);
                for (int tc = t0; tc < t1; tc += 64) {
                    const int t = tc + lane;
                    const bool have = t < t1;
                    bool loaded = false;
                    V3 W[3] = {}, ctr;
                    double rad;
                    if (pm) {
                        if (have) mesh_load(triangles, (size_t)t, Tl, W, ctr, rad);
                        loaded = true;
                        for (unsigned m = pm; m; m &= m - 1) {
                            const int p = __ffs(m) - 1;
                            const double nx = planes[4 * p], ny = planes[4 * p + 1], nz = planes[4 * p + 2], pd = planes[4 * p + 3];
                            for (int k = 0; k < 3; k++) {
                                const double d = feas_plane(nx, ny, nz, pd, W[k].x, W[k].y, W[k].z, 0.0);  // ((n.v) + d), r = 0
                                if (have && d < ec) ec = d;
                            }
                        }
                    }
                    for (int o0 = 0; o0 < No; o0 += 64) {
                        const int o = o0 + lane;
                        const bool near = o < No && !(feas_gap(cx - obstacles[4 * o], cy - obstacles[4 * o + 1],
                                                               cz - obstacles[4 * o + 2], r, obstacles[4 * o + 3]) > cull);
                        unsigned long long m = __ballot(near);
                        if (m && !loaded) {
                            if (have) mesh_load(triangles, (size_t)t, Tl, W, ctr, rad);
                            loaded = true;
                        }
                        for (; m; m &= m - 1) {
                            const int k = o0 + __ffsll(m) - 1;
                            const V3 c = {obstacles[4 * k], obstacles[4 * k + 1], obstacles[4 * k + 2]};
                            if (have) {
                                const double d = sqrt(mesh_point_triangle(c, W[0], W[1], W[2])) - obstacles[4 * k + 3];
                                if (d < ec) ec = d;
                            }
                        }
                    }
                }
            }
        }
    }

    // ---- the arm against itself.  best2 is this thread's least squared distance, lim what a pair must come below to matter:
    // min(cutoff, the least distance anybody has found so far).  A leaf pair, a triangle against a leaf, or a triangle pair, is
    // skipped only where a lower bound of its distance -- the gap of the spheres around the two -- exceeds lim + slack.  The leaf
    // spheres need the slack for the pose (above); the triangles' own spheres are built from the world corners and need it for
    // rounding only.  What is
    // skipped lies above the final minimum or above cutoff, so the outputs have the bits of the plain evaluation.
    double best2 = inf;
    int bcode = -1, bta = -1, btb = -1;
    double* mine = stage + wave * MESH_SLICE;            // [MESH_REC][MESH_STAGE]: the staged triangles' spheres
    int* queue = (int*)(mine + MESH_REC * MESH_STAGE);  // [MESH_QUEUE][2]: triangle pairs the spheres let through
    const unsigned inL = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
    bool done = false;  // somebody has found a distance of 0: nothing can come below it
    for (int i = 0; i + 1 < L && !done; i++) {
        const unsigned m = pair_enable[i] & ~((2u << i) - 1u) & inL;  // j > i only
        const int oi = off[i], ei = off[i + 1];
        if (!m || ei <= oi) continue;
        for (int j = i + 1; j < L && !done; j++) {
            const int oj = off[j], ej = off[j + 1];
            if (!((m >> j) & 1u) || ej <= oj) continue;
            if (feas_gap(BW[4 * i] - BW[4 * j], BW[4 * i + 1] - BW[4 * j + 1], BW[4 * i + 2] - BW[4 * j + 2], BW[4 * i + 3],
                         BW[4 * j + 3]) > cull)
                continue;
            const float* Ti = P + i * 16;
            const float* Tj = P + j * 16;
            const int code = 32 * i + j;
            int qn = 0;  // triangle pairs waiting in this wave's queue (the same number in every lane, below 64 between passes)
            // the narrow phase proper: `cnt` <= 64 queued pairs from entry q0 on, a lane each
            auto evaluate = [&](int q0, int cnt) {
                mesh_wave_sync();  // (the entries the other lanes wrote)
                if (lane < cnt) {
                    const int ta = queue[2 * (q0 + lane)], tb = queue[2 * (q0 + lane) + 1];
                    V3 A[3], B[3], c;
                    double r;
                    mesh_load(triangles, (size_t)ta, Ti, A, c, r);
                    mesh_load(triangles, (size_t)tb, Tj, B, c, r);
                    const double d2 = mesh_triangle_triangle(A, B);
                    if (d2 < best2) {
                        best2 = d2, bcode = code, bta = ta, btb = tb;
                        atomicMin(shared2, (unsigned long long)__double_as_longlong(d2));  // d2 >= 0: ordered as its bits
                    }
                }
                mesh_wave_sync();  // (... are read before they are written again)
            };
            for (int a = oi + wave; a < ei && !done; a += MESH_WAVES) {
                const double ax = X[a], ay = Y[a], az = Z[a], ar = Rr[a];
                int ta0, ta1;
                tri_range(a, ta0, ta1);
                if (ta1 <= ta0) continue;
                int staged = -1;  // the chunk of leaf a whose spheres are in this wave's slice
                for (int b0 = oj; b0 < ej && !done; b0 += 64) {
                    const double lim = fmin(cutoff, sqrt(mesh_shared_min(shared2)));
                    if (lim == 0.0) {
                        done = true;
                        break;
                    }
                    const int bb = min(b0 + lane, ej - 1);
                    const bool near = b0 + lane < ej && !(feas_gap(ax - X[bb], ay - Y[bb], az - Z[bb], ar, Rr[bb]) > lim + FEAS_CULL_SLACK);
                    for (unsigned long long nm = __ballot(near); nm; nm &= nm - 1) {
                        const int bs = b0 + __ffsll(nm) - 1;
                        int tb0, tb1;
                        tri_range(bs, tb0, tb1);
                        for (int ac = ta0; ac < ta1; ac += MESH_STAGE) {
                            const int na = min(MESH_STAGE, ta1 - ac);
                            if (staged != ac) {
                                mesh_wave_sync();  // (the slice's earlier readers are through)
                                if (lane < na) {
                                    V3 W[3], ctr;
                                    double rad;
                                    mesh_load(triangles, (size_t)(ac + lane), Ti, W, ctr, rad);
                                    mine[lane] = ctr.x;
                                    mine[MESH_STAGE + lane] = ctr.y;
                                    mine[2 * MESH_STAGE + lane] = ctr.z;
                                    mine[3 * MESH_STAGE + lane] = rad;
                                }
                                mesh_wave_sync();
                                staged = ac;
                            }
                            // leaf b's sphere against the sphere of each staged triangle (a lane each, nothing is loaded for
                            // it): only these triangles of leaf a can come within the bar of anything in leaf b
                            const double bx = X[bs], by = Y[bs], bz = Z[bs], br = Rr[bs];
                            const int ka = min(lane, na - 1);
                            const unsigned long long am = __ballot(
                                lane < na && !(feas_gap(mine[ka] - bx, mine[MESH_STAGE + ka] - by, mine[2 * MESH_STAGE + ka] - bz,
                                                        mine[3 * MESH_STAGE + ka], br) > lim + FEAS_CULL_SLACK));
                            if (!am) continue;
                            for (int bc = tb0; bc < tb1; bc += 64) {
                                const int tb = min(bc + lane, tb1 - 1);
                                V3 B[3], cb;
                                double rb;
                                mesh_load(triangles, (size_t)tb, Tj, B, cb, rb);
                                // ... and the same the other way round: this lane's triangle against leaf a's sphere
                                const bool have = bc + lane < tb1 && !(feas_gap(cb.x - ax, cb.y - ay, cb.z - az, rb, ar) > lim + FEAS_CULL_SLACK);
                                if (!__ballot(have)) continue;
                                // this lane's bar: the wave's at the start of the pass, or what the lane has found since
                                double bar = fmin(lim, sqrt(best2)) + FEAS_CULL_SLACK;
                                for (unsigned long long km = am; km; km &= km - 1) {
                                    const int k = __ffsll(km) - 1;
                                    const double dx = mine[k] - cb.x, dy = mine[MESH_STAGE + k] - cb.y, dz = mine[2 * MESH_STAGE + k] - cb.z;
                                    // the spheres' gap exceeds the bar: |d| > t with t = bar + r_a + r_b > 0, compared in
                                    // squares with 1e-12 to spare for the roundings of t, t^2 and d^2 (a few 1e-16 each)
                                    const double t = bar + (mine[3 * MESH_STAGE + k] + rb);
                                    const bool pass = have && !(feas_norm2(dx, dy, dz) > (t * t) * 1.000000000001);
                                    const unsigned long long pm = __ballot(pass);
                                    if (!pm) continue;
                                    if (pass) {  // behind the passing lanes below this one
                                        const int at = qn + __popcll(pm & ((1ull << lane) - 1ull));
                                        queue[2 * at] = ac + k;
                                        queue[2 * at + 1] = tb;
                                    }
                                    qn += __popcll(pm);
                                    if (qn >= 64) {  // a full wave of pairs: no lane idles through the long part
                                        evaluate(qn - 64, 64);
                                        qn -= 64;
                                        bar = fmin(lim, sqrt(best2)) + FEAS_CULL_SLACK;
                                    }
                                }
                            }
                        }
                    }
                }
            }
            if (qn > 0 && !done) evaluate(0, qn);  // (with a 0 found nothing that waits can come below it)
        }
    }

    // minima over the workgroup (the staging slices are free now); among equal distances any witness
    __syncthreads();
    double* red = stage;                          // [2][256]: squared mesh distance | environment
    int* redi = (int*)(stage + 2 * MESH_THREADS);  // [3][256]: pair code | triangle of link i | triangle of link j
    red[tid] = best2;
    red[MESH_THREADS + tid] = ec;
    redi[tid] = bcode;
    redi[MESH_THREADS + tid] = bta;
    redi[2 * MESH_THREADS + tid] = btb;
    __syncthreads();
    for (int w = MESH_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w) {
            if (red[tid + w] < red[tid]) {
                red[tid] = red[tid + w];
                redi[tid] = redi[tid + w];
                redi[MESH_THREADS + tid] = redi[MESH_THREADS + tid + w];
                redi[2 * MESH_THREADS + tid] = redi[2 * MESH_THREADS + tid + w];
            }
            if (red[MESH_THREADS + tid + w] < red[MESH_THREADS + tid]) red[MESH_THREADS + tid] = red[MESH_THREADS + tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double d = sqrt(red[0]);
        const bool below = d < cutoff;
        mesh_clear[b] = below ? d : cutoff;
        mesh_pair[b] = below ? redi[0] : -1;
        mesh_tri[2 * b] = below ? redi[MESH_THREADS] : -1;
        mesh_tri[2 * b + 1] = below ? redi[2 * MESH_THREADS] : -1;
        env_clear[b] = red[MESH_THREADS];
    }
}

}  // namespace ehr

using namespace ehr;

extern "C" {

int ehr_mesh_clearance(const float* link_poses, const double* spheres, const int32_t* sphere_offsets, const double* link_bounds,
                       const uint32_t* pair_enable, const double* planes, int n_planes, const double* obstacles, int n_obstacles,
                       uint32_t env_links, double cutoff, int n, int L, const double* triangles, const int32_t* tri_offsets,
                       int n_triangles, double* mesh_clear, int32_t* mesh_pair, int32_t* mesh_tri, double* env_clear,
                       void* stream) {
    if (L < 1 || L > EHR_FEAS_MAX_LINKS || n < 1)
        return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: bad sizes (L %d: 1 <= L <= %d links, n %d >= 1)", L, EHR_FEAS_MAX_LINKS,
                    n);
    if (n_planes < 0 || n_planes > EHR_FEAS_MAX_PLANES || n_obstacles < 0 || n_obstacles > EHR_FEAS_MAX_OBSTACLES)
        return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: bad sizes (%d planes <= %d, %d obstacles <= %d)", n_planes,
                    EHR_FEAS_MAX_PLANES, n_obstacles, EHR_FEAS_MAX_OBSTACLES);
    if (n_triangles < 0 || n_triangles > EHR_MESH_MAX_TRIANGLES)
        return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: bad sizes (T %d <= %d triangles)", n_triangles, EHR_MESH_MAX_TRIANGLES);
    if (!(cutoff > 0.0) || !(cutoff <= 1.7976931348623157e308))
        return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: cutoff %g must be finite and > 0", cutoff);
    if (!link_poses || !sphere_offsets || !link_bounds || !pair_enable || !tri_offsets || !mesh_clear || !mesh_pair || !mesh_tri ||
        !env_clear || (n_planes > 0 && !planes) || (n_obstacles > 0 && !obstacles) || (n_triangles > 0 && !triangles))
        return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: NULL tensor");
    FeasOffsets offs = {};
    for (int l = 0; l <= L; l++) {
        offs.v[l] = sphere_offsets[l];
        if ((l == 0 && offs.v[0] != 0) || (l > 0 && offs.v[l] < offs.v[l - 1]))
            return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: sphere_offsets must ascend from 0 (entry %d is %d)", l, offs.v[l]);
    }
    const int S = offs.v[L];
    if (S > EHR_FEAS_MAX_SPHERES)
        return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: bad sizes (S %d <= %d spheres)", S, EHR_FEAS_MAX_SPHERES);
    if (S > 0 && !spheres) return fail(EHR_ERR_INVALID, "ehr_mesh_clearance: NULL tensor");
    const int Sp = (S + 1) & ~1;
    const size_t lds = mesh_lds_bytes(Sp);
    if (lds > 64 * 1024) {
        // more than the default limit of a launch's dynamic LDS: ask for it (see ehr_config_clearance)
        if (hipFuncSetAttribute((const void*)mesh_clearance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
            (void)hipGetLastError();
    }
    mesh_clearance_kernel<<<(unsigned)n, MESH_THREADS, lds, (hipStream_t)stream>>>(
        link_poses, spheres, offs, link_bounds, pair_enable, planes, n_planes, obstacles, n_obstacles, env_links, cutoff, L, S, Sp,
        triangles, tri_offsets, n_triangles, mesh_clear, mesh_pair, mesh_tri, env_clear);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
