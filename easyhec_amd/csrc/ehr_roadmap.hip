// ehr_roadmap.hip -- single-source shortest paths of at most H edges over the usable edges of a roadmap (easyhec_amd/feasibility.py,
// DESIGN.md section 6v): ehr_roadmap_paths of include/ehr.h, which states the recursion.
//
//   roadmap_paths_kernel : ONE workgroup of 256 threads.  The layers D_0 .. D_H live in global memory (dist [H+1,V]), so V is
//                          not bound by LDS; round r reads layer r-1 and writes layer r, a node per thread and stride, with a
//                          barrier between the rounds (one workgroup: the barrier orders its global writes).  All H rounds
//                          always run, so no barrier depends on data.  Then every node walks its predecessors back to the
//                          source, twice: once to count the hops, once to write the path in order.
//
// Float64, built with -ffp-contract=off; no atomics, no allocation, no synchronisation with the host.  Every index read from
// device memory is checked before it is used: adjacency slots outside 0..A-1, nodes outside 0..V-1 and edges outside 0..E-1 are
// skipped.
#include "ehr_host.h"

#define ROADMAP_THREADS 256

namespace ehr {

__device__ __forceinline__ double roadmap_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

__global__ void __launch_bounds__(ROADMAP_THREADS) roadmap_paths_kernel(
    const int* __restrict__ adj_start, const int* __restrict__ adj_node, const int* __restrict__ adj_edge, const int A,
    const int* __restrict__ edge_status, const double* __restrict__ edge_length, const int V, const int E, const int source,
    const int H, double* dist, int* pred_node, int* pred_edge, int* __restrict__ hops, int* __restrict__ path,
    int* __restrict__ path_edge, int* __restrict__ changed) {
    __shared__ int count[ROADMAP_THREADS];
    const int tid = threadIdx.x;
    const double inf = roadmap_inf();

    for (int v = tid; v < V; v += ROADMAP_THREADS) dist[v] = v == source ? 0.0 : inf;
    __syncthreads();

    for (int r = 1; r <= H; r++) {
        const double* prev = dist + (size_t)(r - 1) * V;
        int improved = 0;
        for (int v = tid; v < V; v += ROADMAP_THREADS) {
            double best = prev[v];
            int bn = -1, be = -1;
            int i0 = adj_start[v], i1 = adj_start[v + 1];
            if (i0 < 0) i0 = 0;
            if (i1 > A) i1 = A;
            for (int i = i0; i < i1; i++) {
                const int u = adj_node[i], e = adj_edge[i];
                if (u < 0 || u >= V || e < 0 || e >= E) continue;
                if (edge_status[e] != 0) continue;
                const double w = edge_length[e];
                if (!(w >= 0.0) || !(w < inf)) continue;
                const double c = prev[u] + w;
                if (c < best) {
                    best = c;
                    bn = u;
                    be = e;
                }
            }
            dist[(size_t)r * V + v] = best;
            pred_node[(size_t)(r - 1) * V + v] = bn;
            pred_edge[(size_t)(r - 1) * V + v] = be;
            improved += bn >= 0;
        }
        count[tid] = improved;
        __syncthreads();  // layer r is written, and every thread's count
        if (tid == 0) {
            int sum = 0;
            for (int t = 0; t < ROADMAP_THREADS; t++) sum += count[t];
            changed[r - 1] = sum;
        }
        __syncthreads();  // (count has been read)
    }

    // the paths: from (r = H, x = v) a carried round is passed over, a recorded one is taken; r only falls, so <= H steps
    for (int v = tid; v < V; v += ROADMAP_THREADS) {
        int* p = path + (size_t)v * (H + 1);
        int* pe = path_edge + (size_t)v * H;
        for (int k = 0; k <= H; k++) p[k] = -1;
        for (int k = 0; k < H; k++) pe[k] = -1;
        int r = H, x = v, h = 0;
        while (x != source) {
            while (r > 0 && pred_node[(size_t)(r - 1) * V + x] < 0) r--;
            if (r == 0) break;
            x = pred_node[(size_t)(r - 1) * V + x];
            r--;
            h++;
        }
        if (x != source) {
            hops[v] = -1;
            continue;
        }
        hops[v] = h;
        r = H, x = v;
        int pos = h;
        p[pos] = v;
        while (x != source) {
            while (r > 0 && pred_node[(size_t)(r - 1) * V + x] < 0) r--;
            if (r == 0) break;
            pe[pos - 1] = pred_edge[(size_t)(r - 1) * V + x];
            x = pred_node[(size_t)(r - 1) * V + x];
            r--;
            pos--;
            p[pos] = x;
        }
    }
}

}  // namespace ehr

using namespace ehr;

extern "C" {

int ehr_roadmap_paths(const int32_t* adj_start, const int32_t* adj_node, const int32_t* adj_edge, int A,
                      const int32_t* edge_status, const double* edge_length, int V, int E, int source, int H, double* dist,
                      int32_t* pred_node, int32_t* pred_edge, int32_t* hops, int32_t* path, int32_t* path_edge, int32_t* changed,
                      void* stream) {
    if (V < 1 || V > EHR_ROADMAP_MAX_NODES || E < 0 || A < 0 || H < 1 || H > EHR_ROADMAP_MAX_HOPS)
        return fail(EHR_ERR_INVALID, "ehr_roadmap_paths: bad sizes (1 <= V %d <= %d nodes, E %d >= 0, A %d >= 0, 1 <= H %d <= %d)", V,
                    EHR_ROADMAP_MAX_NODES, E, A, H, EHR_ROADMAP_MAX_HOPS);
    if (source < 0 || source >= V) return fail(EHR_ERR_INVALID, "ehr_roadmap_paths: source %d outside 0..%d", source, V - 1);
    if (!adj_start || (A > 0 && (!adj_node || !adj_edge)) || (E > 0 && (!edge_status || !edge_length)) || !dist || !pred_node ||
        !pred_edge || !hops || !path || !path_edge || !changed)
        return fail(EHR_ERR_INVALID, "ehr_roadmap_paths: NULL tensor");
    roadmap_paths_kernel<<<1, ROADMAP_THREADS, 0, (hipStream_t)stream>>>(adj_start, adj_node, adj_edge, A, edge_status, edge_length,
                                                                         V, E, source, H, dist, pred_node, pred_edge, hops, path,
                                                                         path_edge, changed);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
