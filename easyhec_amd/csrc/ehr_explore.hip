// ehr_explore.hip -- information-gain exploration (easyhec_amd/info_explorer.py): which candidate joint
// configuration raises the log-determinant of what the frames already pin the most.
//
//   information_gain_kernel : A [N,N] (prior + frames so far), info [Q,S,N,N] (ehr_mask_information's matrices of the candidates'
//                             views) -> gain [Q].  One wave per candidate, four candidates per 256-thread workgroup; each wave
//                             factors up to four scaled matrices (X0 = A and X1 = A + H_q, whole and on the nuisance indices) by
//                             Cholesky in its own padded [32][33] float64 tile of LDS.
//   information_pick_kernel : the best finite gain (lowest index on a tie) -> picked / picked_gain / taken, and A += H_q*.  One
//                             workgroup.
//
// k greedy rounds are 2k stream-ordered launches without a host round trip.  No kernel here allocates, synchronises or uses an
// atomic; every sum has a fixed order, and a candidate's gain depends on A and its own matrices alone: bit-reproducible, and the
// same bits whatever the batch around it.  Plain C++ throughout (the library is built with -ffp-contract=off: a + scale * h is
// a product rounded, then a sum rounded, as numpy evaluates it).
#include "ehr_host.h"

#define IG_N EHR_IG_MAX_PARAMS
#define IG_WAVES 4  // candidates per workgroup

namespace ehr {

__device__ __forceinline__ bool ig_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ double ig_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// H_q[r][c] = scale * (info[0] + info[1] + ...), in view order
__device__ __forceinline__ double ig_candidate_entry(const double* __restrict__ info, int S, int NN, int e, double scale) {
    double h = info[e];
    for (int v = 1; v < S; v++) h += info[(size_t)v * NN + e];
    return scale * h;
}

// ld of the n x n sub-matrix of X = A (+ H_q where `info` is given) on the indices idx[0..n): the matrix is scaled as
// (x_ij s_i) s_j, factored by Cholesky (right-looking, the lower triangle in place in the wave's tile W) and
// ld = 2 sum_j log r_jj, summed in the order of j.  NaN on a pivot that is not positive and finite.  Every thread of the
// WORKGROUP calls this with the same n (the barriers are the workgroup's); the value is uniform over the wave.  n == 0: 0.
__device__ double ig_logdet(double (*W)[IG_N + 1], double* lg, int* failed, const double* __restrict__ A,
                            const double* __restrict__ info, int S, int N, double scale, const double* sv, const int* idx, int n,
                            int lane) {
    const int NN = N * N;
    for (int e = lane; e < n * n; e += 64) {
        const int i = e / n, j = e - i * n, r = idx[i], c = idx[j];
        double x = A[r * N + c];
        if (info) x = x + ig_candidate_entry(info, S, NN, r * N + c, scale);
        W[i][j] = (x * sv[r]) * sv[c];
    }
    if (lane == 0) *failed = 0;
    __syncthreads();
    for (int j = 0; j < n; j++) {
        if (lane == 0) {
            double piv = W[j][j];
            if (!(piv > 0.0) || !ig_finite(piv)) {
                *failed = 1;
                piv = 1.0;
            }
            W[j][j] = sqrt(piv);
        }
        __syncthreads();
        if (lane > j && lane < n) W[lane][j] = W[lane][j] / W[j][j];
        __syncthreads();
        if (lane > j && lane < n)
            for (int k = j + 1; k <= lane; k++) W[lane][k] -= W[lane][j] * W[k][j];
        __syncthreads();
    }
    if (lane < n) lg[lane] = log(W[lane][lane]);
    __syncthreads();
    double s = 0.0;
    for (int j = 0; j < n; j++) s += lg[j];
    const int bad = *failed;
    __syncthreads();  // (the tile, lg and the flag are free for the next call)
    return bad ? ig_nan() : 2.0 * s;
}

__global__ void __launch_bounds__(64 * IG_WAVES) information_gain_kernel(const double* __restrict__ A,
                                                                        const double* __restrict__ info,
                                                                        const int* __restrict__ valid,
                                                                        const int* __restrict__ taken, int Q, int S, int N,
                                                                        double scale, unsigned interest, double* __restrict__ gain) {
    __shared__ double W[IG_WAVES][IG_N][IG_N + 1];
    __shared__ double lg[IG_WAVES][IG_N];
    __shared__ double sv[IG_N];
    __shared__ int idx_all[IG_N], idx_rest[IG_N];
    __shared__ int failed[IG_WAVES];
    __shared__ int a_bad;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned all = N >= 32 ? 0xffffffffu : ((1u << N) - 1u);
    const unsigned rest = all & ~interest;  // the nuisance parameters, marginalised
    const int n_rest = __popc(rest);
    if (tid == 0) a_bad = 0;
    __syncthreads();
    if (tid < N) {
        const double d = A[tid * N + tid];
        const bool ok = d > 0.0 && ig_finite(d);
        sv[tid] = ok ? 1.0 / sqrt(d) : 0.0;
        if (!ok) a_bad = 1;  // (every writer stores the same value)
        idx_all[tid] = tid;
        if ((rest >> tid) & 1u) idx_rest[__popc(rest & ((1u << tid) - 1u))] = tid;
    }
    __syncthreads();
    const int q = blockIdx.x * IG_WAVES + wave;
    const bool live = q < Q;
    const bool open = live && (!valid || valid[q] != 0) && (!taken || taken[q] == 0);
    // a closed candidate's matrices are not read: it goes through the same barriers on A alone
    const double* Hq = open ? info + (size_t)q * S * N * N : nullptr;
    int bad = 0;
    if (Hq)
        for (int e = lane; e < N * N; e += 64) bad |= !ig_finite(ig_candidate_entry(Hq, S, N * N, e, scale));
    bad = __any(bad);
    double m0 = ig_logdet(W[wave], lg[wave], &failed[wave], A, nullptr, S, N, scale, sv, idx_all, N, lane);
    double m1 = ig_logdet(W[wave], lg[wave], &failed[wave], A, Hq, S, N, scale, sv, idx_all, N, lane);
    if (n_rest > 0) {
        m0 = m0 - ig_logdet(W[wave], lg[wave], &failed[wave], A, nullptr, S, N, scale, sv, idx_rest, n_rest, lane);
        m1 = m1 - ig_logdet(W[wave], lg[wave], &failed[wave], A, Hq, S, N, scale, sv, idx_rest, n_rest, lane);
    }
    if (live && lane == 0) {
        double g = m1 - m0;
        if (bad) g = ig_nan();
        if (!open) g = -__longlong_as_double(0x7ff0000000000000ll);
        if (a_bad) g = ig_nan();
        gain[q] = g;
    }
}

__global__ void __launch_bounds__(256) information_pick_kernel(const double* __restrict__ gain, const double* __restrict__ info,
                                                               int Q, int S, int N, double scale, int round,
                                                               double* __restrict__ A, int* __restrict__ taken,
                                                               int* __restrict__ picked, double* __restrict__ picked_gain) {
    __shared__ double bg[256];
    __shared__ int bq[256];
    const int tid = threadIdx.x;
    double g = 0.0;
    int best = -1;
    for (int q = tid; q < Q; q += 256) {  // (ascending q: a later equal gain does not replace an earlier one)
        const double x = gain[q];
        if (ig_finite(x) && (best < 0 || x > g)) {
            g = x;
            best = q;
        }
    }
    bg[tid] = g;
    bq[tid] = best;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            const int o = bq[tid + w];
            const double x = bg[tid + w];
            if (o >= 0 && (bq[tid] < 0 || x > bg[tid] || (x == bg[tid] && o < bq[tid]))) {
                bg[tid] = x;
                bq[tid] = o;
            }
        }
        __syncthreads();
    }
    const int qs = bq[0];
    if (qs < 0) {
        if (tid == 0) {
            picked[round] = -1;
            picked_gain[round] = ig_nan();
        }
        return;
    }
    if (tid == 0) {
        picked[round] = qs;
        picked_gain[round] = bg[0];
        taken[qs] = 1;
    }
    const double* Hq = info + (size_t)qs * S * N * N;
    for (int e = tid; e < N * N; e += 256) A[e] = A[e] + ig_candidate_entry(Hq, S, N * N, e, scale);
}

}  // namespace ehr

using namespace ehr;

extern "C" {

int ehr_information_gain(const double* A, const double* info, const int32_t* valid, const int32_t* taken, int Q, int S, int N,
                         double scale, uint32_t interest_mask, double* gain, void* stream) {
    if (!A || !info || !gain) return fail(EHR_ERR_INVALID, "ehr_information_gain: NULL tensor");
    if (N < 1 || N > EHR_IG_MAX_PARAMS || Q < 1 || S < 1 || (long long)Q + IG_WAVES > 0x7fffffffll)
        return fail(EHR_ERR_INVALID, "ehr_information_gain: bad sizes (Q %d, S %d, N %d: 1 <= N <= %d)", Q, S, N, EHR_IG_MAX_PARAMS);
    information_gain_kernel<<<(unsigned)((Q + IG_WAVES - 1) / IG_WAVES), 64 * IG_WAVES, 0, (hipStream_t)stream>>>(
        A, info, valid, taken, Q, S, N, scale, interest_mask, gain);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

int ehr_information_pick(const double* gain, const double* info, int Q, int S, int N, double scale, int round, double* A,
                         int32_t* taken, int32_t* picked, double* picked_gain, void* stream) {
    if (!gain || !info || !A || !taken || !picked || !picked_gain) return fail(EHR_ERR_INVALID, "ehr_information_pick: NULL tensor");
    if (N < 1 || N > EHR_IG_MAX_PARAMS || Q < 1 || S < 1 || round < 0)
        return fail(EHR_ERR_INVALID, "ehr_information_pick: bad sizes (Q %d, S %d, N %d: 1 <= N <= %d; round %d)", Q, S, N,
                    EHR_IG_MAX_PARAMS, round);
    information_pick_kernel<<<1, 256, 0, (hipStream_t)stream>>>(gain, info, Q, S, N, scale, round, A, taken, picked, picked_gain);
    EHR_LAUNCH_CHECK();
    return EHR_OK;
}

}  // extern "C"
