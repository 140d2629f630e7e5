// ehr_segment_body.h -- the search of ehr_segment_clearance: the STATEMENTS of a kernel's body, included inside the kernels of
// ehr_segment_clearance.hip (not a header of declarations; ehr_segment_core.h has those).
//
// Why text and not a __device__ function: the search reads ~40 fields of the kernel's by-value argument block, many of them
// pointers.  Read in the kernel itself, the compiler knows them for kernel arguments: the pointers are promoted to global
// memory and the fields are loaded where they are used.  Behind a function boundary that is lost -- through a reference the
// kernel's 42 global loads and 18 global stores become flat ones (measured: check_swept +0.5 ms in 27.2), by value every field
// is loaded on entry and 26 more SGPRs spill (167 against 141) -- and even a kernel template over the argument type moves the
// register allocator's choices.  Included as text, segment_clearance_kernel compiles to the machine code it had before the
// search was shared, instruction for instruction.
//
// The including kernel provides, before the #include:
//   A          const SegArgs (or a reference to one inside the kernel's own argument): the argument block
//   SEG_Q0(j)  entry j of this workgroup's start configuration, SEG_Q1(j) of its end configuration (uniform over the workgroup)
// and must be launched with SEG_THREADS threads and seg_lds_bytes of dynamic LDS.  Outputs and the trace row go to index
// blockIdx.x.  Every name the text declares (smem, S, L, J, tid, b, status, ...) lands in the scope that includes it.
//
// One workgroup of 256 threads per segment.  Depth-first bisection over the dyadic intervals of [0,1]; per interval ONE
// evaluation at its centre: the kinematics (joint_forward_view, the bits of ehr_joint_forward), the proxies to the base frame
// in LDS (feas_to_base, the bits of ehr_config_clearance), then every clearance twice, side by side: raw, and lowered by how far
// the spheres involved can travel within the interval's half-width (rates from each sphere's distance to each joint axis AT
// the centre, second order from the chain lengths).  Thread 0 decides (hit / certified / split / out of budget) and the
// decision is broadcast through LDS.
//
// The search needs no stack of its own: the pending intervals of a left-to-right depth-first walk are the right siblings of the
// current interval's ancestors, so (depth, index) of the current interval is the whole state -- see seg_next.
// Float64 throughout, built with -ffp-contract=off; every condition around a barrier is uniform over the workgroup; the loop runs
// at most max_evals times.  No atomics, no allocation, no synchronisation with the host.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = A.S, Sp = A.Sp, L = A.L, J = A.J, Np = A.Np, No = A.No;
    double* X = (double*)smem;
    double* Y = X + Sp;
    double* Z = Y + Sp;
    double* Rr = Z + Sp;
    double* E = Rr + Sp;                        // the spheres' inflation under the current pair's masks
    double* BW = E + Sp;                        // [L][4] bounding spheres, base frame
    double* red = BW + EHR_FEAS_MAX_LINKS * 4;  // [4 waves][6]
    double* G = red + 24;                       // [J][32]
    double* dabs = G + 32 * 32;                 // |d_j|
    double* dd = dabs + 32;                     // d_j
    double* qa = dd + 32;                       // q0_j
    double* qc = qa + 32;                       // q(c)_j
    float* LP = (float*)(qc + 32);              // [L][16]
    float* JF = LP + EHR_FEAS_MAX_LINKS * 16;   // [J][6]
    int* redp = (int*)(JF + EHR_JOINT_MAX_JOINTS * 6);
    int* off = redp + 4;                        // [L + 1]
    int* jkind = off + 36;                      // the kind of the link each active joint moves
    int* ups = jkind + 32;                      // upstream [L]
    int* jbel = ups + 32;                       // joint_below [J]
    int* dec = jbel + 32;                       // thread 0's decision
    unsigned char* skip = (unsigned char*)(dec + 8);  // [No]: the current link's bound clears this obstacle
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const size_t b = blockIdx.x;
    const double cutoff = A.cutoff, margin = A.margin, cull = cutoff + FEAS_CULL_SLACK;
    const double* __restrict__ W = A.reach_radius;
    const double* __restrict__ planes = A.planes;
    const double* __restrict__ obstacles = A.obstacles;

    // the candidate's tables
    int bad = 0;
    if (tid <= L) off[tid] = A.offs.v[tid];
    if (tid < L) ups[tid] = (int)A.upstream[tid];
    if (tid < 32) jkind[tid] = 0;
    if (tid < J) {
        const double a = SEG_Q0(tid), c = SEG_Q1(tid);
        bad = !seg_finite(a) || !seg_finite(c);
        qa[tid] = a;
        dd[tid] = c - a;
        dabs[tid] = fabs(c - a);
        jbel[tid] = (int)A.joint_below[tid];
    }
    __syncthreads();
    if (tid < A.N) {
        const int c = A.qidx[tid];
        if (c >= 0 && c < J) jkind[c] = A.kind[tid];
    }
    bad = __syncthreads_or(bad);

    // thread 0's record of the search
    int status = bad ? 3 : -1, ev = 0, k = A.min_depth, stop_pair = -1;
    unsigned i = 0;
    double t_free = 0.0, cmin_s = cutoff, cmin_e = cutoff, cmin_r = cutoff;
    double stop_s = feas_nan(), stop_e = feas_nan(), stop_r = feas_nan();

    if (!bad) {
        // G[j,l] = sum_{k in up(l), k below j} |d_k| W[k,l], k ascending
        for (int e = tid; e < J * L; e += SEG_THREADS) {
            const int j = e / L, l = e - j * L;
            G[j * 32 + l] = seg_sum((unsigned)ups[l] & (unsigned)jbel[j], J, dabs, W, L, l);
        }
        __syncthreads();
    }

    while (status < 0) {
        const double h = seg_pow2(-(k + 1));  // the half-width; the interval is [a, a + 2 h]
        const double a = (double)(2u * i) * h, c = (double)(2u * i + 1u) * h;
        t_free = a;
        if (ev >= A.max_evals) {  // out of budget between two intervals: no evaluation stopped the search
            status = 2;
            break;
        }
        if (tid < J) qc[tid] = qa[tid] + c * dd[tid];
        __syncthreads();
        joint_forward_view<SEG_THREADS>(A.parent, A.origin, A.kind, A.axis, A.qidx, A.use, A.N, J, L, qc, A.offset, LP, JF);
        __syncthreads();
        bad = 0;
        for (int e = tid; e < L * 16; e += SEG_THREADS) bad |= !feas_finite(LP[e]);
        bad = __syncthreads_or(bad);
        if (bad) {  // a pose that cannot be judged
            if (tid == 0 && A.trace_t) {
                A.trace_t[b * (size_t)A.max_evals + ev] = c;
                for (int q = 0; q < 6; q++) A.trace_val[(b * (size_t)A.max_evals + ev) * 6 + q] = feas_nan();
            }
            ev++;
            status = 3;
            break;
        }
        feas_to_base<SEG_THREADS>(LP, A.spheres, off, A.link_bounds, L, S, X, Y, Z, Rr, BW);
        __syncthreads();

        // v: raw self, env, reach | certified self, env, reach of this thread
        double v[6] = {cutoff, cutoff, cutoff, cutoff, cutoff, cutoff};
        int sp = -1;

        // reach and the environment, per link, the inflation under up(l)
        for (int l = 0; l < L; l++) {
            const int s0 = off[l], s1 = off[l + 1];
            if (s0 == s1) continue;
            const bool env = (Np > 0 || No > 0) && ((A.env_links >> l) & 1u);
            if (!env && !A.reach) continue;
            const unsigned M = (unsigned)ups[l];
            const double C = seg_sum(M, J, dabs, G, 32, l);
            const double far = cutoff - seg_inflate(h, seg_sum(M, J, dabs, W, L, l), C);  // stands for what lies beyond cutoff
            if (A.reach && far < v[5]) v[5] = far;
            unsigned pmask = 0;  // the planes the link's bound does not clear
            if (env) {
                if (far < v[4]) v[4] = far;
                const double bx = BW[4 * l], by = BW[4 * l + 1], bz = BW[4 * l + 2], bR = BW[4 * l + 3];
                for (int p = 0; p < Np; p++)
                    if (!(feas_plane(planes[4 * p], planes[4 * p + 1], planes[4 * p + 2], planes[4 * p + 3], bx, by, bz, bR) > cull))
                        pmask |= 1u << p;
                if (No > 0) {
                    __syncthreads();  // (the previous link's flags have been read)
                    for (int o = tid; o < No; o += SEG_THREADS)
                        skip[o] = feas_gap(bx - obstacles[4 * o], by - obstacles[4 * o + 1], bz - obstacles[4 * o + 2], bR,
                                           obstacles[4 * o + 3]) > cull;
                    __syncthreads();
                }
            }
            for (int s = s0 + tid; s < s1; s += SEG_THREADS) {
                const double cx = X[s], cy = Y[s], cz = Z[s], r = Rr[s];
                const double e = seg_inflate(h, seg_rate(M, J, jkind, JF, dabs, cx, cy, cz, r), C);
                if (A.reach) {
                    const double d = feas_reach(A.reach[3], cx - A.reach[0], cy - A.reach[1], cz - A.reach[2], r);
                    if (d < v[2]) v[2] = d;
                    if (d < cutoff && d - e < v[5]) v[5] = d - e;
                }
                if (!env) continue;
                for (int p = 0; p < Np; p++) {
                    if (!((pmask >> p) & 1u)) continue;
                    const double d = feas_plane(planes[4 * p], planes[4 * p + 1], planes[4 * p + 2], planes[4 * p + 3], cx, cy, cz, r);
                    if (d < v[1]) v[1] = d;
                    if (d < cutoff && d - e < v[4]) v[4] = d - e;
                }
                for (int o = 0; o < No; o++) {
                    if (skip[o]) continue;
                    const double d = feas_gap(cx - obstacles[4 * o], cy - obstacles[4 * o + 1], cz - obstacles[4 * o + 2], r,
                                              obstacles[4 * o + 3]);
                    if (d < v[1]) v[1] = d;
                    if (d < cutoff && d - e < v[4]) v[4] = d - e;
                }
            }
        }

        // the arm against itself: link pairs in the order of their code 32 i + j, as config_clearance_kernel walks them
        const unsigned inL = L >= 32 ? 0xffffffffu : ((1u << L) - 1u);
        for (int li = 0; li + 1 < L; li++) {
            const unsigned m = A.pair_enable[li] & ~((2u << li) - 1u) & inL;  // j > i only
            const int oi = off[li], ni = off[li + 1] - oi;
            if (!m || ni <= 0) continue;
            for (int lj = li + 1; lj < L; lj++) {
                const int oj = off[lj], nj = off[lj + 1] - oj;
                if (!((m >> lj) & 1u) || nj <= 0) continue;
                // joints upstream of both links move them rigidly together
                const unsigned Mi = (unsigned)ups[li] & ~(unsigned)ups[lj], Mj = (unsigned)ups[lj] & ~(unsigned)ups[li];
                const double Ci = seg_sum(Mi, J, dabs, G, 32, li), Cj = seg_sum(Mj, J, dabs, G, 32, lj);
                // the pair's far value: every sphere pair at or beyond cutoff, a culled link pair's included, stays above it
                const double far = cutoff - (seg_inflate(h, seg_sum(Mi, J, dabs, W, L, li), Ci) +
                                             seg_inflate(h, seg_sum(Mj, J, dabs, W, L, lj), Cj));
                if (far < v[3]) v[3] = far;
                if (feas_bound_gap(BW, li, lj) > cull) continue;
                __syncthreads();  // (the previous pair's E has been read)
                for (int s = oi + tid; s < oi + ni; s += SEG_THREADS)
                    E[s] = seg_inflate(h, seg_rate(Mi, J, jkind, JF, dabs, X[s], Y[s], Z[s], Rr[s]), Ci);
                for (int s = oj + tid; s < oj + nj; s += SEG_THREADS)
                    E[s] = seg_inflate(h, seg_rate(Mj, J, jkind, JF, dabs, X[s], Y[s], Z[s], Rr[s]), Cj);
                __syncthreads();
                const int code = 32 * li + lj;
                const bool swap = nj < ni;
                const int a0 = swap ? oj : oi, na = swap ? nj : ni, b0 = swap ? oi : oj, nb = swap ? ni : nj;
                for (int sa = wave; sa < na; sa += SEG_THREADS / 64) {
                    const double ax = X[a0 + sa], ay = Y[a0 + sa], az = Z[a0 + sa], ar = Rr[a0 + sa], ae = E[a0 + sa];
                    for (int sb = b0 + lane; sb < b0 + nb; sb += 64) {
                        const double dx = ax - X[sb], dy = ay - Y[sb], dz = az - Z[sb], rs = ar + Rr[sb];
                        // no square root for a pair beyond cutoff: with t = cutoff + rs > 0, d2 > t^2 (1 + 1e-12) puts the
                        // rounded root above t (1 + 4e-13), that is above cutoff + rs by far more than t's own rounding, and
                        // rounding is monotonic: the gap comes out >= cutoff.  Such a gap replaces no raw minimum (they start
                        // at cutoff) and does not pass the certified value's gate; the pair's far value stands for it.
                        const double t = cutoff + rs, d2 = feas_norm2(dx, dy, dz);
                        if (d2 > (t * t) * 1.000000000001) continue;
                        const double d = sqrt(d2) - rs;  // == feas_gap(dx, dy, dz, ar, Rr[sb])
                        if (d < v[0]) {
                            v[0] = d;
                            sp = code;
                        }
                        if (d < cutoff) {
                            const double ci = d - (ae + E[sb]);
                            if (ci < v[3]) v[3] = ci;
                        }
                    }
                }
            }
        }

        // minima over the workgroup; among equal raw self clearances the lowest pair code
        SEG_MIN_STEP(32) SEG_MIN_STEP(16) SEG_MIN_STEP(8) SEG_MIN_STEP(4) SEG_MIN_STEP(2) SEG_MIN_STEP(1)
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 6; q++) red[6 * wave + q] = v[q];
            redp[wave] = sp;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < SEG_THREADS / 64; w++) {
                const double o = red[6 * w];
                const int op = redp[w];
                if (o < v[0] || (o == v[0] && op < sp && op >= 0)) {
                    v[0] = o;
                    sp = op;
                }
#pragma unroll
                for (int q = 1; q < 6; q++)
                    if (red[6 * w + q] < v[q]) v[q] = red[6 * w + q];
            }
            v[3] -= FEAS_CULL_SLACK;  // the float32 rounding of poses and axes
            v[4] -= FEAS_CULL_SLACK;
            v[5] -= FEAS_CULL_SLACK;
            if (A.trace_t) {
                A.trace_t[b * (size_t)A.max_evals + ev] = c;
#pragma unroll
                for (int q = 0; q < 6; q++) A.trace_val[(b * (size_t)A.max_evals + ev) * 6 + q] = v[q];
            }
            int act;
            if (!(v[0] > margin) || !(v[1] > margin) || !(v[2] >= 0.0)) {
                act = 1;  // hit
            } else if (v[3] > margin && v[4] > margin && v[5] >= 0.0) {
                act = 0;  // the whole interval is certified
                if (v[3] < cmin_s) cmin_s = v[3];
                if (v[4] < cmin_e) cmin_e = v[4];
                if (v[5] < cmin_r) cmin_r = v[5];
            } else if (k < A.max_depth && ev + 1 < A.max_evals) {
                act = 4;  // split, the left half first
            } else {
                act = 2;  // undecided
            }
            if (act == 1 || act == 2) {
                stop_s = v[0];
                stop_e = v[1];
                stop_r = v[2];
                stop_pair = sp;
            }
            dec[0] = act;
        }
        __syncthreads();  // (also: everybody has left the evaluation's LDS before the next one writes it)
        const int act = dec[0];
        ev++;
        if (act == 0) {
            if (!seg_next(A.min_depth, k, i)) {
                status = 0;
                t_free = 1.0;
            }
        } else if (act == 4) {
            k++;
            i *= 2u;
        } else {
            status = act;
        }
    }

    if (tid == 0) {
        A.status[b] = status;
        A.t_free[b] = t_free;
        A.evals[b] = ev;
        A.cert_self[b] = cmin_s;
        A.cert_env[b] = cmin_e;
        A.cert_reach[b] = cmin_r;
        A.stop_self[b] = stop_s;
        A.stop_env[b] = stop_e;
        A.stop_reach[b] = stop_r;
        A.stop_pair[b] = stop_pair;
    }
