"""Reference of the exploration kernels (``ehr_information_gain`` / ``ehr_information_pick``, include/ehr.h) in numpy, with the
factorisations in ``np.longdouble``, the seeded matrix families of the tests and the DERIVED bar of a gain.  Not collected by
pytest; tests/test_explore_reference.py pins it on the CPU, tests/test_gpu_info_explorer.py compares the kernels with it.

What is exact and what is not.  ``H_q = scale * (info[q,0] + info[q,1] + ...)`` and ``X1 = A + H_q`` are float64 expressions
of the contract: the reference evaluates them in float64 in the same order, so both sides factor THE SAME matrices (and the
pick's ``A += H_q`` is compared bit for bit).  The scaling ``s_i = 1 / sqrt(A_ii)`` cancels in a gain exactly -- with
D = diag(s) AS COMPUTED, ``logdet(D X1 D) - logdet(D X0 D) = logdet X1 - logdet X0``, on the complement indices too -- so the
reference factors the scaled matrices with its own (longdouble) s and only the kernel's roundings AFTER the matrices are
formed remain.

The bar of one factorisation of an n x n scaled matrix Xs, u = 2^-53:

  * the two products ``(x_ij s_i) s_j``: an entrywise relative perturbation of at most 2u of D X D;
  * Cholesky's backward error (Higham, Accuracy and Stability, Thm 10.3): the computed factor is exact for Xs + dX with
    ``|dX| <= (n + 1) u |R^T||R|``, and ``(|R^T||R|)_ij <= sqrt(xs_ii xs_jj)`` (Cauchy-Schwarz on the rows of R);
  * to first order ``d logdet = trace(Xs^-1 dX)``, so both together move ``logdet Xs`` by at most
    ``(n + 3) u sum_ij |Xs^-1|_ij sqrt(xs_ii xs_jj)``;
  * ``ld = 2 sum_j log r_jj``: n logarithms of at most one ulp each (2u relative) and n - 1 additions in order, at most
    ``2 (n + 1) u sum_j |log r_jj|``.

A gain is ``(ld(X1) - ld(X1_bb)) - (ld(X0) - ld(X0_bb))``: the sum of the bars of its up to four factorisations, plus the three
subtractions' roundings, ``u (|ld| of the four + |m1| + |m0|)``.  The longdouble reference's own error (u_ld = 2^-64 in the same
formulas) is 2^-11 of this and is left out.  The bar is a first-order bound; it is evaluated with a float64 inverse of Xs,
which is accurate far beyond the bar's own two digits for every matrix of the families below (condition < 1e9).

``MEASURED``: the worst |gain - reference| / bar per GPU case, as printed by tests/test_gpu_info_explorer.py on an MI355X.  A
ratio above 1 is a finding to explain, not a reason to widen the bar."""
import types

import numpy as np

U = 2.0 ** -53
LD = np.longdouble

# worst |gain - reference| / bar per case of tests/test_gpu_info_explorer.py, from the MI355X run (see the module docstring)
MEASURED = {
    "gain N=1 S=1 all": 0.3414, "gain N=1 S=1 all scale=0.37": 0.3723, "gain N=1 S=3 all": 0.3585,
    "gain N=1 S=3 all scale=0.37": 0.4000,
    "gain N=6 S=1 all": 0.0288, "gain N=6 S=1 scattered": 0.0258, "gain N=6 S=1 all scale=0.37": 0.0250,
    "gain N=6 S=3 all": 0.0344, "gain N=6 S=3 scattered": 0.0228, "gain N=6 S=3 all scale=0.37": 0.0246,
    "gain N=13 S=1 all": 0.0107, "gain N=13 S=1 first6": 0.0108, "gain N=13 S=1 scattered": 0.0083,
    "gain N=13 S=1 all scale=0.37": 0.0101,
    "gain N=13 S=3 all": 0.0150, "gain N=13 S=3 first6": 0.0134, "gain N=13 S=3 scattered": 0.0087,
    "gain N=13 S=3 all scale=0.37": 0.0113,
    "gain N=32 S=1 all": 0.0011, "gain N=32 S=1 first6": 0.0009, "gain N=32 S=1 scattered": 0.0010,
    "gain N=32 S=1 all scale=0.37": 0.0011,
    "gain N=32 S=3 all": 0.0007, "gain N=32 S=3 first6": 0.0008, "gain N=32 S=3 scattered": 0.0006,
    "gain N=32 S=3 all scale=0.37": 0.0010,
    "explorer pose": 0.0280, "explorer joints": 0.0100,   # the gauge problem's real matrices (N = 6, N = 12)
}


def candidate_matrix(info_q, scale):
    """H_q of the contract, in float64 and in view order: scale * (info[q,0] + info[q,1] + ...)."""
    h = np.array(info_q[0], dtype=np.float64)
    for v in range(1, info_q.shape[0]):
        h = h + info_q[v]
    return np.float64(scale) * h


def _cholesky_ld(X):
    """Lower Cholesky factor of X in longdouble (column by column), or None on a pivot that is not positive and finite."""
    n = X.shape[0]
    Lf = np.zeros((n, n), dtype=LD)
    for j in range(n):
        piv = X[j, j] - Lf[j, :j] @ Lf[j, :j]
        if not (piv > 0 and np.isfinite(piv)):
            return None
        Lf[j, j] = np.sqrt(piv)
        if j + 1 < n:
            Lf[j + 1:, j] = (X[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return Lf


def logdet_scaled(X, s, idx):
    """(ld, bar) of the sub-matrix of X on ``idx``, scaled by ``s``: ld = 2 sum log r_jj of the longdouble factor; NaN where it
    does not factor.  An empty ``idx`` gives (0, 0)."""
    n = len(idx)
    if n == 0:
        return LD(0), 0.0
    Xs = (X[np.ix_(idx, idx)].astype(LD) * s[idx][:, None]) * s[idx][None, :]
    Lf = _cholesky_ld(Xs)
    if Lf is None:
        return LD(np.nan), np.nan
    lg = np.log(np.diag(Lf))
    ld = 2 * lg.sum()
    X64 = Xs.astype(np.float64)
    d = np.sqrt(np.diag(X64))
    inv = np.abs(np.linalg.inv(X64))
    bar = (n + 3) * U * float((inv * np.outer(d, d)).sum()) + 2 * (n + 1) * U * float(np.abs(lg).sum())
    return ld, bar


def _indices(interest, N):
    a = list(range(N)) if interest is None else sorted(int(i) for i in interest)
    return a, [k for k in range(N) if k not in a]


def interest_mask(interest, N):
    return sum(1 << i for i in _indices(interest, N)[0])


def gain(A, info, valid=None, taken=None, scale=1.0, interest=None):
    """-> (gain [Q] float64, bar [Q]) of the contract of ``ehr_information_gain``; info [Q,S,N,N]; ``interest``: parameter
    indices (None: all).  The bar of a candidate that is -inf or NaN is 0."""
    A, info = np.asarray(A, dtype=np.float64), np.asarray(info, dtype=np.float64)
    Q, N = info.shape[0], A.shape[0]
    out, bars = np.full(Q, np.nan), np.zeros(Q)
    d = np.diag(A)
    if not (np.isfinite(d) & (d > 0)).all():
        return out, bars
    s = 1 / np.sqrt(d.astype(LD))
    everything, rest = list(range(N)), _indices(interest, N)[1]
    f0, bf0 = logdet_scaled(A, s, everything)
    r0, br0 = logdet_scaled(A, s, rest)
    m0 = f0 - r0
    for q in range(Q):
        if (valid is not None and not valid[q]) or (taken is not None and taken[q]):
            out[q] = -np.inf
            continue
        H = candidate_matrix(info[q], scale)
        if not np.isfinite(H).all():
            continue
        X1 = A + H
        f1, bf1 = logdet_scaled(X1, s, everything)
        r1, br1 = logdet_scaled(X1, s, rest)
        m1 = f1 - r1
        out[q] = float(m1 - m0)
        if np.isfinite(out[q]):
            bars[q] = bf0 + br0 + bf1 + br1 + U * float(abs(f0) + abs(r0) + abs(f1) + abs(r1) + abs(m1) + abs(m0))
    return out, bars


def pick(g, info, A, taken, scale=1.0):
    """The contract of ``ehr_information_pick`` on copies: -> (q* or -1, gain or NaN, A, taken)."""
    g = np.asarray(g, dtype=np.float64)
    A, taken = np.array(A, dtype=np.float64), np.array(taken, dtype=np.int32)
    fin = np.isfinite(g)
    if not fin.any():
        return -1, np.nan, A, taken
    q = int(np.flatnonzero(fin & (g == g[fin].max()))[0])
    taken[q] = 1
    return q, float(g[q]), A + candidate_matrix(info[q], scale), taken


def greedy(A, info, k, valid=None, scale=1.0, interest=None):
    """k rounds of gain + pick -> namespace: picked [k], gains [k], bars [k] (the picked gain's), margin [k] (best minus
    second-best gain of the round; inf where there is no second), second_bar [k], A_final, taken, A_rounds (A before each
    round)."""
    A = np.array(A, dtype=np.float64)
    taken = np.zeros(info.shape[0], dtype=np.int32)
    out = types.SimpleNamespace(picked=[], gains=[], bars=[], margin=[], second_bar=[], A_rounds=[])
    for _ in range(k):
        out.A_rounds.append(A.copy())
        g, bars = gain(A, info, valid, taken, scale, interest)
        q, gq, A, taken = pick(g, info, A, taken, scale)
        out.picked.append(q)
        out.gains.append(gq)
        out.bars.append(bars[q] if q >= 0 else 0.0)
        rest = np.flatnonzero(np.isfinite(g) & (np.arange(len(g)) != q))
        if q >= 0 and len(rest):
            j = rest[np.argmax(g[rest])]
            out.margin.append(gq - g[j])
            out.second_bar.append(bars[j])
        else:
            out.margin.append(np.inf)
            out.second_bar.append(0.0)
    out.picked, out.gains = np.array(out.picked, dtype=np.int32), np.array(out.gains)
    out.bars, out.margin, out.second_bar = np.array(out.bars), np.array(out.margin), np.array(out.second_bar)
    out.A_final, out.taken = A, taken
    return out


# ---- the seeded matrix families ------------------------------------------------------------------------------------------
Q_CASE = 67
RANKS = (0, 1, 3, None)  # None: N
DUPLICATES = ((Q_CASE - 1, 1), (Q_CASE - 2, 2))  # (copy, original): exact duplicates, of a rank-1 and a rank-3 candidate
SEEDS = {1: 101, 6: 106, 13: 113, 32: 132}       # one seed per N (chosen in tests/test_explore_reference.py: the pick margins)
SIZES = (1, 6, 13, 32)
VIEWS = (1, 3)


def _sym(M):
    """M with its upper triangle replaced by the lower one: exactly symmetric."""
    return np.tril(M) + np.tril(M, -1).T


def family(N, S, Q=Q_CASE, seed=None):
    """(A [N,N], info [Q,S,N,N]), float64, exactly symmetric.  A = G G^T + prior with the parameters' units spread over
    10^U(-2,2) (metres against radians against log-focal-lengths); candidate q is a sum of S PSD matrices of rank
    RANKS[q % 4] (0: all zeros) in the same units, of an amplitude 10^U(-1, 0.5) of its own; DUPLICATES are exact copies."""
    rng = np.random.default_rng(SEEDS[N] if seed is None else seed)
    d = 10.0 ** rng.uniform(-2, 2, size=N)
    G = rng.normal(size=(N, N + 3)) * d[:, None]
    A = _sym(G @ G.T + np.diag(0.01 * d * d))
    info = np.zeros((Q, S, N, N))
    originals = [orig for _, orig in DUPLICATES]
    for q in range(Q):
        r = RANKS[q % 4]
        r = N if r is None else min(r, N)
        amp = 10.0 ** rng.uniform(-1, 0.5)
        if q in originals:  # weak, so that a duplicated pair never leads a greedy round (a tie there decides nothing)
            amp = 0.03
        for v in range(S):
            V = rng.normal(size=(N, r)) * d[:, None] * amp
            info[q, v] = _sym(V @ V.T)
    for copy, orig in DUPLICATES:
        info[copy] = info[orig]
    return A, info


def interests(N):
    """The interest sets of the kernel cases: all, the first 6 (N > 6) and a scattered set."""
    out = {"all": None}
    if N > 6:
        out["first6"] = list(range(6))
    if N > 1:
        out["scattered"] = [k for k in range(N) if k % 3 == 1 or k == N - 1]
    return out


_CACHE = {}


def expected_gain(N, S, which, scale=1.0):
    """(A, info, interest, gain, bar) of a family and an interest set; computed once per process, never written to."""
    key = ("gain", N, S, which, scale)
    if key not in _CACHE:
        A, info = family(N, S)
        interest = interests(N)[which]
        g, bars = gain(A, info, scale=scale, interest=interest)
        _CACHE[key] = (A, info, interest, g, bars)
    return _CACHE[key]


def expected_greedy(N, S, which, k=5, scale=1.0):
    key = ("greedy", N, S, which, k, scale)
    if key not in _CACHE:
        A, info = family(N, S)
        interest = interests(N)[which]
        _CACHE[key] = (A, info, interest, greedy(A, info, k, scale=scale, interest=interest))
    return _CACHE[key]


PICK_CASES = [(6, 1, "all"), (13, 3, "first6"), (32, 1, "scattered"), (13, 1, "all")]  # the families the GPU pick tests use
