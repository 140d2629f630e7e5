"""tests/lm_prior_reference.py pinned on the CPU: without a prior and with all-zero weights it is tests/lm_reference.py's update
(and tests/lm_rig_reference.py's) field for field; the system it solves is the views' sums plus ONE extra "view" carrying the
prior; the prior's term, the reported calls and the prior-only parameter; and the CPU Levenberg-Marquardt loop on the gauge
problem with ``offset[0]`` free under a prior on it (the total objective is monotone; the trajectory is the one recorded in
``lm_prior_reference.MEASURED``)."""
import copy

import numpy as np
import pytest

import information_reference as IR
import lm_prior_reference as PR
import lm_reference as LR
import lm_rig_reference as RR
from test_lm_reference import toy

FIELDS = ("lam", "nu", "F_acc", "pred", "rho", "F_trial", "iterations", "accepted", "rejected", "reported", "done", "why", "last",
          "count", "retries")


def system(N, B, seed):
    """tests/test_gpu_lm.py's synthetic system (that module needs a GPU to import): SPD matrices, parameters of different
    units, grad = 2 H x for a small x."""
    rng = np.random.default_rng(77 * N + seed)
    scale = 10.0 ** rng.uniform(-2, 2, N)
    info = np.zeros((B, N, N))
    for b in range(B):
        Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
        M = (Q * 10.0 ** rng.uniform(-5, 0, N)) @ Q.T
        info[b] = 0.5 * (M + M.T) * scale[:, None] * scale[None, :]
    x = rng.normal(size=N) * 1e-3 / scale
    grad = np.stack([2.0 * info[b] @ x for b in range(B)])
    return info, grad, rng.integers(10, 500, B), rng.uniform(10, 100, B).astype(np.float32)


def same_state(a, b, what):
    for k in FIELDS:
        assert getattr(a, k) == getattr(b, k), (what, k, getattr(a, k), getattr(b, k))
    for k in ("theta", "delta", "g", "H"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (what, k)


def script(N, B=3):
    """first call, accept, reject, reject, reported, accept: (info, grad, count, loss) per call."""
    i0, g0, c0, l0 = system(N, B, 0)
    i1, g1, c1, _ = system(N, B, 1)
    i2, g2, c2, _ = system(N, B, 2)
    lo = (l0 * np.float32(0.9)).astype(np.float32)
    nan = lo.copy()
    nan[1] = np.nan
    return [(i0, g0, c0, l0), (i1, g1, c1, lo), (i2, g2, c2, lo * np.float32(1.5)), (i2, g2, c2, lo * np.float32(2.0)),
            (i0, g0, c0, nan), (i2, g2, c2, lo * np.float32(0.8))]


@pytest.mark.parametrize("N", [1, 6, 7, 10, 32])
def test_zero_weights_and_no_prior_are_lm_reference(N):
    rng = np.random.default_rng(N)
    theta = rng.uniform(-1, 1, N).astype(np.float32)
    a, b, c = LR.new_state(), PR.new_state(), PR.new_state()
    ta = tb = tc = theta
    for k, (info, grad, count, loss) in enumerate(script(N)):
        ta = LR.update(a, info, grad, count, loss, ta, 1e-12)
        tb = PR.update(b, info, grad, count, loss, tb, None, None, 1e-12)
        tc = PR.update(c, info, grad, count, loss, tc, np.zeros(N), rng.normal(size=N), 1e-12)
        same_state(a, b, f"N={N} call {k}: no prior")
        same_state(a, c, f"N={N} call {k}: zero weights")
        assert ta.tobytes() == tb.tobytes() == tc.tobytes() and c.F_prior == 0.0
    assert (a.accepted, a.rejected, a.reported) == (3, 2, 1)
    fa, fc = LR.update(a, info, grad, count, loss, ta, finalize=True), PR.update(c, info, grad, count, loss, tc, np.zeros(N), np.zeros(N), finalize=True)
    assert fa.tobytes() == fc.tobytes()


def test_zero_weights_are_lm_rig_reference():
    C, F, Bs = 2, 2, [2, 3]
    N = 6 * C + F
    theta = np.random.default_rng(3).uniform(-1, 1, N).astype(np.float32)
    a, c = LR.new_state(), PR.new_state()
    ta = tc = theta
    for what, cams in RR.scripted_calls(C, F, Bs):
        fin = what == "finalize"
        ta = RR.update_rig(a, cams, ta, RR.FTOL, 1e6, fin)
        tc = PR.update_rig(c, cams, tc, np.zeros(N), np.ones(N), RR.FTOL, 1e6, fin)
        same_state(a, c, what)
        assert ta.tobytes() == tc.tobytes()


@pytest.mark.parametrize("N", [6, 10])
def test_the_solved_system_is_the_views_plus_one_prior_view(N):
    """H and g of the solved system: lm_reference's sums over the views continued by ONE more "view" that carries diag(p) and
    2 p (theta_acc - mu) -- on the accepting call and on a rejected one (from the stored linearisation)."""
    rng = np.random.default_rng(10 + N)
    theta = rng.uniform(-1, 1, N).astype(np.float32)
    w = np.where(rng.uniform(size=N) < 0.5, 10.0 ** rng.uniform(-2, 3, N), 0.0)
    w[0], w[N - 1] = 0.0, 7.0
    mu = rng.normal(size=N)
    calls = script(N)
    st, ref = PR.new_state(), LR.new_state()
    t1 = PR.update(st, *calls[0], theta, w, mu, 1e-12)
    LR.update(ref, *calls[0], theta, 1e-12)                      # the data's sums, in view order
    Hv, gv = PR.prior_view(theta.astype(np.float64), w, mu)
    assert np.array_equal(st.H, ref.H) and np.array_equal(st.g, ref.g)
    assert np.array_equal(st.Hp, ref.H + Hv) and np.array_equal(st.gp, ref.g + gv)
    assert np.array_equal(np.diag(st.Hp)[w == 0], np.diag(ref.H)[w == 0]) and np.array_equal(st.gp[w == 0], ref.g[w == 0])
    sol = LR.solve(ref.H + Hv, ref.g + gv, st.lam)
    assert np.array_equal(st.delta, sol[0]) and st.pred == sol[1]
    Fp, bad = PR.prior_term(w, mu, theta)
    F_data = ref.F_acc
    assert not bad and st.F_acc == F_data + Fp and st.F_prior == Fp and Fp > 0
    assert np.isclose(Fp, float(np.sum(w * (theta.astype(np.float64) - mu) ** 2)), rtol=1e-14)
    # a rejected call (a huge data loss): the SAME system at a larger lambda, from the stored data-only H_acc, g_acc
    big = (calls[0][3] * np.float32(50.0)).astype(np.float32)
    PR.update(st, calls[2][0], calls[2][1], calls[2][2], big, t1, w, mu, 1e-12)
    assert st.rejected == 1 and np.array_equal(st.H, ref.H) and np.array_equal(st.g, ref.g)
    assert np.array_equal(st.Hp, ref.H + Hv) and np.array_equal(st.gp, ref.g + gv) and st.lam == 2e-3


def test_prior_term_order_skips_and_reports():
    th = np.array([0.1, -0.2, 0.3], np.float32)
    w, mu = np.array([2.0, 0.0, 0.5]), np.array([0.0, np.nan, 1.0])   # (a NaN mean under p == 0: skipped, not added)
    d = th.astype(np.float64) - np.array([0.0, 0.0, 1.0])
    Fp, bad = PR.prior_term(w, mu, th)
    assert not bad and Fp == (0.0 + (2.0 * d[0]) * d[0]) + (0.5 * d[2]) * d[2]
    for bw, bm in ((np.array([2.0, 1.0, 0.5]), mu), (np.array([2.0, 0.0, -0.5]), mu), (np.array([np.inf, 0.0, 0.5]), mu),
                   (np.array([np.nan, 0.0, 0.5]), mu), (np.array([1e308, 0.0, 1e308]), np.array([1e10, 0.0, 1e10]))):
        assert PR.prior_term(bw, bm, th)[1]
    # a reported call leaves everything but the counters alone
    _, _, _, call = toy(3, 10, 3)
    info, grad, count, loss = call(np.zeros(3))
    st = PR.new_state()
    trial = PR.update(st, info, grad, count, loss, th, np.array([2.0, 0.0, 0.5]), np.array([0.0, 0.0, 1.0]))
    keep = copy.deepcopy(st)
    for bw, bm in ((np.array([2.0, 1.0, 0.5]), mu), (np.array([2.0, 0.0, -0.5]), mu), (np.array([np.inf, 0.0, 0.5]), mu)):
        back = PR.update(st, info, grad, count, loss, trial, bw, bm)
        assert (back == th).all() and st.lam == keep.lam and st.last == -1 and st.F_acc == keep.F_acc and st.F_prior == keep.F_prior
    assert st.reported == 3 and st.iterations == 4 and st.accepted == 1


def test_prior_only_parameter_moves_towards_its_mean():
    _, _, _, call = toy(5, 20, 2)
    info, grad, count, loss = call(np.zeros(5))
    info[:, 2, :], info[:, :, 2], grad[:, 2] = 0.0, 0.0, 0.0
    info[:, 4, :], info[:, :, 4], grad[:, 4] = 0.0, 0.0, 0.0
    th = np.arange(5, dtype=np.float32)
    w, mu = np.array([0.0, 0.0, 3.0, 0.0, 0.0]), np.array([0.0, 0.0, 2.5, 0.0, 0.0])
    st = PR.new_state()
    new = PR.update(st, info, grad, count, loss, th, w, mu)
    assert st.delta[2] != 0.0 and np.sign(st.delta[2]) == np.sign(mu[2] - th[2]) and abs(new[2] - mu[2]) < abs(th[2] - mu[2])
    # alone in its row and column: (p + lambda p) delta = -p (theta - mu)
    assert np.isclose(st.delta[2], -(th[2] - mu[2]) / (1.0 + st.lam), rtol=1e-14)
    assert st.delta[4] == 0.0 and new[4] == 4.0 and (st.delta[[0, 1, 3]] != 0).all()      # no data, no prior: still left out
    ref = LR.new_state()
    LR.update(ref, info, grad, count, loss, th)
    assert np.allclose(st.delta[[0, 1, 3]], ref.delta[[0, 1, 3]], rtol=1e-12)             # the others: as without the prior


def test_cpu_loop_with_a_prior_is_monotone_and_reproduces_measured(oracle, xarm7):
    p = IR.gauge_problem(oracle, xarm7, base=False)
    n = 9
    st, traj, sigma2, weight, theta = PR.cpu_lm_prior_loop(oracle, p, n)
    want = PR.MEASURED["evaluations"][:n + 1]
    print("[lm prior cpu loop] sigma2", sigma2, "weight", weight[6], traj)
    assert np.isclose(sigma2, PR.MEASURED["sigma2"], rtol=1e-6) and np.isclose(weight[6], PR.MEASURED["weight"], rtol=1e-6)
    assert (weight[:6] == 0).all() and weight[6] == sigma2 / PR.SIGMA_OFFSET0 ** 2
    assert [a for _, a, _ in traj] == [a for _, a, _ in want]
    assert np.allclose([F for F, _, _ in traj], [F for F, _, _ in want], rtol=1e-6)
    acc = [F for F, a, _ in traj if a]
    assert all(y < x for x, y in zip(acc, acc[1:])) and st.F_acc == acc[-1]          # the TOTAL objective never rises
    accp = [Fp for _, a, Fp in traj if a]
    assert st.F_prior == accp[-1] and accp[0] == 0.0 and all(f >= 0 for f in accp)
    assert st.F_prior == (weight[6] * float(theta[6])) * float(theta[6])            # (p d) d, the kernel's order
    # the bound the objective's monotonicity gives: p (theta - mu)^2 <= F_acc <= F(start), at every accepted point
    assert abs(float(theta[6])) <= np.sqrt(traj[0][0] / weight[6])
    assert st.accepted + st.rejected + st.reported == st.iterations == n + 1
