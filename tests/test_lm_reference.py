"""tests/lm_reference.py pinned on the CPU: the update on an exactly linear least-squares toy, the damping's schedule on scripted
accept / reject sequences, the exclusion of parameters without information, the reported call, the stopping rules, and the CPU
Levenberg-Marquardt loop on the gauge problem (monotone, and the trajectory recorded in ``lm_reference.MEASURED``)."""
import numpy as np

import information_reference as IR
import lm_reference as LR


def toy(n, m, seed, scale=None):
    """A linear least-squares problem F(x) = |A x - b|^2 in the op's conventions: info = A^T A, grad = 2 A^T (A x - b)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(m, n)) * (np.ones(n) if scale is None else np.asarray(scale))
    b = rng.normal(size=m)
    F = lambda x: float(np.sum((A @ x - b) ** 2))
    call = lambda x: ((A.T @ A)[None], (2.0 * A.T @ (A @ x - b))[None], np.array([m]), np.array([F(x)], np.float64))
    return A, b, F, call


def test_one_step_with_no_damping_lands_on_the_minimum_and_pred_is_the_true_reduction():
    A, b, F, call = toy(6, 40, 0, scale=[1, 10, 100, 1e-2, 1, 3])
    x0 = np.zeros(6)
    st = LR.new_state(lambda0=1e-14)
    info, grad, count, loss = call(x0)
    LR.update(st, info, grad, count, loss, x0.astype(np.float32))
    xmin = np.linalg.lstsq(A, b, rcond=None)[0]
    assert np.allclose(st.theta + st.delta, xmin, rtol=1e-9, atol=0)
    assert np.isclose(st.pred, F(x0) - F(xmin), rtol=1e-9)
    assert st.accepted == 1 and st.iterations == 1 and st.lam == 1e-14 and st.nu == 2.0


def test_lambda_schedule_on_scripted_sequences():
    _, _, _, call = toy(3, 10, 1)
    info, grad, count, _ = call(np.zeros(3))
    th = np.zeros(3, np.float32)
    st = LR.new_state(lambda0=1e-3)
    LR.update(st, info, grad, count, np.array([100.0]), th)                      # first call: accepted, lambda as it was
    assert (st.lam, st.nu, st.accepted) == (1e-3, 2.0, 1)
    LR.update(st, info, grad, count, np.array([100.0]), th)                      # equal loss: NOT strictly lower -> rejected
    assert (st.lam, st.nu, st.rejected) == (2e-3, 4.0, 1)
    LR.update(st, info, grad, count, np.array([101.0]), th)                      # two in a row: nu doubles
    assert (st.lam, st.nu, st.rejected) == (8e-3, 8.0, 2)
    pred = st.pred
    F = 100.0 - 0.5 * pred                                                       # rho = 1/2: the factor is exactly 1
    LR.update(st, info, grad, count, np.array([F]), th)
    assert st.accepted == 2 and st.nu == 2.0 and np.isclose(st.rho, 0.5, rtol=1e-6)
    assert np.isclose(st.lam, 8e-3 * (1.0 - (2.0 * st.rho - 1.0) ** 3), rtol=1e-15)
    lam, pred, Facc = st.lam, st.pred, st.F_acc
    LR.update(st, info, grad, count, np.array([Facc - 10.0 * pred]), th)         # rho >> 1: the factor's floor 1/3
    assert st.lam == lam * (1.0 / 3.0) and st.accepted == 3
    assert st.accepted + st.rejected + st.reported == st.iterations == 5


def test_excluded_parameters_do_not_move():
    _, _, _, call = toy(5, 20, 2)
    info, grad, count, loss = call(np.zeros(5))
    info[:, 2, :], info[:, :, 2] = 0.0, 0.0
    st = LR.new_state()
    new = LR.update(st, info, grad, count, loss, np.arange(5, dtype=np.float32))
    assert st.delta[2] == 0.0 and new[2] == 2.0 and (st.delta[[0, 1, 3, 4]] != 0).all()
    keep = [0, 1, 3, 4]
    d4, pred4, _, _, _ = LR.solve(info[0][np.ix_(keep, keep)], grad[0][keep], st.lam)
    assert np.allclose(st.delta[keep], d4, rtol=1e-12) and np.isclose(st.pred, pred4, rtol=1e-12)


def test_reported_call_and_stopping_rules():
    _, _, _, call = toy(3, 10, 3)
    info, grad, count, loss = call(np.zeros(3))
    th = np.array([1.0, 2.0, 3.0], np.float32)
    st = LR.new_state()
    trial = LR.update(st, info, grad, count, loss, th)
    lam = st.lam
    for bad in ("info", "grad", "loss", "count"):
        i2, g2, c2, l2 = info.copy(), grad.copy(), count.copy(), loss.copy()
        if bad == "info":
            i2[0, 1, 1] = np.nan
        elif bad == "grad":
            g2[0, 0] = np.inf
        elif bad == "loss":
            l2[0] = np.nan
        else:
            c2[0] = -1
        back = LR.update(st, i2, g2, c2, l2, trial)
        assert (back == th).all() and st.lam == lam and st.last == -1
    assert st.reported == 4 and st.iterations == 5 and st.accepted == 1
    # ftol
    st = LR.new_state()
    assert (LR.update(st, info, grad, count, loss, th, ftol=1e30) == th).all() and (st.done, st.why) == (1, 1)
    assert (LR.update(st, info * np.nan, grad, count, loss, th) == th).all() and st.iterations == 1    # done: only restores
    # lambda_max
    st = LR.new_state()
    LR.update(st, info, grad, count, loss, th, lambda_max=1e-3)
    assert (st.done, st.why) == (1, 2)
    # step below float32's spacing: a huge matrix makes delta tiny
    st = LR.new_state()
    LR.update(st, info * 1e20, grad, count, loss, th, ftol=0.0)
    assert (st.done, st.why) == (1, 3)


def test_cpu_loop_on_the_gauge_problem_is_monotone_and_reproduces_measured(oracle, xarm7):
    p = IR.gauge_problem(oracle, xarm7, base=True)
    n = 9
    st, traj, dof = LR.cpu_lm_loop(oracle, p, n)
    want = LR.MEASURED["evaluations"][:n + 1]
    print("[lm cpu loop]", traj)
    assert [a for _, a in traj] == [a for _, a in want]
    assert np.allclose([F for F, _ in traj], [F for F, _ in want], rtol=1e-6)
    acc = [F for F, a in traj if a]
    assert all(y < x for x, y in zip(acc, acc[1:]))
    assert np.isclose(acc[7], LR.MEASURED["F7"], rtol=1e-6) and st.F_acc == acc[-1]
    assert st.accepted + st.rejected + st.reported == st.iterations == n + 1
