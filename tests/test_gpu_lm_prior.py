"""Levenberg-Marquardt under a Gaussian prior on the GPU (``ehr_lm_update_prior``: csrc/ehr_lm.hip, easyhec_amd/lm.py; DESIGN.md
section 6p) against the numpy restatement of tests/lm_prior_reference.py under tests/lm_reference.py's derived bar: the update
kernel alone on synthetic systems, no prior against today's entry point (bytes), the prior-only parameter, the reported calls a
bad prior makes, the MAP solve end to end on the gauge problems, non-interference with a running Adam solve, and the Python
refusals.  tests/test_lm_prior_reference.py pins the reference on the CPU; the rig's form is in tests/test_gpu_lm_rig_prior.py.
Every figure is printed before it is asserted; the measured ones are in profiles/lm_prior.md."""
import ctypes

import numpy as np
import pytest
import torch

import lm_prior_reference as PR
import lm_reference as LR
from test_gpu_fast import problem
from test_gpu_lm import (DEV, FTOL, UH, UW, K_expected, Upd, _loss_at_accepted, _params_of, _stream, gauge, gauge_model, ref_state,
                         system, t32)

pytestmark = pytest.mark.gpu

EPS53 = 2.0 ** -53


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr, fused, lm
    assert _lib.has_lm_prior()
    return _lib, fused, dr, lm


def f64(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


class PUpd(Upd):
    """test_gpu_lm.Upd through the entry point that takes a prior.  entry: "plain" (ehr_lm_update), "prior"
    (ehr_lm_update_prior with ``weight`` / ``mean``; both None: NULL, NULL)."""

    def __init__(self, _lib, N, seed, weight=None, mean=None, entry="prior", **kw):
        super().__init__(_lib, N, seed, **kw)
        self.entry = entry
        self.set_prior(weight, mean)

    def set_prior(self, weight, mean):
        self.weight, self.mean = weight, mean
        self.w_dev = None if weight is None else f64(weight)
        self.m_dev = None if mean is None else f64(mean)

    def call(self, info, grad, count, loss, ftol=1e-6, lambda_max=1e6, finalize=0):
        _lib = self._lib
        ti, tg = f64(info), f64(grad)
        tc = torch.tensor(np.ascontiguousarray(count, np.int64), device=DEV)
        tl = t32(loss)
        intr = self.mask != 0
        args = (_lib.ptr(ti), _lib.ptr(tg), _lib.ptr(tc), _lib.ptr(tl), info.shape[0], self.N, _lib.ptr(self.dof),
                _lib.ptr(self.offset if self.F else None), _lib.ptr(self.free_list), self.F, self.J,
                _lib.ptr(self.theta if intr else None), self.mask, self.tie, _lib.ptr(self.K0 if intr else None),
                _lib.ptr(self.K if intr else None), UH, UW, ctypes.c_double(ftol), ctypes.c_double(lambda_max), finalize,
                _lib.ptr(self.state), _lib.ptr(self.log), 64)
        with torch.cuda.device(DEV):
            if self.entry == "plain":
                _lib.check(_lib.lib().ehr_lm_update(*args, _stream()), "ehr_lm_update")
            else:
                _lib.check(_lib.lib().ehr_lm_update_prior(*args, _lib.ptr(self.w_dev), _lib.ptr(self.m_dev), _stream()),
                           "ehr_lm_update_prior")
            ti.fill_(float("nan")), tg.fill_(float("nan")), tl.fill_(float("nan")), tc.fill_(-7)
        torch.cuda.synchronize()
        return self.ns()


def pref_state(ns):
    """lm_prior_reference's state at the GPU's own previous state."""
    st = ref_state(ns)
    st.F_prior, st.Hp, st.gp = float(ns.F_prior), None, None
    return st


def compare_prior(ns, st, got_params, want_params, what, worst):
    """Exact: lambda, nu, F_acc, F_prior, the counters and flags, theta and the data-only H_acc, g_acc.  delta, pred: the bar
    32 * 2^-53 * cond with cond and the scaling of the POSTERIOR system (st.cond, st.Hp)."""
    assert ns.__dict__["lambda"] == st.lam and ns.nu == st.nu and ns.F_acc == st.F_acc, (what, ns.__dict__["lambda"], st.lam, ns.F_acc, st.F_acc)
    assert ns.F_prior == st.F_prior, (what, ns.F_prior, st.F_prior)
    for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last", "count", "retries"):
        assert int(getattr(ns, k)) == int(getattr(st, k)), (what, k, getattr(ns, k), getattr(st, k))
    if st.accepted:
        assert (ns.theta == st.theta).all() and (ns.H == st.H).all() and (ns.g == st.g).all(), what
    if st.last != -1 and st.delta is not None and st.cond is not None and st.Hp is not None:
        s = np.sqrt(np.where(np.diag(st.Hp) > 0, np.diag(st.Hp), 1.0))
        y, yr = ns.delta * s, st.delta * s
        bar = 32 * EPS53 * st.cond
        ry = float(np.abs(y - yr).max() / max(np.abs(yr).max(), 1e-300)) / bar
        rp = abs(ns.pred - st.pred) / max(abs(st.pred), 1e-300) / bar
        worst[0], worst[1] = max(worst[0], ry), max(worst[1], rp)
        assert ry <= 1.0 and rp <= 1.0, (what, ry, rp, st.cond)
        assert ((st.delta == 0) == (ns.delta == 0)).all(), what
    gp, wp = np.asarray(got_params, np.float32), np.asarray(want_params, np.float32)
    assert (np.abs(gp.astype(np.float64) - wp.astype(np.float64)) <= LR.spacing_f32(wp)).all(), (what, gp, wp)


def pstep(u, info, grad, count, loss, what, worst, **kw):
    kw.setdefault("ftol", FTOL)
    before, now = pref_state(u.ns()), u.params()
    ns = u.call(info, grad, count, loss, **kw)
    want = PR.update(before, info, grad, count, loss, now, u.weight, u.mean, kw["ftol"], kw.get("lambda_max", 1e6),
                     bool(kw.get("finalize", 0)))
    compare_prior(ns, before, u.params(), want, what, worst)
    if u.mask:
        assert K_expected(u).tobytes() == u.K.cpu().numpy().tobytes(), f"{what}: K is not intrinsics_from_theta(theta)"
        if u.tie:
            assert u.theta[0].item() == u.theta[1].item()
    return ns, before


def prior_for(u, info, seed=0):
    """A prior on a SUBSET of u's parameters (the first is always free of it, the last always has one): weights of the order
    of the data's own diagonal (1e-2 .. 10 times it), means a small step from the start."""
    N = u.N
    rng = np.random.default_rng(500 + 10 * N + seed)
    d = np.diag(info.sum(axis=0))
    w = np.where(rng.uniform(size=N) < 0.5, d * 10.0 ** rng.uniform(-2, 1, N), 0.0)
    w[N - 1] = d[N - 1] * 0.5
    if N > 1:
        w[0] = 0.0
    mean = u.params().astype(np.float64) + rng.normal(size=N) * 1e-3 / np.sqrt(np.where(d > 0, d, 1.0)) * np.sqrt(d.max())
    return w, mean


# ---- 1. the update kernel alone ----------------------------------------------------------------------------------------------
def _prior_sequence(_lib, N, worst):
    B = 3
    u = PUpd(_lib, N, 0)
    info, grad, count, loss = system(N, B, 0)
    w, mean = prior_for(u, info)
    u.set_prior(w, mean)
    ns, st = pstep(u, info, grad, count, loss, f"N={N} first call", worst)
    assert ns.accepted == 1 and ns.__dict__["lambda"] == 1e-3 and ns.F_prior > 0 and ns.F_acc == st.F_acc
    info2, grad2, count2, _ = system(N, B, 1)
    lo = (loss * np.float32(0.9)).astype(np.float32)
    ns, st = pstep(u, info2, grad2, count2, lo, f"N={N} accept", worst)
    assert ns.accepted == 2 and ns.nu == 2.0
    info3, grad3, count3, _ = system(N, B, 2)
    accepted, Hd, Fp = ns.theta.copy(), ns.H.copy(), ns.F_prior
    ns, st = pstep(u, info3, grad3, count3, lo * np.float32(1.5), f"N={N} reject", worst)
    assert ns.rejected == 1 and ns.nu == 4.0 and (ns.H == Hd).all() and (ns.theta == accepted).all() and ns.F_prior == Fp
    ns, st = pstep(u, info3, grad3, count3, lo * np.float32(2.0), f"N={N} second reject", worst)
    assert ns.rejected == 2 and ns.nu == 8.0
    lam = ns.__dict__["lambda"]
    l4 = lo.copy()
    l4[1] = np.nan
    ns, st = pstep(u, info, grad, count, l4, f"N={N} reported", worst)
    assert ns.reported == 1 and ns.__dict__["lambda"] == lam and (u.params() == accepted.astype(np.float32)).all()
    ns, st = pstep(u, info3, grad3, count3, lo * np.float32(3.0), f"N={N} third reject", worst)
    assert (u.params() != accepted.astype(np.float32)).any()
    raw = ns.raw
    ns, st = pstep(u, info, grad, count, loss, f"N={N} finalize", worst, finalize=1)
    assert (u.params() == accepted.astype(np.float32)).all() and ns.raw.tobytes() == raw.tobytes()
    log = u.log.cpu().numpy()[:6]
    assert log[:, 1].tolist() == [1, 1, 0, 0, -1, 0] and np.isnan(log[4, 0]) and log[1, 0] == ns.F_acc
    return u


@pytest.mark.parametrize("N", [1, 6, 7, 10, 32])
def test_update_kernel_alone_under_a_prior(env, N):
    _lib = env[0]
    worst = [0.0, 0.0]
    a = _prior_sequence(_lib, N, worst)
    print(f"[lm prior update] N={N}: prior on {int((a.weight != 0).sum())} of {N} parameters; worst |y - y_ref| / (32 2^-53 cond |y|) "
          f"= {worst[0]:.4f}, the same for pred = {worst[1]:.4f}")
    b = _prior_sequence(_lib, N, [0.0, 0.0])                                      # two runs: identical bits
    for x, y in ((a.state, b.state), (a.dof, b.dof), (a.offset, b.offset), (a.theta, b.theta), (a.K, b.K), (a.log, b.log)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# ---- 2. no prior is today's update -------------------------------------------------------------------------------------------
def _plain_sequence(u):
    """first call, accept, two rejects, four reported calls, a reject, finalize -- test_gpu_lm.py's sequence."""
    N, B = u.N, 3
    info, grad, count, loss = system(N, B, 0)
    info2, grad2, count2, _ = system(N, B, 1)
    info3, grad3, count3, _ = system(N, B, 2)
    lo = (loss * np.float32(0.9)).astype(np.float32)
    u.call(info, grad, count, loss, ftol=FTOL)
    u.call(info2, grad2, count2, lo, ftol=FTOL)
    u.call(info3, grad3, count3, lo * np.float32(1.5), ftol=FTOL)
    u.call(info3, grad3, count3, lo * np.float32(2.0), ftol=FTOL)
    l4 = lo.copy()
    l4[1] = np.nan
    u.call(info, grad, count, l4, ftol=FTOL)
    ns = u.call(info3, grad3, count3, lo * np.float32(3.0), ftol=FTOL)
    assert (ns.accepted, ns.rejected, ns.reported) == (2, 3, 1)
    u.call(info, grad, count, loss, ftol=FTOL, finalize=1)
    return u


@pytest.mark.parametrize("N", [1, 6, 7, 10, 32])
def test_no_prior_is_todays_update_byte_for_byte(env, N):
    _lib = env[0]
    mean = np.random.default_rng(N).normal(size=N)
    mean[0] = np.nan                                                              # (under p == 0 nothing of the mean is used)
    runs = [_plain_sequence(PUpd(_lib, N, 0, entry="plain")), _plain_sequence(PUpd(_lib, N, 0)),
            _plain_sequence(PUpd(_lib, N, 0, np.zeros(N), mean))]
    a = runs[0]
    assert a.state[_lib.LM_STATE["F_prior"]].item() == 0.0
    for what, b in (("NULL, NULL", runs[1]), ("all-zero weights", runs[2])):
        for name in ("state", "log", "dof", "offset", "theta", "K"):
            assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), (what, name)


def test_one_null_pointer_is_refused(env):
    _lib = env[0]
    u = PUpd(_lib, 6, 0)
    untouched = u.state.clone()
    info, grad, count, loss = system(6, 2, 0)
    for w, m, lacks in ((np.ones(6), None, "prior_mean"), (None, np.ones(6), "prior_weight")):
        u.set_prior(w, m)
        with pytest.raises(RuntimeError, match=f"prior_weight and prior_mean go together.*{lacks} NULL"):
            u.call(info, grad, count, loss)
    torch.cuda.synchronize()
    assert torch.equal(u.state, untouched)


# ---- 3. a parameter only the prior sees --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 6, 7, 10, 32])
def test_prior_only_parameter_moves_towards_its_mean(env, N):
    _lib = env[0]
    worst = [0.0, 0.0]
    info, grad, count, loss = system(N, 2, 5)
    z = max(N - 2, 0)                                   # no data information, a prior: moves
    z0 = 0 if N >= 3 else None                          # no data information, no prior: left out, as ever
    iz, gz = info.copy(), grad.copy()
    for k in (z, z0):
        if k is not None:
            iz[:, k, :], iz[:, :, k], gz[:, k] = 0.0, 0.0, 0.0
    u = PUpd(_lib, N, 1, zero_theta=False)
    p0 = u.params()
    w, mean = np.zeros(N), np.zeros(N)
    w[z], mean[z] = 2.5, float(p0[z]) + 0.01
    u.set_prior(w, mean)
    ns, st = pstep(u, iz, gz, count, loss, f"N={N} prior-only parameter", worst)
    want = -(float(p0[z]) - mean[z]) / (1.0 + 1e-3)     # alone in its row and column: (p + lambda p) delta = -p (theta - mu)
    print(f"[lm prior only] N={N}: parameter {z}: theta {p0[z]!r}, mu {mean[z]!r}, delta {ns.delta[z]!r} (closed form {want!r}); "
          f"worst ratios {worst[0]:.4f}, {worst[1]:.4f}")
    assert ns.delta[z] != 0.0 and ns.delta[z] > 0 and np.isclose(ns.delta[z], want, rtol=1e-12)
    assert abs(float(u.params()[z]) - mean[z]) < abs(float(p0[z]) - mean[z]) and ns.H[z, z] == 0.0 and ns.g[z] == 0.0
    if z0 is not None:
        assert ns.delta[z0] == 0.0 and u.params()[z0] == p0[z0]
        assert (ns.delta[[k for k in range(N) if k not in (z, z0)]] != 0).all()


# ---- 4. a bad prior reports the call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 32])
def test_bad_prior_reports_the_call(env, N):
    _lib = env[0]
    worst = [0.0, 0.0]
    info, grad, count, loss = system(N, 3, 0)
    u = PUpd(_lib, N, 0)
    w, mean = prior_for(u, info)
    u.set_prior(w, mean)
    ns, _ = pstep(u, info, grad, count, loss, f"N={N} first call", worst)
    accepted, lam, raw = ns.theta.astype(np.float32), ns.__dict__["lambda"], ns.raw.copy()
    assert (u.params() != accepted).any()
    k = N - 1                                                                     # (it has a prior)
    for i, what in enumerate(("NaN mean under a positive weight", "negative weight", "infinite weight")):
        w2, m2 = w.copy(), mean.copy()
        if i == 0:
            m2[k] = np.nan
        elif i == 1:
            w2[k] = -w[k]
        else:
            w2[k] = np.inf
        u.dof.add_(0.25)                                                          # a trial is in the pointers
        u.set_prior(w2, m2)
        ns, _ = pstep(u, info, grad, count, (loss * np.float32(0.5)).astype(np.float32), f"N={N} {what}", worst)
        assert ns.reported == i + 1 and ns.last == -1 and ns.__dict__["lambda"] == lam and (u.params() == accepted).all()
        changed = np.flatnonzero(ns.raw != raw)
        assert set(changed.tolist()) <= {_lib.LM_STATE["reported"], _lib.LM_STATE["iterations"], _lib.LM_STATE["last"]}, changed
    u.set_prior(w, mean)                                                          # the good prior again: the solve goes on
    ns, _ = pstep(u, info, grad, count, (loss * np.float32(0.5)).astype(np.float32), f"N={N} after the reports", worst)
    assert ns.accepted == 2 and ns.reported == 3


# ---- 5. end to end: the MAP solve on the gauge problems ----------------------------------------------------------------------
BOUND = 1e-3     # rad (offset[0]) or theta units: how far the prior lets a parameter go, by the derivation below


def _gauge_step(oracle, xarm7, kind):
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    p = gauge(oracle, xarm7, kind != "offset0-gauge")
    model, batch, qp = gauge_model(p)
    if kind == "offset0-gauge":
        return JointPoseStep(model, batch, p.rb, qp, free=[0]), ["offset[0]"]
    return IntrinsicsPoseStep(model, batch, free=("f", "cx", "cy")), ["theta[f]", "theta[cx]", "theta[cy]"]


@pytest.mark.parametrize("kind", ["offset0-gauge", "f-cx-cy"])
def test_map_solve_on_the_gauge_problem(env, oracle, xarm7, kind):
    """The prior's mean is the start value, so the prior term is 0 at the start; the total objective never rises, so at every
    accepted point  p_k (theta_k - mu_k)^2 <= F_prior <= F_acc <= F_data(start),  i.e.  |theta_k - mu_k| <= sqrt(F_data(start)
    / p_k).  p_k = F_data(start) / BOUND^2 makes that bound BOUND (sigma2 = F_data(start), sigma_k = BOUND)."""
    _lib, fused, dr, lm = env
    st, held = _gauge_step(oracle, xarm7, kind)
    o = lm.LevenbergMarquardt(st)
    F0, count0 = o.evaluate()
    prior = lm.make_prior(o, {nm: BOUND for nm in held}, sigma2=F0)
    o.set_prior(prior)
    w, mu = prior.weight.cpu().numpy(), prior.mean.cpu().numpy()
    idx = [o.names.index(nm) for nm in held]
    assert (np.delete(w, idx) == 0).all() and (w[idx] == F0 / BOUND ** 2).all() and (mu == 0).all()
    bound = np.sqrt(F0 / w[idx])
    worst = 0.0
    for it in range(14):
        o.iterate(1)
        s = o.state()
        if s.accepted:
            worst = max(worst, float(np.abs(s.theta[idx] - mu[idx]).max()))
            assert (np.abs(s.theta[idx] - mu[idx]) <= bound).all(), (it, s.theta[idx], bound)
        if s.done:
            break
    o.finalize()
    s, tr = o.state(), o.trajectory()
    fused.check_status(st.glctx)
    acc = tr[tr[:, 1] == 1, 0]
    params = _params_of(o)
    F = _loss_at_accepted(fused, dr, o)
    Fp, bad = PR.prior_term(w, mu, params)
    print(f"[lm prior end to end] {kind}: F_data(start) {F0!r}, p = {w[idx][0]:.6g}; accepted objectives {np.round(acc, 3).tolist()}; "
          f"{s.accepted} accepted, {s.rejected} rejected, {s.reported} reported, done {s.done} ({LR.WHY[s.why]}); F_acc {s.F_acc!r} = "
          f"data {F!r} + prior {s.F_prior!r} (host {Fp!r}); held parameters {params[idx].tolist()}, worst |theta - mu| "
          f"{worst:.3g} <= bound {bound[0]:.3g}")
    assert tr[0, 0] == F0 and (np.diff(acc) < 0).all() and len(acc) >= 2 and acc[-1] == s.F_acc   # (two: one real descent step)
    assert (params == s.theta.astype(np.float32)).all()
    assert not bad and s.F_prior == Fp                                           # the host's float64 evaluation, exactly
    assert s.F_acc == F + s.F_prior                                              # the update's one addition
    assert s.F_acc - s.F_prior == F                                              # the data's loss at the accepted point
    assert s.accepted + s.rejected + s.reported == s.iterations
    # the same start without a prior: how far the held parameters drift (profiles/lm_prior.md; measured, not asserted)
    st2, _ = _gauge_step(oracle, xarm7, kind)
    o2 = lm.LevenbergMarquardt(st2)
    o2.iterate(14).finalize()
    s2 = o2.state()
    print(f"[lm prior end to end] {kind}: without a prior the same parameters end at {_params_of(o2)[idx].tolist()}, loss {s2.F_acc!r} "
          f"({s2.accepted} accepted of {s2.iterations})")


def test_solve_lm_under_the_default_prior(env, oracle, xarm7):
    """solve_lm(prior_sigma="default"): sigma2 from one evaluation at the start, PRIOR_SIGMA on offset[0] alone; the result
    carries both parts of the objective, the data's report and the posterior's."""
    _lib, fused, dr, lm = env
    from easyhec_amd.info_explorer import PRIOR_SIGMA
    st, _ = _gauge_step(oracle, xarm7, "offset0-gauge")
    F0, count0 = lm.LevenbergMarquardt(st).evaluate()
    res = lm.solve_lm(st, max_iters=10, prior_sigma="default")
    pr = res.prior
    sigma2 = F0 / max(count0 - 7, 1)
    print(f"[lm prior solve] sigma2 {pr.sigma2!r} (loss {F0!r} / (count {count0} - 7)); weight {pr.weight.cpu().numpy().tolist()}; loss "
          f"{res.loss!r} = data {res.data_loss!r} + prior {res.prior_loss!r}; {res.accepted} accepted of {res.iterations}, {res.why}")
    assert pr.sigma2 == sigma2 and pr.names == res.lm.names and np.isinf(pr.sigma[:6]).all() and pr.sigma[6] == PRIOR_SIGMA["revolute"]
    assert pr.weight.cpu().numpy().tolist() == [0.0] * 6 + [sigma2 / PRIOR_SIGMA["revolute"] ** 2]
    assert res.loss == res.state.F_acc and res.prior_loss == res.state.F_prior and res.data_loss == res.loss - res.prior_loss
    assert res.trajectory[0, 0] == F0 and res.loss < F0
    assert (res.report.H == res.state.H).all() and res.report.loss == res.data_loss
    post = res.posterior
    assert post.H_views.shape == (2, 7, 7) and (post.H_views[0] == res.state.H).all()
    assert (post.H_views[1] == np.diag(pr.weight.cpu().numpy())).all() and post.sigma2() == pr.sigma2
    assert post.H[6, 6] == res.state.H[6, 6] + pr.weight[6].item() and np.isfinite(post.covariance()).all()
    plain = lm.solve_lm(_gauge_step(oracle, xarm7, "offset0-gauge")[0], max_iters=2)
    assert plain.prior is None and plain.posterior is None and plain.prior_loss == 0.0 and plain.data_loss == plain.loss


# ---- 6. beside Adam, and the refusals ----------------------------------------------------------------------------------------
def test_lm_under_a_prior_leaves_adam_and_a_captured_chain_alone(env, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 3, 120, 160, 0.125)
    model = make()
    st = FusedPoseStep(model, batch)
    st.capture()
    for _ in range(10):
        st.step()
    torch.cuda.synchronize()
    snap = lambda: [st.exp_avg.clone(), st.exp_avg_sq.clone(), st.step_t.clone(), st.hist_row.clone(), model.history_ops.clone()]
    a = snap()
    res = lm.solve_lm(st, max_iters=5, prior_sigma={"rotation": 0.1}, sigma2=1.0)
    torch.cuda.synchronize()
    for x, y in zip(a, snap()):
        assert torch.equal(x, y)
    assert res.accepted >= 1 and int(st.step_t) == 10 and st._graph and res.prior_loss >= 0.0
    st.step()                                                                    # the captured chain still replays
    torch.cuda.synchronize()
    assert int(st.step_t) == 11 and bool(torch.isfinite(st.loss).all())
    st.release_graph()


def test_refusals(env, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd import lm_multi
    from easyhec_amd.joint_calib import JointPoseStep
    from test_gpu_joint_offsets import _views_qpos
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    st = JointPoseStep(make(), batch, xarm7, _views_qpos(xarm7, 2), free=[1, 2])
    o = lm.LevenbergMarquardt(st)
    assert o.names[6:] == ["offset[1]", "offset[2]"]
    for kw, match in ((dict(prior_sigma=0.0), "every sigma is > 0"), (dict(prior_sigma=-1.0), "every sigma is > 0"),
                      (dict(prior_sigma=float("nan")), "every sigma is > 0"), (dict(prior_sigma={"offset[1]": -0.1}), "every sigma is > 0"),
                      (dict(prior_sigma=[0.1] * 7), "sequence of N = 8"), (dict(prior_sigma={"offset[5]": 0.1}), "keys are parameter names"),
                      (dict(prior_sigma="loose"), "'default'"), (dict(prior_sigma=0.1, prior_mean={"offset[1]": float("inf")}), "mean under a finite sigma"),
                      (dict(prior_sigma=0.1, prior_mean=[0.0] * 5), "sequence of N = 8"), (dict(prior_sigma=0.1, prior_mean={"dof[9]": 0.0}), "keys are parameter names"),
                      (dict(prior_sigma=0.1, sigma2=0.0), "sigma2 must be finite and > 0"), (dict(prior_sigma=0.1, sigma2=-2.0), "sigma2 must be finite and > 0")):
        with pytest.raises(ValueError, match=match):
            lm.make_prior(o, sigma2=kw.pop("sigma2", 1.0), **kw)
    pr = lm.make_prior(o, [None, float("inf"), 0.1, None, None, None, 0.05, None], sigma2=2.0, prior_mean={"offset[1]": 0.01})
    assert pr.weight.cpu().numpy().tolist() == [0, 0, 2.0 / 0.1 ** 2, 0, 0, 0, 2.0 / 0.05 ** 2, 0]
    assert pr.mean.cpu().numpy()[[2, 6]].tolist() == [float(st.model.dof[2].item()), 0.01]      # a pose coordinate: its value now
    pr = lm.make_prior(st, "default", sigma2=1.0)                                # a step object: a driver is made for the call
    assert pr.weight.cpu().numpy().tolist() == [0.0] * 6 + [1.0 / 0.05 ** 2] * 2 and (pr.mean.cpu().numpy() == 0).all()
    with pytest.raises(ValueError, match="pass prior_sigma as well"):
        lm.solve_lm(st, sigma2=1.0)
    other = lm.make_prior(lm.LevenbergMarquardt(JointPoseStep(make(), batch, xarm7, _views_qpos(xarm7, 2), free=[3])), 0.1, sigma2=1.0)
    with pytest.raises(ValueError, match="the prior was made for"):
        lm.LevenbergMarquardt(st, prior=other)
    with pytest.raises(ValueError, match="multi-start solve: it is pose-only"):
        lm_multi.solve_lm_multi(None, None, None, prior_sigma="default")
    with pytest.raises(ValueError, match="multi-start solve: it is pose-only"):
        lm_multi.solve_global_lm(None, None, None, 4, 2, sigma2=1.0)
    import easyhec_amd
    assert easyhec_amd.make_prior is lm.make_prior and easyhec_amd.LmPrior is lm.LmPrior
