"""Float64 numpy restatement of the Levenberg-Marquardt update UNDER A GAUSSIAN PRIOR (``ehr_lm_update_prior``,
``ehr_lm_update_rig_prior``: csrc/ehr_lm.hip, include/ehr.h), beside tests/lm_reference.py and
tests/lm_rig_reference.py whose ``solve``, ``spacing_f32``, ``gather`` and bars it reuses.  CPU only, not collected by pytest.

The objective is the MAP estimate's

    F(theta) = sum_views w (mask - ref)^2 + sum_k p_k (theta_k - mu_k)^2,        p_k = sigma2 / sigma_k^2,

and the ORDER of the operations is the contract (the library is built without fused multiply-add, so every line below is one
rounding where the kernel has one):

a. the prior's term at the trial, the float32 parameters as the pointers hold them: ``d_k = (double) theta_k - mu_k``,
   ``Fp = sum_k (p_k * d_k) * d_k`` for k ascending from 0.0; terms with ``p_k == 0`` are skipped.  A non-finite Fp, a
   non-finite mu_k where p_k != 0, or a p_k that is negative or not finite reports the call;
b. accept / reject on ``F = F_data + Fp`` (one addition); an accept stores Fp as ``F_prior``;
c. the stored H_acc, g_acc, theta_acc stay the data's; the system that is solved is, accepted or rejected,
   ``H_acc + diag(p)`` and ``g_acc[k] + 2.0 * p_k * (theta_acc[k] - mu_k)`` (only where p_k != 0);
d. the scaled damped Cholesky solve, pred, the stopping rule (``ftol * F_acc`` with the TOTAL F_acc) and the trial run on that
   system (``lm_reference.solve``): a parameter without data information but with p_k > 0 moves, towards mu_k.

What is exact and what has a bar is lm_reference's: lambda, nu, F_acc, F_prior, the counters, the flags, theta and the
data-only H_acc / g_acc involve no rounding the kernel could do differently; delta and pred go through a factorisation and
are held to ``32 * 2^-53 * cond`` with cond the condition number of the POSTERIOR scaled damped matrix (``st.cond``; the
scaling that turns delta into y is the posterior diagonal's, ``st.Hp``).

With ``weight is None`` every function here is lm_reference's / lm_rig_reference's, operation for operation; with all-zero
weights the values are the same too (``F_data + 0.0``, nothing added to H or g).

The CPU loop
------------
``cpu_lm_prior_loop`` runs ``update`` on ``information_reference.gauge_problem(base=False)`` -- xArm7 without its base link, 4
views, 120x160 -- with ``offset[0]`` free: joint 0's zero error trades against the camera rotation (a gauge direction, H is
singular).  The prior is on ``offset[0]`` alone: sigma = 0.05 rad (``info_explorer.PRIOR_SIGMA["revolute"]``), mean 0, sigma2 =
loss / max(count - N, 1) of the start.  Its trajectory is MEASURED below; tests/test_lm_prior_reference.py reproduces it."""
import numpy as np
import torch

import information_reference as IR
import lm_reference as LR
import lm_rig_reference as RR

SIGMA_OFFSET0 = 0.05      # rad: info_explorer.PRIOR_SIGMA["revolute"]

# The CPU loop on gauge_problem(base=False), offset[0] free, the prior above, lambda_0 = 1e-3, this file's
# ``cpu_lm_prior_loop`` (float64, oracle-driven), 2026-10-20: per evaluation (evaluation 0 is the start) the TOTAL objective,
# whether it was accepted, and the prior's term of it.
MEASURED = {
    "sigma2": 31.007418738471138,         # loss / max(count - 7, 1) at the start
    "weight": 12402.967495388453,         # sigma2 / 0.05^2: p of offset[0]
    "evaluations": [(2232.534149169922, True, 0.0), (1881.4831936476241, True, 0.0035488722335049825),
                    (1489.5943644185745, True, 0.002933754512089323), (1186.5706043091525, True, 9.344489469098483e-05),
                    (810.8018955103153, True, 1.562750274041403e-05), (480.14612333834805, True, 5.1742855665134046e-06),
                    (181.32753463553746, True, 9.136136257754735e-07), (115.71263323255559, True, 9.962101333947372e-08),
                    (170.43048859369523, False, 7.269437048849567e-09), (170.4304123215509, False, 2.9070446903469612e-08)],
}


def new_state(lambda0=1e-3):
    st = LR.new_state(lambda0)
    st.F_prior, st.Hp, st.gp = 0.0, None, None
    return st


def prior_term(weight, mean, theta_now):
    """(Fp, bad) of step a. at the float32 parameters ``theta_now``."""
    w, mu = np.asarray(weight, np.float64), np.asarray(mean, np.float64)
    th = np.asarray(theta_now, np.float32).astype(np.float64)
    Fp, bad = 0.0, False
    with np.errstate(all="ignore"):
        for k in range(len(w)):                       # k ascending
            if not (w[k] >= 0.0) or not np.isfinite(w[k]):
                bad = True
            elif w[k] != 0.0:
                bad = bad or not np.isfinite(mu[k])
                d = th[k] - mu[k]
                Fp = Fp + (w[k] * d) * d
    return float(Fp), bool(bad or not np.isfinite(Fp))


def posterior_system(H, g, theta_acc, weight, mean):
    """Step c.: the system steps 4-6 solve, from the stored (data-only) linearisation."""
    Hp, gp = np.array(H, np.float64, copy=True), np.array(g, np.float64, copy=True)
    w, mu = np.asarray(weight, np.float64), np.asarray(mean, np.float64)
    for k in range(len(w)):
        if w[k] != 0.0:
            Hp[k, k] = Hp[k, k] + w[k]
            gp[k] = gp[k] + 2.0 * w[k] * (theta_acc[k] - mu[k])
    return Hp, gp


def prior_view(theta_acc, weight, mean):
    """The prior as one extra "view" of the normal equations: (diag(p) [N,N], 2 p (theta_acc - mu) [N])."""
    w, mu = np.asarray(weight, np.float64), np.asarray(mean, np.float64)
    with np.errstate(all="ignore"):
        gk = np.where(w != 0.0, 2.0 * w * (np.asarray(theta_acc, np.float64) - np.where(w != 0.0, mu, 0.0)), 0.0)
    return np.diag(w), gk


def _tail(st, H, g, F_data, count, bad, theta_now, weight, mean, ftol, lambda_max):
    """Steps a.-d. and 2-6 on a gathered system; returns the float32 parameters the call leaves in the pointers."""
    have = st.accepted > 0
    prior = weight is not None
    Fp = 0.0
    if prior:
        Fp, pbad = prior_term(weight, mean, theta_now)
        bad = bad or pbad
    st.iterations += 1
    if bad:
        st.reported += 1
        st.last = -1
        return st.theta.astype(np.float32) if have else theta_now
    F = F_data + Fp if prior else F_data
    accept = (not have) or F < st.F_acc
    if accept:
        if have:
            st.rho = (st.F_acc - F) / st.pred
            t = 2.0 * st.rho - 1.0
            st.lam *= max(1.0 / 3.0, 1.0 - t * t * t)
        else:
            st.rho = 0.0
        st.nu = 2.0
        st.F_acc, st.count, st.accepted = F, count, st.accepted + 1
        if prior:
            st.F_prior = Fp
        st.H, st.g, st.theta = H, g, theta_now.astype(np.float64)
    else:
        st.lam *= st.nu
        st.nu *= 2.0
        st.rejected += 1
    st.last, st.F_trial = int(accept), F
    st.Hp, st.gp = posterior_system(st.H, st.g, st.theta, weight, mean) if prior else (st.H, st.g)
    sol, tries = LR.solve(st.Hp, st.gp, st.lam), 0
    while sol is None and tries < LR.MAX_RETRIES:
        st.lam *= st.nu
        st.nu *= 2.0
        tries += 1
        sol = LR.solve(st.Hp, st.gp, st.lam)
    st.retries += tries
    if sol is None:
        st.done, st.why = 1, 4
        return st.theta.astype(np.float32)
    st.delta, st.pred, st.y, st.cond, _ = sol
    small = bool(((st.delta == 0) | (np.abs(st.delta) < LR.spacing_f32(st.theta.astype(np.float32)))).all())
    why = 1 if st.pred <= ftol * st.F_acc else (2 if st.lam >= lambda_max else (3 if small else 0))
    if why:
        st.done, st.why = 1, why
        return st.theta.astype(np.float32)
    return (st.theta + st.delta).astype(np.float32)


def update(st, info, grad, count, loss, theta_now, weight=None, mean=None, ftol=1e-6, lambda_max=1e6, finalize=False):
    """One ``ehr_lm_update_prior``.  st: ``new_state()`` (modified in place); info, grad, count, loss, theta_now:
    ``lm_reference.update``'s; weight, mean [N] float64 (both None: no prior).  Returns the float32 parameters the call leaves
    in the pointers."""
    assert (weight is None) == (mean is None)
    info, grad = np.asarray(info, np.float64), np.asarray(grad, np.float64)
    theta_now = np.asarray(theta_now, np.float32)
    if finalize or st.done:
        return st.theta.astype(np.float32) if st.accepted > 0 else theta_now
    H, g, F = np.zeros(info.shape[1:]), np.zeros(grad.shape[1:]), 0.0
    with np.errstate(all="ignore"):
        for b in range(info.shape[0]):          # view order
            H, g, F = H + info[b], g + grad[b], F + float(np.float32(loss[b]))
    bad = not (np.isfinite(H).all() and np.isfinite(g).all() and np.isfinite(F)) or bool((np.asarray(count) < 0).any())
    return _tail(st, H, g, F, int(np.asarray(count).sum()), bad, theta_now, weight, mean, ftol, lambda_max)


def update_rig(st, cams, theta_now, weight=None, mean=None, ftol=1e-6, lambda_max=1e6, finalize=False):
    """One ``ehr_lm_update_rig_prior``: ``lm_rig_reference.gather``'s head, then the same steps; weight, mean [6 C + F]."""
    assert (weight is None) == (mean is None)
    theta_now = np.asarray(theta_now, np.float32)
    if finalize or st.done:
        return st.theta.astype(np.float32) if st.accepted > 0 else theta_now
    H, g, F, count, bad = RR.gather(cams)
    return _tail(st, H, g, F, count, bad, theta_now, weight, mean, ftol, lambda_max)


# ---- the CPU loop ---------------------------------------------------------------------------------------------------------
def gauge_offset_evaluation(oracle, p, theta, free=(0,)):
    """info [B,N,N], grad [B,N], count [B], loss [B] of the gauge problem ``p`` at theta = (dof[0..5], offset[free]) (float32),
    from information_reference: the float64-built matrix and tangents ``information_of`` uses for a JointPoseStep."""
    from easyhec_amd import information as I
    theta = np.asarray(theta, np.float32)
    dof = torch.as_tensor(theta[:6].copy())
    J = int(p.rb.chain.dof)
    off = np.zeros(J)
    off[list(free)] = theta[6:].astype(np.float64)
    qp = np.zeros((p.q.shape[0], J))
    qp[:, :min(J, p.q.shape[1])] = p.q[:, :J]
    lp = torch.from_numpy(p.rb.link_poses_batch(qp + off[None]))
    K = torch.from_numpy(p.K.astype(np.float32).astype(np.float64))
    tang = torch.cat([I.pose_tangents(K, p.H, p.W, dof, lp), I.joint_tangents(p.rb, p.q, off, list(free), K, p.H, p.W, dof)])
    mvp = I._mvp64(K, p.H, p.W, I._f64(dof), lp, 0.001, 10.0).to(torch.float32).numpy()
    e = IR.information_reference(oracle, p.meshes, mvp, tang.to(torch.float32).numpy(), p.ref)
    return e.info, e.grad, e.count, e.loss.astype(np.float32)


def cpu_lm_prior_loop(oracle, p, evaluations, sigma=SIGMA_OFFSET0, lambda0=1e-3, ftol=1e-6, lambda_max=1e6):
    """``evaluations`` + 1 calls of ``update`` from the problem's start with offset[0] = 0 -> (state, list of (total objective,
    accepted, prior term of the trial) per evaluation, sigma2, weight [7], the accepted parameters)."""
    st = new_state(lambda0)
    theta = np.concatenate([np.asarray(p.dof, np.float32).reshape(6), np.zeros(1, np.float32)])
    N = len(theta)
    mean = np.zeros(N)
    weight, sigma2, traj = None, None, []
    for _ in range(evaluations + 1):
        if st.done:
            break
        info, grad, count, loss = gauge_offset_evaluation(oracle, p, theta)
        if weight is None:                      # sigma2 from the start point, fixed for the solve (InformationReport.sigma2)
            F0 = 0.0
            for x in loss:
                F0 += float(x)
            sigma2 = F0 / max(int(count.sum()) - N, 1)
            weight = np.zeros(N)
            weight[6] = sigma2 / sigma ** 2
        Fp, _ = prior_term(weight, mean, theta)
        theta = update(st, info, grad, count, loss, theta, weight, mean, ftol, lambda_max)
        traj.append((st.F_trial, bool(st.last == 1), Fp))
    return st, traj, sigma2, weight, st.theta.astype(np.float32)
