"""Float64 numpy restatement of ``ehr_lm_update_rig_arrow`` (csrc/ehr_lm.hip, include/ehr.h): the rig's
Levenberg-Marquardt update with per-camera intrinsics on its block-arrow system.  CPU only, not collected by pytest.

The system
----------
Camera c frees ``I_c`` intrinsics (a free set as ``IntrinsicsPoseStep`` takes it; may be empty), ``P_c = 6 + I_c``,
``base_c = P_0 + ... + P_{c-1}``, ``S0 = base_C``, ``N = S0 + F``, in the order

    cam0.dof[0..5], cam0.theta[...], cam1.dof[0..5], cam1.theta[...], ..., offset[free_list[0..F)]

and camera c's local index (``ehr_lm_linearize``'s order: dof, offsets, intrinsics) embeds as ``i < 6 -> base_c + i``,
``6 + f -> S0 + f``, ``6 + F + q -> base_c + 6 + q`` (``embed_index``).  ``gather`` is ``lm_rig_reference.gather`` with that
rule: per camera the sums from 0.0 in view order, the cleared system, every camera ``+=`` in camera order, F and count from 0.0
in camera order; any camera's bad sum reports the call rig-wide.

The solve
---------
``update_rig_arrow`` solves through the DENSE ``lm_reference.solve`` on the assembled [N,N] matrix: it knows nothing of the
arrow structure, so a wrong border, a wrong embedding or a missed Schur term in the kernel shows.  The kernel's block
elimination is the dense right-looking Cholesky in the system's order with the updates by structurally zero blocks left out
(``block_solve`` restates it in numpy for the CPU test), so the bar is ``lm_reference``'s derivation with ``n = N``:

    |y - y_ref| <= max(32, N) * 2^-53 * cond * |y|_inf        |pred - pred_ref| <= max(32, N) * 2^-53 * cond * pred

with cond the condition number of the scaled damped matrix.  Everything else is exact: lambda, nu, F_acc, the counters, the
flags, theta, g, H.  On the CPU, seeds 0..6 and lambda = 1e-3, 1e-5: ``lm_reference.solve`` always succeeds on SHAPES,
cond <= 3.5e4, and ``block_solve`` differs from the dense solve by at most 0.009 of the bar
(tests/test_lm_rig_arrow_reference.py)."""
import numpy as np

import lm_reference as LR
import lm_rig_reference as RR

EPS53 = 2.0 ** -53
ALL4 = ("fx", "fy", "cx", "cy")


def parse_free(free):
    """(free4 [4] of 0/1, tie, I) of one camera's free set (None or (): none)."""
    names = [] if free is None else ([free] if isinstance(free, str) else list(free))
    tie = "f" in names
    free4 = [int(tie or "fx" in names), int(tie or "fy" in names), int("cx" in names), int("cy" in names)]
    return free4, tie, sum(free4) - int(tie)


def layout(frees, F):
    """(P [C], base [C + 1], N) of the system for the cameras' free sets and F free joints."""
    P = [6 + parse_free(fr)[2] for fr in frees]
    base = [0]
    for x in P:
        base.append(base[-1] + x)
    return P, base, base[-1] + F


def embed_index(c, frees, F):
    """Where camera c's local parameters 0 .. 6 + F + I_c - 1 (dof, offsets, intrinsics) live in the rig's system."""
    P, base, _ = layout(frees, F)
    return list(range(base[c], base[c] + 6)) + list(range(base[-1], base[-1] + F)) + list(range(base[c] + 6, base[c] + P[c]))


def names(frees, free_joints):
    out = []
    for c, fr in enumerate(frees):
        free4, tie, _ = parse_free(fr)
        th = (["f"] if tie else [n for n, on in zip(("fx", "fy"), free4[:2]) if on]) + [n for n, on in zip(("cx", "cy"), free4[2:]) if on]
        out += [f"cam{c}.dof[{i}]" for i in range(6)] + [f"cam{c}.theta[{n}]" for n in th]
    return out + [f"offset[{j}]" for j in free_joints]


def gather(cams, frees, F):
    """cams: one ``(info [B_c,Nc,Nc], grad [B_c,Nc], count [B_c], loss [B_c])`` per camera, Nc = 6 + F + I_c ->
    (H [N,N], g [N], F, count, bad), every sum in the stated order."""
    _, _, N = layout(frees, F)
    H, g, Fs, count, bad = np.zeros((N, N)), np.zeros(N), 0.0, 0, False
    with np.errstate(all="ignore"):
        for c, (info, grad, cnt, loss) in enumerate(cams):
            info, grad = np.asarray(info, np.float64), np.asarray(grad, np.float64)
            idx = embed_index(c, frees, F)
            Nc = len(idx)
            assert info.shape[1:] == (Nc, Nc) and grad.shape[1:] == (Nc,)
            S, s, Fc, nc = np.zeros((Nc, Nc)), np.zeros(Nc), 0.0, 0
            for b in range(info.shape[0]):      # view order
                S, s, Fc, nc = S + info[b], s + grad[b], Fc + float(np.float32(loss[b])), nc + int(cnt[b])
            bad = bad or not (np.isfinite(S).all() and np.isfinite(s).all() and np.isfinite(Fc)) or bool((np.asarray(cnt) < 0).any())
            H[np.ix_(idx, idx)] += S            # camera order: the corner gets its C terms one camera at a time
            g[idx] += s
            Fs, count = Fs + Fc, count + nc
        bad = bad or not np.isfinite(Fs)
    return H, g, Fs, count, bad


def update_rig_arrow(st, cams, frees, F, theta_now, ftol=1e-6, lambda_max=1e6, finalize=False, prior=None):
    """One ``ehr_lm_update_rig_arrow``.  st: ``lm_reference.new_state()`` (modified in place; ``st.F_prior`` is added under a
    prior); theta_now [N] float32: the parameters as the pointers hold them, in the system's order; prior: None or
    (weight [N], mean [N]).  Returns the float32 parameters the call leaves in the pointers."""
    theta_now = np.asarray(theta_now, np.float32)
    have = st.accepted > 0
    if finalize or st.done:
        return st.theta.astype(np.float32) if have else theta_now
    H, g, Fv, count, bad = gather(cams, frees, F)
    Fp = 0.0
    if prior is not None:
        w, mu = np.asarray(prior[0], np.float64), np.asarray(prior[1], np.float64)
        bad = bad or not (np.isfinite(w).all() and (w >= 0).all()) or not np.isfinite(mu[w != 0]).all()
        if not bad:
            for k in range(len(w)):             # k ascending from 0.0, p_k == 0 skipped
                if w[k] != 0.0:
                    d = float(theta_now[k]) - mu[k]
                    Fp += (w[k] * d) * d
            bad = not np.isfinite(Fp)
    st.iterations += 1
    if bad:                                     # rig-wide: every pose, every theta and the offsets go back
        st.reported += 1
        st.last = -1
        return st.theta.astype(np.float32) if have else theta_now
    Fv = Fv + Fp if prior is not None else Fv
    accept = (not have) or Fv < st.F_acc
    if accept:
        if have:
            st.rho = (st.F_acc - Fv) / st.pred
            t = 2.0 * st.rho - 1.0
            st.lam *= max(1.0 / 3.0, 1.0 - t * t * t)
        else:
            st.rho = 0.0
        st.nu = 2.0
        st.F_acc, st.count, st.accepted = Fv, count, st.accepted + 1
        st.H, st.g, st.theta = H, g, theta_now.astype(np.float64)
        if prior is not None:
            st.F_prior = Fp
    else:
        st.lam *= st.nu
        st.nu *= 2.0
        st.rejected += 1
    st.last, st.F_trial = int(accept), Fv
    Hs, gs = st.H, st.g
    if prior is not None:                       # the prior joins the system that is solved, never the stored one
        Hs, gs = st.H.copy(), st.g.copy()
        for k in range(len(w)):
            if w[k] != 0.0:
                Hs[k, k] += w[k]
                gs[k] += 2.0 * w[k] * (st.theta[k] - mu[k])
    sol, tries = LR.solve(Hs, gs, st.lam), 0
    while sol is None and tries < LR.MAX_RETRIES:
        st.lam *= st.nu
        st.nu *= 2.0
        tries += 1
        sol = LR.solve(Hs, gs, st.lam)
    st.retries += tries
    if sol is None:
        st.done, st.why = 1, 4
        return st.theta.astype(np.float32)
    st.delta, st.pred, st.y, st.cond, _ = sol
    st.Hs = Hs
    small = bool(((st.delta == 0) | (np.abs(st.delta) < LR.spacing_f32(st.theta.astype(np.float32)))).all())
    why = 1 if st.pred <= ftol * st.F_acc else (2 if st.lam >= lambda_max else (3 if small else 0))
    if why:
        st.done, st.why = 1, why
        return st.theta.astype(np.float32)
    return (st.theta + st.delta).astype(np.float32)


def block_solve(H, g, lam, P, F):
    """The kernel's step 4 in numpy, in its order: per camera ``A_c = L_c L_c^T`` right-looking, ``W_c^T = B_c^T L_c^-T``,
    ``z_c = L_c^-1 r_c``; the corner and its right-hand side lose ``W_c^T W_c`` and ``W_c^T z_c`` camera by camera, row by row;
    the corner's Cholesky, ``y_s``, ``y_c``.  Returns (delta, pred, y) or None where a pivot fails."""
    H, g = np.asarray(H, np.float64), np.asarray(g, np.float64)
    N = H.shape[0]
    S0 = N - F
    d = np.diag(H)
    live = d > 0
    s = np.where(live, 1.0 / np.sqrt(np.where(live, d, 1.0)), 0.0)
    A = (H * s[:, None]) * s[None, :]
    Hs = A.copy()
    A[np.diag_indices(N)] = np.where(live, np.diag(A) + lam, 1.0)
    r = -0.5 * g * s
    y = np.zeros(N)

    def chol_cols(rows_lo, cols):               # right-looking over the columns `cols`, updating rows up to rows_lo's end
        for j in cols:
            if not (A[j, j] > 0 and np.isfinite(A[j, j])):
                return False
            A[j, j] = np.sqrt(A[j, j])
            below = [k for k in cols if k > j] + rows_lo
            for t in below:
                A[t, j] = A[t, j] / A[j, j]
            y[j] = r[j] / A[j, j]
            for t in below:
                for k in [k for k in cols if j < k <= t]:
                    A[t, k] -= A[t, j] * A[k, j]
                if t < S0:
                    r[t] -= A[t, j] * y[j]
        return True

    base = 0
    corner = list(range(S0, N))
    for Pc in P:
        cols = list(range(base, base + Pc))
        if not chol_cols(corner, cols):
            return None
        base += Pc
    base = 0
    for Pc in P:                                # the Schur terms: camera order, then row order
        for k in range(base, base + Pc):
            for f in corner:
                for f2 in corner:
                    if f2 <= f:
                        A[f, f2] -= A[f, k] * A[f2, k]
                r[f] -= A[f, k] * y[k]
        base += Pc
    for j in corner:
        if not (A[j, j] > 0 and np.isfinite(A[j, j])):
            return None
        A[j, j] = np.sqrt(A[j, j])
        for t in range(j + 1, N):
            A[t, j] = A[t, j] / A[j, j]
        for t in range(j + 1, N):
            for k in range(j + 1, t + 1):
                A[t, k] -= A[t, j] * A[k, j]
    for j in corner:
        y[j] = r[j] / A[j, j]
        for t in range(j + 1, N):
            r[t] -= A[t, j] * y[j]
    for j in reversed(corner):
        y[j] = y[j] / A[j, j]
        for t in range(S0, j):
            y[t] -= A[j, t] * y[j]
    base = 0
    for Pc in P:
        for i in range(base, base + Pc):
            for f in reversed(corner):
                y[i] -= A[f, i] * y[f]
        for j in reversed(range(base, base + Pc)):
            y[j] = y[j] / A[j, j]
            for t in range(base, j):
                y[t] -= A[j, t] * y[j]
        base += Pc
    pred = float(y @ (Hs @ y) + 2.0 * lam * (y @ y))
    return y * s, pred, y


def bar(N, cond):
    return max(32, N) * EPS53 * cond


# ---- the update-kernel test's inputs ------------------------------------------------------------------------------------------
FTOL = RR.FTOL
# (C, F, free set per camera, B_c)
SHAPES = [
    (1, 0, [("f",)], [2]),
    (1, 3, [("cx", "cy")], [2]),
    (2, 3, [None, None], [2, 3]),                                   # also fits the dense kernel
    (2, 2, [ALL4, ("f",)], [1, 2]),                                 # ragged blocks
    (3, 7, [("cx", "cy"), None, ALL4], [2, 1, 3]),
    (6, 2, [None] * 6, [1] * 6),                                    # past 32 without intrinsics
    (4, 6, [ALL4] * 4, [1, 2, 1, 2]),
    (16, 22, [ALL4] * 16, [1] * 16),                                # the maximum: N = 182
]
SCRIPT = [("first", 1.0, 1), ("accept", 0.9, 1), ("reject", 1.5, 0), ("nan-loss", 0.8, -1), ("bad-count", 0.8, -1),
          ("zero-diagonal", 0.8, 1), ("zero-intrinsics", 0.75, 1), ("finalize", 0.7, None)]   # (what, loss factor, `last`)


def rig_system(C, F, frees, Bs, seed):
    """One ``lm_multi_reference.system(6 + F + I_c, B_c, seed + 1000 c)`` per camera."""
    import lm_multi_reference as MR
    return [MR.system(6 + F + parse_free(frees[c])[2], Bs[c], seed + 1000 * c) for c in range(C)]


def zeroed_parameter(frees, F):
    """The parameter "zero-diagonal" leaves without information: the last offset (without free joints: the last camera's
    dof[5])."""
    P, base, N = layout(frees, F)
    return N - 1 if F else base[-2] + 5


def zeroed_intrinsics(frees, F):
    """The parameter "zero-intrinsics" leaves without information: camera 0's LAST intrinsics parameter (a camera 0 without
    intrinsics: its dof[4]), and its local index in camera 0's own system."""
    P, base, _ = layout(frees, F)
    if P[0] > 6:
        return P[0] - 1, 6 + F + (P[0] - 6) - 1
    return 4, 4


def scripted_calls(C, F, frees, Bs, seed=0):
    """A list of ``(what, cams)``: call k works on ``rig_system(..., seed + k)`` with every camera's loss scaled by SCRIPT's
    factor and, planted: a NaN in camera 1's loss only (camera 0's where there is one camera), ``count = -1`` in the last
    camera only, for "zero-diagonal" ``zeroed_parameter``'s row, column and gradient entry zeroed in every camera that sees it,
    for "zero-intrinsics" the same for ``zeroed_intrinsics`` in camera 0."""
    base = [cam[3] for cam in rig_system(C, F, frees, Bs, seed)]
    calls = []
    for k, (what, factor, _) in enumerate(SCRIPT):
        cams = [[np.array(x, copy=True) for x in cam] for cam in rig_system(C, F, frees, Bs, seed + k)]
        for c in range(C):
            cams[c][3] = (base[c] * np.float32(factor)).astype(np.float32)
        if what == "nan-loss":
            cams[min(1, C - 1)][3][0] = np.nan
        elif what == "bad-count":
            cams[C - 1][2][Bs[C - 1] - 1] = -1
        elif what == "zero-diagonal":
            for c in (range(C) if F else [C - 1]):
                z = 6 + F - 1 if F else 5
                cams[c][0][:, z, :], cams[c][0][:, :, z], cams[c][1][:, z] = 0.0, 0.0, 0.0
        elif what == "zero-intrinsics":
            z = zeroed_intrinsics(frees, F)[1]
            cams[0][0][:, z, :], cams[0][0][:, :, z], cams[0][1][:, z] = 0.0, 0.0, 0.0
        calls.append((what, [tuple(cam) for cam in cams]))
    return calls


# ---- the CPU loop -------------------------------------------------------------------------------------------------------------
# The end-to-end scene (tests/test_gpu_lm_rig_arrow.py's last test): two ``information_reference.gauge_problem(base=True)``
# cameras at azimuths 60 and 150 degrees, 4 views of 120x160 each; every camera's GIVEN K has its focal lengths scaled off the K
# the masks were rendered with; the poses start from ``p.init``, the free joints [1, 3] from zero.
RIG_AZIMUTHS, RIG_FOCAL_SCALES, RIG_FREE_JOINTS, RIG_EVALUATIONS = (60.0, 150.0), (1.03, 0.98), (1, 3), 8


def rig_problems(oracle, robot):
    """The two cameras' gauge problems and their given (wrong) intrinsics, float32."""
    import information_reference as IR
    ps = [IR.gauge_problem(oracle, robot, phi_deg=phi, base=True) for phi in RIG_AZIMUTHS]
    Ks = []
    for p, s in zip(ps, RIG_FOCAL_SCALES):
        K = np.array(p.K, np.float64)
        K[0, 0], K[1, 1] = K[0, 0] * s, K[1, 1] * s
        Ks.append(K.astype(np.float32))
    return ps, Ks


def rig_evaluation(oracle, p, K0, dof, offsets, theta, free_joints, free):
    """info [B,Nc,Nc], grad [B,Nc], count [B], loss [B] of one camera's own system (dof, offsets, intrinsics) at the float32
    parameters, from information_reference with the tangents of easyhec_amd.information's float64 builders."""
    import torch
    import information_reference as IR
    from easyhec_amd import information as I
    from easyhec_amd.intrinsics_calib import intrinsics_from_theta
    J = int(p.rb.chain.dof)
    qp = np.zeros((p.q.shape[0], J))
    qp[:, :p.q.shape[1]] = p.q
    off = np.asarray(offsets, np.float32).astype(np.float64)
    lp = torch.from_numpy(p.rb.link_poses_batch(qp + off[None]))
    K = torch.from_numpy(intrinsics_from_theta(K0, theta, p.H, p.W).astype(np.float64))
    dof = torch.as_tensor(np.asarray(dof, np.float32))
    tang = [I.pose_tangents(K, p.H, p.W, dof, lp)]
    if len(free_joints):
        tang.append(I.joint_tangents(p.rb, qp, off, list(free_joints), K, p.H, p.W, dof))
    if free:
        tang.append(I.intrinsics_tangents(K0, theta, free, p.H, p.W, dof, lp)[0])
    D = torch.cat(tang).to(torch.float32).numpy()
    mvp = I._mvp64(K, p.H, p.W, I._f64(dof), lp, 0.001, 10.0).to(torch.float32).numpy()
    e = IR.information_reference(oracle, p.meshes, mvp, D, p.ref)
    return e.info, e.grad, e.count, e.loss.astype(np.float32)


def cpu_rig_loop(oracle, ps, K0s, free_joints, frees, evaluations, lambda0=1e-3, ftol=1e-6, lambda_max=1e6):
    """``lm_reference.cpu_lm_loop`` for a rig: ``evaluations`` + 1 calls of ``update_rig_arrow`` from the start (evaluation 0 is
    the start itself) -> (state, list of (loss, accepted) per evaluation, the accepted parameters in the system's order)."""
    C, F = len(ps), len(free_joints)
    P, base, N = layout(frees, F)
    J = int(ps[0].rb.chain.dof)
    parsed = [parse_free(fr) for fr in frees]
    els = [LR.intrinsics_elements(f4, tie) for f4, tie, _ in parsed]
    st = LR.new_state(lambda0)
    theta = np.zeros(N, np.float32)
    for c, p in enumerate(ps):
        theta[base[c]:base[c] + 6] = np.asarray(p.dof, np.float32)
    traj = []
    for _ in range(evaluations + 1):
        if st.done:
            break
        off = np.zeros(J, np.float32)
        off[list(free_joints)] = theta[base[-1]:]
        cams = []
        for c, p in enumerate(ps):
            th4 = np.zeros(4, np.float32)
            for q, e in enumerate(els[c]):
                th4[list(e)] = theta[base[c] + 6 + q]
            cams.append(rig_evaluation(oracle, p, K0s[c], theta[base[c]:base[c] + 6], off, th4, free_joints, frees[c]))
        theta = update_rig_arrow(st, cams, frees, F, theta, ftol, lambda_max)
        traj.append((st.F_trial, bool(st.last == 1)))
    return st, traj, st.theta.astype(np.float32)


# ``cpu_rig_loop`` on ``rig_problems`` with the free joints {1, 3}, lambda_0 = 1e-3, RIG_EVALUATIONS evaluations (float64,
# oracle-driven), 2026-10-20: the summed loss of every evaluation (evaluation 0 is the start) and whether it was accepted, once
# with both cameras' tied focal length freed ("f") and once with both K fixed at the given (wrong) ones, from the same start.
MEASURED = {
    "freed": {
        "evaluations": [(7886.222076416016, True), (7159.735809326172, True), (6537.54833984375, True),
                       (5757.802001953125, True), (4918.867080688477, True), (4290.278648376465, True),
                       (3732.8035430908203, True), (3189.0125465393066, True), (2690.9645233154297, True)],
        "F": 2690.9645233154297,     # the accepted loss after RIG_EVALUATIONS evaluations: what the GPU solve is held against (x 1.5)
    },
    "fixed": {
        "evaluations": [(7886.222076416016, True), (7146.224884033203, True), (6502.94580078125, True),
                       (5767.632080078125, True), (5054.549331665039, True), (4392.724472045898, True),
                       (3817.0846939086914, True), (3404.05525970459, True), (2895.348945617676, True)],
        "F": 2895.348945617676,
    },
}
