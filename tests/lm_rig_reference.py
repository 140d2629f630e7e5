"""Float64 numpy restatement of ``ehr_lm_update_rig`` (csrc/ehr_lm.hip, include/ehr.h): the update of
the Levenberg-Marquardt solve over a camera rig.  CPU only, not collected by pytest.

The head
--------
C cameras share F joint offsets; camera c hands in its own ``info_c [B_c,Nc,Nc]``, ``grad_c [B_c,Nc]``, ``count_c [B_c]``,
``loss_c [B_c]`` with ``Nc = 6 + F``.  The system has ``N = 6 C + F`` parameters in ``rig_information``'s order -- cam0.dof[0..5],
cam1.dof[0..5], ..., the offsets -- and the ORDER of every sum is the contract:

* per camera, in camera order: ``S_c = sum_b info_c[b]``, ``s_c = sum_b grad_c[b]``, ``F_c = sum_b (double) loss_c[b]``,
  ``n_c = sum_b count_c[b]``, each from 0.0 in view order (``lm_reference.update``'s sums);
* H and g are cleared, then every camera is embedded in camera order, each entry ``+=``: local index i < 6 -> 6 c + i, local
  6 + f -> 6 C + f (``embed_index``; ``rig_information``'s ``np.ix_`` rule).  A pose-pose and a pose-offset block has one term,
  the offset-offset block C terms in camera order, the block between two different cameras' poses stays 0.0;
* ``F = F_0 + F_1 + ...``, ``count = n_0 + n_1 + ...`` in camera order, from 0.0;
* bad (the call is REPORTED for the whole rig): any camera's S_c, s_c or F_c, or F, is not finite, or any count is < 0.

With C = 1 every value is ``lm_reference.update``'s: ``0.0 + x`` changes no x that was itself summed from 0.0.

The tail
--------
Accept or reject with Nielsen's schedule, the retries, the stopping rule and the trial ``fl32(theta_acc + delta)`` are
``lm_reference.update``'s, restated here on the gathered system on top of ``lm_reference.solve``, ``spacing_f32`` and
``new_state``; the bars for ``delta`` and ``pred`` are that file's (``32 * 2^-53 * cond``)."""
import numpy as np

import lm_reference as LR


def embed_index(c, C, F):
    """Where camera c's local parameters 0 .. 6 + F - 1 live in the rig's system."""
    return list(range(6 * c, 6 * c + 6)) + list(range(6 * C, 6 * C + F))


def gather(cams):
    """cams: one ``(info [B_c,Nc,Nc], grad [B_c,Nc], count [B_c], loss [B_c])`` per camera -> (H [N,N], g [N], F, count, bad),
    every sum in the order stated above."""
    C = len(cams)
    Nc = np.asarray(cams[0][0]).shape[1]
    F_joints = Nc - 6
    N = 6 * C + F_joints
    H, g, F, count, bad = np.zeros((N, N)), np.zeros(N), 0.0, 0, False
    with np.errstate(all="ignore"):
        for c, (info, grad, cnt, loss) in enumerate(cams):
            info, grad = np.asarray(info, np.float64), np.asarray(grad, np.float64)
            assert info.shape[1:] == (Nc, Nc) and grad.shape[1:] == (Nc,)
            S, s, Fc, nc = np.zeros((Nc, Nc)), np.zeros(Nc), 0.0, 0
            for b in range(info.shape[0]):      # view order
                S, s, Fc, nc = S + info[b], s + grad[b], Fc + float(np.float32(loss[b])), nc + int(cnt[b])
            bad = bad or not (np.isfinite(S).all() and np.isfinite(s).all() and np.isfinite(Fc)) or bool((np.asarray(cnt) < 0).any())
            idx = embed_index(c, C, F_joints)
            H[np.ix_(idx, idx)] += S            # camera order: the offsets' block gets its C terms one camera at a time
            g[idx] += s
            F, count = F + Fc, count + nc
        bad = bad or not np.isfinite(F)
    return H, g, F, count, bad


def update_rig(st, cams, theta_now, ftol=1e-6, lambda_max=1e6, finalize=False):
    """One ``ehr_lm_update_rig``.  st: ``lm_reference.new_state()`` (modified in place); cams: as for :func:`gather`;
    theta_now [6 C + F] float32: the parameters as the pointers hold them.  Returns the float32 parameters the call leaves in
    the pointers (every camera's dof, then the free joints' offsets)."""
    theta_now = np.asarray(theta_now, np.float32)
    have = st.accepted > 0
    if finalize or st.done:
        return st.theta.astype(np.float32) if have else theta_now
    H, g, F, count, bad = gather(cams)
    st.iterations += 1
    if bad:                                     # rig-wide: every pose and the offsets go back to the accepted point
        st.reported += 1
        st.last = -1
        return st.theta.astype(np.float32) if have else theta_now
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
        st.H, st.g, st.theta = H, g, theta_now.astype(np.float64)
    else:
        st.lam *= st.nu
        st.nu *= 2.0
        st.rejected += 1
    st.last, st.F_trial = int(accept), F
    sol, tries = LR.solve(st.H, st.g, st.lam), 0
    while sol is None and tries < LR.MAX_RETRIES:
        st.lam *= st.nu
        st.nu *= 2.0
        tries += 1
        sol = LR.solve(st.H, st.g, st.lam)
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


# The update-kernel test's calls (tests/test_gpu_lm_rig.py), SCRIPTED so that the inputs alone decide what each call does: the
# loss of every camera as a factor of its first loss, and what is planted.  tests/test_lm_rig_reference.py pins it on the CPU.
FTOL = 1e-12   # as tests/test_gpu_lm.py: the synthetic systems' predicted reductions are small next to their losses
SHAPES = [(1, 3, [2]), (2, 0, [2, 3]), (2, 1, [1, 4]), (3, 7, [2, 1, 3]), (4, 7, [1, 1, 1, 1]), (5, 2, [2, 2, 2, 2, 2])]
SCRIPT = [("first", 1.0, 1), ("accept", 0.9, 1), ("reject", 1.5, 0), ("nan-loss", 0.8, -1), ("bad-count", 0.8, -1),
          ("zero-diagonal", 0.8, 1), ("finalize", 0.7, None)]          # (what, loss factor, the `last` flag it leaves)


def scripted_calls(C, F, Bs, seed=0):
    """A list of ``(what, cams)``: call k works on ``rig_system(C, F, Bs, seed + k)`` -- fresh inputs per call -- with every
    camera's loss scaled by SCRIPT's factor and, planted: a NaN in camera 1's loss only (camera 0's where there is one camera),
    ``count = -1`` in the last camera only, and for "zero-diagonal" the LAST offset's row, column and gradient entry zeroed in
    every camera, so that its diagonal entry of the rig's system is exactly 0 (without free joints: the last camera's
    dof[5])."""
    base = [cam[3] for cam in rig_system(C, F, Bs, seed)]
    calls = []
    for k, (what, factor, _) in enumerate(SCRIPT):
        cams = [[np.array(x, copy=True) for x in cam] for cam in rig_system(C, F, Bs, seed + k)]
        for c in range(C):
            cams[c][3] = (base[c] * np.float32(factor)).astype(np.float32)
        if what == "nan-loss":
            cams[min(1, C - 1)][3][0] = np.nan
        elif what == "bad-count":
            cams[C - 1][2][Bs[C - 1] - 1] = -1
        elif what == "zero-diagonal":
            for c in (range(C) if F else [C - 1]):
                z = 6 + F - 1
                cams[c][0][:, z, :], cams[c][0][:, :, z], cams[c][1][:, z] = 0.0, 0.0, 0.0
        calls.append((what, [tuple(cam) for cam in cams]))
    return calls


def zeroed_parameter(C, F):
    """The parameter of the rig's system that "zero-diagonal" leaves without information."""
    return 6 * C + F - 1


def rig_system(C, F, Bs, seed):
    """One ``lm_multi_reference.system(6 + F, B_c, ...)`` per camera: SPD matrices with parameters of different units,
    ``grad = 2 H x`` for a small x, counts and float32 losses.  A list of C tuples, for :func:`gather`."""
    import lm_multi_reference as MR
    return [MR.system(6 + F, Bs[c], seed + 1000 * c) for c in range(C)]
