"""The joint kernels (csrc/ehr_joint.hip: ehr_joint_forward, ehr_joint_forward_multi, ehr_joint_backward_adam,
ehr_rig_backward_adam; the joint branch of ehr_lm_linearize, csrc/ehr_lm.hip) on the synthetic kinematic trees of
tests/joint_table_cases.py: revolute axes with an x component, branches with active joints below them, revolute joints behind
prismatic ones, 32 joints on 64 links with bit 31 of ``upstream`` set, a serial walk of 64 frames, a free list of 26 joints
(6 + 26 = 32 parameters).  tests/test_joint_table_cases.py pins the cases and shows, with deliberately wrong copies of the
reference, that the bars below would catch a kernel that is wrong in any of these.

No tolerance of its own.  link_poses, joint_frames, offset gradients and Adam: the rules of tests/test_gpu_joint_offsets.py;
the rig: tests/test_gpu_rig.py's; the tangents: ``lm_reference.tangent_ratio <= 1`` as in tests/test_gpu_lm_tangent_shapes.py;
the chain on a branched arm: the bars of test_chain_tracks_autograd_through_differentiable_kinematics.  Outputs are filled with
NaN before each call and finite after it.  Every figure is printed before it is asserted; the measured ones are in
profiles/joint_table_shapes.md."""
import ctypes

import numpy as np
import pytest
import torch

import joint_reference as JR
import joint_table_cases as C
import lm_reference as LR
import pose_reference as R
import rig_reference as RR
from test_gpu_fast import problem
from test_gpu_joint_offsets import (QTY, AutogradJointSolve, _adam_errs, _Bwd, _bits, _dev, _dev_table, _forward, _stream,
                                    _views_qpos)
from test_gpu_lm_tangent_shapes import FAR, NEAR, dofs, linearize, pose_forward, t32
from test_gpu_rig import RIG_CAMERAS, RIG_NEAR_FAR, _Cam, _fresh_offsets, _pose_adam, _pose_state, _rig_call

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = R.U
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib
    assert _lib.has_joint_offsets() and _lib.has_rig() and _lib.has_lm() and _lib.has_lm_multi_calib()
    return _lib


def _ti(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV)


def _upstream_i32(t):
    return _ti(np.asarray(t["upstream"]).astype(np.uint32).view(np.int32))


def _idle_joints(t, J):
    """Active joints no rendered link hangs from."""
    seen = 0
    for u in t["upstream"]:
        seen |= int(u)
    return np.array([not (seen >> j) & 1 for j in range(J)], dtype=bool)


def _run_bwd(c, red, state=None, hyper=None):
    """tests/test_gpu_joint_offsets.py's ``_run_bwd`` with grad_out filled with NaN before the call: ehr_joint_forward, then one
    ehr_joint_backward_adam -> ((offsets, m, v, step, grad_out), link_poses, joint_frames)."""
    lp, jf = _forward(c["t"], c["q"], c["off"])
    tc_jac = torch.full((7, 16), float("nan"), device=DEV)
    tc_jac[0] = _dev(c["Tc"].reshape(16))
    J = c["J"]
    b = _Bwd(c["t"], *(state if state is not None else (c["off"], np.zeros(J), np.zeros(J), 0)), c["free"])
    b.grad.fill_(float("nan"))
    out = b.step(_dev(c["g"]), tc_jac, _dev(c["K"]), c["H"], c["W"], c["near"], c["far"], lp, jf, _dev(red),
                 hyper or R.hyper32("default"))
    return out, lp.cpu().numpy(), jf.cpu().numpy()


# ---- 1. forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_forward_kinematics_and_joint_frames(env, name):
    t = C.case(name).table
    bad = []
    for B in (1, 5):
        q, off = C.qpos(name, B), C.offsets(name)
        lp, jf = _forward(t, q, off)
        lp2, jf2 = _forward(t, q, off)
        assert torch.equal(lp, lp2) and torch.equal(jf, jf2), "two runs differ"
        lp, jf = lp.cpu().numpy(), jf.cpu().numpy()
        _, lp64, jf64 = JR.fk(t, q, off)
        _, _, jf32 = JR.fk(t, q, off, dtype=F32)
        want = lp64.astype(np.float32)
        d_lp = float((np.abs(lp.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
        s = float(np.abs(jf64).max())
        e32, eh = R.rel_err(jf32, jf64, s), R.rel_err(jf, jf64, s)
        same = float((lp.view(np.uint32) == want.view(np.uint32)).mean())
        print(f"[joint table shapes] {name} B={B}: link_poses worst {d_lp / U:.2f} units ({same:.4f} bit-equal) | "
              f"joint_frames e32 {e32:.2e} hip {eh:.2e} bound {R.bound(e32):.2e}")
        if not (d_lp <= U and eh <= R.bound(e32) and np.isfinite(lp).all() and np.isfinite(jf).all()):
            bad.append((B, d_lp, eh))
    assert not bad, bad


def _forward_multi(_lib, t, q, off):
    """ehr_joint_forward_multi: q [Bv,J], off [P,J] -> (link_poses [P*Bv,L,4,4], joint_frames [P*Bv,J,6]), NaN before."""
    d = _dev_table(t)
    tab = [_lib.ptr(d[k]) for k in ("parent", "origin", "kind", "axis", "qidx", "use")]
    (Bv, J), P = q.shape, off.shape[0]
    N, L = t["parent"].shape[0], t["use"].shape[0]
    lp = torch.full((P * Bv, L, 4, 4), float("nan"), device=DEV)
    jf = torch.full((P * Bv, J, 6), float("nan"), device=DEV)
    qd, od = _dev(q.astype(np.float64)), _dev(off.astype(np.float32))
    _lib.check(_lib.lib().ehr_joint_forward_multi(*tab, N, J, L, _lib.ptr(qd), _lib.ptr(od), P, Bv, _lib.ptr(lp), _lib.ptr(jf),
                                                  _stream()), "ehr_joint_forward_multi")
    torch.cuda.synchronize()
    return lp, jf


@pytest.mark.parametrize("name", ["tree", "full"])
def test_multi_start_views_are_the_solo_kernel_s_rows(env, name):
    t = C.case(name).table
    P, Bv = 3, 2
    q = C.qpos(name, Bv)
    off = np.stack([C.offsets(name, seed=p) for p in range(P)])
    lp, jf = _forward_multi(env, t, q, off)
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(jf).all())
    for p in range(P):
        lp1, jf1 = _forward(t, q, off[p])
        for j in range(Bv):
            assert torch.equal(lp[p * Bv + j], lp1[j]), (p, j, "link_poses")
            assert torch.equal(jf[p * Bv + j], jf1[j]), (p, j, "joint_frames")
    assert not torch.equal(lp[:Bv], lp[Bv:2 * Bv]) and not torch.equal(lp[Bv:2 * Bv], lp[2 * Bv:])


# ---- 2. the offset gradient -----------------------------------------------------------------------------------------------------
GRAD_B = {name: (1, 5) for name in C.NAMES}
GRAD_B["full"] = (1, 5, 9)      # 9 views x 32 links = 288 pairs: one full tile of 256 and a partial one


@pytest.mark.parametrize("pattern", ["all", "frozen"])
@pytest.mark.parametrize("name", C.NAMES)
def test_offset_gradient_against_the_float64_reference(env, name, pattern):
    bad = []
    for B in GRAD_B[name]:
        e32, eh = 0.0, 0.0
        for draw in range(2):
            c = C.bwd_case(name, B, draw, pattern)
            red = np.array([1, 2, 3, 4, 5, 6, 7, 1], np.float32)      # red[7] = 1: grad_out is the sum itself
            (p, m, v, step, grad), lp, jf = _run_bwd(c, red)
            (_, _, _, _, grad2), _, _ = _run_bwd(c, red)
            assert np.array_equal(_bits(grad), _bits(grad2)), "two runs differ"
            args = (c["t"], c["g"], c["Tc"], c["K"], c["H"], c["W"], c["near"], c["far"], lp, jf)
            s64, scale = JR.offset_gradient(*args)
            s32, _ = JR.offset_gradient(*args, dtype=F32)
            fr = c["free"].astype(bool)
            assert step == 1 and np.isfinite(grad).all() and np.isfinite(lp).all() and np.isfinite(jf).all()
            assert (grad[~fr] == 0).all() and not np.signbit(grad[~fr]).any(), grad      # exactly +0 where not free
            idle = _idle_joints(c["t"], c["J"])
            assert (scale[idle] == 0).all() and (grad[idle] == 0).all()                  # nothing rendered hangs from the joint
            live = fr & (scale > 0)
            assert live.any() == (fr & ~idle).any() and (grad[fr & ~live] == 0).all()
            if live.any():
                assert (np.abs(s64[live]) > 0).any()
                e32 = max(e32, R.rel_err(s32[live], s64[live], scale[live]))
                eh = max(eh, R.rel_err(grad[live], s64[live], scale[live]))
        print(f"[joint table shapes] {name} {pattern} B={B}: offset gradient e32 {e32:.2e} hip {eh:.2e} bound {R.bound(e32):.2e}")
        if not eh <= R.bound(e32):
            bad.append((B, e32, eh))
    assert not bad, bad
    if name == "full":
        assert C.bwd_case(name, 9, 0, pattern)["g"].shape[:2] == (9, 32) and (pattern == "all" or C.free_mask(name, pattern)[31] == 0)


# ---- 3. Adam on 32 joints --------------------------------------------------------------------------------------------------------
def _moments(J, t0, seed):
    rng = np.random.default_rng(seed)
    return ((rng.normal(size=J) * 10 * (t0 > 0)).astype(np.float32), (rng.uniform(1, 400, size=J) * (t0 > 0)).astype(np.float32))


def test_adam_one_step_on_32_joints(env):
    """The rule of test_adam_one_step_from_a_given_state on ``full``: the reference is given the kernel's own grad_out."""
    bad = []
    for hname in R.ADAM_HYPER:
        h = R.hyper32(hname)
        for t0 in (9, 999):
            e32, eh = dict.fromkeys(QTY, 0.0), dict.fromkeys(QTY, 0.0)
            for draw in range(2):
                c = C.bwd_case("full", 3, draw, "frozen")
                J, fr = c["J"], c["free"].astype(bool)
                assert J == 32 and fr[30] and not fr[31]
                m0, v0 = _moments(J, t0, 100 * t0 + draw)
                red = np.array([0, 0, 0, 0, 0, 0, 5, 1], np.float32)
                got, _, _ = _run_bwd(c, red, state=(c["off"], m0, v0, t0), hyper=h)
                assert got[3] == t0 + 1 and all(np.isfinite(x).all() for x in (got[0], got[1], got[2], got[4]))
                r64 = JR.adam_step(c["off"], m0, v0, t0, got[4], red, fr, *h)
                r32 = JR.adam_step(c["off"], m0, v0, t0, got[4], red, fr, *h, dtype=F32)
                assert np.array_equal(_bits(got[4][fr]), _bits(r64[4][fr]))
                for qi, x0 in enumerate((c["off"], m0, v0)):   # a joint that is not free keeps its bits
                    assert np.array_equal(_bits(got[qi][~fr]), _bits(x0[~fr]))
                _adam_errs(r32, r64, e32, fr)
                _adam_errs(got, r64, eh, fr)
            for q in QTY:
                ok = eh[q] <= R.bound(e32[q])
                print(f"[joint table shapes] full adam one step {hname} t0={t0} {q}: e32 {e32[q]:.2e} hip {eh[q]:.2e} bound "
                      f"{R.bound(e32[q]):.2e} {'ok' if ok else 'FAIL'}")
                if not ok:
                    bad.append((hname, t0, q, e32[q], eh[q]))
    assert not bad, bad


@pytest.mark.parametrize("slot,value", [(0, float("nan")), (6, float("inf")), (7, float("-inf")), (3, 3.1e38)])
def test_non_finite_red_leaves_all_32_offsets_alone(env, slot, value):
    c = C.bwd_case("full", 3, 1)
    J, fr = c["J"], c["free"].astype(bool)
    assert J == 32 and fr.all()
    m0, v0 = _moments(J, 9, 5)
    red = np.array([1, 2, 3, 4, 5, 6, 7, 3], np.float32)
    clean, _, _ = _run_bwd(c, red, state=(c["off"], m0, v0, 9))
    live = ~_idle_joints(c["t"], J)
    assert clean[3] == 10 and (_bits(clean[0][live]) != _bits(c["off"][live])).all()        # every joint with a rendered link moves
    red[slot] = np.float32(value)
    got, _, _ = _run_bwd(c, red, state=(c["off"], m0, v0, 9))
    assert np.array_equal(_bits(got[0]), _bits(c["off"])) and np.array_equal(_bits(got[1]), _bits(m0))
    assert np.array_equal(_bits(got[2]), _bits(v0)) and got[3] == 9
    assert np.isnan(got[4]).all()


# ---- 4. the rig ------------------------------------------------------------------------------------------------------------------
RIG_B = (1, 4, 9)
RIG_N = (2.0, 25.0, 5.0)     # red_c[7]; their sum is 32: an exact quotient


def _nan_grad(b):
    b.grad.fill_(float("nan"))
    return b


def _rig_cameras(name, pattern):
    cams = []
    for k, B in enumerate(RIG_B):
        c = C.bwd_case(name, B, k, pattern)
        c["off"] = C.offsets(name)                                   # one arm: every camera walks the same offsets
        (c["K"], c["H"], c["W"]), (c["near"], c["far"]) = RIG_CAMERAS[k], RIG_NEAR_FAR[k]
        rng = np.random.default_rng(40 + k)
        red = np.concatenate([rng.normal(size=6) * 1e3, [rng.uniform(10, 1e4), RIG_N[k]]]).astype(np.float32)
        cams.append(_Cam(c, red, _pose_state(rng, 3 + k)))
        cams[-1].loss.fill_(float("nan"))
        cams[-1].grad.fill_(float("nan"))
    assert len({(c.c["H"], c.c["W"]) for c in cams}) == 3 and not np.array_equal(cams[0].c["Tc"], cams[1].c["Tc"])
    return cams


@pytest.mark.parametrize("pattern", ["all", "frozen"])
@pytest.mark.parametrize("name", ["tree", "full"])
def test_rig_of_three_cameras_against_the_float64_reference(env, name, pattern):
    cams = _rig_cameras(name, pattern)
    t, fr = cams[0].c["t"], cams[0].c["free"].astype(bool)
    n = float(sum(RIG_N))
    p, m, v, step, grad = _rig_call(cams, _nan_grad(_fresh_offsets(cams)))
    grad2 = _rig_call(_rig_cameras(name, pattern), _nan_grad(_fresh_offsets(cams)))[4]
    assert np.array_equal(_bits(grad), _bits(grad2)), "two runs differ"
    refs = [c.ref() for c in cams]
    assert all(np.isfinite(r["lp"]).all() and np.isfinite(r["jf"]).all() for r in refs)
    T64, scale = RR.rig_sum(t, refs)
    T32, _ = RR.rig_sum(t, refs, dtype=F32)
    assert step == 1 and np.isfinite(grad).all() and all(np.isfinite(x).all() for x in (p, m, v))
    assert (grad[~fr] == 0).all() and not np.signbit(grad[~fr]).any(), grad        # exactly +0 where not free
    idle = _idle_joints(t, len(fr))
    live = fr & (scale > 0)
    assert live.any() and (grad[fr & ~live] == 0).all() and (grad[idle] == 0).all()
    e32 = R.rel_err(T32[live] / np.float32(n), T64[live] / n, scale[live] / n)
    eh = R.rel_err(grad[live], T64[live] / n, scale[live] / n)
    print(f"[joint table shapes] {name} {pattern} rig of 3 cameras, B {RIG_B}: offset gradient e32 {e32:.2e} hip {eh:.2e} bound "
          f"{R.bound(e32):.2e}")
    assert eh <= R.bound(e32)
    per = RR.camera_sums(t, refs)                                    # every camera contributes
    assert all(np.abs(s[live]).max() > 0 for s, _ in per)
    for c in cams:                                                   # every camera's pose took ehr_pose_adam's step on its own red
        want, got = _pose_adam(c), c.pose()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want))


# ---- 5. the tangents of the Levenberg-Marquardt solve ----------------------------------------------------------------------------
LM_FREE = {"prismatic_mid": list(range(6)), "tree": list(range(8)),
           "full": [j for j in range(32) if j not in (3, 8, 13, 18, 23, 28)]}      # 26 joints: 6 + 26 = 32 parameters


def _joints_below(name):
    """{prismatic joint j: [revolute joints r on a link below the link j moves]}, from the table of every link."""
    c = C.case(name)
    every = c.chain.joint_table(range(len(c.chain.link_order)))
    kinds = JR.joint_kinds(every)
    out = {}
    for i, r in enumerate(every["qidx"]):
        if r >= 0 and kinds[r] == 1:
            for j in range(len(kinds)):
                if kinds[j] == 2 and (int(every["upstream"][i]) >> j) & 1:
                    out.setdefault(j, []).append(int(r))
    return out


@pytest.mark.parametrize("name", ["prismatic_mid", "tree", "full"])
def test_joint_tangents(env, name):
    _lib = env
    t = C.case(name).table
    J, L, B = C.case(name).chain.dof, t["use"].shape[0], 3
    kinds = JR.joint_kinds(t)
    free = LM_FREE[name]
    assert 6 + len(free) <= 32 and {int(kinds[j]) for j in free} == {1, 2}
    if name == "full":
        assert len(free) == 26 and 0 in free and 31 in free
    q, off = C.qpos(name, B), C.offsets(name)
    lp, jf = _forward(t, q, off)
    up = np.asarray(t["upstream"])
    joints = (jf, _upstream_i32(t), _ti(kinds), _ti(free))
    K, H, W = R.SMALL_K, 131, 97
    dof = dofs()["w0.3"]
    tdof, tK = t32(dof), t32(K)
    mvp, dmvp = linearize(_lib, tdof, tK, lp, H, W, joints=joints)
    assert torch.equal(mvp, pose_forward(_lib, tdof, tK, lp, H, W)), "mvp is not ehr_pose_forward's"
    _, lp64, jf64 = JR.fk(t, q, off)
    D, Dabs = JR.pose_derivatives(t, lp64, jf64), JR.pose_derivatives(t, lp64, jf64, absolute=True)
    _, ref, Sabs = LR.tangents(dof, K, H, W, NEAR, FAR, lp.cpu().numpy(), D, Dabs, free)
    got = dmvp.cpu().numpy()
    assert got.shape == ref.shape == (6 + len(free), B, L, 4, 4) and np.isfinite(got).all() and bool(torch.isfinite(mvp).all())
    row = lambda j: 6 + free.index(j)
    rp = LR.tangent_ratio(got[:6], ref[:6], Sabs[:6])
    rj = LR.tangent_ratio(got[6:], ref[6:], Sabs[6:], roundings=3)
    zero = [(l, j) for l in range(L) for j in free if not (int(up[l]) >> j) & 1]
    below = _joints_below(name)
    pris = [(l, j) for l in range(L) for j in free
            if kinds[j] == 2 and (int(up[l]) >> j) & 1 and any((int(up[l]) >> r) & 1 for r in below.get(j, []))]
    rpris = max(LR.tangent_ratio(got[row(j), :, l], ref[row(j), :, l], Sabs[row(j), :, l], roundings=3) for l, j in pris)
    print(f"[joint table shapes] {name} ({L} links, {len(free)} free joints): pose tangents worst |d - ref| / bar = {rp:.3f}, joint "
          f"tangents {rj:.3f}; {len(pris)} blocks of a prismatic joint with revolute joints downstream: {rpris:.3f}; {len(zero)} "
          f"(link, joint) blocks exactly zero")
    assert rp <= 1.0 and rj <= 1.0 and rpris <= 1.0
    assert len(pris) >= 1 and len(zero) >= 1
    for l, j in zero:
        assert (got[row(j), :, l] == 0).all(), (l, j)
    for l, j in pris:
        assert (np.abs(ref[row(j), :, l]).max(axis=(1, 2)) > 0).all() and (got[row(j), :, l] != 0).any()
    if name == "full":
        assert (np.abs(got[row(31)]).max() > 0) and (np.abs(got[row(0)]).max() > 0)

    # the multi-start kernel: P x Bv virtual views, every hypothesis its own pose, K and offsets
    P, Bv = 2, 2
    d = dofs()
    qv = C.qpos(name, Bv)
    offs = np.stack([C.offsets(name, seed=p) for p in range(P)])
    lpm, jfm = _forward_multi(_lib, t, qv, offs)
    dofm = t32(np.stack([d["w0.3"], d["w1e-3"]]))
    Km = np.stack([K, K]).astype(np.float32)
    Km[1, 0, 0] *= 1.01
    Km[1, 1, 2] += 1.0
    Km = t32(Km)
    N = 6 + len(free)
    mvpm = torch.full((P * Bv, L, 4, 4), float("nan"), device=DEV)
    dmvpm = torch.full((N, P * Bv, L, 4, 4), float("nan"), device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_lm_linearize_multi_calib(
            _lib.ptr(dofm), _lib.ptr(Km), _lib.ptr(lpm), P, Bv, L, H, W, ctypes.c_float(NEAR), ctypes.c_float(FAR), _lib.ptr(jfm),
            _lib.ptr(joints[1]), _lib.ptr(joints[2]), _lib.ptr(joints[3]), len(free), J, 0, 0, N, _lib.ptr(mvpm), _lib.ptr(dmvpm),
            _stream()), "ehr_lm_linearize_multi_calib")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mvpm).all()) and bool(torch.isfinite(dmvpm).all())
    for p in range(P):
        v = slice(p * Bv, (p + 1) * Bv)
        m1, d1 = linearize(_lib, dofm[p].contiguous(), Km[p].contiguous(), lpm[v].contiguous(), H, W,
                           joints=(jfm[v].contiguous(),) + joints[1:])
        assert torch.equal(mvpm[v], m1), (p, "mvp")
        assert torch.equal(dmvpm[:, v], d1), (p, "dmvp")
    assert not torch.equal(mvpm[:Bv], mvpm[Bv:])


# ---- 6. the chain on a branched arm ----------------------------------------------------------------------------------------------
CHAIN_SCALE = 0.25                       # of the 1280x720 intrinsics, recentred: the boxes are about 16 pixels across at 120x160
CHAIN_FREE = [0, 1, 2, 3, 5, 6, 7]       # every joint a rendered link hangs from (joint 4 moves nothing that is rendered)


def chain_rows(scale=CHAIN_SCALE, free=CHAIN_FREE, steps=12):
    """JointPoseStep against AutogradJointSolve on the branched arm: per step (loss a, loss j, max |d dof|, max |d offsets|),
    and the two steppers."""
    from easyhec_amd.joint_calib import JointPoseStep
    rb = C.tree_robot()
    cfg, make, batch = problem(rb, 2, 120, 160, scale)
    qp = _views_qpos(rb, 2)
    table = rb.joint_table()
    ma, mj = make(), make()
    ref = AutogradJointSolve(ma, batch, table, qp, free)
    js = JointPoseStep(mj, batch, rb, qp, free=free)
    rows = []
    for it in range(steps):
        la, lj = float(ref.step()), float(js.step())
        rows.append((la, lj, float((ma.dof.detach() - mj.dof.detach()).abs().max()),
                     float((ref.offsets.detach() - js.offsets).abs().max()), float(js.offsets.abs().max())))
    return rows, ref, js, batch


def test_chain_on_a_branched_arm_tracks_autograd(env):
    """The branched ``tree`` arm with one box of 12 triangles per rendered link, 2 views of 120x160, 12 steps; the scene: the
    camera of test_gpu_fast.problem at a quarter of the 1280x720 intrinsics sees every branch, and every joint with a rendered
    link below it is free."""
    rows, ref, js, batch = chain_rows()
    assert float(batch["mask"].sum()) > 200 and js.free_joints == CHAIN_FREE and js.J == 8 and js.L == 7
    moved = 0.0
    for it, (la, lj, d_dof, d_off, size) in enumerate(rows):
        moved = max(moved, size)
        print(f"[joint table shapes] tree chain step {it}: loss {la:.4f} / {lj:.4f} | max |d dof| {d_dof:.2e} | max |d offsets| {d_off:.2e}")
    for it, (la, lj, d_dof, d_off, size) in enumerate(rows):
        bar = 5e-5 if it < 3 else 1e-2
        assert np.isfinite([la, lj]).all() and d_dof <= bar and d_off <= bar, (it, d_dof, d_off)
    assert moved > 1e-3 and float(js.offsets[4]) == 0.0
    assert int(js.offset_step_t) == 12 and int(js.step_t) == 12
    assert float(js.offset_grad[4]) == 0.0 and bool((js.offset_grad[CHAIN_FREE].abs() > 0).all())
