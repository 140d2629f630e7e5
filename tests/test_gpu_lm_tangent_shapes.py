"""ehr_lm_linearize and ehr_lm_linearize_multi (csrc/ehr_lm.hip) through the C ABI at the shapes and branches the solves'
own cases never reach: 448 and 3 808 matrices (two and fifteen workgroups) from the link poses of tests/link_scenes.py, the
exponential map at and on both sides of its clamp (squared angle 1e-4), prismatic joints with their upstream bit set (the
table of every link reaches the grippers' fingers), every path of lm_intrinsics_element, and P x Bv virtual views.  The
matrix is ehr_pose_forward's bit for bit; the tangents are held to lm_reference.tangent_ratio <= 1 against
lm_reference.tangents (one float32 rounding of the value; three roundings of the scale for the joints); blocks without an
upstream joint are exactly zero; and the GPU tangents go on into ehr_mask_information on 32 links, against the reference
built from the same array.  No tolerance of its own.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import info_scene_cases as C
import information_reference as IR
import joint_reference as JR
import link_scenes as S
import lm_reference as LR
import pose_reference as PR
from test_gpu_information import call
from test_gpu_joint_offsets import _forward, _robot, _table

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NEAR, FAR = 0.001, 10.0


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib
    assert _lib.has_lm() and _lib.has_lm_multi()
    return _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def t32(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def linearize(_lib, dof, K, lp, H, W, joints=None, free4_mask=0, tie=0):
    """ehr_lm_linearize on device tensors -> (mvp [B,L,4,4], dmvp [N,B,L,4,4]) device tensors, filled with NaN before.
    joints: (joint_frames [B,J,6], upstream [L] uint32 bits as int32, joint_kind [J], free_list [F]) device tensors."""
    B, L = lp.shape[:2]
    F = 0 if joints is None else int(joints[3].shape[0])
    J = 0 if joints is None else int(joints[2].shape[0])
    Fi = sum((free4_mask >> i) & 1 for i in range(4)) - (1 if tie else 0)
    N = 6 + F + Fi
    mvp = torch.full((B, L, 4, 4), float("nan"), device=DEV)
    dmvp = torch.full((N, B, L, 4, 4), float("nan"), device=DEV)
    jf, up, jk, fl = joints if joints is not None else (None, None, None, None)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_lm_linearize(
            _lib.ptr(dof), _lib.ptr(K), _lib.ptr(lp), B, L, H, W, ctypes.c_float(NEAR), ctypes.c_float(FAR), _lib.ptr(jf),
            _lib.ptr(up), _lib.ptr(jk), _lib.ptr(fl), F, J, free4_mask, tie, N, _lib.ptr(mvp), _lib.ptr(dmvp), _stream()),
            "ehr_lm_linearize")
    torch.cuda.synchronize()
    return mvp, dmvp


def pose_forward(_lib, dof, K, lp, H, W):
    B, L = lp.shape[:2]
    mvp, tcj = torch.full((B, L, 4, 4), float("nan"), device=DEV), torch.empty((7, 16), device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_pose_forward(_lib.ptr(dof), _lib.ptr(K), _lib.ptr(lp), B, L, H, W, ctypes.c_float(NEAR),
                                               ctypes.c_float(FAR), _lib.ptr(mvp), _lib.ptr(tcj), None, None, 0, _stream()),
                   "ehr_pose_forward")
    torch.cuda.synchronize()
    return mvp


dofs = C.lm_dofs      # identity, w1e-3, below_clamp, above_clamp, w0.3 (tests/test_info_scene_cases.py pins where they lie)


# ---- a. link scenes from the pose -------------------------------------------------------------------------------------------
def _check_pose_tangents(_lib, case, name, dof):
    s = S.scene_of(case)
    K32, lp32 = s.K.astype(np.float32), s.link_poses.astype(np.float32)
    tdof, tK, tlp = t32(dof), t32(K32), t32(lp32)
    mvp, dmvp = linearize(_lib, tdof, tK, tlp, s.H, s.W)
    assert torch.equal(mvp, pose_forward(_lib, tdof, tK, tlp, s.H, s.W)), f"{case} {name}: mvp is not ehr_pose_forward's"
    _, ref, Sabs = LR.tangents(dof, K32, s.H, s.W, NEAR, FAR, lp32)
    assert np.isfinite(ref).all() and ref.shape == (6, s.B, s.L, 4, 4)
    got = dmvp.cpu().numpy()
    assert np.isfinite(got).all()
    r = LR.tangent_ratio(got, ref, Sabs)
    print(f"[lm tangent shapes] {case} {name} ({7 * s.B * s.L} matrices): pose tangents worst |d - ref| / bar = {r:.3f}")
    assert r <= 1.0, (case, name, r)
    return mvp, dmvp


@pytest.mark.parametrize("name", ["identity", "w1e-3", "below_clamp", "above_clamp", "w0.3"])
@pytest.mark.parametrize("case", ["full32", "units513"])
def test_pose_tangents_of_link_scenes(env, case, name):
    _check_pose_tangents(env, case, name, dofs()[name])


@pytest.mark.parametrize("name", ["identity", "w0.3"])
def test_linearize_into_information_at_32_links(env, oracle, name):
    """ehr_lm_linearize's mvp and dmvp on full32's link poses go into mask_information as they are; the result is held
    against information_reference on the downloaded arrays."""
    from easyhec_amd import dr, fused, information as I
    from test_gpu_fused_loss import link_scene
    s = S.scene_of("full32")
    mvp, dmvp = _check_pose_tangents(env, "full32", name, dofs()[name])
    ref = C.expected0(oracle, "full32").ref
    e = IR.information_reference(oracle, s.meshes, mvp.cpu().numpy(), dmvp.cpu().numpy(), ref)
    out = call(I, dr.RasterizeCudaContext(), link_scene(fused, s, DEV), mvp, dmvp, ref, DEV)
    IR.check(out.info, out.grad, out.count, e, f"linearize -> information full32 {name}")
    assert (e.count > 100).all() and (e.S > 0).all()


# ---- b. prismatic joints -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["xarm7", "franka"])
def test_joint_tangents_with_prismatic_joints_upstream(env, robot):
    """The table of EVERY link: the fingers hang behind prismatic joints.  link_poses and joint_frames from ehr_joint_forward
    at seeded joint angles and small non-zero offsets; every active joint is free."""
    _lib = env
    t, rb = _table(robot, True), _robot(robot)
    J, L, B = rb.chain.dof, t["use"].shape[0], 3
    kinds = JR.joint_kinds(t)
    lim = rb.chain.limits()
    rng = np.random.default_rng(77)
    q = rng.uniform(lim[:, 0], lim[:, 1], size=(B, J))
    off = np.where(kinds == 2, rng.uniform(0.001, 0.005, J), rng.uniform(-0.05, 0.05, J)).astype(np.float32)
    free = [j for j in range(J) if kinds[j] in (1, 2)]
    assert any(kinds[j] == 2 for j in free) and 6 + len(free) <= 32
    lp, jf = _forward(t, q, off)
    up = np.asarray(t["upstream"])
    joints = (jf, torch.tensor(up.astype(np.uint32).view(np.int32), device=DEV), torch.tensor(kinds.astype(np.int32), device=DEV),
              torch.tensor(free, dtype=torch.int32, device=DEV))
    K, H, W = PR.SMALL_K, 131, 97
    dof = dofs()["w0.3"]
    tdof, tK = t32(dof), t32(K)
    mvp, dmvp = linearize(_lib, tdof, tK, lp, H, W, joints=joints)
    assert torch.equal(mvp, pose_forward(_lib, tdof, tK, lp, H, W))
    _, lp64, jf64 = JR.fk(t, q, off)
    D, Dabs = JR.pose_derivatives(t, lp64, jf64), JR.pose_derivatives(t, lp64, jf64, absolute=True)
    _, ref, Sabs = LR.tangents(dof, K, H, W, NEAR, FAR, lp.cpu().numpy(), D, Dabs, free)
    got = dmvp.cpu().numpy()
    assert got.shape == ref.shape == (6 + len(free), B, L, 4, 4) and np.isfinite(got).all()
    rp = LR.tangent_ratio(got[:6], ref[:6], Sabs[:6])
    rj = LR.tangent_ratio(got[6:], ref[6:], Sabs[6:], roundings=3)
    zero = [(l, j) for l in range(L) for j in free if not (int(up[l]) >> j) & 1]
    pris = [(l, j) for l in range(L) for j in free if kinds[j] == 2 and (int(up[l]) >> j) & 1]
    rpris = max(LR.tangent_ratio(got[6 + free.index(j), :, l], ref[6 + free.index(j), :, l], Sabs[6 + free.index(j), :, l],
                                 roundings=3) for l, j in pris)
    print(f"[lm tangent shapes] {robot}, every link ({L}), joints {free}: pose tangents worst |d - ref| / bar = {rp:.3f}, joint "
          f"tangents {rj:.3f} (prismatic blocks {pris}: {rpris:.3f}); {len(zero)} (link, joint) blocks exactly zero")
    assert rp <= 1.0 and rj <= 1.0
    for l, j in zero:
        assert (got[6 + free.index(j), :, l] == 0).all(), (l, j)
    assert len(pris) >= 1 and len(zero) >= 1
    for l, j in pris:                                    # the translation column alone, through PF @ Tc: not zero
        assert (np.abs(ref[6 + free.index(j), :, l]).max(axis=(1, 2)) > 0).all() and (got[6 + free.index(j), :, l] != 0).any()


# ---- c. intrinsics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie,mask", [(1, 3), (1, 7), (1, 15), (0, 1), (0, 2), (0, 5), (0, 10), (0, 15)])
def test_intrinsics_tangents_of_every_mask(env, tie, mask):
    _lib = env
    s = S.scene_of("L5")
    K32, lp32 = s.K.astype(np.float32), s.link_poses.astype(np.float32)
    dof = dofs()["w0.3"]
    tdof, tK, tlp = t32(dof), t32(K32), t32(lp32)
    mvp, dmvp = linearize(_lib, tdof, tK, tlp, s.H, s.W, free4_mask=mask, tie=tie)
    assert torch.equal(mvp, pose_forward(_lib, tdof, tK, tlp, s.H, s.W))
    free4 = [(mask >> i) & 1 for i in range(4)]
    _, ref, Sabs = LR.tangents(dof, K32, s.H, s.W, NEAR, FAR, lp32, free4=free4, tie=bool(tie))
    got = dmvp.cpu().numpy()
    assert got.shape == ref.shape and ref.shape[0] == 6 + len(LR.intrinsics_elements(free4, bool(tie))) and np.isfinite(got).all()
    rp, ri = LR.tangent_ratio(got[:6], ref[:6], Sabs[:6]), LR.tangent_ratio(got[6:], ref[6:], Sabs[6:])
    print(f"[lm tangent shapes] L5 intrinsics mask {mask} tie {tie}: pose tangents worst |d - ref| / bar = {rp:.3f}, intrinsics "
          f"tangents {ri:.3f}")
    assert rp <= 1.0 and ri <= 1.0
    assert all((np.abs(ref[k]).max() > 0) for k in range(6, ref.shape[0]))


# ---- d. the multi-start kernel -------------------------------------------------------------------------------------------------
def test_linearize_multi_blocks_are_the_solo_kernel_s_at_32_links(env):
    _lib = env
    s = S.scene_of("full32")
    P, Bv, L = 3, s.B, s.L
    assert Bv == 2
    d = dofs()
    dof = t32(np.stack([d["w0.3"], d["identity"], d["below_clamp"]]))
    tK, tlp = t32(s.K), t32(s.link_poses)
    mvp = torch.full((P * Bv, L, 4, 4), float("nan"), device=DEV)
    dmvp = torch.full((6, P * Bv, L, 4, 4), float("nan"), device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_lm_linearize_multi(_lib.ptr(dof), _lib.ptr(tK), _lib.ptr(tlp), P, Bv, L, s.H, s.W,
                                                     ctypes.c_float(NEAR), ctypes.c_float(FAR), _lib.ptr(mvp), _lib.ptr(dmvp),
                                                     _stream()), "ehr_lm_linearize_multi")
    torch.cuda.synchronize()
    for p in range(P):
        m1, d1 = linearize(_lib, dof[p].contiguous(), tK, tlp, s.H, s.W)
        v = slice(p * Bv, (p + 1) * Bv)
        assert torch.equal(mvp[v], m1), (p, "mvp")
        assert torch.equal(dmvp[:, v], d1), (p, "dmvp")
    assert bool(torch.isfinite(mvp).all()) and bool(torch.isfinite(dmvp).all()) and not torch.equal(mvp[:Bv], mvp[Bv:2 * Bv])
