"""ehr_mask_information (vb_info_kernel, csrc/ehr_vbuf.hip) and easyhec_amd/information.py on the GPU: parity with the float64
reference of tests/information_reference.py under its derived per-entry bars, consistency with ehr_render_mask_loss, the exact
algebra of the op (symmetry, scaling, permutation, determinism), views and chunks, weights, spilled pairs, non-interference
with a running solve, the reports of the gauge scenes and the refusals.  tests/test_information_reference.py pins the
reference and the scenes on the CPU.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import fused_loss_reference as R
import information_reference as IR
import weighted_loss_reference as WR
from test_gpu_fast import problem

pytestmark = pytest.mark.gpu

KEYS = [("xarm7",) + shape for shape in R.SOFT_SHAPES] + [("ties",)]
KEY_IDS = ["120x160", "100x150", "ties"]
U = IR.U


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused, information
    return fused, information, dr, torch.device("cuda:0")


def link_scene(fused, meshes, dev):
    return fused.LinkScene([v for v, _ in meshes], [f for _, f in meshes], dev)


_SCENES = {}


def scene_of(fused, s, dev):
    if s.name not in _SCENES:
        _SCENES[s.name] = link_scene(fused, s.meshes, dev)
    return _SCENES[s.name]


def call(I, ctx, scene, mvp, D, ref, dev, weight=None, want_loss=False, want_grad_mvp=False, check=True):
    """mask_information on host arrays (device tensors are passed on as they are) -> namespace of numpy arrays."""
    from easyhec_amd import fused
    t = lambda a: a if torch.is_tensor(a) or a is None else torch.tensor(np.ascontiguousarray(a), device=dev)
    out = I.mask_information(ctx, scene, t(mvp), t(D), t(ref), weight=t(weight), want_loss=want_loss, want_grad_mvp=want_grad_mvp)
    torch.cuda.synchronize()
    if check:
        fused.check_status(ctx)
    out.info, out.grad, out.count = out.info.cpu().numpy(), out.grad.cpu().numpy(), out.count.cpu().numpy()
    out.loss = None if out.loss is None else out.loss.cpu().numpy()
    out.grad_mvp = None if out.grad_mvp is None else out.grad_mvp.cpu().numpy()
    return out


def same(a, b):
    return (a.info == b.info).all() and (a.grad == b.grad).all() and (a.count == b.count).all()


# ---- 1. parity with the reference ----------------------------------------------------------------------------------------
# (the tie scene has no unperturbed pose to render "own_aa" from: its references are fused_loss_reference.TIE_REFS)
CASES = [(k, kind) for k in KEYS[:2] for kind in ("uniform", "own_aa")] + [(KEYS[2], kind) for kind in ("uniform", "binary")]


@pytest.mark.parametrize("N", [6, 1, 17, 32])
@pytest.mark.parametrize("key,kind", CASES, ids=[f"{KEY_IDS[KEYS.index(k)]}-{kind}" for k, kind in CASES])
def test_parity_with_the_reference(env, oracle, xarm7, key, kind, N):
    """count exact (on the tie scene under tangents its abutting links share: between the reference's lower and upper count,
    see information_reference.information_reference); every info and grad entry within its derived bar (2 C_J u S, (C_J + 1) u Sg); entries without scale
    exactly zero (the tie scene's depth tangents)."""
    fused, I, dr, dev = env
    e0 = R.expected_for(oracle, xarm7, key, kind)
    D, _, e = IR.expected_for(oracle, xarm7, key, kind, N)
    out = call(I, dr.RasterizeCudaContext(), scene_of(fused, e0.s, dev), e0.s.mvp, D, e0.ref, dev)
    IR.check(out.info, out.grad, out.count, e, f"parity {e0.s.name} {kind} N={N}")
    assert e.count.sum() > 0 and (e.S > 0).any()


# ---- 2. consistency with the existing op ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS[:2], ids=KEY_IDS[:2])
def test_consistent_with_render_mask_loss(env, oracle, xarm7, key):
    """loss and grad_mvp of the call are render_mask_loss's bit for bit; grad[b,k] = sum_l <grad_mvp[b,l], dmvp[k,b,l]> within
    the two float32 budgets (the composite stage's block bar contracted with |dmvp|, plus the information op's own)."""
    fused, I, dr, dev = env
    from test_gpu_fused import run
    e0 = R.expected_for(oracle, xarm7, key, "uniform")
    D, _, e = IR.expected_for(oracle, xarm7, key, "uniform", 17)
    scene = scene_of(fused, e0.s, dev)
    out = call(I, dr.RasterizeCudaContext(), scene, e0.s.mvp, D, e0.ref, dev, want_loss=True, want_grad_mvp=True)
    _, loss, gm = run(fused, dr.RasterizeCudaContext(), scene, e0.s.mvp, e0.ref, dev)
    assert (out.loss == loss).all() and (out.grad_mvp == gm).all()
    D64 = D.astype(np.float64)
    g2 = np.einsum("blrc,kblrc->bk", gm.astype(np.float64), D64)
    bar = np.einsum("bl,kbl->bk", R.block_bar(e0.c.A), np.abs(D64).sum(axis=(3, 4))) + IR.grad_bar(e.Sg, e.L)
    d = np.abs(out.grad - g2)
    print(f"[info vs grad_mvp] {e0.s.name}: worst |grad - <grad_mvp, dmvp>| / bar = {(d / bar).max():.4f}")
    assert (d <= bar).all()


# ---- 3. exact algebra ------------------------------------------------------------------------------------------------------
def test_exact_algebra(env, oracle, xarm7):
    fused, I, dr, dev = env
    key = KEYS[0]
    e0 = R.expected_for(oracle, xarm7, key, "uniform")
    D, _, e = IR.expected_for(oracle, xarm7, key, "uniform", 17)
    scene, ctx = scene_of(fused, e0.s, dev), dr.RasterizeCudaContext()
    a = call(I, ctx, scene, e0.s.mvp, D, e0.ref, dev)
    # symmetric, diagonal >= 0, smallest eigenvalue >= -bar
    assert (a.info == a.info.transpose(0, 2, 1)).all()
    assert (np.diagonal(a.info, axis1=1, axis2=2) >= 0).all()
    for b in range(a.info.shape[0]):
        lo, bar = np.linalg.eigvalsh(a.info[b])[0], np.linalg.norm(IR.info_bar(e.S[b], e.L))
        print(f"[info psd] view {b}: smallest eigenvalue {lo:.3e}, bar {bar:.3e}")
        assert lo >= -bar
    # a zero tangent: an exactly zero row and column; the others untouched
    Dz = D.copy()
    Dz[3] = 0
    z = call(I, ctx, scene, e0.s.mvp, Dz, e0.ref, dev)
    assert (z.info[:, 3] == 0).all() and (z.info[:, :, 3] == 0).all() and (z.grad[:, 3] == 0).all()
    keep = [k for k in range(17) if k != 3]
    assert (z.info[:, keep][:, :, keep] == a.info[:, keep][:, :, keep]).all() and (z.grad[:, keep] == a.grad[:, keep]).all()
    # doubling one tangent doubles its row and column and quadruples the diagonal entry, bit for bit
    D2 = D.copy()
    D2[5] *= 2
    d = call(I, ctx, scene, e0.s.mvp, D2, e0.ref, dev)
    want = a.info.copy()
    want[:, 5] *= 2
    want[:, :, 5] *= 2
    assert (d.info == want).all() and (d.grad[:, 5] == 2 * a.grad[:, 5]).all() and (d.count == a.count).all()
    # permuting the parameters permutes the outputs
    perm = np.random.default_rng(0).permutation(17)
    p = call(I, ctx, scene, e0.s.mvp, D[perm], e0.ref, dev)
    assert (p.info == a.info[:, perm][:, :, perm]).all() and (p.grad == a.grad[:, perm]).all() and (p.count == a.count).all()
    # two calls, and two contexts
    assert same(a, call(I, ctx, scene, e0.s.mvp, D, e0.ref, dev))
    assert same(a, call(I, dr.RasterizeCudaContext(), scene, e0.s.mvp, D, e0.ref, dev))


# ---- 4. views and chunks -------------------------------------------------------------------------------------------------
def test_every_view_equals_its_single_view_call(env, oracle, xarm7):
    fused, I, dr, dev = env
    key = KEYS[1]
    e0 = R.expected_for(oracle, xarm7, key, "uniform")
    D, _, _ = IR.expected_for(oracle, xarm7, key, "uniform", 6)
    scene = scene_of(fused, e0.s, dev)
    a = call(I, dr.RasterizeCudaContext(), scene, e0.s.mvp, D, e0.ref, dev, want_loss=True)
    one = dr.RasterizeCudaContext()
    for b in range(e0.s.B):
        s = call(I, one, scene, e0.s.mvp[b:b + 1], D[:, b:b + 1], e0.ref[b:b + 1], dev, want_loss=True)
        assert (s.info[0] == a.info[b]).all() and (s.grad[0] == a.grad[b]).all() and s.count[0] == a.count[b]
        assert s.loss[0] == a.loss[b]


def test_many_views_go_through_in_chunks(env, xarm7):
    """70 views x 8 links = 560 (view, link) units: two chunks (64 + 6), the shape of test_gpu_fused.py's chunk test.  The
    slots of the first chunk are read before the second overwrites them: every view equals its view in a single-chunk call."""
    fused, I, dr, dev = env
    from test_gpu_fused import workload
    B, H, W, scale = 70, 96, 128, 0.1
    K, lp, Tc, mvp = workload(xarm7, H, W, scale, B, seed=11)
    rng = np.random.default_rng(11)
    ref = (rng.uniform(size=(B, H, W)) > 0.8).astype(np.float32)
    D = (rng.normal(size=(6,) + mvp.shape) * np.abs(mvp).max()).astype(np.float32)
    scene = link_scene(fused, xarm7.meshes, dev)
    a = call(I, dr.RasterizeCudaContext(), scene, mvp, D, ref, dev, want_loss=True)
    assert (a.count > 0).all()                                                   # jobs, and pairs, in every view
    small = dr.RasterizeCudaContext()
    for lo in (0, 30, 60):                                                       # one of them across the chunk border
        sl = slice(lo, lo + 10)
        s = call(I, small, scene, mvp[sl], D[:, sl], ref[sl], dev, want_loss=True)
        assert (s.info == a.info[sl]).all() and (s.grad == a.grad[sl]).all() and (s.count == a.count[sl]).all()
        assert (s.loss == a.loss[sl]).all()


# ---- 5. weights ------------------------------------------------------------------------------------------------------------
def test_weights(env, oracle, xarm7):
    fused, I, dr, dev = env
    key = KEYS[0]
    e0 = R.expected_for(oracle, xarm7, key, "uniform")
    D, _, e = IR.expected_for(oracle, xarm7, key, "uniform", 6)
    scene, ctx = scene_of(fused, e0.s, dev), dr.RasterizeCudaContext()
    a = call(I, ctx, scene, e0.s.mvp, D, e0.ref, dev, want_loss=True)
    ones = call(I, ctx, scene, e0.s.mvp, D, e0.ref, dev, weight=np.ones_like(e0.ref), want_loss=True)
    assert same(a, ones) and (a.loss == ones.loss).all()
    zero = call(I, ctx, scene, e0.s.mvp, D, e0.ref, dev, weight=np.zeros_like(e0.ref))
    assert (zero.info == 0).all() and (zero.grad == 0).all() and (zero.count == 0).all()
    for pattern in ("real", "tiles"):
        Dw, w, ew = IR.expected_for(oracle, xarm7, key, "uniform", 6, weight=pattern)
        if pattern == "tiles":
            assert WR.zeroed_tiles_with_a_job(w, ew.si) > 0
        out = call(I, ctx, scene, e0.s.mvp, Dw, e0.ref, dev, weight=w)
        IR.check(out.info, out.grad, out.count, ew, f"weights {pattern} {e0.s.name}")
    # a bound reference against an unbound one (no weights)
    ctx2 = dr.RasterizeCudaContext()
    tref = torch.tensor(e0.ref, device=dev)
    fused._ensure_plan(ctx2, scene, e0.s.B, e0.s.H, e0.s.W)
    fused.bind_ref(ctx2, scene, tref)
    bound = call(I, ctx2, scene, e0.s.mvp, D, tref, dev, want_loss=True)
    fused.bind_ref(ctx2, scene, None)
    assert same(a, bound) and (a.loss == bound.loss).all()


# ---- 6. spilled pairs and a small pool -----------------------------------------------------------------------------------
def checkerboard():
    """One 32 x 8 tile: link 0 is a checkerboard of pixel-sized quads (the quads of test_gpu_fused.py's overflow scene): four
    blended pairs per covered pixel, 512 in the one job, eight times VB_JOB_ITEMS = 64 -- the rest of the list lives in the spill
    pool.  Link 1 repeats the first eight columns at another depth: there the links' sum passes 1 and the gate is shut."""
    H, W = 8, 32
    meshes = []
    for l, xmax in enumerate((W, 8)):
        v, f = [], []
        for y in range(H):
            for x in range(xmax):
                if (x + y) % 2 == 0:
                    cx, cy = (x + 0.5) / W * 2 - 1, (y + 0.5) / H * 2 - 1
                    hx, hy = 0.6 / W, 0.6 / H
                    n = len(v)
                    v += [[cx - hx, cy - hy, 0], [cx + hx, cy - hy, 0], [cx + hx, cy + hy, 0], [cx - hx, cy + hy, 0]]
                    f += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
        meshes.append((np.array(v, np.float32), np.array(f, np.int32)))
    mvp = np.tile(np.eye(4, dtype=np.float32)[None, None], (1, 2, 1, 1))
    mvp[0, :, 3, 3] = 1.0 + 0.01 * np.arange(2)
    ref = (np.random.default_rng(5).uniform(size=(1, H, W)) > 0.5).astype(np.float32)
    D = np.stack([G @ mvp.astype(np.float64) for G in IR.se3_generators()]).astype(np.float32)
    return meshes, mvp, ref, D


def test_spilled_pairs_and_a_small_pool(env, oracle):
    fused, I, dr, dev = env
    meshes, mvp, ref, D = checkerboard()
    e = IR.information_reference(oracle, meshes, mvp, D, ref)
    scene = link_scene(fused, meshes, dev)
    out = call(I, dr.RasterizeCudaContext(), scene, mvp, D, ref, dev)
    IR.check(out.info, out.grad, out.count, e, "spilled pairs 8x32x2")
    assert e.count[0] > 64
    os.environ["EHR_VB_SPILL_ITEMS"] = "100"              # (read at plan time)
    try:
        ctx = dr.RasterizeCudaContext()
        rep = call(I, ctx, scene, mvp, D, ref, dev, want_loss=True, check=False)
    finally:
        del os.environ["EHR_VB_SPILL_ITEMS"]
    assert np.isnan(rep.info).all() and np.isnan(rep.grad).all() and (rep.count == -1).all() and np.isnan(rep.loss).all()
    with pytest.raises(RuntimeError, match="overflow"):
        fused.check_status(ctx)


# ---- 7. non-interference ---------------------------------------------------------------------------------------------------
def _solve(make, batch, build, graph, probe):
    from easyhec_amd.information import information_of
    model = make()
    st = build(model, batch)
    if graph:
        st.capture()
    rep = None
    for it in range(30):
        st.step()
        if probe and it == 9:
            rep = information_of(st)
    torch.cuda.synchronize()
    state = [model.dof.detach().clone(), st.exp_avg.clone(), st.exp_avg_sq.clone(), st.step_t.clone(), st.hist_row.clone(),
             model.history_ops[:32].clone(), st.loss.clone()]
    if hasattr(st, "offsets"):
        state += [st.offsets.clone(), st.offset_exp_avg.clone(), st.offset_exp_avg_sq.clone(), st.offset_step_t.clone()]
    st.release_graph()
    return state, rep


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_information_of_does_not_disturb_a_solve(xarm7, graph):
    """30 steps of FusedPoseStep with information_of(step) after step 10, eager and from a captured graph: dof, Adam state and
    history_ops bit-equal to 30 steps without the call."""
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 3, 120, 160, 0.125)
    build = lambda m, b: FusedPoseStep(m, b)
    plain, _ = _solve(make, batch, build, graph, False)
    probed, rep = _solve(make, batch, build, graph, True)
    for x, y in zip(plain, probed):
        assert torch.equal(x, y)
    assert rep.names == [f"dof[{i}]" for i in range(6)] and rep.count > 0 and np.isfinite(rep.eigenvalues).all()
    assert int(plain[3]) == 30


def test_information_of_does_not_disturb_a_joint_solve(xarm7):
    from easyhec_amd.joint_calib import JointPoseStep
    from test_gpu_joint_offsets import _views_qpos
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    build = lambda m, b: JointPoseStep(m, b, xarm7, qp)
    plain, _ = _solve(make, batch, build, True, False)
    probed, rep = _solve(make, batch, build, True, True)
    for x, y in zip(plain, probed):
        assert torch.equal(x, y)
    assert rep.names == [f"dof[{i}]" for i in range(6)] + [f"offset[{j}]" for j in range(1, 7)]


# ---- 8. reports ------------------------------------------------------------------------------------------------------------
def _joint_step(p, free, dev):
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.rb_solver import RBSolver
    cfg, batch, qp = IR.gauge_batch(p, dev)
    return JointPoseStep(RBSolver(cfg, meshes=p.rb.meshes).to(dev), batch, p.rb, qp, free=free)


def _against_reference(rep, H_ref, S_ref, L, what):
    """The GPU report's matrix within the per-entry bars, its scaled eigenvalues within the bound they give (Weyl)."""
    from easyhec_amd.information import InformationReport
    bar = IR.info_bar(S_ref, L)
    d = np.abs(rep.H - H_ref)
    ref = InformationReport(H_ref[None], rep.names)
    tol = IR.scaled_tolerance(H_ref, S_ref, L)
    de = np.abs(rep.eigenvalues - ref.eigenvalues).max()
    print(f"[report] {what}: worst |H - H_ref| / bar = {(d[bar > 0] / bar[bar > 0]).max():.4f}; eigenvalues {rep.eigenvalues}; "
          f"reference {ref.eigenvalues}; worst difference {de:.2e}, bound {tol:.2e}")
    assert (d <= bar).all() and de <= tol
    return ref, tol


def test_reports_show_the_first_joint_gauge_and_its_control(env, oracle, xarm7):
    """xArm7 without its base link, one camera, 4 views.  Joint 0 freed: the scaled matrix has ONE eigenvalue that is small
    next to the following one (reference: 4e-16 against 1.3e-2; the kernel's bars allow 2e-4), and its direction is the
    reference's, with offset[0] and a rotation of the pose among its three largest components.  Joint 0 frozen (pose only): no
    eigenvalue is small (reference: consecutive ratios >= 0.12, condition 416)."""
    fused, I, dr, dev = env
    p = IR.gauge_problem(oracle, xarm7)
    _, _, names, e = IR.gauge_reference(oracle, p, [0])
    rep = I.information_of(_joint_step(p, [0], dev))
    assert rep.names == names
    ref, tol = _against_reference(rep, e.info.sum(axis=0), e.S.sum(axis=0), e.L, "joint 0 free")
    assert rep.count == int(e.count.sum())
    assert rep.eigenvalues[0] * 1e3 <= rep.eigenvalues[1]                       # small: a factor 1e3 below the next one
    assert len(rep.weak_directions(1e-3)) == 1
    v, vr = rep.eigenvectors[:, 0], ref.eigenvectors[:, 0]
    sin = np.sqrt(max(0.0, 1.0 - float(v @ vr) ** 2))
    print(f"[report] gauge direction {rep.direction(0)[:4]}; angle to the reference's {sin:.2e}")
    assert sin <= 2.0 * tol / (ref.eigenvalues[1] - ref.eigenvalues[0])          # (Davis-Kahan)
    top = [nm for nm, _ in rep.direction(0)[:3]]
    assert "offset[0]" in top and any(nm in top for nm in ("dof[3]", "dof[4]", "dof[5]"))
    # control
    _, _, names0, e0 = IR.gauge_reference(oracle, p, [])
    rep0 = I.information_of(_joint_step(p, [], dev))
    assert rep0.names == names0
    _against_reference(rep0, e0.info.sum(axis=0), e0.S.sum(axis=0), e0.L, "joint 0 frozen")
    assert rep0.weak_directions(1e-3) == [] and (rep0.eigenvalues[:-1] / rep0.eigenvalues[1:]).min() >= 0.012
    assert rep0.condition <= 4160


def test_rig_information_second_camera_pins_joint_0(env, oracle, xarm7):
    """Two cameras on the whole arm, joint 0 freed.  Camera A frames the base link out: alone it cannot tell joint 0's zero error
    from its own rotation (marginal information of offset[0]: 9e-10 in the reference, zero to rounding).  Camera B, from
    another azimuth, sees the base: in the rig the marginal information is 29.07 (reference), 3e10 times camera A's own.  The
    kernel's float32 J leaves camera A's Schur complement at the size of its entries' rounding, so what is asserted of the GPU
    report is the floor the scenes were chosen for: at least 1e3 times camera A's own."""
    fused, I, dr, dev = env
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.rig_calib import RigJointStep
    pa = IR.gauge_problem(oracle, xarm7, IR.GAUGE_AZIMUTHS[0], base=True, frame_base_out=True)
    pb = IR.gauge_problem(oracle, xarm7, IR.GAUGE_AZIMUTHS[1], base=True)
    ea, eb = IR.gauge_reference(oracle, pa, [0])[3], IR.gauge_reference(oracle, pb, [0])[3]
    models, batches, qps = [], [], []
    for p in (pa, pb):
        cfg, batch, qp = IR.gauge_batch(p, dev)
        models.append(RBSolver(cfg, meshes=p.rb.meshes).to(dev))
        batches.append(batch)
        qps.append(qp)
    rig = RigJointStep(models, batches, xarm7, qps, free=[0])
    rep = I.rig_information(rig)
    assert rep.names == [f"cam{c}.dof[{i}]" for c in range(2) for i in range(6)] + ["offset[0]"]
    Hc, Sc = IR.embed_rig([ea, eb], 1)
    _against_reference(rep, Hc.sum(axis=0), Sc.sum(axis=0), ea.L, "rig of two cameras")
    one = I.information_of(rig.cameras[0])
    _against_reference(one, ea.info.sum(axis=0), ea.S.sum(axis=0), ea.L, "camera A alone")
    ma, mr = one.marginal_information("offset[0]")[0, 0], rep.marginal_information("offset[0]")[0, 0]
    print(f"[report] marginal information of offset[0]: camera A alone {ma:.3e}, rig {mr:.3e}")
    assert mr >= 1e3 * abs(ma) and mr > 1.0


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(env, oracle, xarm7):
    fused, I, dr, dev = env
    key = KEYS[0]
    e0 = R.expected_for(oracle, xarm7, key, "uniform")
    D = IR.tangents_for(xarm7, key, 32)
    scene, ctx = scene_of(fused, e0.s, dev), dr.RasterizeCudaContext()
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    mvp, ref = t(e0.s.mvp), t(e0.ref)
    with pytest.raises(RuntimeError, match="1 <= N <= 32"):
        I.mask_information(ctx, scene, mvp, t(D[:0]), ref)
    with pytest.raises(RuntimeError, match="1 <= N <= 32"):
        I.mask_information(ctx, scene, mvp, t(np.concatenate([D, D[:1]])), ref)
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        I.mask_information(ctx, scene, mvp, torch.tensor(D), ref)
    with pytest.raises(RuntimeError, match=r"dmvp must have shape"):
        I.mask_information(ctx, scene, mvp, t(D[:, :1]), ref)
    # the C entry point refuses a bad N itself, with a message
    from easyhec_amd import _lib
    fused._ensure_plan(ctx, scene, e0.s.B, e0.s.H, e0.s.W)
    out = I._outputs(33, e0.s.B, e0.s.L, dev, False, False)
    with pytest.raises(RuntimeError, match="tangents"):
        I._launch(ctx, scene, mvp, t(np.concatenate([D, D[:1]])), ref, out.info, out.grad, out.count, None, None)
    assert _lib.has_information()
    from easyhec_amd.multistart import MultiStartPoseStep, sample_starts
    from easyhec_amd.synthetic import camera_Tc_c2b
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    ms = MultiStartPoseStep(make(), batch, sample_starts(camera_Tc_c2b(), 2, 0.002, 0.3, seed=2))
    with pytest.raises(ValueError, match="multi-start"):
        I.information_of(ms)
