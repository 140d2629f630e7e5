"""The exploration kernels (csrc/ehr_explore.hip) and easyhec_amd/info_explorer.py on the GPU: the gains against the longdouble
reference of tests/explore_reference.py under its derived bar, the exact properties of the contract (zero matrices, duplicates,
flags, batch independence, determinism), the pick (ties, nothing finite, the update of A bit for bit, greedy selection against
the reference, the chain rule), the explorer's chain on the gauge problem, non-interference with a running solve, the refusals
and the online loop.  tests/test_explore_reference.py pins the reference and the inputs on the CPU.  Every figure is printed
before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import explore_reference as ER
import information_reference as IR
from test_gpu_fast import problem

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
Q = ER.Q_CASE


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, info_explorer
    assert _lib.has_information_gain()
    return _lib, info_explorer


def dev64(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ratio_line(what, g, ref, bars):
    ok = np.isfinite(ref)
    r = np.abs(g[ok] - ref[ok]) / bars[ok]
    print(f"[explore ratio] {what}: worst |gain - ref| / bar = {r.max():.4f} (recorded: {ER.MEASURED.get(what)})")
    return r


# ---- 1. the gain kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ER.VIEWS)
@pytest.mark.parametrize("N", ER.SIZES)
def test_gain_kernel_on_synthetic_matrices(env, N, S):
    _lib, IE = env
    for which in ER.interests(N):
        A, info, interest, ref, bars = ER.expected_gain(N, S, which)
        tA, tinfo = dev64(A), dev64(info)
        g = host(IE.information_gain(tA, tinfo, interest=interest))
        r = ratio_line(f"gain N={N} S={S} {which}", g, ref, bars)
        assert np.isfinite(g).all() and (r <= 1.0).all()
        assert (bits(g[0::4]) == 0).all()                                            # zero H_q: exactly +0.0
        for copy, orig in ER.DUPLICATES:
            assert bits(g[copy]) == bits(g[orig])
        assert (bits(host(IE.information_gain(tA, tinfo, interest=interest))) == bits(g)).all()   # two runs
        # the flags: closed candidates get -inf and their (NaN-filled) matrices are not read; NaN / inf in an open one: NaN
        bad = info.copy()
        valid, taken = np.ones(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
        valid[[3, 64]], taken[[7, 66]] = 0, 1
        bad[[3, 64, 7, 66]] = np.nan
        bad[11, S - 1, N - 1, 0], bad[12, 0, 0, 0] = np.nan, np.inf
        f = host(IE.information_gain(tA, dev64(bad), valid=valid, taken=taken, interest=interest))
        closed, nan = [3, 64, 7, 66], [11, 12]
        assert (f[closed] == -np.inf).all() and np.isnan(f[nan]).all()
        rest = np.setdiff1d(np.arange(Q), closed + nan)
        assert (bits(f[rest]) == bits(g[rest])).all()
        # a zero on A's diagonal: every gain is NaN
        A0 = A.copy()
        A0[N // 2, N // 2] = 0.0
        assert np.isnan(host(IE.information_gain(dev64(A0), tinfo, interest=interest))).all()
    # the scale: H_q = scale * (sum), against the reference at that scale
    A, info, interest, ref, bars = ER.expected_gain(N, S, "all", scale=0.37)
    g = host(IE.information_gain(dev64(A), dev64(info), scale=0.37))
    assert (ratio_line(f"gain N={N} S={S} all scale=0.37", g, ref, bars) <= 1.0).all()


# ---- 2. batch independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,which", [(13, 3, "first6"), (32, 1, "scattered"), (1, 1, "all")])
def test_a_gain_does_not_depend_on_the_batch(env, N, S, which):
    _lib, IE = env
    A, info, interest, _, _ = ER.expected_gain(N, S, which)
    tA = dev64(A)
    g = host(IE.information_gain(tA, dev64(info), interest=interest))
    for q in (0, 63, 64, 66):
        one = host(IE.information_gain(tA, dev64(info[q:q + 1]), interest=interest))
        assert bits(one[0]) == bits(g[q]), (q, one[0], g[q])
    moved = host(IE.information_gain(tA, dev64(info[::-1]), interest=interest))       # ... nor on the position
    assert (bits(moved[::-1]) == bits(g)).all()


# ---- 3. the pick ------------------------------------------------------------------------------------------------------------
def pick_call(_lib, gain, info, A, taken, scale=1.0, rounds=1, r=0):
    """ehr_information_pick on host arrays -> (picked [rounds], picked_gain [rounds], A, taken) as numpy."""
    tg, ti, tA = dev64(gain), dev64(info), dev64(A)
    tt = torch.tensor(np.asarray(taken, dtype=np.int32), device=DEV)
    picked = torch.full((rounds,), -7, dtype=torch.int32, device=DEV)
    pg = torch.full((rounds,), 123.0, dtype=torch.float64, device=DEV)
    Qn, S, N = info.shape[0], info.shape[1], info.shape[2]
    _lib.check(_lib.lib().ehr_information_pick(_lib.ptr(tg), _lib.ptr(ti), Qn, S, N, float(scale), r, _lib.ptr(tA), _lib.ptr(tt),
                                               _lib.ptr(picked), _lib.ptr(pg),
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ehr_information_pick")
    return host(picked), host(pg), host(tA), host(tt)


def test_pick_ties_and_nothing_finite(env):
    _lib, IE = env
    N, S, scale = 6, 3, 0.37
    A, info = ER.family(N, S)
    rng = np.random.default_rng(0)
    big = np.concatenate([info] * 9)[:600]                                           # 600 candidates: several per thread
    for hi, lo in ((300, 10), (270, 20), (44, 300), (599, 598)):                     # equal best gains in two threads
        gain = rng.uniform(0, 1, size=600)
        gain[[hi, lo]] = 2.5
        gain[5], gain[6], gain[7] = np.inf, np.nan, -np.inf                          # never win
        picked, pg, A1, taken = pick_call(_lib, gain, big, A, np.zeros(600), scale=scale)
        q = min(hi, lo)
        assert picked[0] == q and pg[0] == 2.5 and taken.sum() == 1 and taken[q] == 1
        want = A + ER.candidate_matrix(big[q], scale)                                # numpy: A + scale * (sum in order)
        assert (bits(A1) == bits(want)).all() and (A1 == A1.T).all()
    none = np.full(600, -np.inf)
    none[::3], none[1::3] = np.nan, np.inf
    tk = np.zeros(600, dtype=np.int32)
    tk[17] = 1
    picked, pg, A1, taken = pick_call(_lib, none, big, A, tk, scale=scale, rounds=3, r=1)
    assert picked.tolist() == [-7, -1, -7] and np.isnan(pg[1]) and pg[0] == 123.0 and pg[2] == 123.0   # only its round
    assert (bits(A1) == bits(A)).all() and (taken == tk).all()


@pytest.mark.parametrize("case", ER.PICK_CASES, ids=lambda c: f"N{c[0]}-S{c[1]}-{c[2]}")
def test_greedy_selection_against_the_reference(env, case):
    _lib, IE = env
    N, S, which = case
    A, info, interest, gr = ER.expected_greedy(N, S, which)
    tA = dev64(A)
    sel = IE.greedy_select(tA, dev64(info), 5, interest=interest)
    picked, gains, A_final, taken = host(sel.picked), host(sel.gains), host(sel.A_final), host(sel.taken)
    r = np.abs(gains - gr.gains) / gr.bars
    print(f"[explore greedy] N={N} S={S} {which}: picked {picked.tolist()} (reference {gr.picked.tolist()}), "
          f"worst |gain - ref| / bar = {r.max():.4f}")
    assert picked.tolist() == gr.picked.tolist() and (r <= 1.0).all()
    assert len(set(picked.tolist())) == 5 and taken.sum() == 5 and (taken[picked] == 1).all()
    assert (bits(A_final) == bits(gr.A_final)).all() and (A_final == A_final.T).all()
    assert (bits(host(tA)) == bits(A)).all()                                         # the caller's A is not written
    # the chain rule, for the marginal of the interest set, within the summed bars
    s = 1 / np.sqrt(np.diag(A).astype(np.longdouble))
    rest = ER._indices(interest, N)[1]
    m = lambda X: ER.logdet_scaled(X, s, list(range(N)))[0] - ER.logdet_scaled(X, s, rest)[0]
    total = float(m(A_final) - m(A))
    print(f"[explore greedy] chain rule: sum of gains {gains.sum()!r}, ld(A_final) - ld(A_0) {total!r}, bars {gr.bars.sum():.3e}")
    assert abs(gains.sum() - total) <= gr.bars.sum()


def test_greedy_selection_runs_out_of_candidates(env):
    _lib, IE = env
    A, info = ER.family(13, 1)
    valid = np.zeros(Q, dtype=bool)
    valid[[9, 30, 51]] = True
    sel = IE.greedy_select(dev64(A), dev64(info), 5, valid=valid)
    picked, gains, taken = host(sel.picked), host(sel.gains), host(sel.taken)
    assert sorted(picked[:3].tolist()) == [9, 30, 51] and picked[3:].tolist() == [-1, -1]
    assert np.isfinite(gains[:3]).all() and np.isnan(gains[3:]).all() and taken.sum() == 3
    ref = ER.greedy(A, info, 5, valid=valid)
    assert picked.tolist() == ref.picked.tolist() and (bits(host(sel.A_final)) == bits(ref.A_final)).all()


def test_kernel_refusals(env):
    _lib, IE = env
    A, info = ER.family(6, 1)
    with pytest.raises(RuntimeError, match="1 <= N <= 32"):
        IE.information_gain(dev64(np.eye(33)), dev64(np.zeros((2, 33, 33))))
    with pytest.raises(RuntimeError, match="CUDA/HIP tensor"):
        IE.information_gain(torch.tensor(A), dev64(info))
    with pytest.raises(RuntimeError, match="info must have shape"):
        IE.information_gain(dev64(A), dev64(info[:, :, :5]))
    g, tA, ti = torch.empty((Q,), dtype=torch.float64, device=DEV), dev64(A), dev64(info)
    args = lambda Qn, S, N: (_lib.ptr(tA), _lib.ptr(ti), None, None, Qn, S, N, 1.0, 63, _lib.ptr(g), None)
    for Qn, S, N in ((0, 1, 6), (Q, 0, 6), (Q, 1, 0), (Q, 1, 33)):                   # the C entry point refuses them itself
        assert _lib.lib().ehr_information_gain(*args(Qn, S, N)) != 0
        assert b"bad sizes" in _lib.lib().ehr_last_error()


# ---- 4. the explorer on the gauge problem ---------------------------------------------------------------------------------
_GAUGE = {}


def gauge(oracle, xarm7):
    if "p" not in _GAUGE:
        _GAUGE["p"] = IR.gauge_problem(oracle, xarm7, base=True)
    return _GAUGE["p"]


def make_step(p, kind, extra_q=None):
    """A step on the gauge problem; ``extra_q``: one more frame with that joint vector appended last (its mask: zeros)."""
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.rb_solver import RBSolver
    cfg, batch, qp = IR.gauge_batch(p, DEV)
    if extra_q is not None:
        q1 = np.zeros((1, qp.shape[1]))
        q1[0, :len(extra_q)] = extra_q
        qp = np.concatenate([qp, q1])
        lp1 = torch.tensor(p.rb.link_poses_batch(q1), dtype=torch.float32, device=DEV)
        batch = {"mask": torch.cat([batch["mask"], torch.zeros_like(batch["mask"][:1])]),
                 "link_poses": torch.cat([batch["link_poses"], lp1]), "K": batch["K"][:1].repeat(qp.shape[0], 1, 1)}
    model = RBSolver(cfg, meshes=p.rb.meshes).to(DEV)
    return FusedPoseStep(model, batch) if kind == "pose" else JointPoseStep(model, batch, p.rb, qp)


def behind_the_camera(p, lp_row):
    """The link poses of one candidate moved 10 m against the camera's viewing direction: nothing of the arm is in front of it."""
    Tc = np.asarray(p.init, dtype=np.float64)
    back = np.eye(4)
    back[2, 3] = -10.0
    T = torch.tensor(np.linalg.inv(Tc) @ back @ Tc, dtype=torch.float32, device=DEV)
    return T[None] @ lp_row


def lm_matrix(step):
    from easyhec_amd.lm import LevenbergMarquardt
    return LevenbergMarquardt(step).iterate(1).state().H


def sum_in_order(H):
    s = np.array(H[0])
    for b in range(1, len(H)):
        s = s + H[b]
    return s


@pytest.mark.parametrize("kind", ["pose", "joints"])
def test_explorer_on_the_gauge_problem(env, oracle, xarm7, kind):
    _lib, IE = env
    from easyhec_amd import dr, fused, information
    p = gauge(oracle, xarm7)
    step = make_step(p, kind)
    ex = IE.InformationExplorer(step, robot=p.rb)
    N = 6 if kind == "pose" else 12
    assert ex.N == N and ex.names == [f"dof[{i}]" for i in range(6)] + ([] if kind == "pose" else [f"offset[{j}]" for j in range(1, 7)])
    assert ex.interest == list(range(6))
    q9 = p.rb.sample_qpos(9, np.random.default_rng(7), scale=0.5)
    q10 = np.concatenate([q9, q9[:1]])
    lp, jf = ex.kinematics(q10)
    lp[9] = behind_the_camera(p, lp[9])
    poses = dict(link_poses=lp, joint_frames=jf)
    info, count = ex.candidate_information(q10, **poses)
    hinfo, hcount = host(info), host(count)
    print(f"[explorer {kind}] pixel counts of the candidates {hcount.tolist()}")
    assert (hcount[:9] > 0).all() and hcount[9] == 0 and (hinfo[9] == 0).all() and (hinfo == hinfo.transpose(0, 2, 1)).all()
    # the kinematics hook changes nothing: the first nine are what the joint vectors alone give
    i9, c9 = ex.candidate_information(q9)
    assert (bits(host(i9)) == bits(hinfo[:9])).all() and (host(c9) == hcount[:9]).all()
    # ... and equal mask_information on a fresh context with the matrices of the same linearize call, whatever the reference
    mvp, dmvp = ex._linearize(lp, jf, 10)
    scene = fused.LinkScene([v for v, _ in p.rb.meshes], [f for _, f in p.rb.meshes], DEV)
    zero = torch.zeros((10, p.H, p.W), device=DEV)
    rnd = torch.rand((10, p.H, p.W), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    for ref in (zero, rnd):
        out = information.mask_information(dr.RasterizeCudaContext(), scene, mvp, dmvp, ref)
        assert (bits(host(out.info)) == bits(hinfo)).all() and (host(out.count) == hcount).all()
    # chunks, a ragged last one included
    ex4 = IE.InformationExplorer(step, robot=p.rb, chunk_candidates=4)
    i4, c4 = ex4.candidate_information(q10, **poses)
    assert (bits(host(i4)) == bits(hinfo)).all() and (host(c4) == hcount).all()
    # rejected candidates are not rendered: their rows are zero, their (NaN) link poses reach no kernel, the others keep their bits
    ok = np.ones(10, dtype=bool)
    ok[[1, 8]] = False
    lp_nan = lp.clone()
    lp_nan[[1, 8]] = float("nan")
    iv, cv = ex.candidate_information(q10, ok, link_poses=lp_nan, joint_frames=jf)
    iv, cv = host(iv), host(cv)
    assert (bits(iv[ok]) == bits(hinfo[ok])).all() and (cv[ok] == hcount[ok]).all() and (iv[~ok] == 0).all() and (cv[~ok] == 0).all()
    # the current frames: the matrix Levenberg-Marquardt holds after its first iteration (on a step of its own: LM moves it)
    cur = ex.current_information()
    H0 = host(cur.H0)
    H_lm = lm_matrix(make_step(p, kind))
    assert H0.shape == (4, N, N) and (bits(sum_in_order(H0)) == bits(H_lm)).all()
    # the gains on these matrices, within the bar of the reference
    A0 = host(ex.prior_matrix())
    s2 = float(host(cur.loss).astype(np.float64).sum() / max(int(host(cur.count).sum()) - N, 1))
    want_A0 = sum_in_order(H0) + s2 * np.diag(1.0 / ex.prior_sigma ** 2)
    assert np.abs(A0 - want_A0).max() <= 4 * ER.U * np.abs(want_A0).max() and (A0 == A0.T).all()
    gains = host(ex.score(q10, **poses))
    ref, bars = ER.gain(A0, hinfo[:, None], interest=ex.interest)
    r = ratio_line(f"explorer {kind}", gains, ref, bars)
    print(f"[explorer {kind}] gains {gains.tolist()}")
    assert (r <= 1.0).all() and (gains[:9] > 0).all() and bits(gains[9]) == 0         # out of frame: exactly +0.0
    # select: the reference's picks; the frame out of view is not among them
    sel = ex.select(q10, k=3, **poses)
    picked = host(sel.picked)
    gr = ER.greedy(A0, hinfo[:, None], 3, interest=ex.interest)
    assert (gr.margin > 2 * np.maximum(gr.bars, gr.second_bar)).all()                # (the pick is decided)
    assert picked.tolist() == gr.picked.tolist() and 9 not in picked.tolist()
    assert (bits(host(sel.A_final)) == bits(gr.A_final)).all() and sel.report.names == ex.names
    assert (sel.report.H == gr.A_final).all()
    # what a pick adds is what the frame adds: a step rebuilt with the picked frame appended last (its mask is immaterial)
    qs = int(picked[0])
    H5 = lm_matrix(make_step(p, kind, extra_q=q10[qs]))
    assert (bits(sum_in_order(H0) + hinfo[qs]) == bits(H5)).all()
    # forward: SpaceExplorer.forward's dictionary shape
    valid = np.ones(10, dtype=bool)
    valid[qs] = False
    out = ex.forward(q10, valid=valid, **poses)
    assert sorted(out) == ["gain", "gain_max", "gain_mean", "gain_min", "gains", "qpos", "qpos_idx"]
    assert int(out["qpos_idx"]) != qs and valid[int(out["qpos_idx"])]
    assert float(out["gain"]) == float(out["gain_max"]) >= float(out["gain_mean"]) >= float(out["gain_min"]) > 0
    assert out["gains"][qs] == -np.inf and (out["qpos"] == q10[int(out["qpos_idx"])]).all()
    with pytest.raises(RuntimeError, match="no valid qpos found"):
        ex.forward(q10, valid=np.zeros(10, dtype=bool), **poses)


# ---- 5. non-interference ----------------------------------------------------------------------------------------------------
def _solve(make, batch, build, graph, probe, robot):
    from easyhec_amd.info_explorer import InformationExplorer
    model = make()
    st = build(model, batch)
    if graph:
        st.capture()
    sel = None
    for it in range(20):
        st.step()
        if probe and it == 9:
            sel = InformationExplorer(st, robot=robot).select(robot.sample_qpos(5, np.random.default_rng(1), scale=0.5), k=2)
    torch.cuda.synchronize()
    state = [model.dof.detach().clone(), st.exp_avg.clone(), st.exp_avg_sq.clone(), st.step_t.clone(), st.hist_row.clone(),
             model.history_ops[:24].clone(), st.loss.clone()]
    if hasattr(st, "offsets"):
        state += [st.offsets.clone(), st.offset_exp_avg.clone(), st.offset_exp_avg_sq.clone(), st.offset_step_t.clone()]
    st.release_graph()
    return state, sel


@pytest.mark.parametrize("kind,graph", [("pose", False), ("pose", True), ("joints", True)], ids=["eager", "graph", "joints-graph"])
def test_select_does_not_disturb_a_solve(env, xarm7, kind, graph):
    """10 steps, select, 10 steps: bit-equal to 20 uninterrupted steps, eager and from a captured chain."""
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    from test_gpu_joint_offsets import _views_qpos
    cfg, make, batch = problem(xarm7, 3, 120, 160, 0.125)
    if kind == "pose":
        build = lambda m, b: FusedPoseStep(m, b)
    else:
        qp = _views_qpos(xarm7, 3)
        build = lambda m, b: JointPoseStep(m, b, xarm7, qp)
    plain, _ = _solve(make, batch, build, graph, False, xarm7)
    probed, sel = _solve(make, batch, build, graph, True, xarm7)
    for x, y in zip(plain, probed):
        assert torch.equal(x, y)
    picked = host(sel.picked)
    assert int(plain[3]) == 20 and (picked >= 0).all() and picked[0] != picked[1] and (host(sel.gains) > 0).all()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_explorer_refusals(env, xarm7, monkeypatch):
    _lib, IE = env
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.multistart import MultiStartPoseStep, sample_starts
    from easyhec_amd.rig_calib import RigJointStep
    from easyhec_amd.synthetic import camera_Tc_c2b
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    ms = MultiStartPoseStep(make(), batch, sample_starts(camera_Tc_c2b(), 2, 0.002, 0.3, seed=2))
    with pytest.raises(ValueError, match="multi-start"):
        IE.InformationExplorer(ms, robot=xarm7)
    with pytest.raises(ValueError, match="rig"):
        IE.InformationExplorer(RigJointStep.__new__(RigJointStep), robot=xarm7)
    st = FusedPoseStep(make(), batch)
    st.distributed = True
    with pytest.raises(ValueError, match="data-parallel"):
        IE.InformationExplorer(st, robot=xarm7)
    st.distributed = False
    with pytest.raises(TypeError, match="not a launch-chain step"):
        IE.InformationExplorer(object())
    with pytest.raises(ValueError, match="pass robot="):
        IE.InformationExplorer(st)
    with pytest.raises(ValueError, match="offset\\[1\\]"):
        IE.InformationExplorer(st, robot=xarm7, interest=["dof[0]", "offset[1]"])     # (a pose step frees no offset)
    with pytest.raises(ValueError, match="> 0"):
        IE.InformationExplorer(st, robot=xarm7, prior_sigma={"rotation": 0.0})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="being captured"):
        IE.InformationExplorer(st, robot=xarm7)
    monkeypatch.undo()
    ex = IE.InformationExplorer(st, robot=xarm7)
    monkeypatch.setattr(_lib, "has_information_gain", lambda: False)                 # a library without the symbols
    for call in (lambda: IE.InformationExplorer(st, robot=xarm7), lambda: IE.information_gain(dev64(np.eye(2)), dev64(np.zeros((1, 2, 2)))),
                 lambda: IE.greedy_select(dev64(np.eye(2)), dev64(np.zeros((1, 2, 2))), 1)):
        with pytest.raises(RuntimeError, match="no exploration kernels"):
            call()
    monkeypatch.undo()
    import easyhec_amd
    assert easyhec_amd.InformationExplorer is IE.InformationExplorer and ex.N == 6


# ---- 7. the online loop -----------------------------------------------------------------------------------------------------
def test_online_loop_explores_by_information(env, xarm7):
    from easyhec_amd import render_api
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.online import OnlineCalibration
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    H, W = 120, 160
    K = np.array(scaled_K(XARM7_K_1280x720, 0.125, W, H, True), dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    init = perturb_pose(Tc_gt)
    logs = {}
    for explore in ("information", "variance"):
        rng = np.random.default_rng(1)
        asked, offered = [], []

        def capture(qpos):
            asked.append(np.array(qpos))
            return render_api.nvdiffrast_render_xarm_api(None, Tc_gt, qpos, H, W, K)

        def candidates(_round):
            cand, valid = xarm7.sample_qpos(12, rng, scale=0.9), np.ones(12, dtype=bool)
            valid[[2, 7]] = False
            offered.append((cand, valid))
            return cand, valid

        loop = OnlineCalibration(xarm7, K, H, W, init, capture, candidates, num_epochs=60, explore_iters=2, sample=4, start=10,
                                 explore=explore)
        Tc = loop.fit(np.zeros(7))
        logs[explore] = loop.log
        print(f"[online {explore}] {loop.log}")
        assert np.isfinite(Tc).all() and [r["frames"] for r in loop.log] == [1, 2] and len(asked) == 2 and len(offered) == 1
        cand, valid = offered[0]
        hit = [i for i in range(12) if (cand[i] == asked[1]).all()]
        assert len(hit) == 1 and valid[hit[0]]                                        # the frame it asked for: a valid candidate
    r = logs["information"][0]
    assert np.isfinite(r["info_gain"]) and r["info_gain"] > 0 and r["info_gain"] >= r["gain_mean"] > 0
    assert sorted(r) == sorted(["round", "frames", "mask_loss", "solve_s", "explore_s", "info_gain", "gain_mean", "candidates"])
    assert sorted(logs["variance"][0]) == sorted(["round", "frames", "mask_loss", "solve_s", "explore_s", "variance", "var_mean",
                                                  "candidates"])
    assert sorted(logs["variance"][1]) == sorted(logs["information"][1]) == sorted(["round", "frames", "mask_loss", "solve_s"])
    with pytest.raises(ValueError, match="'variance' or 'information'"):
        OnlineCalibration(xarm7, K, H, W, init, None, None, explore="entropy")
