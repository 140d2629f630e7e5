"""The rig's Levenberg-Marquardt update on its block-arrow system on the GPU (csrc/ehr_lm.hip: lm_update_rig_arrow_kernel,
easyhec_amd/lm_rig.py with ``solver="arrow"``) against the numpy restatement of
tests/lm_rig_arrow_reference.py, whose solve is the DENSE one: the update kernel alone on synthetic systems up to the maximum
N = 182, against the dense rig kernel where both apply, the entry point's refusals, one camera against the solo solve with
joints and intrinsics, the composition of one iteration, the loss the solve reports, monotone descent along a gauge direction
without and with a prior, more than 32 parameters with real rendering, a reported iteration, non-interference with the rig's
Adam state, and the solve end to end against the CPU loop.  tests/test_lm_rig_arrow_reference.py pins the reference on the
CPU.  Every figure is printed before it is asserted."""
import ctypes
import types

import numpy as np
import pytest
import torch

import information_reference as IR
import lm_reference as LR
import lm_rig_arrow_reference as AR
import lm_rig_reference as RR
from test_gpu_fast import problem
from test_gpu_joint_offsets import _pose_errors, _views_qpos
from test_gpu_lm import DEV, _stream, ref_state, t32
from test_gpu_rig import _two_cameras

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr, fused, lm, lm_rig
    assert _lib.has_lm_rig_arrow()
    return _lib, fused, dr, lm, lm_rig


def dense_H(_lib, s, P, F):
    """The packed H_acc of an arrow state block (host float64) as the dense [N,N] matrix."""
    base = np.concatenate([[0], np.cumsum(P)]).astype(int)
    S0 = int(base[-1])
    H = np.zeros((S0 + F, S0 + F))
    for c, Pc in enumerate(P):
        at = _lib.LM_ARROW_H + c * _lib.LM_ARROW_CAMERA_STRIDE
        panel = s[at:at + 360].reshape(10, 36)
        bt = s[at + _lib.LM_ARROW_BORDER_T:at + _lib.LM_ARROW_CAMERA_STRIDE].reshape(26, 10)
        b = base[c]
        H[b:b + Pc, b:b + Pc] = panel[:Pc, :Pc]
        H[b:b + Pc, S0:] = panel[:Pc, 10:10 + F]
        H[S0:, b:b + Pc] = bt[:F, :Pc]
    H[S0:, S0:] = s[_lib.LM_ARROW_CORNER:_lib.LM_ARROW_CORNER + 676].reshape(26, 26)[:F, :F]
    return H


def arrow_ns(_lib, state, P, F):
    s = state.cpu().numpy()
    N = int(sum(P)) + F
    ns = types.SimpleNamespace(**{k: s[i] for k, i in _lib.LM_STATE.items()})
    ns.theta = s[_lib.LM_ARROW_THETA:_lib.LM_ARROW_THETA + N]
    ns.delta = s[_lib.LM_ARROW_DELTA:_lib.LM_ARROW_DELTA + N]
    ns.g = s[_lib.LM_ARROW_G:_lib.LM_ARROW_G + N]
    ns.H = dense_H(_lib, s, P, F)
    ns.raw = s.copy()
    return ns


def compare(ns, st, got_params, want_params, what, worst, N):
    """test_gpu_lm.py's ``compare`` with the bar max(32, N) 2^-53 cond.  Exact: lambda, nu, F_acc, counters, flags, the stored
    linearisation.  delta, pred: the bar.  The parameters: within one float32 spacing."""
    assert ns.__dict__["lambda"] == st.lam and ns.nu == st.nu and ns.F_acc == st.F_acc, (what, ns.__dict__["lambda"], st.lam)
    for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last", "count", "retries"):
        assert int(getattr(ns, k)) == int(getattr(st, k)), (what, k, getattr(ns, k), getattr(st, k))
    if st.accepted:
        assert (ns.theta == st.theta).all() and (ns.H == st.H).all() and (ns.g == st.g).all(), what
    if st.last != -1 and st.delta is not None and st.cond is not None:
        Hs = getattr(st, "Hs", st.H)
        s = np.sqrt(np.where(np.diag(Hs) > 0, np.diag(Hs), 1.0))
        y, yr = ns.delta * s, st.delta * s
        bar = AR.bar(N, st.cond)
        ry = float(np.abs(y - yr).max() / max(np.abs(yr).max(), 1e-300)) / bar
        rp = abs(ns.pred - st.pred) / max(abs(st.pred), 1e-300) / bar
        worst[0], worst[1] = max(worst[0], ry), max(worst[1], rp)
        assert ry <= 1.0 and rp <= 1.0, (what, ry, rp, st.cond)
        assert ((st.delta == 0) == (ns.delta == 0)).all(), what
    gp, wp = np.asarray(got_params, np.float32), np.asarray(want_params, np.float32)
    assert (np.abs(gp.astype(np.float64) - wp.astype(np.float64)) <= LR.spacing_f32(wp)).all(), (what, gp, wp)


# ---- 1. the update kernel alone ----------------------------------------------------------------------------------------------
K_BASE = np.array([[226.7, 0, 81.3], [0, 226.6, 61.2], [0, 0, 1]], np.float32)


class ArrowUpd:
    """The tensors one ehr_lm_update_rig_arrow works on, without a renderer: per camera its own dof, theta, K0, K and (H, W)."""

    def __init__(self, _lib, C, F, frees, Bs, seed=0, lambda0=1e-3):
        self._lib, self.C, self.F, self.frees, self.Bs = _lib, C, F, frees, Bs
        self.P, self.base, self.N = AR.layout(frees, F)
        rng = np.random.default_rng(100 * C + F + seed)
        self.J = 32
        self.free = sorted(rng.permutation(self.J)[:F].tolist())
        self.free_list = torch.tensor(self.free, dtype=torch.int32, device=DEV) if F else None
        self.dofs = [t32(rng.uniform(-1, 1, 6)) for _ in range(C)]
        self.offset = t32(rng.uniform(-0.05, 0.05, self.J))
        self.offset0 = self.offset.clone()
        self.parsed = [AR.parse_free(fr) for fr in frees]
        self.masks = [sum(b << i for i, b in enumerate(f4)) for f4, _, _ in self.parsed]
        self.els = [LR.intrinsics_elements(f4, tie) for f4, tie, _ in self.parsed]
        self.HW = [(120 + 8 * c, 160 + 16 * c) for c in range(C)]                  # distinct image sizes
        self.thetas, self.K0s, self.Ks = [], [], []
        from easyhec_amd.intrinsics_calib import intrinsics_from_theta
        for c in range(C):
            th = rng.uniform(-0.02, 0.02, 4).astype(np.float32)
            if self.parsed[c][1]:
                th[1] = th[0]
            k0 = K_BASE.copy()
            k0[0, 0], k0[1, 1], k0[0, 2], k0[1, 2] = k0[0, 0] + 3 * c, k0[1, 1] + 2 * c, k0[0, 2] + c, k0[1, 2] - c
            self.thetas.append(t32(th))
            self.K0s.append(t32(k0))
            # (a fixed camera's K: something only it holds, so that "untouched" means something)
            self.Ks.append(t32(intrinsics_from_theta(k0, th, *self.HW[c]) if self.masks[c] else k0 * np.float32(1.01)))
        self.theta0, self.K_first = [t.clone() for t in self.thetas], [k.clone() for k in self.Ks]
        st = np.zeros(_lib.LM_ARROW_STATE_DOUBLES)
        st[0], st[1] = lambda0, 2.0
        self.state = torch.from_numpy(st).to(DEV)
        self.log = torch.full((64, 4), float("nan"), dtype=torch.float64, device=DEV)

    def params(self):
        out = []
        for c in range(self.C):
            th = self.thetas[c].cpu().numpy()
            out += [self.dofs[c].cpu().numpy(), np.array([th[e[0]] for e in self.els[c]], np.float32)]
        out.append(self.offset.cpu().numpy()[self.free])
        return np.concatenate(out).astype(np.float32)

    def ns(self):
        return arrow_ns(self._lib, self.state, self.P, self.F)

    def array(self, dev):
        L = self._lib
        rows = []
        for c, (i, g, n, l) in enumerate(dev):
            m = self.masks[c]
            rows.append(L.LmRigArrowCamera(i.data_ptr(), g.data_ptr(), n.data_ptr(), l.data_ptr(), self.dofs[c].data_ptr(),
                                           self.thetas[c].data_ptr() if m else None, self.K0s[c].data_ptr() if m else None,
                                           self.Ks[c].data_ptr() if m else None, self.Bs[c], self.HW[c][0], self.HW[c][1], m,
                                           int(self.parsed[c][1])))
        return (L.LmRigArrowCamera * self.C)(*rows)

    def call(self, cams, ftol=AR.FTOL, lambda_max=1e6, finalize=0, prior=None):
        _lib = self._lib
        dev = [(torch.tensor(np.ascontiguousarray(i, np.float64), device=DEV), torch.tensor(np.ascontiguousarray(g, np.float64), device=DEV),
                torch.tensor(np.ascontiguousarray(c, np.int64), device=DEV), t32(l)) for i, g, c, l in cams]
        pw = pm = None
        if prior is not None:
            pw, pm = (torch.tensor(np.ascontiguousarray(x, np.float64), device=DEV) for x in prior)
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().ehr_lm_update_rig_arrow(
                self.array(dev), self.C, _lib.ptr(self.offset if self.F else None), _lib.ptr(self.free_list), self.F, self.J,
                ctypes.c_double(ftol), ctypes.c_double(lambda_max), finalize, _lib.ptr(self.state), _lib.ptr(self.log), 64,
                _lib.ptr(pw), _lib.ptr(pm), _stream()), "ehr_lm_update_rig_arrow")
            for i, g, c, l in dev:   # the call has read its inputs when the next one starts: garbage proves nothing is read later
                i.fill_(float("nan")), g.fill_(float("nan")), l.fill_(float("nan")), c.fill_(-7)
        torch.cuda.synchronize()
        return self.ns()

    def check_intrinsics(self, what, written):
        """K == intrinsics_from_theta(K0, theta) bit for bit in every camera with free intrinsics once the kernel has written
        (before: as constructed); a fixed camera's K and the elements of theta that are not free: untouched."""
        from easyhec_amd.intrinsics_calib import intrinsics_from_theta
        for c in range(self.C):
            th, K = self.thetas[c].cpu().numpy(), self.Ks[c].cpu().numpy()
            if self.masks[c] and written:
                want = intrinsics_from_theta(self.K0s[c].cpu().numpy(), th, *self.HW[c])
                assert want.tobytes() == K.tobytes(), f"{what}: camera {c}'s K is not intrinsics_from_theta(K0, theta)"
                if self.parsed[c][1]:
                    assert th[0] == th[1], f"{what}: camera {c}'s tied focal entries differ"
            else:
                assert torch.equal(self.Ks[c], self.K_first[c]), f"{what}: camera {c}'s K moved"
            fixed = [i for i in range(4) if not (self.masks[c] >> i) & 1]
            assert torch.equal(self.thetas[c][fixed], self.theta0[c][fixed]), f"{what}: camera {c}'s fixed theta moved"


def _arrow_update_sequence(_lib, C, F, frees, Bs, worst):
    u = ArrowUpd(_lib, C, F, frees, Bs)
    N, base = u.N, u.base
    accepted, z, zi = None, AR.zeroed_parameter(frees, F), AR.zeroed_intrinsics(frees, F)[0]
    for k, (what, cams) in enumerate(AR.scripted_calls(C, F, frees, Bs)):
        before, now = ref_state(u.ns()), u.params()
        fin = what == "finalize"
        raw = u.state.cpu().numpy().copy()
        ns = u.call(cams, finalize=int(fin))
        want = AR.update_rig_arrow(before, cams, frees, F, now, AR.FTOL, 1e6, fin)
        compare(ns, before, u.params(), want, f"C={C} F={F} {what}", worst, N)
        u.check_intrinsics(f"C={C} F={F} {what}", True)
        if what in ("nan-loss", "bad-count", "finalize"):   # every pose, every theta and the offsets: the accepted ones, bit for bit
            assert u.params().tobytes() == accepted.tobytes() == want.tobytes(), what
            assert fin or ns.last == -1
            assert ns.__dict__["lambda"] == before.lam
        if fin:
            assert ns.raw.tobytes() == raw.tobytes()
        if ns.last == 1 and not fin:
            accepted = ns.theta.astype(np.float32)
        if what == "reject":
            assert ns.rejected == 1 and ns.nu == 4.0 and (ns.H == before.H).all() and (u.params() != accepted).any()
        for name, q in (("zero-diagonal", z), ("zero-intrinsics", zi)):
            if what == name:
                assert ns.H[q, q] == 0.0 and ns.delta[q] == 0.0 and u.params()[q] == accepted[q]
                assert (np.delete(ns.delta, q) != 0).all()
    assert (ns.accepted, ns.rejected, ns.reported, ns.iterations, ns.done) == (4, 1, 2, 7, 0)
    for a in range(C):           # the blocks between two different cameras: exactly zero in the dense H
        for b in range(C):
            if a != b:
                assert (ns.H[base[a]:base[a + 1], base[b]:base[b + 1]] == 0).all()
    log = u.log.cpu().numpy()[:7]
    assert log[:, 1].tolist() == [1, 1, 0, -1, -1, 1, 1] and np.isnan(log[3:5, 0]).all() and np.isnan(u.log.cpu().numpy()[7:]).all()
    keep = [j for j in range(u.J) if j not in u.free]        # the joints that are not free stay
    assert torch.equal(u.offset[keep], u.offset0[keep])
    return u


@pytest.mark.parametrize("C,F,frees,Bs", AR.SHAPES)
def test_update_kernel_alone(env, C, F, frees, Bs):
    _lib = env[0]
    worst = [0.0, 0.0]
    a = _arrow_update_sequence(_lib, C, F, frees, Bs, worst)
    print(f"[lm rig arrow update] C={C} F={F} B={Bs} (N={a.N}): worst |y - y_ref| / (max(32, N) 2^-53 cond |y|) = {worst[0]:.4f}, "
          f"the same for pred = {worst[1]:.4f}")
    b = _arrow_update_sequence(_lib, C, F, frees, Bs, [0.0, 0.0])                  # two runs: identical bits
    for x, y in [(a.state, b.state), (a.offset, b.offset), (a.log, b.log)] + list(zip(a.dofs, b.dofs)) + \
            list(zip(a.thetas, b.thetas)) + list(zip(a.Ks, b.Ks)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_update_kernel_under_a_prior(env):
    """The prior's term joins F, its weights and pull the system that is solved; the stored H, g stay the data's."""
    _lib = env[0]
    C, F, frees, Bs = AR.SHAPES[4]
    u = ArrowUpd(_lib, C, F, frees, Bs)
    rng = np.random.default_rng(5)
    w = np.where(rng.uniform(size=u.N) < 0.5, 10.0 ** rng.uniform(-2, 2, u.N), 0.0)
    mu = rng.normal(size=u.N) * 0.01
    worst = [0.0, 0.0]
    for what, cams in AR.scripted_calls(C, F, frees, Bs)[:3]:
        before, now = ref_state(u.ns()), u.params()
        before.F_prior = float(u.ns().F_prior)
        ns = u.call(cams, prior=(w, mu))
        want = AR.update_rig_arrow(before, cams, frees, F, now, AR.FTOL, 1e6, False, prior=(w, mu))
        compare(ns, before, u.params(), want, f"prior {what}", worst, u.N)
        assert ns.F_prior == before.F_prior and ns.F_prior > 0
        u.check_intrinsics(f"prior {what}", True)
    print(f"[lm rig arrow update] under a prior: worst ratios {worst[0]:.4f}, {worst[1]:.4f}; F_prior {ns.F_prior!r}")


# ---- 2. against the dense rig kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,F,Bs", RR.SHAPES)
def test_against_the_dense_rig_kernel(env, C, F, Bs):
    """The same inputs to ehr_lm_update_rig and to the arrow entry (no intrinsics): the exact fields are equal, delta and pred
    within the bar of each other; whether they are bit-equal is printed."""
    _lib = env[0]
    from test_gpu_lm_rig import RigUpd, _ns
    frees = [None] * C
    d, a = RigUpd(_lib, C, F, Bs), ArrowUpd(_lib, C, F, frees, Bs)
    for c in range(C):
        a.dofs[c].copy_(d.dofs[c])
    a.offset.copy_(d.offset)
    a.free, a.free_list = d.free, d.free_list
    N, same = 6 * C + F, True
    for what, cams in RR.scripted_calls(C, F, Bs):
        fin = int(what == "finalize")
        nd, na = d.call(cams, finalize=fin), a.call(cams, finalize=fin)
        for k in _lib.LM_STATE:
            if k != "pred":
                assert nd.__dict__[k] == na.__dict__[k], (what, k)
        assert (nd.theta == na.theta).all() and (nd.g == na.g).all() and (nd.H == na.H).all(), what
        if fin or nd.last == -1:    # the accepted parameters, written back: the same bits
            assert d.params().tobytes() == a.params().tobytes(), what
        else:
            assert (np.abs(d.params().astype(np.float64) - a.params()) <= LR.spacing_f32(d.params())).all(), what
        if nd.accepted:
            sol = LR.solve(nd.H, nd.g, nd.__dict__["lambda"])
            bar = AR.bar(N, sol[3])
            s = np.sqrt(np.where(np.diag(nd.H) > 0, np.diag(nd.H), 1.0))
            ry = float(np.abs((nd.delta - na.delta) * s).max() / np.abs(nd.delta * s).max()) / bar
            rp = abs(nd.pred - na.pred) / abs(nd.pred) / bar
            assert ry <= 1.0 and rp <= 1.0, (what, ry, rp)
        same = same and nd.delta.tobytes() == na.delta.tobytes() and nd.pred == na.pred and d.params().tobytes() == a.params().tobytes()
    print(f"[lm rig arrow vs dense] C={C} F={F} B={Bs}: delta, pred and the parameters bit-equal to ehr_lm_update_rig's: {same}")


# ---- 3. refusals of the entry point ------------------------------------------------------------------------------------------
def test_update_entry_refuses_bad_arguments(env):
    _lib = env[0]
    u = ArrowUpd(_lib, 2, 1, [("f",), None], [1, 2])
    untouched = u.state.clone()
    t = [torch.zeros(64, dtype=torch.float64, device=DEV) for _ in range(8)]
    L = _lib.lib()

    def cam(mask=0, tie=0, B=1, null=None, intr=True):
        ptrs = [x.data_ptr() for x in t]
        if not intr:
            ptrs[5] = ptrs[6] = ptrs[7] = None
        if null is not None:
            ptrs[null] = None
        return _lib.LmRigArrowCamera(*ptrs, B, 48, 64, mask, tie)

    def call(cams, C, F=1, pw=None, pm=None, free_list=True):
        arr = (_lib.LmRigArrowCamera * max(len(cams), 1))(*cams)
        return L.ehr_lm_update_rig_arrow(arr, C, _lib.ptr(u.offset), _lib.ptr(u.free_list if free_list else None), F, u.J,
                                         ctypes.c_double(1e-6), ctypes.c_double(1e6), 0, _lib.ptr(u.state), None, 0, _lib.ptr(pw),
                                         _lib.ptr(pm), _stream())

    one = torch.ones(64, dtype=torch.float64, device=DEV)
    cases = [("no camera", lambda: call([cam()], 0), "1 <= C"),
             ("17 cameras", lambda: call([cam()] * 17, 17), "17 cameras"),
             ("a NULL pointer", lambda: call([cam(), cam(null=3)], 2), "camera 1 has a NULL pointer"),
             ("B_1 = 0", lambda: call([cam(), cam(B=0)], 2), "camera 1 has B 0 < 1"),
             ("F + I_c = 27", lambda: call([cam(), cam(mask=15)], 2, F=23), "camera 1 has 23 free joints + 4 free intrinsics"),
             ("mask 16", lambda: call([cam(mask=16)], 1), "camera 0 has bad free intrinsics (mask 16"),
             ("tie without fx", lambda: call([cam(), cam(mask=2, tie=1)], 2), "camera 1 has bad free intrinsics (mask 2, tie_focal 1)"),
             ("free mask, no theta", lambda: call([cam(), cam(mask=3, intr=False)], 2), "camera 1 has free intrinsics (mask 3) but no theta"),
             ("one prior pointer", lambda: call([cam()], 1, pw=one), "prior_weight and prior_mean go together"),
             ("the other prior pointer", lambda: call([cam()], 1, pm=one), "prior_weight and prior_mean go together"),
             ("free joints, no list", lambda: call([cam()], 1, free_list=False), "free joints need offset and the list")]
    for what, run, match in cases:
        rc = run()
        msg = L.ehr_last_error().decode()
        print(f"[lm rig arrow update] refused ({what}): code {rc}: {msg}")
        assert rc != 0 and match in msg, (what, msg)
    rc = L.ehr_lm_update_rig_arrow(None, 1, _lib.ptr(u.offset), _lib.ptr(u.free_list), 1, u.J, ctypes.c_double(1e-6),
                                   ctypes.c_double(1e6), 0, _lib.ptr(u.state), None, 0, None, None, _stream())
    assert rc != 0 and "NULL" in L.ehr_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(u.state, untouched)


# ---- the solve through RigLM -------------------------------------------------------------------------------------------------
def _make_rig(xarm7, free, cams=None, **kw):
    from easyhec_amd.rig_calib import RigJointStep
    cams = _two_cameras(xarm7) if cams is None else cams
    models = [make() for _, make, _, _ in cams]
    return RigJointStep(models, [b for _, _, b, _ in cams], xarm7, [q for _, _, _, q in cams], free=free, **kw)


def _ns(_lib, o):
    return arrow_ns(_lib, o.state_block, o.block_sizes, o.F)


def _check_K(o, what):
    """Every camera with free intrinsics: K == intrinsics_from_theta(K0, theta) bit for bit, in the unit's own buffer."""
    from easyhec_amd.intrinsics_calib import intrinsics_from_theta
    for c, u in enumerate(o.units):
        if u.theta is not None:
            want = intrinsics_from_theta(u.K0.cpu().numpy(), u.theta.cpu().numpy(), u.H, u.W)
            assert want.tobytes() == u.cam.K.cpu().numpy().tobytes(), f"{what}: camera {c}"


# ---- 4. one camera: the solo solve with joints and intrinsics ------------------------------------------------------------------
def test_one_camera_against_the_solo_solve_with_joints_and_intrinsics(env, xarm7):
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.intrinsics_calib import JointIntrinsicsPoseStep
    from easyhec_amd.rig_calib import RigJointStep
    cfg, make, batch = problem(xarm7, 2, 48, 64, 0.05)
    qp = _views_qpos(xarm7, 2)
    free_i = ("f", "cx", "cy")
    solo = lm.LevenbergMarquardt(JointIntrinsicsPoseStep(make(), batch, xarm7, qp, free=[1, 3], free_intrinsics=free_i))
    rig = RigJointStep([make()], [batch], xarm7, [qp], free=[1, 3])
    K_given, K_before = rig.cameras[0].K, batch["K"].clone()
    arrow = lm_rig.RigLM(rig, free_intrinsics=free_i)
    assert arrow.solver == "arrow" and arrow.N == solo.N == 11 and rig.cameras[0].K.data_ptr() != K_given.data_ptr()
    assert arrow.names == [f"cam0.dof[{i}]" for i in range(6)] + ["cam0.theta[f]", "cam0.theta[cx]", "cam0.theta[cy]", "offset[1]", "offset[3]"]
    assert solo.names == [f"dof[{i}]" for i in range(6)] + ["offset[1]", "offset[3]", "theta[f]", "theta[cx]", "theta[cy]"]
    perm = [0, 1, 2, 3, 4, 5, 8, 9, 10, 6, 7]                 # the arrow order's parameter k is the solo order's perm[k]
    solo.iterate(1), arrow.iterate(1)
    torch.cuda.synchronize()
    fused.check_status(solo.step.glctx), fused.check_status(rig.cameras[0].glctx)
    a, b = solo.state(), arrow.state()
    assert a.F_acc == b.F_acc and a.accepted == b.accepted == 1 and a.count == b.count
    assert (a.H[np.ix_(perm, perm)] == b.H).all() and (a.g[perm] == b.g).all() and (a.theta[perm] == b.theta).all()
    cond = LR.solve(b.H, b.g, b.__dict__["lambda"])[3]
    s = np.sqrt(np.where(np.diag(b.H) > 0, np.diag(b.H), 1.0))
    ry = float(np.abs((a.delta[perm] - b.delta) * s).max() / np.abs(b.delta * s).max()) / AR.bar(11, cond)
    pa, pb = solo.parameters()[perm], arrow.parameters()
    print(f"[lm rig arrow C=1] F_acc {b.F_acc!r}; |delta - solo's| / bar = {ry:.4f} (cond {cond:.3g}); trial parameters equal: "
          f"{pa.tobytes() == pb.tobytes()}")
    assert ry <= 1.0
    assert (np.abs(pa.astype(np.float64) - pb) <= LR.spacing_f32(pa)).all() and (pa != a.theta[perm].astype(np.float32)).any()
    _check_K(arrow, "one camera")
    assert torch.equal(batch["K"], K_before) and torch.equal(K_given, K_before[0])   # the caller's tensor is never written


# ---- 5. composition ----------------------------------------------------------------------------------------------------------
def test_iterate_is_its_pieces(env, xarm7):
    """Three consecutive iterations of two cameras of different image size and different free sets, each against: per camera
    ehr_joint_forward, ehr_lm_linearize (its own mask, tying and N_c) into buffers of the test's own and mask_information on
    them; then the reference update from the GPU's own previous state."""
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd import information
    rig = _make_rig(xarm7, [1, 3])
    frees = [("f",), ("cx", "cy")]
    o = lm_rig.RigLM(rig, free_intrinsics=frees)
    assert o.N == 17 and o.block_sizes == [7, 8] and [u.N for u in o.units] == [9, 10]
    assert [(u.H, u.W) for u in o.units] == [(120, 160), (96, 128)]
    worst = [0.0, 0.0]
    for it in range(3):
        before, now = ref_state(_ns(_lib, o)), o.parameters()
        mine, own = [], []
        for u in o.units:
            keep = (u.mvp, u.dmvp)
            u.mvp, u.dmvp = torch.empty_like(keep[0]), torch.empty_like(keep[1])
            with torch.cuda.device(DEV):
                u._forward_kinematics(_stream())
                u._linearize(_stream())
            mine.append(information.mask_information(u.glctx, u.scene, u.mvp, u.dmvp, u.ref, want_loss=True))
            own.append((u.mvp, u.dmvp))
            u.mvp, u.dmvp = keep
        o.iterate(1)
        torch.cuda.synchronize()
        for c, (u, m, (own_mvp, own_dmvp)) in enumerate(zip(o.units, mine, own)):
            fused.check_status(u.glctx)
            assert torch.equal(own_mvp, u.mvp) and torch.equal(own_dmvp, u.dmvp), c
            for x, y in ((m.info, u.out.info), (m.grad, u.out.grad), (m.count, u.out.count), (m.loss, u.out.loss)):
                assert torch.equal(x, y), c
        cams = [(m.info.cpu().numpy(), m.grad.cpu().numpy(), m.count.cpu().numpy(), m.loss.cpu().numpy()) for m in mine]
        want = AR.update_rig_arrow(before, cams, frees, 2, now)
        compare(_ns(_lib, o), before, o.parameters(), want, f"arrow rig iteration {it}", worst, o.N)
        _check_K(o, f"iteration {it}")
    s = o.state()
    print(f"[lm rig arrow composition] worst delta / pred ratios {worst[0]:.4f}, {worst[1]:.4f}; F_acc {s.F_acc:.3f}, {s.accepted} accepted")
    assert s.accepted >= 1 and s.iterations == 3 and (s.H == _ns(_lib, o).H).all()


# ---- 6. the loss is the solve's loss -----------------------------------------------------------------------------------------
def _loss_at_accepted(fused, dr, o):
    """sum_c (sum_b (double) loss) of render_mask_loss (another context) on the linearize kernel's mvp -- each camera's
    rewritten K -- at the rig's parameters, in the update's order, weights included."""
    F, per = 0.0, []
    for u in o.units:
        with torch.cuda.device(DEV):
            u._forward_kinematics(_stream())
            u._linearize(_stream())
        w = u.weight.clone() if u.weight is not None else None
        _, loss = fused.render_mask_loss(dr.RasterizeCudaContext(), u.scene, u.mvp.clone(), u.ref.clone(), want_mask=False, weight=w)
        torch.cuda.synchronize()
        Fc = 0.0
        for x in loss.detach().cpu().numpy():
            Fc += float(x)
        per.append(Fc)
        F += Fc
    return F, per


def test_accepted_loss_is_render_mask_loss(env, xarm7):
    _lib, fused, dr, lm, lm_rig = env
    cams = _two_cameras(xarm7)
    cfg1, make1, batch1, qp1 = cams[1]
    w = torch.ones_like(batch1["mask"])
    w[:, :, :w.shape[2] // 2] = 0.5                                                # half of camera 1's pixels count half
    cams[1] = (cfg1, make1, dict(batch1, weight=w), qp1)
    o = lm_rig.RigLM(_make_rig(xarm7, [1, 3], cams=cams), free_intrinsics=[("f",), ("fx", "fy", "cx", "cy")])
    o.iterate(6).finalize()
    s = o.state()
    F, per = _loss_at_accepted(fused, dr, o)
    print(f"[lm rig arrow loss] F_acc {s.F_acc!r}, render_mask_loss at the accepted parameters and Ks {F!r} = {per}; {s.accepted} "
          f"accepted of {s.iterations}")
    assert F == s.F_acc and s.accepted >= 2
    _check_K(o, "after finalize")
    from easyhec_amd.intrinsics_calib import intrinsics_from_theta
    for c, (u, K) in enumerate(zip(o.units, o.intrinsics())):                      # finalize leaves the ACCEPTED K
        th4 = np.zeros(4, np.float32)
        for q, el in enumerate(u.elements):
            th4[el] = np.float32(s.theta[sum(o.block_sizes[:c]) + 6 + q])
        if u.layout.tie_focal:
            th4[1] = th4[0]
        assert K.numpy().tobytes() == intrinsics_from_theta(u.K0.cpu().numpy(), th4, u.H, u.W).tobytes(), c
        assert (K.numpy() != u.K0.cpu().numpy()).any()


# ---- 7. monotone and deterministic along a gauge direction, without and with a prior -------------------------------------------
def test_monotone_and_deterministic_with_a_gauge_direction_and_under_the_default_prior(env, xarm7):
    """("cx", "cy") free in both cameras: a principal-point shift is nearly a small camera rotation, H is nearly singular, the
    damping carries it.  Then the same under prior_sigma="default"."""
    _lib, fused, dr, lm, lm_rig = env
    ends = []
    for _ in range(2):
        rig = _make_rig(xarm7, [1, 3])
        o = lm_rig.RigLM(rig, free_intrinsics=("cx", "cy"))
        o.iterate(12).finalize()
        s, tr = o.state(), o.trajectory()
        for cam in rig.cameras:
            fused.check_status(cam.glctx)
        ends.append((o.state_block.cpu().numpy().tobytes(), o.log.cpu().numpy().tobytes(), o.parameters().tobytes(),
                     b"".join(K.numpy().tobytes() for K in o.intrinsics())))
    acc = tr[tr[:, 1] == 1, 0]
    print(f"[lm rig arrow monotone] accepted losses {np.round(acc, 2).tolist()}; {s.accepted} accepted, {s.rejected} rejected, "
          f"{s.reported} reported, done {s.done} ({LR.WHY[s.why]}), lambda {s.__dict__['lambda']:.3g}, condition of the scaled "
          f"H_acc {o.report(s).condition:.3g}")
    assert (np.diff(acc) < 0).all() and len(acc) >= 2 and acc[-1] == s.F_acc
    assert s.accepted + s.rejected + s.reported == s.iterations and (s.iterations == 12 or s.done)
    p = o.parameters()
    assert np.isfinite(p).all() and (p == s.theta.astype(np.float32)).all()
    assert ends[0] == ends[1]
    # under the default prior: offsets near zero, intrinsics near the given K, no prior on a pose
    rig = _make_rig(xarm7, [1, 3])
    res = lm_rig.solve_lm_rig(rig, max_iters=12, prior_sigma="default", free_intrinsics=("cx", "cy"))
    pr, tr = res.prior, res.trajectory
    acc = tr[tr[:, 1] == 1, 0]
    kinds = lm._prior_kinds(res.lm.names, res.lm.joint_kinds())
    print(f"[lm rig arrow prior] accepted objectives {np.round(acc, 2).tolist()}; data loss {res.data_loss:.3f}, prior loss "
          f"{res.prior_loss!r}, sigma2 {pr.sigma2:.4g}; kinds {kinds}")
    assert kinds == (["translation"] * 3 + ["rotation"] * 3 + ["principal"] * 2) * 2 + ["revolute"] * 2
    assert [np.isfinite(x) for x in pr.sigma] == ([False] * 6 + [True] * 2) * 2 + [True] * 2
    assert (np.diff(acc) < 0).all() and acc[-1] == res.loss and res.accepted >= 2
    assert res.prior_loss == res.state.F_prior > 0 and res.data_loss == res.loss - res.prior_loss
    cov = res.posterior.covariance()
    assert np.isfinite(cov).all() and cov.shape == (18, 18)
    again = lm.make_prior(res.lm, {"cam1.theta[cx]": 0.01, "revolute": 0.02}, sigma2=1.0)   # the names are make_prior's
    assert np.isfinite(again.sigma).sum() == 3 and again.names == res.lm.names


# ---- 8. past 32 parameters with real rendering -----------------------------------------------------------------------------------
def test_six_cameras_are_38_parameters(env, xarm7):
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.rig_calib import RigJointStep
    cfg, make, batch = problem(xarm7, 1, 48, 64, 0.05)
    qp = _views_qpos(xarm7, 1)
    six = RigJointStep([make() for _ in range(6)], [batch] * 6, xarm7, [qp] * 6, free=[1, 3])
    with pytest.raises(ValueError, match="38 parameters.*room for 5 cameras"):
        lm_rig.RigLM(six)
    with pytest.raises(ValueError, match="free_intrinsics needs solver='arrow'"):
        lm_rig.RigLM(six, free_intrinsics="f", solver="dense")
    o = lm_rig.RigLM(six, solver="arrow")
    assert o.N == 38 and o.state_block.shape == (_lib.LM_ARROW_STATE_DOUBLES,) == (11188,)
    o.iterate(3).finalize()
    torch.cuda.synchronize()
    for cam in six.cameras:
        fused.check_status(cam.glctx)
    s, tr = o.state(), o.trajectory()
    acc = tr[tr[:, 1] == 1, 0]
    print(f"[lm rig arrow N=38] losses {tr[:, 0].tolist()}, flags {tr[:, 1].tolist()}; F_acc {s.F_acc!r}")
    assert s.iterations == 3 and s.reported == 0 and (np.diff(acc) < 0).all() and acc[-1] == s.F_acc and s.F_acc <= tr[0, 0]
    assert o.report(s).H.shape[-2:] == (38, 38) and all(torch.equal(K, batch["K"][0].cpu()) for K in o.intrinsics())


# ---- 9. a reported iteration -------------------------------------------------------------------------------------------------
def test_reported_iteration_is_rig_wide_and_recovered(env, xarm7, monkeypatch):
    """tests/test_gpu_lm_rig.py's close-up under a slot-limited plan on camera 0, with every camera's focal length free: the
    first iterations are reported for the whole rig, camera 0's plan is made again with every slot, and the solve ends on the
    bits -- poses, Ks, offsets -- of a solve that had every slot."""
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.rig_calib import RigJointStep
    from test_gpu_fused import workload
    H, W, B = 64, 96, 2
    K, lp, Tc, _ = workload(xarm7, H, W, 0.075, B, seed=3)
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 2.5
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    ref = torch.zeros((B, H, W), device=DEV)
    ref[:, 10:50, 20:70] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=DEV),
             "K": torch.tensor(K, dtype=torch.float32, device=DEV)[None].repeat(B, 1, 1)}
    qp = _views_qpos(xarm7, B, seed=3)
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    ends = []
    for slack in ([None, 0.0], [0.0, 0.0]):
        models = [RBSolver(cfg, meshes=xarm7.meshes).to(DEV) for _ in range(2)]
        rig = RigJointStep(models, [batch, batch], xarm7, [qp, qp], slack=slack)
        res = lm_rig.solve_lm_rig(rig, max_iters=6, check_every=2, free_intrinsics="f")
        if slack[0] is None:
            assert res.reported >= 1 and res.recoveries == ["camera 0: job slots"] and [c.slack for c in rig.cameras] == [0.0, 0.0]
        else:
            assert res.reported == 0 and res.recoveries == []
        assert res.iterations - res.reported >= 6 or res.done
        _check_K(res.lm, "after the solve")
        ends.append(([m.dof.detach().clone() for m in models], rig.offsets.clone(), res, res.lm.intrinsics()))
    a, b = ends[0][2], ends[1][2]
    print(f"[lm rig arrow reported] limited plan: {a.reported} reported of {a.iterations}, F_acc {a.loss:.3f}, recoveries "
          f"{a.recoveries}; every slot: {b.iterations} iterations, F_acc {b.loss:.3f}")
    assert all(torch.equal(x, y) for x, y in zip(ends[0][0], ends[1][0])) and torch.equal(ends[0][1], ends[1][1])
    assert all(torch.equal(x, y) for x, y in zip(ends[0][3], ends[1][3]))
    assert a.loss == b.loss and (a.state.theta == b.state.theta).all() and (a.state.H == b.state.H).all()
    assert a.state.__dict__["lambda"] == b.state.__dict__["lambda"] and a.accepted == b.accepted


# ---- 10. beside Adam ---------------------------------------------------------------------------------------------------------
def test_lm_leaves_the_rigs_adam_state_alone_and_adam_runs_on_the_refined_K(env, xarm7):
    _lib, fused, dr, lm, lm_rig = env
    rig = _make_rig(xarm7, [1, 2, 3])
    for _ in range(5):
        rig.step()
    torch.cuda.synchronize()

    def snap():
        s = [rig.offset_exp_avg.clone(), rig.offset_exp_avg_sq.clone(), rig.offset_step_t.clone()]
        for cam in rig.cameras:
            s += [cam.exp_avg.clone(), cam.exp_avg_sq.clone(), cam.step_t.clone(), cam.hist_row.clone(), cam.model.history_ops.clone()]
        return s

    a = snap()
    given = [cam.K.clone() for cam in rig.cameras]
    res = lm_rig.solve_lm_rig(rig, max_iters=5, free_intrinsics=["f", None])
    torch.cuda.synchronize()
    for x, y in zip(a, snap()):
        assert torch.equal(x, y)
    Ks = res.lm.intrinsics()
    print(f"[lm rig arrow beside Adam] F_acc {res.loss!r}, {res.accepted} accepted of {res.iterations}; camera 0's focal lengths "
          f"{given[0][0, 0].item():.3f}, {given[0][1, 1].item():.3f} -> {Ks[0][0, 0].item():.3f}, {Ks[0][1, 1].item():.3f}")
    assert res.accepted >= 2 and int(rig.offset_step_t) == 5 and [int(cam.step_t) for cam in rig.cameras] == [5, 5]
    assert not torch.equal(Ks[0], given[0].cpu()) and torch.equal(Ks[1], given[1].cpu())
    assert res.report.names == res.lm.names == [f"cam0.dof[{i}]" for i in range(6)] + ["cam0.theta[f]"] + \
        [f"cam1.dof[{i}]" for i in range(6)] + [f"offset[{j}]" for j in (1, 2, 3)]
    assert (res.lm.parameters() == res.state.theta.astype(np.float32)).all() and (res.report.H == res.state.H).all()
    losses = torch.stack([rig.step().clone() for _ in range(5)])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all()) and int(rig.offset_step_t) == 10 and [int(cam.step_t) for cam in rig.cameras] == [10, 10]
    # the Adam steps rendered with the refined K: the rig's camera array holds the solve's buffer, and nobody rewrote it
    assert [row[2] for row in rig._cams_key] == [cam.K.data_ptr() for cam in rig.cameras]
    assert torch.equal(rig.cameras[0].K.cpu(), Ks[0])


# ---- 11. end to end against the CPU loop -------------------------------------------------------------------------------------
def test_end_to_end_against_the_cpu_loop(env, oracle, xarm7):
    """lm_rig_arrow_reference's scene: two gauge cameras a quarter turn apart, 4 views of 120x160 each, given focal lengths 3 %
    too long and 2 % too short, free joints [1, 3] from zero, the tied focal length of each camera free.  The GPU solve's
    accepted loss against the CPU loop's after RIG_EVALUATIONS evaluations, x 1.5: razor-edge pixels flip between the float32
    GPU render and the reference (tests/test_gpu_lm.py::test_solve_from_the_start_pose_against_the_cpu_loop's factor)."""
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.rig_calib import RigJointStep
    ps, Ks = AR.rig_problems(oracle, xarm7)
    models, batches, qps = [], [], []
    for p, K in zip(ps, Ks):
        cfg, batch, qp = IR.gauge_batch(p, DEV)
        batch["K"] = torch.tensor(K, device=DEV)[None].repeat(batch["mask"].shape[0], 1, 1)
        models.append(RBSolver(cfg, meshes=p.rb.meshes).to(DEV))
        batches.append(batch)
        qps.append(qp)
    rig = RigJointStep(models, batches, ps[0].rb, qps, free=list(AR.RIG_FREE_JOINTS))
    res = lm_rig.solve_lm_rig(rig, max_iters=12, free_intrinsics="f")
    want = AR.MEASURED["freed"]["F"]
    tr = res.trajectory
    print(f"[lm rig arrow end to end] first evaluation {tr[0, 0]:.2f} -> F_acc {res.loss:.2f} in {res.iterations} iterations "
          f"({res.accepted} accepted, {res.rejected} rejected, {res.reported} reported), stopped by {res.why}; the CPU loop after "
          f"{AR.RIG_EVALUATIONS} evaluations: {want:.2f} (freed), {AR.MEASURED['fixed']['F']:.2f} (K fixed)")
    for c, (p, K0, K) in enumerate(zip(ps, Ks, res.lm.intrinsics())):
        t, r = _pose_errors(rig.cameras[c].model, p.Tc)
        print(f"[lm rig arrow end to end] camera {c}: focal scale given {K0[0, 0] / p.K[0, 0]:.4f} -> recovered "
              f"{K[0, 0].item() / p.K[0, 0]:.4f}, {K[1, 1].item() / p.K[1, 1]:.4f}; pose error {t * 1e3:.2f} mm, {r:.3f} deg")
    print(f"[lm rig arrow end to end] offsets {np.degrees(rig.offsets.cpu().numpy()[list(AR.RIG_FREE_JOINTS)]).round(3).tolist()} deg (truth 0)")
    acc = tr[tr[:, 1] == 1, 0]
    assert (np.diff(acc) < 0).all() and acc[-1] == res.loss
    assert res.loss <= 1.5 * want
