"""The rig's Levenberg-Marquardt update under a Gaussian prior on the GPU (``ehr_lm_update_rig_prior``: csrc/ehr_lm.hip,
easyhec_amd/lm_rig.py): the update kernel alone -- one camera against the solo kernel under the same prior
(bytes), two and five cameras (N = 32) against the numpy restatement of tests/lm_prior_reference.py -- no prior against today's
entry point (bytes), a bad prior reported rig-wide, and the one-camera rig's solve against ``solve_lm`` under the same prior.
tests/test_gpu_lm_prior.py holds the solo form and the bars; every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import lm_prior_reference as PR
import lm_rig_reference as RR
from test_gpu_fast import problem
from test_gpu_joint_offsets import _views_qpos
from test_gpu_lm import DEV, _stream, t32
from test_gpu_lm_prior import PUpd, compare_prior, f64, pref_state
from test_gpu_lm_rig import RigUpd, _ns

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, fused, lm, lm_rig
    assert _lib.has_lm_prior() and _lib.has_lm_rig()
    return _lib, fused, lm, lm_rig


class PRigUpd(RigUpd):
    """test_gpu_lm_rig.RigUpd through the entry point that takes a prior.  entry: "plain" (ehr_lm_update_rig) or "prior"
    (ehr_lm_update_rig_prior with ``weight`` / ``mean``; both None: NULL, NULL)."""

    def __init__(self, _lib, C, F, Bs, weight=None, mean=None, entry="prior", **kw):
        super().__init__(_lib, C, F, Bs, **kw)
        self.entry = entry
        self.set_prior(weight, mean)

    def set_prior(self, weight, mean):
        self.weight, self.mean = weight, mean
        self.w_dev = None if weight is None else f64(weight)
        self.m_dev = None if mean is None else f64(mean)

    def call(self, cams, ftol=RR.FTOL, lambda_max=1e6, finalize=0):
        _lib = self._lib
        dev = [(f64(i), f64(g), torch.tensor(np.ascontiguousarray(c, np.int64), device=DEV), t32(l)) for i, g, c, l in cams]
        arr = (_lib.LmRigCamera * self.C)(*[_lib.LmRigCamera(i.data_ptr(), g.data_ptr(), c.data_ptr(), l.data_ptr(), d.data_ptr(), B)
                                            for (i, g, c, l), d, B in zip(dev, self.dofs, self.Bs)])
        args = (arr, self.C, _lib.ptr(self.offset if self.F else None), _lib.ptr(self.free_list), self.F, self.J,
                ctypes.c_double(ftol), ctypes.c_double(lambda_max), finalize, _lib.ptr(self.state), _lib.ptr(self.log), 64)
        with torch.cuda.device(DEV):
            if self.entry == "plain":
                _lib.check(_lib.lib().ehr_lm_update_rig(*args, _stream()), "ehr_lm_update_rig")
            else:
                _lib.check(_lib.lib().ehr_lm_update_rig_prior(*args, _lib.ptr(self.w_dev), _lib.ptr(self.m_dev), _stream()),
                           "ehr_lm_update_rig_prior")
            for i, g, c, l in dev:
                i.fill_(float("nan")), g.fill_(float("nan")), l.fill_(float("nan")), c.fill_(-7)
        torch.cuda.synchronize()
        return _ns(_lib, self.state, self.N)


def rig_prior(u, cams, seed=0):
    """A prior on a SUBSET of the rig's parameters (cam0.dof[0] always free of it, the last parameter always has one): weights
    of the order of the gathered system's own diagonal, means a small step from the start."""
    N = u.N
    rng = np.random.default_rng(900 + N + seed)
    d = np.diag(RR.gather(cams)[0])
    w = np.where(rng.uniform(size=N) < 0.5, d * 10.0 ** rng.uniform(-2, 1, N), 0.0)
    w[0], w[N - 1] = 0.0, d[N - 1] * 0.5
    mean = u.params().astype(np.float64) + rng.normal(size=N) * 1e-3 / np.sqrt(np.where(d > 0, d, 1.0)) * np.sqrt(d.max())
    return w, mean


def _rig_prior_sequence(_lib, C, F, Bs, worst):
    """lm_rig_reference's scripted calls (first, accept, reject, two reported, an accept with a zeroed parameter, finalize)
    under a prior; the zeroed parameter is the last one, which HAS a prior: it is not left out."""
    u = PRigUpd(_lib, C, F, Bs)
    calls = RR.scripted_calls(C, F, Bs)
    w, mean = rig_prior(u, calls[0][1])
    u.set_prior(w, mean)
    accepted, z = None, RR.zeroed_parameter(C, F)
    for what, cams in calls:
        before, now = pref_state(_ns(_lib, u.state, u.N)), u.params()
        fin = what == "finalize"
        raw = u.state.cpu().numpy().copy()
        ns = u.call(cams, finalize=int(fin))
        want = PR.update_rig(before, cams, now, w, mean, RR.FTOL, 1e6, fin)
        compare_prior(ns, before, u.params(), want, f"C={C} F={F} {what}", worst)
        if what in ("nan-loss", "bad-count", "finalize"):
            assert u.params().tobytes() == accepted.tobytes() == want.tobytes(), what
            assert fin or ns.last == -1
            assert ns.__dict__["lambda"] == before.lam
        if fin:
            assert ns.raw.tobytes() == raw.tobytes()
        if ns.last == 1 and not fin:
            accepted = ns.theta.astype(np.float32)
        if what == "zero-diagonal":
            assert ns.H[z, z] == 0.0 and ns.g[z] == 0.0 and ns.delta[z] != 0.0            # the prior alone moves it
            assert np.sign(ns.delta[z]) == np.sign(mean[z] - ns.theta[z])
    assert (ns.accepted, ns.rejected, ns.reported, ns.iterations, ns.done) == (3, 1, 2, 6, 0) and ns.F_prior > 0
    return u


@pytest.mark.parametrize("C,F,Bs", [(2, 2, [2, 3]), (5, 2, [2, 2, 2, 2, 2])])
def test_rig_update_kernel_alone_under_a_prior(env, C, F, Bs):
    _lib = env[0]
    worst = [0.0, 0.0]
    a = _rig_prior_sequence(_lib, C, F, Bs, worst)
    print(f"[lm rig prior update] C={C} F={F} B={Bs} (N={6 * C + F}): prior on {int((a.weight != 0).sum())} parameters; worst "
          f"|y - y_ref| / (32 2^-53 cond |y|) = {worst[0]:.4f}, the same for pred = {worst[1]:.4f}")
    b = _rig_prior_sequence(_lib, C, F, Bs, [0.0, 0.0])                            # two runs: identical bits
    for x, y in [(a.state, b.state), (a.offset, b.offset), (a.log, b.log)] + list(zip(a.dofs, b.dofs)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_one_camera_rig_kernel_is_the_solo_kernel_under_the_same_prior(env):
    """(C, F, B_c) = (1, 3, [2]): the rig's kernel and the solo kernel on the same inputs, parameters and prior -- state block,
    log, dof and offsets byte for byte."""
    _lib = env[0]
    C, F, Bs = 1, 3, [2]
    N = 9
    r = PRigUpd(_lib, C, F, Bs)
    s = PUpd(_lib, 7, 0)                                  # (any solo shape: its tensors are replaced by the rig's values)
    s.N, s.F, s.mask, s.tie, s.els = N, F, 0, 0, []
    s.free, s.free_list = r.free, r.free_list.clone()
    s.dof, s.offset = r.dofs[0].clone(), r.offset.clone()
    calls = RR.scripted_calls(C, F, Bs)
    w, mean = rig_prior(r, calls[0][1])
    r.set_prior(w, mean)
    s.set_prior(w, mean)
    for what, cams in calls:
        fin = int(what == "finalize")
        nr = r.call(cams, finalize=fin)
        info, grad, count, loss = cams[0]
        nsolo = s.call(info, grad, count, loss, ftol=RR.FTOL, finalize=fin)
        for name, x, y in (("state", r.state, s.state), ("log", r.log, s.log), ("dof", r.dofs[0], s.dof), ("offset", r.offset, s.offset)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (what, name)
    print(f"[lm rig prior C=1] F_acc {nr.F_acc!r} (prior {nr.F_prior!r}); {int(nr.accepted)} accepted, {int(nr.rejected)} rejected, "
          f"{int(nr.reported)} reported: the solo kernel's bytes")
    assert (nr.accepted, nr.rejected, nr.reported) == (3, 1, 2) and nr.F_prior > 0


def test_no_prior_is_todays_rig_update_byte_for_byte(env):
    _lib = env[0]
    C, F, Bs = 2, 2, [2, 3]
    N = 6 * C + F
    mean = np.random.default_rng(1).normal(size=N)
    mean[3] = np.nan
    runs = [PRigUpd(_lib, C, F, Bs, entry="plain"), PRigUpd(_lib, C, F, Bs), PRigUpd(_lib, C, F, Bs, np.zeros(N), mean)]
    for u in runs:
        for what, cams in RR.scripted_calls(C, F, Bs):
            u.call(cams, finalize=int(what == "finalize"))
    a = runs[0]
    assert a.state[_lib.LM_STATE["F_prior"]].item() == 0.0 and a.state[_lib.LM_STATE["accepted"]].item() == 3
    for what, b in (("NULL, NULL", runs[1]), ("all-zero weights", runs[2])):
        for name, x, y in [("state", a.state, b.state), ("log", a.log, b.log), ("offset", a.offset, b.offset)] + \
                [(f"dof {c}", a.dofs[c], b.dofs[c]) for c in range(C)]:
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (what, name)


def test_bad_prior_reports_the_call_rig_wide(env):
    _lib = env[0]
    C, F, Bs = 2, 2, [2, 3]
    u = PRigUpd(_lib, C, F, Bs)
    calls = RR.scripted_calls(C, F, Bs)
    w, mean = rig_prior(u, calls[0][1])
    u.set_prior(w, mean)
    worst = [0.0, 0.0]
    ns = u.call(calls[0][1])
    accepted, lam = ns.theta.astype(np.float32), ns.__dict__["lambda"]
    assert (u.params()[:6] != accepted[:6]).any() and (u.params()[6:12] != accepted[6:12]).any()
    k = u.N - 1
    for i, what in enumerate(("NaN mean under a positive weight", "negative weight", "infinite weight")):
        w2, m2 = w.copy(), mean.copy()
        if i == 0:
            m2[k] = np.nan
        elif i == 1:
            w2[k] = -w[k]
        else:
            w2[k] = np.inf
        for d in u.dofs:
            d.add_(0.25)                                                          # a trial is in every camera's pointers
        u.set_prior(w2, m2)
        before, now = pref_state(_ns(_lib, u.state, u.N)), u.params()
        ns = u.call(calls[1][1])
        want = PR.update_rig(before, calls[1][1], now, w2, m2, RR.FTOL)
        compare_prior(ns, before, u.params(), want, what, worst)
        assert ns.reported == i + 1 and ns.last == -1 and ns.__dict__["lambda"] == lam
        assert u.params().tobytes() == accepted.tobytes()                          # every camera's pose and the offsets


# ---- the solve ---------------------------------------------------------------------------------------------------------------
def test_one_camera_rig_solve_under_a_prior_is_the_solo_solve(env, xarm7):
    """solve_lm_rig(prior_sigma="default") on a one-camera rig against solve_lm(prior_sigma="default") on the JointPoseStep, 8
    iterations: the default prior holds the offsets and no pose coordinate under either naming (``cam0.dof[i]`` / ``dof[i]``),
    sigma2 comes from each solve's own evaluation at the start -- state block, log, dof, offsets and link poses byte for byte."""
    _lib, fused, lm, lm_rig = env
    from easyhec_amd.info_explorer import PRIOR_SIGMA
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.rig_calib import RigJointStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    mj, mr = make(), make()
    js = JointPoseStep(mj, batch, xarm7, qp, free=[1, 2, 3])
    rig = RigJointStep([mr], [batch], xarm7, [qp], free=[1, 2, 3])
    a = lm.solve_lm(js, max_iters=8, check_every=4, prior_sigma="default")
    b = lm_rig.solve_lm_rig(rig, max_iters=8, check_every=4, prior_sigma="default")
    torch.cuda.synchronize()
    fused.check_status(js.glctx), fused.check_status(rig.cameras[0].glctx)
    print(f"[lm rig prior C=1] solo: loss {a.loss!r} = data {a.data_loss!r} + prior {a.prior_loss!r}, {a.accepted} accepted of "
          f"{a.iterations}; rig: loss {b.loss!r}, {b.accepted} accepted of {b.iterations}; sigma2 {a.prior.sigma2!r} / {b.prior.sigma2!r}")
    assert b.prior.names == [f"cam0.dof[{i}]" for i in range(6)] + ["offset[1]", "offset[2]", "offset[3]"]
    assert a.prior.sigma2 == b.prior.sigma2 and torch.equal(a.prior.weight, b.prior.weight) and torch.equal(a.prior.mean, b.prior.mean)
    assert a.prior.weight.cpu().numpy().tolist() == [0.0] * 6 + [a.prior.sigma2 / PRIOR_SIGMA["revolute"] ** 2] * 3
    for what, x, y in (("state block", a.lm.state_block, b.lm.state_block), ("log", a.lm.log, b.lm.log),
                       ("dof", mj.dof.detach(), mr.dof.detach()), ("offsets", js.offsets, rig.offsets),
                       ("link_poses", js.link_poses, rig.cameras[0].link_poses)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), what
    assert a.accepted >= 2 and a.iterations >= 8 and a.prior_loss > 0 and b.posterior.H_views.shape == (2, 9, 9)


def test_rig_refusals(env, xarm7):
    _lib, fused, lm, lm_rig = env
    from easyhec_amd.rig_calib import RigJointStep
    cfg, make, batch = problem(xarm7, 1, 48, 64, 0.05)
    qp = _views_qpos(xarm7, 1)
    rig = RigJointStep([make(), make()], [batch, batch], xarm7, [qp, qp], free=[1, 3])
    o = lm_rig.RigLM(rig)
    pr = lm.make_prior(o, {"rotation": 0.2, "cam1.dof[0]": 0.01, "offset[3]": 0.02}, sigma2=4.0)
    want = np.zeros(14)
    want[[3, 4, 5, 9, 10, 11]], want[6], want[13] = 4.0 / 0.2 ** 2, 4.0 / 0.01 ** 2, 4.0 / 0.02 ** 2
    assert pr.weight.cpu().numpy().tolist() == want.tolist() and np.isinf(pr.sigma[12])
    assert pr.mean.cpu().numpy()[6] == float(rig.cameras[1].model.dof[0].item())   # a pose coordinate: its value now
    for kw, match in ((dict(prior_sigma={"dof[0]": 0.1}), "keys are parameter names"), (dict(prior_sigma=[0.1] * 8), "sequence of N = 14"),
                      (dict(prior_sigma=-0.1), "every sigma is > 0"), (dict(prior_sigma=0.1, sigma2=0.0), "sigma2 must be finite")):
        with pytest.raises(ValueError, match=match):
            lm.make_prior(o, sigma2=kw.pop("sigma2", 1.0), **kw)
    with pytest.raises(ValueError, match="pass prior_sigma as well"):
        lm_rig.solve_lm_rig(rig, prior_mean={"offset[1]": 0.0})
