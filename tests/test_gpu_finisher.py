"""The composite stage's finisher: one designated workgroup of the step's last composite launch waits until the arrival
counters of the eight XCDs hold the number of workgroups that had work -- a number every workgroup derives from the
launch's tables -- and then runs the finish stage (accumulators -> loss / gradient -> pose backward -> Adam).  These
cases sit at the ends of that count: launches where almost no workgroup has work, launches where every workgroup has
several items, the zero-fill form, and many consecutive launches eager and replayed from a graph (the counters re-arm)."""
import ctypes

import pytest
import torch

from test_gpu_fast import problem

pytestmark = pytest.mark.gpu

STATE = ["mvp", "tc_jac", "loss_b", "grad_mvp", "red", "loss", "grad", "exp_avg", "exp_avg_sq", "step_t"]


def _piecewise_step(fb, mb):
    """One solver step on (fb, mb) through the stand-alone kernels around the stateless ehr_render_mask_loss."""
    from easyhec_amd import _lib, fused
    lib = _lib.lib()
    f = lambda x: ctypes.c_float(float(x))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dof, hist = mb.dof.data, mb.history_ops
    _lib.check(lib.ehr_pose_forward(_lib.ptr(dof), _lib.ptr(fb.K), _lib.ptr(fb.link_poses), fb.B, fb.L, fb.H, fb.W,
                                    f(fb.near), f(fb.far), _lib.ptr(fb.mvp), _lib.ptr(fb.tc_jac),
                                    _lib.ptr(fb.hist_row), _lib.ptr(hist), hist.shape[0], stream), "fwd")
    fb.hist_row += 1
    fused._launch(fb.glctx, fb.scene, fb.mvp, fb.ref, None, fb.loss_b, fb.grad_mvp)
    _lib.check(lib.ehr_pose_backward(_lib.ptr(fb.grad_mvp), _lib.ptr(fb.loss_b), _lib.ptr(fb.K),
                                     _lib.ptr(fb.link_poses), _lib.ptr(fb.tc_jac), fb.B, fb.L, fb.H, fb.W,
                                     f(fb.near), f(fb.far), _lib.ptr(fb.red), stream), "bwd")
    _lib.check(lib.ehr_pose_adam(_lib.ptr(dof), _lib.ptr(fb.exp_avg), _lib.ptr(fb.exp_avg_sq), _lib.ptr(fb.step_t),
                                 _lib.ptr(fb.red), f(fb.lr), f(fb.betas[0]), f(fb.betas[1]), f(fb.eps), f(fb.wd),
                                 _lib.ptr(fb.loss), _lib.ptr(fb.grad), stream), "adam")


@pytest.mark.parametrize("B,H,W,scale,bound", [
    (1, 480, 640, 0.5, True),      # one view, bound reference: a few dozen of the 1536 workgroups have an item
    (8, 240, 320, 0.25, False),    # unbound reference: every tile of every view is an item
    (64, 120, 160, 0.125, True),   # 64 views: several (view, link) tables' worth of items
])
def test_solver_step_equals_the_stateless_path_at_both_ends_of_the_arrival_count(xarm7, B, H, W, scale, bound):
    """Loss, gradient and pose of ehr_solver_step against pose forward -> ehr_render_mask_loss -> pose backward -> Adam
    from the same state, bit for bit, over several steps."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, B, H, W, scale)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    fused.bind_ref(fb.glctx, fb.scene, None)  # the stateless path: every tile streams
    if not bound:
        fused.bind_ref(fa.glctx, fa.scene, None)
    for it in range(4):
        fa.step()
        _piecewise_step(fb, mb)
        torch.cuda.synchronize()
        for name in STATE + ["hist_row"]:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data)
        assert bool(torch.isfinite(fa.loss).all()) and float(fa.loss_b.min()) >= 0
    assert int(fa.step_t.item()) == 4
    fused.check_status(fa.glctx)


@pytest.mark.parametrize("B,L", [
    (1, 1),     # one (view, link) pair: a single thread row of the pose backward has work
    (22, 3),    # 66 pairs: two more than the finisher parks in LDS, and not a multiple of the 4 pairs a wave row takes
    (9, 7),     # 63 pairs: one short of the LDS window
])
def test_solver_step_equals_the_stateless_path_at_odd_pair_counts(xarm7, B, L):
    """The same bit-equality with the scene cut down to the first L links of the robot (reference masks rendered from that
    scene), at 160x120: pair counts B * L below 4, just below and just above the 64 link poses the finisher reads from LDS."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, B, 120, 160, 0.125, links=L)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    assert fa.B * fa.L == B * L and fa.scene.num_links == L
    fused.bind_ref(fb.glctx, fb.scene, None)
    for it in range(4):
        fa.step()
        _piecewise_step(fb, mb)
        torch.cuda.synchronize()
        for name in STATE + ["hist_row"]:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data)
        assert bool(torch.isfinite(fa.loss).all()) and float(fa.loss_b.min()) >= 0
    assert int(fa.step_t.item()) == 4 and float(fa.ref.sum()) > 0
    fused.check_status(fa.glctx)


def test_fifty_steps_eager_and_fifty_replayed_end_on_the_same_pose(xarm7):
    """The arrival counters are re-armed inside the launch: 50 eager steps and 50 replays of the captured step end on
    the same pose and optimiser state bit for bit, and the loss has moved (the steps were real ones)."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 3, 240, 320, 0.25)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    fb.capture()
    fa.step()
    fb.step()
    torch.cuda.synchronize()
    first = float(fa.loss)
    for _ in range(49):
        fa.step()
        fb.step()
    torch.cuda.synchronize()
    for name in STATE:
        assert torch.equal(getattr(fa, name), getattr(fb, name)), name
    assert torch.equal(ma.dof.data, mb.dof.data) and torch.equal(ma.history_ops[:50], mb.history_ops[:50])
    assert int(fa.step_t.item()) == 50 and int(fb.step_t.item()) == 50
    assert float(fa.loss) < first
    fused.check_status(fa.glctx)
    fused.check_status(fb.glctx)
    fb.release_graph()


@pytest.mark.parametrize("B,H,W,scale", [(1, 480, 640, 0.5), (3, 240, 320, 0.25)])
def test_with_mask_step_on_a_bound_reference_equals_the_unbound_form(xarm7, B, H, W, scale):
    """The zero-fill form (bound reference and a mask output) against the unbound form, which writes every tile itself:
    same mask, losses, gradient and pose, bit for bit, into a mask buffer that held garbage."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, B, H, W, scale)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    fused.bind_ref(fb.glctx, fb.scene, None)
    for it in range(3):
        fa.mask.fill_(float("nan"))
        fb.mask.fill_(float("nan"))
        fa.step(want_mask=True)
        fb.step(want_mask=True)
        torch.cuda.synchronize()
        assert torch.equal(fa.mask, fb.mask), it
        assert float(fa.mask.sum()) > 0 and float((fa.mask == 0).float().mean()) > 0.5
        for name in STATE:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data)
    fused.check_status(fa.glctx)
