"""Checkpoints keep loading: for every stepper a state dict WRITTEN OUT here, in the layout DESIGN.md documents (6f, 6g, 6h:
torch.optim.Adam-shaped ``state`` / ``param_groups`` plus ``joint_offsets`` / ``intrinsics``), loads, and ``state_dict()``
returns it key for key and value for value.  The literals are the contract; they do not come from a ``state_dict()`` call."""
import pytest
import torch

from test_gpu_fast import problem
from test_gpu_joint_offsets import _views_qpos

pytestmark = pytest.mark.gpu

J = 9                      # xArm7's active joints: 7 arm + 2 gripper
FREE_J = [1, 2, 3, 4, 5, 6]
FREE_I = ["f", "cx"]
OFFSET_LR, OFFSET_WD, INTR_LR, INTR_WD = 0.002, 0.001, 0.001, 0.01


def _moments(n, seed, step):
    """A state entry of n elements whose values are exact in float32 and differ between entries."""
    k = torch.arange(1, n + 1, dtype=torch.float32)
    return {"step": torch.tensor(float(step)), "exp_avg": (k - seed) / 64.0, "exp_avg_sq": (k + seed) / 4096.0}


def _group(lr, wd, i):
    return {"lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": wd, "amsgrad": False, "maximize": False,
            "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False,
            "params": [i]}


def _offsets():
    off = torch.zeros(J)
    off[1:7] = torch.tensor([0.5, -0.25, 0.125, -0.0625, 0.03125, -0.015625]) / 16.0
    return off


def _same(a, b, path="sd"):
    assert type(a) is type(b), (path, type(a), type(b))
    if isinstance(a, dict):
        assert list(a.keys()) == list(b.keys()), (path, list(a.keys()), list(b.keys()))
        for k in a:
            _same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), (path, a, b)
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    elif torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device and torch.equal(a, b), (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.fixture(scope="module")
def scene(xarm7):
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    return make, batch, _views_qpos(xarm7, 2)


def _roundtrip(step, sd):
    step.load_state_dict(sd)
    _same(sd, step.state_dict())


def test_pose_step(scene):
    from easyhec_amd.fast import FusedPoseStep
    make, batch, _ = scene
    _roundtrip(FusedPoseStep(make(), batch),
               {"state": {0: _moments(6, 1, 7)}, "param_groups": [_group(0.003, 0.0005, 0)]})


def test_joint_step(scene, xarm7):
    from easyhec_amd.joint_calib import JointPoseStep
    make, batch, qp = scene
    js = JointPoseStep(make(), batch, xarm7, qp, offset_lr=OFFSET_LR, offset_weight_decay=OFFSET_WD)
    _roundtrip(js, {"state": {0: _moments(6, 1, 7), 1: _moments(J, 2, 5)},
                    "param_groups": [_group(0.003, 0.0005, 0), _group(OFFSET_LR, OFFSET_WD, 1)],
                    "joint_offsets": {"offsets": _offsets(), "free": FREE_J}})
    assert torch.equal(js.offsets.cpu(), _offsets()) and int(js.offset_step_t) == 5 and int(js.step_t) == 7


def test_intrinsics_step(scene):
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep, intrinsics_from_theta
    make, batch, _ = scene
    K0, theta = batch["K"][0].cpu(), torch.tensor([0.0078125, 0.0078125, -0.00390625, 0.0])
    st = IntrinsicsPoseStep(make(), batch, free=("f", "cx"), intrinsics_lr=INTR_LR, intrinsics_weight_decay=INTR_WD)
    _roundtrip(st, {"state": {0: _moments(6, 1, 7), 1: _moments(4, 3, 6)},
                    "param_groups": [_group(0.003, 0.0005, 0), _group(INTR_LR, INTR_WD, 1)],
                    "intrinsics": {"theta": theta, "K0": K0, "free": FREE_I, "group": 1}})
    assert torch.equal(st.K.cpu(), torch.from_numpy(intrinsics_from_theta(K0.numpy(), theta.numpy(), 120, 160)))


def test_joint_intrinsics_step(scene, xarm7):
    from easyhec_amd.intrinsics_calib import JointIntrinsicsPoseStep
    make, batch, qp = scene
    theta = torch.tensor([0.0078125, 0.0078125, -0.00390625, 0.0])
    st = JointIntrinsicsPoseStep(make(), batch, xarm7, qp, free_intrinsics=("f", "cx"), offset_lr=OFFSET_LR,
                                 offset_weight_decay=OFFSET_WD, intrinsics_lr=INTR_LR, intrinsics_weight_decay=INTR_WD)
    _roundtrip(st, {"state": {0: _moments(6, 1, 7), 1: _moments(J, 2, 5), 2: _moments(4, 3, 6)},
                    "param_groups": [_group(0.003, 0.0005, 0), _group(OFFSET_LR, OFFSET_WD, 1), _group(INTR_LR, INTR_WD, 2)],
                    "joint_offsets": {"offsets": _offsets(), "free": FREE_J},
                    "intrinsics": {"theta": theta, "K0": batch["K"][0].cpu(), "free": FREE_I, "group": 2}})


def test_two_camera_rig(scene, xarm7):
    from easyhec_amd.rig_calib import RigJointStep
    make, batch, qp = scene
    rig = RigJointStep([make(), make()], [batch, batch], xarm7, [qp, qp], offset_lr=OFFSET_LR, offset_weight_decay=OFFSET_WD)
    _roundtrip(rig, {"state": {0: _moments(6, 1, 7), 1: _moments(6, 4, 7), 2: _moments(J, 2, 7)},
                     "param_groups": [_group(0.003, 0.0005, 0), _group(0.003, 0.0005, 1), _group(OFFSET_LR, OFFSET_WD, 2)],
                     "joint_offsets": {"offsets": _offsets(), "free": FREE_J, "cameras": 2}})
    assert [int(c.step_t) for c in rig.cameras] == [7, 7] and torch.equal(rig.cameras[1].exp_avg.cpu(), _moments(6, 4, 7)["exp_avg"])
