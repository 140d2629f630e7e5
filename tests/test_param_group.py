"""``AdamGroup`` (the one parameter-group type under the pose, the joint offsets and the intrinsics) and the refusals every
calibration solve makes before it constructs a step: host logic, on the CPU."""
import pytest
import torch

from easyhec_amd.chain_step import check_solver_settings
from easyhec_amd.config import Cfg
from easyhec_amd.fast import refuse_unsupported
from easyhec_amd.param_group import AdamGroup

CPU = torch.device("cpu")
GROUP0 = {"lr": 0.003, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0005, "amsgrad": False, "params": [0]}


def test_a_fresh_group():
    g = AdamGroup(3, CPU, 0.002, 0.001, [0.5, -0.25, 0.0])
    assert g.param.dtype == torch.float32 and g.param.tolist() == [0.5, -0.25, 0.0]
    assert g.step_t.dtype == torch.int32 and g.step_t.tolist() == [0]
    for t in (g.exp_avg, g.exp_avg_sq, g.grad):
        assert t.dtype == torch.float32 and t.tolist() == [0.0, 0.0, 0.0]
    assert AdamGroup(6, CPU, 0.003, 0.0005).param is None          # (the pose: the model owns the parameter)
    e = g.state_entry()
    assert list(e) == ["step", "exp_avg", "exp_avg_sq"] and e["step"].shape == () and e["step"].dtype == torch.float32
    assert g.param_group(GROUP0, 2) == dict(GROUP0, lr=0.002, weight_decay=0.001, params=[2]) and GROUP0["params"] == [0]


def test_state_entry_is_a_copy_and_load_state_is_in_place():
    g = AdamGroup(2, CPU, 0.003, 0.0, [0.0, 0.0])
    views = (g.param, g.exp_avg, g.exp_avg_sq, g.step_t)
    saved = {"step": torch.tensor(5.0), "exp_avg": torch.tensor([0.25, -0.5]), "exp_avg_sq": torch.tensor([0.125, 0.0625])}
    g.load_state(saved, [1.0, 2.0])
    assert all(a is b for a, b in zip(views, (g.param, g.exp_avg, g.exp_avg_sq, g.step_t)))
    assert g.param.tolist() == [1.0, 2.0] and g.step_t.tolist() == [5]
    e = g.state_entry()
    assert float(e["step"]) == 5.0 and torch.equal(e["exp_avg"], saved["exp_avg"]) and torch.equal(e["exp_avg_sq"], saved["exp_avg_sq"])
    e["exp_avg"].zero_()
    assert g.exp_avg.tolist() == [0.25, -0.5]
    g.load_state(None)                                           # (a state without the group: everything stays)
    g.load_state(None, [3.0, 4.0])                               # (the parameters alone)
    assert g.param.tolist() == [3.0, 4.0] and g.exp_avg.tolist() == [0.25, -0.5] and g.step_t.tolist() == [5]
    with pytest.raises(RuntimeError):
        g.load_state(dict(saved, exp_avg=torch.zeros(3)))        # (another group's moments)


def test_check_saved_refuses_other_settings_in_the_callers_words():
    g = AdamGroup(2, CPU, 0.002, 0.001, [0.0, 0.0])
    g.check_saved({"lr": 0.002, "weight_decay": 0.001}, "the offsets' group", "step")
    g.check_saved({}, "the offsets' group", "step")              # (settings that were not saved are not judged)
    with pytest.raises(ValueError, match=r"the offsets' group was saved with lr 0.004 / weight decay 0.001, this step has 0.002 / 0.001"):
        g.check_saved({"lr": 0.004, "weight_decay": 0.001}, "the offsets' group", "step")
    with pytest.raises(ValueError, match=r"group 2 was saved with lr 0.002 / weight decay 0.0, this rig has"):
        g.check_saved({"lr": 0.002, "weight_decay": 0.0}, "group 2", "rig")


def test_refusals_keep_their_order_and_the_callers_wording():
    msgs = ("no multi-start: why", "no data-parallel job: why", "no kernel: rebuild")
    never = lambda: pytest.fail("the library was asked although the call is refused anyway")
    with pytest.raises(ValueError, match="no multi-start: why"):
        refuse_unsupported({"starts": None, "rccl": True}, never, *msgs)
    for kw in ({"rccl": True}, {"p2p": True}):
        with pytest.raises(ValueError, match="no data-parallel job: why"):
            refuse_unsupported(kw, never, *msgs)
    with pytest.raises(RuntimeError, match="no kernel: rebuild"):
        refuse_unsupported({"lr": 0.1}, lambda: False, *msgs)
    refuse_unsupported({"lr": 0.1, "rccl": None, "p2p": False}, lambda: True, *msgs)


def test_solver_settings_check():
    cfg = Cfg()
    assert check_solver_settings(cfg) == {"lr": cfg.solver.max_lr, "weight_decay": cfg.solver.weight_decay}
    cfg.solver.do_grad_clip = True
    with pytest.raises(ValueError, match="^the launch chain implements the reference's default solver only"):
        check_solver_settings(cfg)
    cfg.solver.do_grad_clip, cfg.solver.optimizer = False, "SGD"
    with pytest.raises(ValueError, match="^fast path implements the reference's default solver only"):
        check_solver_settings(cfg, "fast path")
