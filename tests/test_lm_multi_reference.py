"""tests/lm_multi_reference.py and the host side of easyhec_amd/lm_multi.py pinned on the CPU: the multi update as a loop of
the solo reference, the scripted inputs of the update-kernel test (they show accept, reject, a report and a stop by
themselves), ``group_basins`` on hand-made poses, and the ranking of a ``MultiLmResult``."""
import numpy as np
import pytest

import lm_multi_reference as MR
import lm_reference as LR


def rot(axis, deg):
    a, (x, y, z) = np.radians(deg), np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def pose(t=(0, 0, 0), axis=(0, 0, 1), deg=0.0):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(axis, deg), t
    return T


def test_update_multi_is_a_loop_of_the_solo_update():
    N, P, Bv = 6, 3, 2
    calls = MR.scripted_calls(N, P, Bv)
    multi, dof = [LR.new_state() for _ in range(P)], MR.start_dof(P)
    solo, sdof = [LR.new_state() for _ in range(P)], MR.start_dof(P)
    for info, grad, count, loss in calls:
        MR.update_multi(multi, info, grad, count, loss, dof, Bv, N, ftol=MR.FTOL)
        for p in range(P):
            v = slice(p * Bv, (p + 1) * Bv)
            sdof[p, :N] = LR.update(solo[p], info[v], grad[v], count[v], loss[v], sdof[p, :N].copy(), MR.FTOL)
        assert dof.tobytes() == sdof.tobytes()
        for a, b in zip(multi, solo):
            assert (a.lam, a.nu, a.F_acc, a.iterations, a.accepted, a.rejected, a.reported, a.done) == \
                   (b.lam, b.nu, b.F_acc, b.iterations, b.accepted, b.rejected, b.reported, b.done)
            assert (a.theta == b.theta).all() and (a.H == b.H).all()
    # finalize: the accepted poses, nothing else
    before = [(s.lam, s.iterations) for s in multi]
    MR.update_multi(multi, *calls[0], dof, Bv, N, ftol=MR.FTOL, finalize=True)
    assert [(s.lam, s.iterations) for s in multi] == before
    assert all((dof[p, :N] == multi[p].theta.astype(np.float32)).all() for p in range(P))


@pytest.mark.parametrize("N", [1, 6])
@pytest.mark.parametrize("P,Bv", [(1, 1), (3, 2)])
def test_the_scripted_calls_show_accept_reject_report_and_stop(N, P, Bv):
    """The inputs of tests/test_gpu_lm_multi.py's update test do, by themselves, what ``SCRIPT`` says: checked here with
    ``lm_reference.update`` so that the GPU test can assert it on the solo kernel's states."""
    calls = MR.scripted_calls(N, P, Bv)
    assert len(calls) >= 6
    states, dof = [LR.new_state() for _ in range(P)], MR.start_dof(P)
    moved = []
    for c, (info, grad, count, loss) in enumerate(calls):
        prev = dof.copy()
        MR.update_multi(states, info, grad, count, loss, dof, Bv, N, ftol=MR.FTOL)
        for p, st in enumerate(states):
            last, done = MR.expected_flags(p, c)
            assert (st.last, st.done) == (last, done), (N, p, c, st.last, st.done, st.why)
        moved.append((dof != prev).any(axis=1))
    s0 = states[0]
    assert s0.accepted >= 2 and s0.rejected >= 1 and s0.done == 1 and s0.why == 1 and s0.iterations == 5
    if P > 1:
        assert states[1].reported == 1 and states[1].done == 0 and states[2].done == 0
        assert moved[-1][1] and not moved[-1][0]          # hypothesis 0 is done and stays; hypothesis 1 still moves
        # a different system per hypothesis
        assert not np.array_equal(calls[0][0][:Bv], calls[0][0][Bv:2 * Bv])


def test_system_is_the_solo_test_s_generator():
    info, grad, count, loss = MR.system(6, 3, 0)
    assert info.shape == (3, 6, 6) and grad.shape == (3, 6) and loss.dtype == np.float32
    assert all(np.linalg.eigvalsh(info[b]).min() > 0 for b in range(3)) and np.allclose(info, info.transpose(0, 2, 1), rtol=1e-12)

def test_group_basins():
    from easyhec_amd.lm_multi import group_basins
    # two clusters 5 mm apart
    poses = [pose((0, 0, 0)), pose((0.005, 0, 0)), pose((0.0002, 0, 0)), pose((0.0052, 0, 0))]
    assert group_basins(poses, [0, 1, 2, 3]) == [[0, 2], [1, 3]]
    assert group_basins(poses, [3, 2, 1, 0]) == [[3, 1], [2, 0]]
    # rotations: 0.05 degrees apart merge, 0.2 degrees apart do not; both tolerances must hold
    assert group_basins([pose(), pose(deg=0.05)], [0, 1]) == [[0, 1]]
    assert group_basins([pose(), pose(deg=0.2)], [0, 1]) == [[0], [1]]
    assert group_basins([pose(), pose((0.002, 0, 0), deg=0.05)], [0, 1]) == [[0], [1]]
    assert group_basins([pose(axis=(1, 2, 3), deg=40.0), pose(axis=(1, 2, 3), deg=40.05)], [1, 0]) == [[1, 0]]
    # rank order decides the representative: 0 -- 0.8 mm -- 1 -- 0.8 mm -- 2 in a row
    chain = [pose((0, 0, 0)), pose((0.0008, 0, 0)), pose((0.0016, 0, 0))]
    assert group_basins(chain, [0, 1, 2]) == [[0, 1], [2]]
    assert group_basins(chain, [1, 0, 2]) == [[1, 0, 2]]
    assert group_basins(chain, [2, 0, 1]) == [[2, 1], [0]]
    # a NaN pose comes last, in a basin of its own
    bad = np.full((4, 4), np.nan)
    assert group_basins([bad, pose(), pose((0.0001, 0, 0)), bad], [0, 3, 1, 2]) == [[1, 2], [0], [3]]
    # the tolerances are arguments
    assert group_basins(poses, [0, 1, 2, 3], trans_tol_m=0.01) == [[0, 1, 2, 3]]
    assert group_basins([pose(), pose(deg=0.2)], [0, 1], rot_tol_deg=0.25) == [[0, 1]]


def test_result_ranking_ties_go_to_the_lower_index():
    import types
    import torch
    from easyhec_amd import lm_multi
    P = 4
    losses = [3.0, 1.0, 1.0, float("nan")]

    def ns(p):
        return types.SimpleNamespace(F_acc=losses[p] if losses[p] == losses[p] else 0.0, accepted=int(losses[p] == losses[p]),
                                     rejected=0, reported=0, iterations=1, done=1, why=1, count=10, H=np.eye(6), g=np.zeros(6))

    class Fake:
        def __init__(self):
            self.P, self.dof, self.names = P, torch.zeros((P, 6)), list(lm_multi.NAMES)
            self.dof[:, 0] = torch.arange(P) * 0.01

        def state(self):
            return [ns(p) for p in range(P)]

        def trajectory(self, p):
            return np.zeros((1, 4))

        report = lm_multi.MultiStartLM.report

    res = lm_multi._result(Fake(), [])
    assert res.ranking == [1, 2, 0, 3] and res.winner == 1
    assert np.isnan(res.losses[3]) and res.losses.dtype == np.float64 and res.losses[:3].tolist() == [3.0, 1.0, 1.0]
    assert res.basins == [[1], [2], [0], [3]] and res.why == ["ftol"] * 4 and res.report.loss == 1.0
