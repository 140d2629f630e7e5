"""Which exchange a data-parallel ``FusedPoseStep`` attempts (``easyhec_amd.fast.choose_exchange``: a pure function of the
constructor's arguments, two environment variables and the process group's backend), and that the solo and the multi-start
steppers share one implementation of the step / capture / recovery protocol.  No process group, no device."""
import pytest

T, F = True, False

# (distributed, backend), rccl, p2p, EHR_COMM, EHR_TRY_RCCL -> (try_p2p, p2p_required, try_rccl, rccl_required)
CASES = [
    ((F, None), None, None, "", None, (F, F, F, F)),
    ((F, None), True, None, "", None, (F, F, T, T)),      # a single-rank communicator
    ((F, None), None, True, "", None, (F, F, F, F)),      # p2p is never attempted without a process group
    ((T, "nccl"), None, None, "", None, (T, F, T, F)),    # the default: p2p first, RCCL as the fall-back
    ((T, "gloo"), None, None, "", None, (F, F, F, F)),
    ((T, "gloo"), None, None, "", "1", (F, F, T, F)),
    ((T, "gloo"), None, None, "p2p", None, (T, F, F, F)),
    ((T, "nccl"), None, None, "rccl", None, (F, F, T, F)),
    ((T, "nccl"), None, None, "torch", None, (F, F, F, F)),
    ((T, "nccl"), True, None, "torch", None, (F, F, T, T)),
    ((T, "gloo"), None, True, "", None, (T, T, F, F)),
    ((T, "nccl"), False, None, "", None, (F, F, F, F)),   # an explicit rccl also switches the p2p default off
    ((T, "gloo"), None, False, "p2p", None, (F, F, F, F)),
]


@pytest.mark.parametrize("group,rccl,p2p,comm_env,try_rccl,want", CASES)
def test_choose_exchange_reproduces_the_selection_table(group, rccl, p2p, comm_env, try_rccl, want):
    from easyhec_amd.fast import choose_exchange
    distributed, backend = group
    ex = choose_exchange(rccl, p2p, comm_env, try_rccl, distributed, backend)
    assert (ex.try_p2p, ex.p2p_required, ex.try_rccl, ex.rccl_required) == want
    assert tuple(ex) == want + (distributed and rccl is None,)
    assert all(type(x) is bool for x in ex)


def test_a_successful_peer_memory_exchange_replaces_the_all_reduce():
    from easyhec_amd.fast import choose_exchange
    ex = choose_exchange(None, None, "", None, True, "nccl")
    assert ex.try_p2p and ex.try_rccl
    assert ex.after_p2p(True) == (True, False)    # (p2p, rccl): RCCL is not even attempted
    assert ex.after_p2p(False) == (False, True)   # a failed, non-mandatory attempt falls through to RCCL
    assert choose_exchange(None, None, "p2p", None, True, "gloo").after_p2p(False) == (False, False)


def test_the_two_steppers_share_the_chain_protocol():
    from easyhec_amd.chain_step import _ChainStep
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.multistart import MultiStartPoseStep
    for name in ("step", "_poll", "capture", "release_graph", "recover_from_overflow"):
        assert getattr(FusedPoseStep, name) is getattr(MultiStartPoseStep, name) is getattr(_ChainStep, name), name
        assert name not in FusedPoseStep.__dict__ and name not in MultiStartPoseStep.__dict__, name
