"""The polling loop under ``solve_lm`` and ``solve_lm_multi`` (``easyhec_amd.lm._run_to_convergence``), driven by a fake
driver: no device, no library.  The fake's ``states()`` returns namespaces of ``iterations``, ``reported`` and ``done`` --
all the loop reads -- and its ``iterate(n)`` advances every hypothesis that is not done by n iterations, of which a script
says how many are reported.  Also: the job-slot rule of ``chain_step._PlannedContext`` against the five lines both former
copies consisted of."""
import types

import pytest

MAX_ITERS, CHECK_EVERY = 12, 5


class FakeDriver:
    """P hypotheses.  ``done_after[p]``: hypothesis p is done once it has taken that many iterations (None: never; 0: from
    the start); a done hypothesis's ``iterations`` stays frozen.  ``reports``: per ``iterate`` call, how many of its
    iterations are reported for every running hypothesis (missing: 0)."""

    def __init__(self, done_after, reports=()):
        self.P = len(done_after)
        self.done_after, self.reports = list(done_after), list(reports)
        self.iterations, self.reported = [0] * self.P, [0] * self.P
        self.iterate_args, self.finalized, self.reads = [], 0, 0

    def _done(self, p):
        return self.done_after[p] is not None and self.iterations[p] >= self.done_after[p]

    def states(self):
        self.reads += 1
        return [types.SimpleNamespace(iterations=self.iterations[p], reported=self.reported[p], done=int(self._done(p)))
                for p in range(self.P)]

    def iterate(self, n):
        assert self.finalized == 0 and n >= 1
        k = len(self.iterate_args)
        rep = self.reports[k] if k < len(self.reports) else 0
        self.iterate_args.append(n)
        for p in range(self.P):
            if not self._done(p):
                self.iterations[p] += n
                self.reported[p] += min(rep, n)
        return self

    def finalize(self):
        self.finalized += 1
        return self


class Hooks:
    def __init__(self, answers="job slots"):
        self.answers, self.recovered, self.status_checks = answers, 0, 0

    def recover(self):
        self.recovered += 1
        a = self.answers
        return a if not isinstance(a, list) else a[self.recovered - 1]

    def check_status(self):
        self.status_checks += 1


def run(driver, hooks=None, who="solve_lm"):
    from easyhec_amd.lm import _run_to_convergence
    hooks = hooks or Hooks()
    return _run_to_convergence(driver, MAX_ITERS, CHECK_EVERY, hooks.recover, hooks.check_status, who), hooks


def test_a_one_hypothesis_never_done_nothing_reported():
    d = FakeDriver([None])
    rec, h = run(d)
    assert d.iterate_args == [5, 5, 2] and d.finalized == 1 and h.recovered == 0 and rec == [] and h.status_checks == 0
    assert d.reads == 4  # one read per round: three rounds that iterate, one that stops


def test_b_reported_iterations_are_recovered_from_and_taken_again():
    d = FakeDriver([None], reports=[2])
    rec, h = run(d)
    # effective 3 after the first batch, then 8, then 12
    assert d.iterate_args == [5, 5, 4] and h.recovered == 1 and rec == ["job slots"] and d.finalized == 1
    assert d.iterations[0] - d.reported[0] == MAX_ITERS and h.status_checks == 0


def test_c_one_hypothesis_done_after_the_first_batch():
    d = FakeDriver([5])
    rec, h = run(d)
    assert d.iterate_args == [5] and d.finalized == 1 and rec == [] and h.recovered == 0


def test_d_a_done_hypothesis_neither_stops_nor_prolongs_the_loop():
    d = FakeDriver([5, None])
    rec, h = run(d, who="solve_lm_multi")
    assert d.iterate_args == [5, 5, 2] and d.finalized == 1 and rec == []
    assert d.iterations == [5, 12]  # hypothesis 0 frozen at 5: neither `min` nor the stop looks at it


def test_e_every_hypothesis_done_stops_the_loop():
    d = FakeDriver([5, 3])
    run(d)
    assert d.iterate_args == [5] and d.finalized == 1
    d = FakeDriver([0, 0])  # done from the start: nothing is enqueued, the accepted parameters are still put back
    run(d)
    assert d.iterate_args == [] and d.finalized == 1


def test_f_reports_in_every_round_raise_after_four_recoveries():
    d = FakeDriver([None, None], reports=[1] * 10)
    h = Hooks()
    with pytest.raises(RuntimeError, match="solve_lm_multi: iterations keep being reported"):
        run(d, h, who="solve_lm_multi")
    # the status hook runs on the fifth rise, after the fifth recovery attempt and before the raise
    assert h.recovered == 5 and h.status_checks == 1 and d.finalized == 0 and len(d.iterate_args) == 5


def test_f_four_rounds_of_reports_are_still_recovered_from():
    d = FakeDriver([None], reports=[1, 1, 1, 1])
    rec, h = run(d)
    assert rec == ["job slots"] * 4 and h.recovered == 4 and h.status_checks == 0 and d.finalized == 1
    assert d.iterations[0] - d.reported[0] == MAX_ITERS


def test_g_a_recovery_that_found_nothing_is_not_noted():
    d = FakeDriver([None], reports=[2, 1])
    rec, h = run(d, Hooks([False, "general-triangle pass"]))
    assert h.recovered == 2 and rec == ["general-triangle pass"] and d.finalized == 1


def test_the_sum_of_reported_counts_not_each_hypothesis():
    """A rise of ANY hypothesis's ``reported`` is a rise of the sum: one recovery per round, not one per hypothesis."""
    d = FakeDriver([None, None, None], reports=[1])
    rec, h = run(d)
    assert h.recovered == 1 and rec == ["job slots"]


# ---- the job-slot rule: one copy, equal to what the solo steppers and MultiStartLM each had ----------------------------------
def former_rule(slack, env, H, W):
    """The five lines ``_ChainStep._init_chain`` and ``MultiStartLM.__init__`` both consisted of."""
    if slack is None and "EHR_VB_SLACK" not in env:
        ntiles = ((W + 31) // 32) * ((H + 7) // 8)
        return max(0.5, 256.0 / ntiles)
    return float(env["EHR_VB_SLACK"]) if slack is None else float(slack)


@pytest.mark.parametrize("user", ["_ChainStep", "MultiStartPoseStep", "MultiStartLM"])
@pytest.mark.parametrize("HW", [(64, 96), (120, 160), (720, 1280)])
@pytest.mark.parametrize("env", [None, "0", "1.0"])
@pytest.mark.parametrize("slack", [None, 0, 0.5, 2])
def test_slack_rule_is_the_former_rule_for_both_users(monkeypatch, slack, env, HW, user):
    from easyhec_amd import chain_step, lm_multi, multistart
    cls = {"_ChainStep": chain_step._ChainStep, "MultiStartPoseStep": multistart.MultiStartPoseStep,
           "MultiStartLM": lm_multi.MultiStartLM}[user]
    assert cls._init_plan is chain_step._PlannedContext._init_plan and "_init_plan" not in cls.__dict__
    assert cls._plan_and_bind is chain_step._PlannedContext._plan_and_bind
    if env is None:
        monkeypatch.delenv("EHR_VB_SLACK", raising=False)
    else:
        monkeypatch.setenv("EHR_VB_SLACK", env)
    obj = cls.__new__(cls)
    obj.H, obj.W = HW
    planned = []
    obj._plan_and_bind = lambda: planned.append(obj.slack)  # (no device here: the rule is what is under test)
    obj._init_plan(slack)
    want = former_rule(slack, {} if env is None else {"EHR_VB_SLACK": env}, *HW)
    assert obj.slack == want and type(obj.slack) is float and planned == [want]
    if slack is None and env is None:
        assert want == {(64, 96): 256.0 / 24, (120, 160): 256.0 / 75, (720, 1280): 0.5}[HW]
