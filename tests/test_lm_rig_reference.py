"""tests/lm_rig_reference.py on the CPU: with one camera the rig's update IS ``lm_reference.update``; the embedding is
``rig_information``'s ``np.ix_`` rule; the blocks between two different cameras' poses are exactly zero; a bad camera reports
the call for the whole rig.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import lm_multi_reference as MR
import lm_reference as LR
import lm_rig_reference as RR

FTOL = MR.FTOL
STATE_FIELDS = ("lam", "nu", "F_acc", "pred", "rho", "F_trial", "iterations", "accepted", "rejected", "reported", "done", "why",
                "last", "count", "retries")


def _same_state(a, b):
    for k in STATE_FIELDS:
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))
    for k in ("theta", "delta", "g", "H"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), k


def test_one_camera_is_lm_reference_update():
    """accept, accept, reject, reported, finalize on SPD systems: every state field and the returned parameters are equal."""
    F, B = 3, 2
    N = 6 + F
    base = MR.system(N, B, MR.SEED0)[3]
    script = [(1.0, "a"), (0.9, "a"), (1.5, "r"), (0.8, "n"), (0.7, "f")]
    a, b = LR.new_state(), LR.new_state()
    ta = tb = np.random.default_rng(3).uniform(-1, 1, N).astype(np.float32)
    for call, (factor, what) in enumerate(script):
        info, grad, count, _ = MR.system(N, B, MR.SEED0 + call)
        loss = (base * np.float32(factor)).astype(np.float32)
        if what == "n":
            grad = grad.copy()
            grad[B - 1, N - 1] = np.nan
        fin = what == "f"
        ta = LR.update(a, info, grad, count, loss, ta, FTOL, 1e6, fin)
        tb = RR.update_rig(b, [(info, grad, count, loss)], tb, FTOL, 1e6, fin)
        print(f"[rig reference] C=1 call {call} ({what}): last {b.last}, lambda {b.lam!r}, F_acc {b.F_acc!r}")
        _same_state(a, b)
        assert ta.tobytes() == tb.tobytes()
        assert b.last == {"a": 1, "r": 0, "n": -1, "f": -1}[what]
    assert (b.accepted, b.rejected, b.reported, b.iterations, b.done) == (2, 1, 1, 4, 0)
    assert np.array_equal(tb, b.theta.astype(np.float32))      # reported, then finalize: the accepted parameters


def test_embedding_is_rig_informations_rule_and_cross_camera_blocks_are_zero():
    C, F, Bs = 3, 2, [2, 1, 3]
    N, Nc = 6 * C + F, 6 + F
    rng = np.random.default_rng(11)
    cams = [(rng.normal(size=(B, Nc, Nc)), rng.normal(size=(B, Nc)), rng.integers(1, 50, B), rng.uniform(1, 9, B).astype(np.float32))
            for B in Bs]
    H, g, Fsum, count, bad = RR.gather(cams)
    want_H, want_g = np.zeros((N, N)), np.zeros(N)
    for c, (info, grad, _, _) in enumerate(cams):              # rig_information, word for word
        Hc, gc = np.zeros((N, N)), np.zeros(N)
        idx = list(range(6 * c, 6 * c + 6)) + list(range(6 * C, N))
        S, s = np.zeros((Nc, Nc)), np.zeros(Nc)
        for b in range(info.shape[0]):
            S, s = S + info[b], s + grad[b]
        Hc[np.ix_(idx, idx)] = S
        gc[idx] = s
        want_H, want_g = want_H + Hc, want_g + gc
    print(f"[rig reference] C=3 F=2: max |H - rule| {np.abs(H - want_H).max()}, max |g - rule| {np.abs(g - want_g).max()}")
    assert np.array_equal(H, want_H) and np.array_equal(g, want_g) and not bad
    assert count == sum(int(c[2].sum()) for c in cams)
    want_F = 0.0
    for _, _, _, loss in cams:
        Fc = 0.0
        for x in loss:
            Fc += float(x)
        want_F += Fc
    assert Fsum == want_F
    for a in range(C):
        for b in range(C):
            block = H[6 * a:6 * a + 6, 6 * b:6 * b + 6]
            if a != b:
                assert (block == 0).all() and not np.signbit(block).any(), (a, b)
            else:
                assert (block != 0).all()
    assert (H[6 * C:, 6 * C:] != 0).all() and (H[:6 * C, 6 * C:] != 0).all()
    assert RR.embed_index(1, C, F) == [6, 7, 8, 9, 10, 11, 18, 19]


@pytest.mark.parametrize("C,F,Bs", RR.SHAPES)
def test_the_script_does_what_it_says(C, F, Bs):
    """The GPU update test's calls, on the reference: every call leaves the flag SCRIPT names, none stops the solve, the
    zeroed parameter does not move and every other one does."""
    N = 6 * C + F
    st = LR.new_state()
    theta = np.random.default_rng(7).uniform(-1, 1, N).astype(np.float32)
    margin = np.inf
    for what, cams in RR.scripted_calls(C, F, Bs):
        theta = RR.update_rig(st, cams, theta, RR.FTOL, 1e6, what == "finalize")
        want = dict((w, l) for w, _, l in RR.SCRIPT)[what]
        if want is not None:
            assert st.last == want, (what, st.last)
        if st.last != -1 and what != "finalize":
            margin = min(margin, st.pred / (RR.FTOL * st.F_acc))
        if what == "zero-diagonal":
            z = RR.zeroed_parameter(C, F)
            assert st.H[z, z] == 0.0 and st.delta[z] == 0.0 and (np.delete(st.delta, z) != 0).all()
            assert theta[z] == np.float32(st.theta[z])
    print(f"[rig script] C={C} F={F} B={Bs}: accepted {st.accepted}, rejected {st.rejected}, reported {st.reported}; "
          f"smallest pred / (ftol F) of a call that must not stop = {margin:.3g}")
    assert (st.accepted, st.rejected, st.reported, st.iterations, st.done) == (3, 1, 2, 6, 0)
    assert theta.tobytes() == st.theta.astype(np.float32).tobytes()


def test_one_bad_camera_reports_the_whole_rig():
    C, F, Bs = 3, 1, [2, 1, 2]
    N = 6 * C + F
    st = LR.new_state()
    theta0 = np.random.default_rng(5).uniform(-1, 1, N).astype(np.float32)
    trial = RR.update_rig(st, RR.rig_system(C, F, Bs, 0), theta0, FTOL)
    assert st.accepted == 1 and (trial != theta0).any()
    for what in ("loss", "count", "info"):
        cams = [tuple(np.array(x, copy=True) for x in cam) for cam in RR.rig_system(C, F, Bs, 1)]
        if what == "loss":
            cams[1][3][0] = np.nan
        elif what == "count":
            cams[2][2][1] = -1
        else:
            cams[0][0][1, 6, 2] = np.inf
        lam, rep = st.lam, st.reported
        back = RR.update_rig(st, cams, trial, FTOL)
        print(f"[rig reference] bad {what}: reported {st.reported}, last {st.last}")
        assert st.reported == rep + 1 and st.last == -1 and st.lam == lam and st.accepted == 1
        assert back.tobytes() == theta0.tobytes()
