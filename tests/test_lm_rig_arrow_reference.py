"""tests/lm_rig_arrow_reference.py pinned on the CPU: the embedding rule, equality with tests/lm_rig_reference.py where there
are no intrinsics, the block elimination in the kernel's order against the dense solve under the derived bar, the script of
the update-kernel test, and the CPU loop's measured trajectories."""
import copy

import numpy as np
import pytest

import lm_reference as LR
import lm_rig_arrow_reference as AR
import lm_rig_reference as RR


def test_embedding_rule():
    frees, F = [("cx", "cy"), None, AR.ALL4], 7
    P, base, N = AR.layout(frees, F)
    assert (P, base, N) == ([8, 6, 10], [0, 8, 14, 24], 31)
    for c in range(3):
        idx = AR.embed_index(c, frees, F)
        I = P[c] - 6
        assert len(idx) == 6 + F + I
        for i in range(6):
            assert idx[i] == base[c] + i
        for f in range(F):
            assert idx[6 + f] == base[-1] + f
        for q in range(I):
            assert idx[6 + F + q] == base[c] + 6 + q
    every = sorted(set(sum((AR.embed_index(c, frees, F) for c in range(3)), [])))
    assert every == list(range(N))
    assert AR.names([("f", "cy"), None], [1, 3]) == [f"cam0.dof[{i}]" for i in range(6)] + ["cam0.theta[f]", "cam0.theta[cy]"] + \
        [f"cam1.dof[{i}]" for i in range(6)] + ["offset[1]", "offset[3]"]
    assert [AR.parse_free(x) for x in (None, (), "f", ("fx", "cy"), AR.ALL4)] == \
        [([0, 0, 0, 0], False, 0), ([0, 0, 0, 0], False, 0), ([1, 1, 0, 0], True, 1), ([1, 0, 0, 1], False, 2), ([1, 1, 1, 1], False, 4)]
    # without intrinsics: rig_information's order
    for c in range(3):
        assert AR.embed_index(c, [None] * 3, 4) == RR.embed_index(c, 3, 4)


@pytest.mark.parametrize("C,F,Bs", RR.SHAPES)
def test_without_intrinsics_it_is_the_dense_rig_reference(C, F, Bs):
    """lm_rig_reference's shapes and scripted calls: the same states and parameters, exactly."""
    rng = np.random.default_rng(C + 10 * F)
    theta = rng.uniform(-1, 1, 6 * C + F).astype(np.float32)
    a, b, ta, tb = LR.new_state(), LR.new_state(), theta.copy(), theta.copy()
    for what, cams in RR.scripted_calls(C, F, Bs):
        fin = what == "finalize"
        ta = RR.update_rig(a, cams, ta, RR.FTOL, 1e6, fin)
        tb = AR.update_rig_arrow(b, cams, [None] * C, F, tb, RR.FTOL, 1e6, fin)
        assert ta.tobytes() == tb.tobytes(), what
        for k in ("lam", "nu", "F_acc", "pred", "rho", "F_trial", "iterations", "accepted", "rejected", "reported", "done", "why",
                  "last", "count", "retries", "cond"):
            assert getattr(a, k) == getattr(b, k), (what, k)
        for k in ("theta", "delta", "g", "H"):
            assert (getattr(a, k) == getattr(b, k)).all(), (what, k)


@pytest.mark.parametrize("C,F,frees,Bs", AR.SHAPES)
def test_block_elimination_is_within_the_bar_of_the_dense_solve(C, F, frees, Bs):
    P, base, N = AR.layout(frees, F)
    worst, worst_cond = 0.0, 0.0
    for seed in range(7):
        H, g, _, _, bad = AR.gather(AR.rig_system(C, F, frees, Bs, seed), frees, F)
        assert not bad
        for a in range(C):       # the blocks between two different cameras: exactly zero
            for b in range(C):
                if a != b:
                    assert (H[base[a]:base[a + 1], base[b]:base[b + 1]] == 0).all()
        for lam in (1e-3, 1e-5):
            sol = LR.solve(H, g, lam)
            assert sol is not None
            delta, pred, y, cond, _ = sol
            got = AR.block_solve(H, g, lam, P, F)
            assert got is not None
            bar = AR.bar(N, cond)
            ry = float(np.abs(got[2] - y).max() / np.abs(y).max()) / bar
            rp = abs(got[1] - pred) / abs(pred) / bar
            worst, worst_cond = max(worst, ry, rp), max(worst_cond, cond)
    print(f"[lm rig arrow reference] C={C} F={F} N={N}: block elimination vs dense solve, worst ratio to the bar {worst:.4f}, "
          f"worst cond {worst_cond:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("C,F,frees,Bs", AR.SHAPES)
def test_script_does_what_it_says(C, F, frees, Bs):
    P, base, N = AR.layout(frees, F)
    st = LR.new_state()
    theta = np.random.default_rng(N).uniform(-1, 1, N).astype(np.float32)
    z, zi = AR.zeroed_parameter(frees, F), AR.zeroed_intrinsics(frees, F)[0]
    for (what, cams), (_, _, last) in zip(AR.scripted_calls(C, F, frees, Bs), AR.SCRIPT):
        before = copy.deepcopy(st)
        theta = AR.update_rig_arrow(st, cams, frees, F, theta, AR.FTOL, 1e6, what == "finalize")
        if last is not None:
            assert st.last == last and not st.done, (what, st.last, st.why)
        if last == -1:
            assert st.lam == before.lam and theta.tobytes() == st.theta.astype(np.float32).tobytes()
        if what == "zero-diagonal":
            assert st.H[z, z] == 0.0 and st.delta[z] == 0.0 and (np.delete(st.delta, z) != 0).all()
        if what == "zero-intrinsics":
            assert st.H[zi, zi] == 0.0 and st.delta[zi] == 0.0 and (np.delete(st.delta, zi) != 0).all()
    assert (st.accepted, st.rejected, st.reported, st.iterations, st.done, st.retries) == (4, 1, 2, 7, 0, 0)
    assert theta.tobytes() == st.theta.astype(np.float32).tobytes()


def test_cpu_loop_reproduces_measured_and_freeing_the_focal_lengths_pays(oracle, xarm7):
    """Both trajectories of ``MEASURED`` (rtol 1e-6), and: from the same start, after the same number of evaluations, the loop
    that may refine every camera's focal length has the lower accepted loss -- the planted 3 % / 2 % focal errors matter."""
    ps, Ks = AR.rig_problems(oracle, xarm7)
    ends = {}
    for what, frees in (("freed", ["f", "f"]), ("fixed", [None, None])):
        st, traj, theta = AR.cpu_rig_loop(oracle, ps, Ks, AR.RIG_FREE_JOINTS, frees, AR.RIG_EVALUATIONS)
        want = AR.MEASURED[what]
        print(f"[lm rig arrow cpu loop] {what}: {traj}; accepted parameters {np.round(theta, 4).tolist()}")
        assert [a for _, a in traj] == [a for _, a in want["evaluations"]]
        assert np.allclose([F for F, _ in traj], [F for F, _ in want["evaluations"]], rtol=1e-6)
        assert np.isclose(st.F_acc, want["F"], rtol=1e-6)
        acc = [F for F, a in traj if a]
        assert all(y < x for x, y in zip(acc, acc[1:])) and st.F_acc == acc[-1]
        ends[what] = st.F_acc
    assert ends["freed"] < ends["fixed"]
