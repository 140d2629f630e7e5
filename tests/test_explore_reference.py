"""CPU checks of tests/explore_reference.py -- the reference the exploration kernels are compared with on the GPU
(tests/test_gpu_info_explorer.py) -- of the seeded families' pick margins, of the explorer's argument errors that need no
device, and of the ctypes table."""
import numpy as np
import pytest

import explore_reference as ER


def _slogdet_gain(A, H, interest):
    """logdet of the marginal information by numpy's LU, in float64."""
    N = A.shape[0]
    a, b = ER._indices(interest, N)

    def m(X):
        ld = np.linalg.slogdet(X)[1]
        return ld - (np.linalg.slogdet(X[np.ix_(b, b)])[1] if b else 0.0)
    return m(A + H) - m(A)


@pytest.mark.parametrize("N", ER.SIZES)
def test_reference_against_slogdet(N):
    """The longdouble reference against np.linalg.slogdet (float64, LU): within the reference's bar plus the same first-order
    bound for the LU side, taken as another bar (both are backward stable with constants of the order of n u)."""
    for S in ER.VIEWS:
        for which in ER.interests(N):
            A, info, interest, g, bars = ER.expected_gain(N, S, which)
            for q in range(0, ER.Q_CASE, 5):
                want = _slogdet_gain(A, ER.candidate_matrix(info[q], 1.0), interest)
                assert abs(g[q] - want) <= 2 * bars[q] + 1e-300, (N, S, which, q, g[q], want, bars[q])


@pytest.mark.parametrize("N", ER.SIZES)
def test_gain_properties(N):
    """Gain >= 0 within the bar (H_q is PSD); zero matrices give exactly 0; duplicates the same value; the flags."""
    for S in ER.VIEWS:
        for which in ER.interests(N):
            A, info, interest, g, bars = ER.expected_gain(N, S, which)
            assert np.isfinite(g).all() and (g >= -bars).all()
            assert (g[0::4] == 0.0).all() and (bars > 0).all()
            for copy, orig in ER.DUPLICATES:
                assert g[copy] == g[orig]
    A, info = ER.family(6, 1)
    valid = np.ones(ER.Q_CASE, dtype=np.int32)
    valid[3] = 0
    taken = np.zeros(ER.Q_CASE, dtype=np.int32)
    taken[7] = 1
    bad = info.copy()
    bad[3], bad[7], bad[11, 0, 2, 2] = np.nan, np.nan, np.inf
    g, _ = ER.gain(A, bad, valid, taken)
    assert g[3] == -np.inf and g[7] == -np.inf and np.isnan(g[11]) and np.isfinite(np.delete(g, [3, 7, 11])).all()
    A0 = A.copy()
    A0[2, 2] = 0.0
    assert np.isnan(ER.gain(A0, info)[0]).all()


@pytest.mark.parametrize("case", ER.PICK_CASES, ids=lambda c: f"N{c[0]}-S{c[1]}-{c[2]}")
def test_pick_margins_and_chain_rule(case):
    """A condition on the INPUTS of the GPU pick tests: in every greedy round the reference's best and second-best gain
    differ by more than twice the bar (of either), so the kernel's pick is decided; and the chain rule
    sum(picked gains) == ld(A_final) - ld(A_0), for the marginal of the interest set, within the summed bars."""
    N, S, which = case
    A, info, interest, gr = ER.expected_greedy(N, S, which)
    print(f"[pick margins] N={N} S={S} {which}: picked {gr.picked.tolist()}, margin / bar "
          f"{(gr.margin / np.maximum(gr.bars, gr.second_bar)).min():.3g}")
    assert (gr.picked >= 0).all() and len(set(gr.picked.tolist())) == len(gr.picked)
    assert (gr.margin > 2 * np.maximum(gr.bars, gr.second_bar)).all()
    assert (gr.A_final == gr.A_final.T).all()
    s = 1 / np.sqrt(np.diag(A).astype(np.longdouble))
    a, b = ER._indices(interest, N)
    m = lambda X: ER.logdet_scaled(X, s, list(range(N)))[0] - ER.logdet_scaled(X, s, b)[0]
    total = float(m(gr.A_final) - m(A))
    assert abs(gr.gains.sum() - total) <= gr.bars.sum(), (gr.gains.sum(), total, gr.bars.sum())


def test_explorer_argument_errors_need_no_device():
    from easyhec_amd import info_explorer as IE
    names = [f"dof[{i}]" for i in range(6)] + ["offset[1]", "offset[7]", "theta[f]", "theta[cx]"]
    assert IE.interest_indices(names, "pose") == list(range(6))
    assert IE.interest_indices(names, "all") == list(range(10))
    assert IE.interest_indices(names, ["theta[f]", "dof[2]"]) == [2, 8]
    with pytest.raises(ValueError, match="offset\\[3\\]"):
        IE.interest_indices(names, ["dof[0]", "offset[3]"])
    kinds = IE.parameter_kinds(names, joint_kind=[1, 1, 1, 1, 1, 1, 1, 2])
    assert kinds == ["translation"] * 3 + ["rotation"] * 3 + ["revolute", "prismatic", "focal", "principal"]
    s = IE.prior_sigmas(names, kinds)
    assert s.tolist() == [0.05] * 3 + [0.1] * 3 + [0.05, 0.01, 0.05, 0.02]
    assert IE.prior_sigmas(names, kinds, {"rotation": 0.2, "offset[7]": 0.5})[[3, 7]].tolist() == [0.2, 0.5]
    for bad in (0.0, -1.0, {"focal": 0.0}, [0.1] * 9 + [float("nan")]):
        with pytest.raises(ValueError, match="> 0"):
            IE.prior_sigmas(names, kinds, bad)
    with pytest.raises(ValueError, match="keys"):
        IE.prior_sigmas(names, kinds, {"offset[2]": 0.1})


def test_ctypes_table_holds_the_exploration_symbols():
    import os
    from easyhec_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    assert "ehr_information_gain" in _lib.SIGNATURES and "ehr_information_pick" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ehr_information_gain"][1]) == 11 and len(_lib.SIGNATURES["ehr_information_pick"][1]) == 12
    assert _lib.has_information_gain()
