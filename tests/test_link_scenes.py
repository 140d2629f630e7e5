"""CPU side of tests/test_gpu_link_scenes.py: every case of tests/link_scenes.py is pinned against the oracle and the float64
block reference before a kernel is compared with either, and meets what its GPU case assumes -- the link and triangle counts
it is named for, empty links that are really empty, few blocks without gradient, block scales far above the fixed-point
grid -- so that a later change of seed or placement cannot silently empty a case."""
import numpy as np
import pytest

import fused_loss_reference as R
import link_scenes as S


def test_patch_has_exactly_the_triangles_asked_for():
    rng = np.random.default_rng(0)
    for n in sorted(set(S.C32)):
        for unshared in (False, True):
            v, f = S.patch(n, rng, unshared)
            assert v.shape == ((3 * n if unshared else v.shape[0]), 3) and f.shape == (n, 3)
            assert v.dtype == np.float32 and f.dtype == np.int32
            if n:
                assert (np.unique(f) == np.arange(v.shape[0])).all()                 # no unused vertex
                a, b, c = v[f[:, 0], :2], v[f[:, 1], :2], v[f[:, 2], :2]
                area = 0.5 * np.abs((b - a)[:, 0] * (c - a)[:, 1] - (b - a)[:, 1] * (c - a)[:, 0])
                assert area.min() > 0 and np.abs(v[:, 2]).max() > 0


def test_cases_have_the_counts_they_are_named_for():
    full = S.scene_of("full32")
    assert full.L == 32 and full.B * full.L == 64 and full.arrays[1].shape[0] == 20024
    assert [i for i, e in enumerate(S.empty_links(full)) if e] == [3, 10, 22]
    per_link = np.diff(full.arrays[2])
    assert ((per_link + 63) // 64).max() > 64                                        # a link of more than 64 clusters
    assert {1, 63, 64, 65, 129} <= set(per_link.tolist())
    assert S.scene_of("units512").B * 32 == 512 and S.scene_of("units513").B * 32 > 512
    assert S.scene_of("units513").B % (512 // 32) == 1                               # chunks of 16 + 1 views
    p7 = S.scene_of("prime7")
    assert p7.L == 7 and 512 // 7 == 73 and p7.B == 74 and S.empty_links(p7)[-1]     # chunks of 73 + 1, an empty link last
    assert S.scene_of("L13x5").B * S.scene_of("L13x5").L == 65
    assert [S.scene_of(f"L{n}").L for n in (2, 3, 5, 13, 17, 31)] == [2, 3, 5, 13, 17, 31]
    # the plan's choice of the vertex form (V > 1.5 T: lazy) follows from the scene alone
    lazy = S.scene_of("full32_lazy")
    assert lazy.arrays[0].shape[0] == 3 * lazy.arrays[1].shape[0] > 1.5 * lazy.arrays[1].shape[0]
    assert not full.arrays[0].shape[0] > 1.5 * full.arrays[1].shape[0]
    lazy_cases = {k for k in S.CASES if S.scene_of(k).arrays[0].shape[0] > 1.5 * S.scene_of(k).arrays[1].shape[0]}
    assert lazy_cases == {"full32_lazy", "only_one_live"}                            # (one triangle: V = 3 T as well)


@pytest.mark.parametrize("case,kind", S.RUNS, ids=S.RUN_IDS)
def test_oracle_equals_the_composition(oracle, case, kind):
    e = S.expected_of(oracle, case, kind)
    c = e.c
    assert (e.m_ref == c.mask).all()
    assert (np.abs(e.l_ref - c.loss) <= 1e-6 * np.abs(c.loss)).all()
    ratio = R.worst_block_ratio(e.g_ref, c)
    assert ratio <= R.K_ROUNDINGS, ratio
    assert (e.g_ref[:, :, 2, :] == 0).all() and (c.G[:, :, 2, :] == 0).all()


@pytest.mark.parametrize("case,kind", S.RUNS, ids=S.RUN_IDS)
def test_scenes_meet_what_their_gpu_cases_assume(oracle, case, kind):
    e = S.expected_of(oracle, case, kind)
    s, c = e.s, e.c
    empty = S.empty_links(s)
    dead = c.A == 0
    assert dead[:, empty].all() and (e.g_ref[:, empty] == 0).all() and (c.si[:, empty] == 0).all()
    live_links = dead[:, ~empty]
    n_dead, n_all = int(live_links.sum()), live_links.size
    min_a = float(c.A[~dead].min()) if (~dead).any() else float("nan")
    print(f"[link scene] {case} {kind}: {n_dead} of {n_all} blocks of non-empty links without gradient "
          f"({100.0 * n_dead / n_all:.1f} %), min A of the others {min_a:.3g}, ties {R.tie_counts(c)}")
    if case in S.MASK_ONLY:
        assert dead.all() and (e.g_ref == 0).all() and (c.G == 0).all()
    elif case in S.SUBTILE:
        assert (~dead).any()
    else:
        assert n_dead <= 0.25 * n_all, (case, n_dead, n_all)
    assert (c.A[~dead] >= S.n_tiles(s) * 2.0 ** -8).all(), (case, min_a)
    assert c.loss.max() < 2.0 ** 31 * 1e-3
    if case not in S.MASK_ONLY:
        assert (c.sum32 > 0).any() and ((c.sum32 > 0) & (c.sum32 < 1)).any()          # something drawn, something blended
    if case in ("full32", "units512", "prime7"):
        assert R.tie_counts(c)["three"] > 0
    if kind == "wide":
        assert e.ref.min() < -0.4 and e.ref.max() > 1.9
