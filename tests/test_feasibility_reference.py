"""The host side of the feasibility filter (easyhec_amd/feasibility.py) and the reference the kernel is held to
(tests/feasibility_reference.py), without a GPU: the proxy spheres cover their triangles and are deterministic, the automatic
pair lists of the packaged robots, the reference on cases with answers known by hand, the ABI entry and its refusals (the
library refuses bad sizes before it touches a device)."""
import ctypes

import numpy as np
import pytest

import feasibility_reference as FR
from easyhec_amd import feasibility as F
from easyhec_amd.robot import load_robot


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def grid_mesh(n_tris, seed=0):
    """A bumpy strip of ``n_tris`` triangles (vertices float32, as the packaged meshes are)."""
    rng = np.random.default_rng(seed)
    cols = n_tris // 2 + 2
    v = np.array([[0.01 * c, 0.01 * r, 0.0] for c in range(cols) for r in range(2)]) + rng.normal(0, 0.002, (2 * cols, 3))
    f = []
    for c in range(cols - 1):
        f += [[2 * c, 2 * c + 1, 2 * c + 2], [2 * c + 1, 2 * c + 3, 2 * c + 2]]
    return v.astype(np.float32), np.asarray(f[:n_tris], dtype=np.int32).reshape(-1, 3)


def assert_covered(v, f, leaf_triangles):
    sph, leaves = F.link_spheres(v, f, leaf_triangles, return_leaves=True)
    assert sph.shape == (len(leaves), 4)
    if f.shape[0] == 0:
        assert sph.shape[0] == 0
        return sph
    assert sorted(np.concatenate(leaves).tolist()) == list(range(f.shape[0]))       # every triangle in exactly one leaf
    v64 = np.asarray(v, dtype=np.float64)
    for s, idx in zip(sph, leaves):
        assert 1 <= idx.shape[0] <= leaf_triangles
        pts = v64[np.asarray(f)[idx].reshape(-1)]
        assert (np.sqrt(((pts - s[:3]) ** 2).sum(axis=1)) <= s[3]).all()
    return sph


@pytest.mark.parametrize("name", ["xarm7", "franka"])
def test_leaf_spheres_cover_their_triangles(name):
    rb = load_robot(name)
    for v, f in rb.meshes:
        sph = assert_covered(v, f, 64)
        assert sph.shape[0] >= f.shape[0] / 64
        b = F.link_bound(v, sph)                                                    # the link's bound holds vertices and spheres
        v64 = np.asarray(v, dtype=np.float64)
        assert (np.linalg.norm(v64 - b[:3], axis=1) <= b[3]).all()
        assert (np.linalg.norm(sph[:, :3] - b[:3], axis=1) + sph[:, 3] <= b[3] * (1 + 1e-15)).all()
        assert np.allclose(b[:3], 0.5 * (v64.min(axis=0) + v64.max(axis=0)), rtol=0, atol=0)


@pytest.mark.parametrize("n_tris", [0, 1, 65])
def test_small_meshes(n_tris):
    v, f = grid_mesh(n_tris)
    sph = assert_covered(v, f, 64)
    assert sph.shape[0] == {0: 0, 1: 1, 65: 2}[n_tris]
    if n_tris == 65:
        _, leaves = F.link_spheres(v, f, 64, return_leaves=True)
        assert [len(l) for l in leaves] == [32, 33]                                 # n // 2 to the first half
    assert_covered(v, f, 1)                                                         # ... down to one triangle per leaf
    assert F.link_bound(v[:0], sph[:0]).tolist() == [0, 0, 0, 0]


def test_link_spheres_are_deterministic(xarm7):
    v, f = xarm7.meshes[3]
    a, b = F.link_spheres(v, f, 64), F.link_spheres(v.copy(), f.copy(), 64)
    assert (bits(a) == bits(b)).all()
    s1, o1, b1 = F.robot_proxies(xarm7, 64)
    s2, o2, b2 = F.robot_proxies(load_robot("xarm7"), 64)
    assert (bits(s1) == bits(s2)).all() and (o1 == o2).all() and (bits(b1) == bits(b2)).all()
    assert o1[0] == 0 and o1[-1] == s1.shape[0] <= 4096


@pytest.mark.parametrize("name,added", [("xarm7", [(2, 4), (2, 5)]), ("franka", [(5, 7), (5, 8), (6, 8)])])
def test_automatic_pair_lists(name, added):
    rb = load_robot(name)
    sph, off, _ = F.robot_proxies(rb, 64)
    pairs, ignored = F.enabled_pairs(rb, sph, off, margin=0.0)
    L = rb.num_links
    print(f"[feasibility pairs] {name}: {[(d['pair'], d['reason'], round(d['clearance'], 5)) for d in ignored]}")
    assert sorted(d["pair"] for d in ignored if d["reason"] == "settle") == added
    structural = sorted(d["pair"] for d in ignored if d["reason"] in ("adjacent", "rigid"))
    assert structural == [(i, i + 1) for i in range(L - 1)]                          # a serial arm: every link and the next
    assert sorted(pairs + [d["pair"] for d in ignored]) == [(i, j) for i in range(L) for j in range(i + 1, L)]
    assert all(d["clearance"] <= 0.0 for d in ignored if d["reason"] == "settle")
    # an explicit list replaces the automatic one; the structural rules stay
    pairs2, ignored2 = F.enabled_pairs(rb, sph, off, margin=0.0, ignore_pairs=[(5, 0)])
    assert sorted(d["pair"] for d in ignored2 if d["reason"] == "listed") == [(0, 5)] and added[0] in pairs2
    w = F.pair_words(pairs, L)
    assert FR.pairs_of(w, L) == pairs


def test_box_planes():
    p = F.box_planes(*F.REFERENCE_WORKSPACE)
    inside, outside = np.array([0.4, 0.0, 0.2]), np.array([0.4, 0.0, 1.2])
    assert p.shape == (6, 4) and (p[:, :3] @ inside + p[:, 3] > 0).all() and (p[:, :3] @ outside + p[:, 3] < 0).sum() == 1
    assert np.isclose(p[:, :3] @ inside + p[:, 3], [0.6, 0.6, 0.5, 0.5, 0.7, 0.8]).all()
    with pytest.raises(ValueError):
        F.box_planes((0, 0, 0), (1, 0, 1))


# ---- the reference on cases with known answers --------------------------------------------------------------------------------
def translation(x, y, z):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = x, y, z
    return T


def two_triangle_links():
    """Two links of one triangle each: proxies by link_spheres, the second link moved along x."""
    v = np.array([[0, 0, 0], [0.03, 0, 0], [0, 0.04, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    s = F.link_spheres(v, f)
    assert s.shape == (1, 4) and np.allclose(s[0], [0.015, 0.02, 0.0, 0.025])        # the 3-4-5 triangle: hypotenuse / 2
    return np.concatenate([s, s]), np.array([0, 1, 2], dtype=np.int32)


def test_reference_two_links_at_a_known_distance():
    sph, off = two_triangle_links()
    r = sph[0, 3]
    lp = np.stack([np.stack([translation(0, 0, 0), translation(d, 0, 0)]) for d in (0.125, 0.0625, 0.5)])
    pe = np.array([2, 0], dtype=np.uint32)
    sc, sp, ec, rc = FR.clearance(lp, sph, off, pe, cutoff=0.25)
    assert sc[0] == 0.125 - (r + r) and sc[1] == 0.0625 - (r + r) and sp[:2].tolist() == [1, 1]
    assert sc[2] == 0.25 and sp[2] == -1                                             # beyond cutoff: cutoff, and no pair
    assert (ec == 0.25).all() and (rc == 0.25).all()                                 # no planes, no reach
    # all pairs disabled; bits j <= i mean nothing
    sc, sp, _, _ = FR.clearance(lp, sph, off, np.array([1, 3], dtype=np.uint32), cutoff=0.25)
    assert (sc == 0.25).all() and (sp == -1).all()


def test_reference_plane_reach_cutoff():
    sph, off = two_triangle_links()
    r = sph[0, 3]
    lp = np.stack([np.stack([translation(0, 0, 0.25), translation(0, 0, 0.0625)])])
    plane = np.array([[0.0, 0.0, 1.0, 0.0]])
    _, _, ec, _ = FR.clearance(lp, sph, off, np.zeros(2, dtype=np.uint32), planes=plane, env_links=0b10, cutoff=1.0)
    assert ec[0] == 0.0625 - r                                                       # link 1 alone is tested
    _, _, ec, _ = FR.clearance(lp, sph, off, np.zeros(2, dtype=np.uint32), planes=plane, env_links=0b01, cutoff=1.0)
    assert ec[0] == 0.25 - r
    _, _, ec, _ = FR.clearance(lp, sph, off, np.zeros(2, dtype=np.uint32), planes=plane, env_links=0b01, cutoff=0.125)
    assert ec[0] == 0.125                                                            # min(value, cutoff)
    obstacle = np.array([[sph[0, 0], sph[0, 1], 0.5, 0.125]])
    _, _, ec, _ = FR.clearance(lp, sph, off, np.zeros(2, dtype=np.uint32), obstacles=obstacle, env_links=0b01, cutoff=1.0)
    assert ec[0] == 0.25 - (r + 0.125)
    reach = np.array([sph[0, 0], sph[0, 1], 0.0, 0.5])
    _, _, _, rc = FR.clearance(lp, sph, off, np.zeros(2, dtype=np.uint32), reach=reach, cutoff=1.0)
    assert rc[0] == 0.5 - (0.25 + r)                                                 # the farther sphere decides
    reach[3] = 0.125
    _, _, _, rc = FR.clearance(lp, sph, off, np.zeros(2, dtype=np.uint32), reach=reach, cutoff=1.0)
    assert rc[0] == 0.125 - (0.25 + r) < 0


def test_reference_nan_pose_single_link_and_validity():
    sph, off = two_triangle_links()
    lp = np.stack([np.stack([translation(0, 0, 0), translation(0.125, 0, 0)])] * 3)
    lp[1, 1, 3, 0] = np.nan                                                          # any entry, the last row included
    sc, sp, ec, rc = FR.clearance(lp, sph, off, np.array([2, 0], dtype=np.uint32), planes=np.array([[0, 0, 1.0, 1.0]]),
                                  env_links=3, cutoff=0.5)
    assert np.isnan([sc[1], ec[1], rc[1]]).all() and sp[1] == -1
    assert sc[0] == sc[2] == 0.125 - 2 * sph[0, 3] and ec[0] == ec[2] == 0.5 and sp[0] == sp[2] == 1
    assert FR.validity(sc, ec, rc, 0.01).tolist() == [True, False, True]
    lp[1, 1, 3, 0] = np.inf
    assert np.isnan(FR.clearance(lp, sph, off, np.array([2, 0], dtype=np.uint32))[0][1])
    # L = 1: nothing to pair
    sc, sp, ec, rc = FR.clearance(lp[:, :1], sph[:1], off[:2], np.array([0xffffffff], dtype=np.uint32), cutoff=0.5)
    assert (sc == 0.5).all() and (sp == -1).all()
    # the reduction over path steps: a NaN step and a colliding middle step reject; the first worst step is reported
    red = FR.reduce_steps(np.array([0.2, 0.005, 0.2, 0.2, np.nan, 0.2]), np.array([-1, 37, -1, -1, -1, -1]), np.full(6, 0.25),
                          np.full(6, 0.25), 3, 0.01)
    assert red["valid"].tolist() == [False, False] and red["worst_step"].tolist() == [1, 1] and red["self_pair"].tolist() == [37, -1]
    assert red["self_clear"][0] == 0.005 and np.isnan(red["self_clear"][1])


# ---- the ABI entry --------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_bound():
    from easyhec_amd import _lib
    assert "ehr_config_clearance" in _lib.SIGNATURES
    assert _lib.has_feasibility() and _lib.lib().ehr_version() == 8
    import easyhec_amd
    assert easyhec_amd.FeasibilityFilter is F.FeasibilityFilter and easyhec_amd.link_spheres is F.link_spheres


def test_the_library_refuses_bad_sizes_before_it_touches_a_device():
    from easyhec_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)                                                      # never dereferenced: every call is refused

    def call(L=2, n=1, offsets=(0, 1, 2), n_planes=0, n_obstacles=0, cutoff=0.25):
        off = np.ascontiguousarray(np.resize(np.asarray(offsets, dtype=np.int32), max(L, 0) + 1) if len(offsets) != L + 1
                                   else np.asarray(offsets, dtype=np.int32))
        rc = lib.ehr_config_clearance(p, p, off.ctypes.data_as(ctypes.c_void_p), p, p, p, n_planes, p, n_obstacles, 0, None,
                                      cutoff, n, L, p, p, p, p, None)
        return rc, lib.ehr_last_error().decode()

    for kw, msg in ((dict(L=0), "1 <= L <= 32"), (dict(L=33), "1 <= L <= 32"), (dict(n=0), "n 0 >= 1"),
                    (dict(n_planes=17), "planes <= 16"), (dict(n_obstacles=1025), "obstacles <= 1024"),
                    (dict(cutoff=0.0), "finite and > 0"), (dict(cutoff=float("nan")), "finite and > 0"),
                    (dict(cutoff=float("inf")), "finite and > 0"), (dict(cutoff=-1.0), "finite and > 0"),
                    (dict(offsets=(0, 4000, 4097)), "S 4097 <= 4096"), (dict(offsets=(0, 5, 4)), "ascend from 0"),
                    (dict(offsets=(1, 2, 3)), "ascend from 0")):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
