"""tests/mesh_clearance_reference.py -- the numpy restatement of ``ehr_mesh_clearance`` that tests/test_gpu_mesh_clearance.py
holds the kernel to -- pinned on the CPU: analytic triangle pairs with exactly representable coordinates, degenerate triangles,
the two entry points against each other, and a sandwich between the sphere proxies below and a point sampling above."""
import numpy as np

import feasibility_reference as FR
import mesh_clearance_reference as MR


def tri(*corners):
    return np.array(corners, dtype=np.float64).reshape(3, 3)


BIG = tri((0, 0, 0), (4, 0, 0), (0, 4, 0))


def both_ways(A, B):
    d = float(MR.triangle_triangle(A, B))
    assert d == float(MR.triangle_triangle(B, A))
    for k in range(1, 3):                                                 # any corner first
        assert d == float(MR.triangle_triangle(np.roll(A, k, axis=0), B))
    return d


def test_parallel_triangles_at_half():
    A = tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    assert both_ways(A, A + np.array([0, 0, 0.5])) == 0.25                 # squared: exactly 0.5


def test_vertex_over_face():
    B = tri((1, 1, 0.25), (1, 2, 1.25), (2, 1, 1.25))
    assert both_ways(BIG, B) == 0.0625
    f = MR.feature_distances2(BIG, B)
    assert f[3] == 0.0625 and f[6:].min() > 0.0625                        # the vertex test finds it, no edge pair does


def test_crossing_edges_at_a_known_gap():
    A = tri((-1, 0, 0), (1, 0, 0), (0, 0, -2))
    B = tri((0, -1, 0.5), (0, 1, 0.5), (0, 0, 2.5))
    assert both_ways(A, B) == 0.25
    f = MR.feature_distances2(A, B)
    assert f[6] == 0.25 and f[:6].min() > 0.25                            # edge 0 against edge 0, no vertex test


def test_coplanar_overlap_is_zero():
    A = tri((0, 0, 0), (2, 0, 0), (0, 2, 0))
    assert both_ways(A, tri((0.5, 0.5, 0), (3, 0.5, 0), (0.5, 3, 0))) == 0.0
    assert both_ways(A, A) == 0.0


def test_an_edge_through_the_middle_of_a_large_triangle():
    A = tri((-10, -10, 0), (10, -10, 0), (0, 10, 0))
    B = tri((0, 0, -1), (0, 0, 1), (0.5, 0, 1))
    assert MR.feature_distances2(A, B).min() > 0.1 ** 2                   # all 15 features are far ...
    assert bool(MR.pierced(A, B)) and both_ways(A, B) == 0.0              # ... and the triangles intersect
    assert not bool(MR.pierced(A, B + np.array([0, 0, 2.0])))             # above the plane: no piercing, the vertex at 1
    assert both_ways(A, B + np.array([0, 0, 2.0])) == 1.0
    assert not bool(MR.pierced(A, B + np.array([30.0, 0, 0])))            # across the plane, outside the triangle


def test_degenerate_triangles():
    line = tri((0, 0, 1), (1, 0, 1), (2, 0, 1))                           # zero area, three distinct corners
    twice = tri((0, 0, 1), (0, 0, 1), (1, 0, 2))                          # a repeated corner
    point = tri((0, 3, 4), (0, 3, 4), (0, 3, 4))
    for D in (line, twice):
        f = MR.feature_distances2(BIG, D)
        assert np.isfinite(f).all() and both_ways(BIG, D) == 1.0
    assert both_ways(point, tri((0, 0, 0), (0, 0, 0), (0, 0, 0))) == 25.0  # two points
    assert both_ways(BIG, point) == 16.0
    # a degenerate triangle does not hide its edges: the needle goes through the face, and lies 0.5 beside a sliver's edge
    needle = tri((0.5, 0.5, -1), (0.5, 0.5, 1), (0.5, 0.5, 1))
    assert both_ways(BIG, needle) == 0.0 and MR.feature_distances2(BIG, needle).min() > 0.1
    assert both_ways(line, tri((1, 0.5, 0), (1, 0.5, 2), (1, 0.5, 2))) == 0.25
    # ... and the vertex test of a zero-area triangle is its edges' (an obstacle's centre against it)
    p = (np.float64(1.5), np.float64(2.0), np.float64(1.0))
    a, b, c = MR._corners(line)
    assert float(MR.point_triangle(p, a, b, c)) == 4.0


CASES = {"[1,1]": dict(counts=[1, 1], n=6), "[5,3]": dict(counts=[5, 3], n=6, leaf_triangles=4, n_planes=2, n_obstacles=3),
         "ragged": dict(counts=[0, 1, 20, 9, 33], n=3, leaf_triangles=8, n_planes=3, n_obstacles=5, pairs="random")}


def test_the_two_entry_points_agree():
    for k, (name, kw) in enumerate(CASES.items()):
        case = MR.make_case(40 + k, cutoff=0.08, **kw)
        mc, mp, mt, ec = MR.reference_of(case)
        cc, cp, ct, ce = MR.reference_of(case, culled=True)
        print(f"[mesh reference] {name}: mesh_clear {mc.tolist()}, env_clear {ec.tolist()}")
        assert (mc.view(np.int64) == cc.view(np.int64)).all() and (ec.view(np.int64) == ce.view(np.int64)).all()
        assert (mp == cp).all() and ((mt >= 0).all(axis=1) == (mp >= 0)).all()
        for b in np.nonzero(mp >= 0)[0]:
            for t in (mt[b], ct[b]):
                assert MR.witness_distance(case["link_poses"][b], case["triangles"], case["tri_offsets"], case["offsets"], *t) == mc[b]


def sampled(n=8):
    u, v = np.meshgrid(np.arange(n) / (n - 1.0), np.arange(n) / (n - 1.0), indexing="ij")
    keep = u + v <= 1.0
    return np.stack([1.0 - u[keep] - v[keep], u[keep], v[keep]], axis=1)  # [36,3] barycentric weights


def test_sandwich_between_proxies_and_samples():
    """proxy clearance <= mesh clearance + 1e-6 (every triangle lies inside its leaf's sphere, up to the float32 pose), and
    mesh clearance <= the least distance between points sampled on the triangles (they are points OF the triangles)."""
    bary = sampled()
    seen = 0
    for k, kw in enumerate((dict(counts=[5, 3], leaf_triangles=4), dict(counts=[7, 2, 12], leaf_triangles=3))):
        case = MR.make_case(60 + k, n=8, cutoff=10.0, spread=0.5, **kw)
        mc, mp, mt, _ = MR.reference_of(case)
        sc = FR.clearance(case["link_poses"], case["spheres"], case["offsets"], case["pair_enable"], cutoff=10.0)[0]
        S = int(case["offsets"][-1])
        tri_link = np.repeat(np.arange(len(kw["counts"])), np.diff(case["offsets"]))[np.repeat(np.arange(S), np.diff(case["tri_offsets"]))]
        for b in range(8):
            W = MR.world_triangles(case["link_poses"][b], case["triangles"], tri_link)
            pts = np.einsum("sk,tkc->tsc", bary, W)                        # [T,36,3]
            low = np.inf
            for i, j in FR.pairs_of(case["pair_enable"], len(kw["counts"])):
                A, B = pts[tri_link == i].reshape(-1, 3), pts[tri_link == j].reshape(-1, 3)
                low = min(low, np.sqrt(((A[:, None] - B[None]) ** 2).sum(axis=2)).min())
            print(f"[mesh reference] sandwich {k}/{b}: proxies {sc[b]:.6f} <= mesh {mc[b]:.6f} <= sampled {low:.6f}")
            assert sc[b] <= mc[b] + 1e-6 and mc[b] <= low + 1e-12
            seen += mc[b] > 0
    assert seen >= 4                                                      # (not all of them intersecting)
