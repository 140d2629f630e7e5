"""Float64 restatement of ``ehr_mesh_clearance`` (include/ehr.h, csrc/ehr_mesh_clearance.hip) in numpy: the contract's
expressions operation by operation (numpy rounds every product and sum on its own, as the library built with -ffp-contract=off
does; division and square root are correctly rounded on both sides), the branches as selections.  A minimum is exact in any order,
so the kernel is compared bit for bit.  Two entry points:

    clearance         brute force: every triangle pair of every enabled link pair, every vertex against every plane, every
                      triangle against every obstacle
    clearance_culled  for the packaged arm: leaf pairs whose proxy gap exceeds ``cutoff + 1e-6`` are skipped, and of the rest the
                      triangle pairs whose own bounding spheres (about the world corners' mean) are further apart than that.
                      What is skipped lies above cutoff, so the outputs are those of ``clearance``
                      (tests/test_mesh_clearance_reference.py holds the two equal on synthetic cases).

CPU only; also here: the synthetic cases of the GPU tests (``make_case``)."""
import numpy as np

import feasibility_reference as FR

NAN = float("nan")
SLACK = 1e-6


# ---- the contract's expressions: vectors are tuples (x, y, z) of arrays that broadcast --------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _clamp01(x):
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))


def _ratio(num, den):
    """num / den where den > 0, else 0."""
    return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)


def _min(a, b):
    return np.where(b < a, b, a)


def _norm2(d):
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def point_segment(p, a, b):
    ab, ap = _sub(b, a), _sub(p, a)
    e = _dot(ab, ab)
    t = np.where(e > 0.0, _clamp01(_ratio(_dot(ap, ab), e)), 0.0)
    q = (a[0] + ab[0] * t, a[1] + ab[1] * t, a[2] + ab[2] * t)
    return _norm2(_sub(p, q))


def point_triangle(p, a, b, c):
    """Squared distance of p to triangle a b c: the closest point by Voronoi region; a triangle of zero area is its edges."""
    ab, ac = _sub(b, a), _sub(c, a)
    n = _cross(ab, ac)
    flat = ~(_dot(n, n) > 0.0)
    ap, bp, cp = _sub(p, a), _sub(p, b), _sub(p, c)
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    s = (va + vb) + vc
    wbc = _ratio(e43, e43 + e56)
    conds = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0),
             (d6 >= 0.0) & (d5 <= d6), (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0)]
    zero, one = np.zeros_like(s), np.ones_like(s)
    v = np.select(conds, [zero, one, _ratio(d1, d1 - d3), zero, zero, 1.0 - wbc], default=_ratio(vb, s))
    w = np.select(conds, [zero, zero, zero, one, _ratio(d2, d2 - d6), wbc], default=_ratio(vc, s))
    q = ((a[0] + ab[0] * v) + ac[0] * w, (a[1] + ab[1] * v) + ac[1] * w, (a[2] + ab[2] * v) + ac[2] * w)
    face = _norm2(_sub(p, q))
    edges = _min(_min(point_segment(p, a, b), point_segment(p, b, c)), point_segment(p, c, a))
    return np.where(flat, edges, face)


def segment_segment(p1, q1, p2, q2):
    d1, d2, r = _sub(q1, p1), _sub(q2, p2), _sub(p1, p2)
    a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
    gen = (a > 0.0) & (e > 0.0)
    den = a * e - b * b
    s0 = np.where(den > 0.0, _clamp01(_ratio(b * f - c * e, den)), 0.0)
    t0 = _ratio(b * s0 + f, e)
    s_lo, s_hi = _clamp01(_ratio(-c, a)), _clamp01(_ratio(b - c, a))
    s = np.where(gen, np.where(t0 < 0.0, s_lo, np.where(t0 > 1.0, s_hi, s0)), np.where(a > 0.0, s_lo, 0.0))
    t = np.where(gen, _clamp01(t0), np.where(a > 0.0, 0.0, np.where(e > 0.0, _clamp01(_ratio(f, e)), 0.0)))
    c1 = (p1[0] + d1[0] * s, p1[1] + d1[1] * s, p1[2] + d1[2] * s)
    c2 = (p2[0] + d2[0] * t, p2[1] + d2[1] * t, p2[2] + d2[2] * t)
    return _norm2(_sub(c1, c2))


def pierces(p, q, a, b, c):
    n = _cross(_sub(b, a), _sub(c, a))
    sp, sq = _dot(n, _sub(p, a)), _dot(n, _sub(q, a))
    across = ((sp > 0.0) & (sq < 0.0)) | ((sp < 0.0) & (sq > 0.0))
    d, pa, pb, pc = _sub(q, p), _sub(a, p), _sub(b, p), _sub(c, p)
    u, v, w = _dot(d, _cross(pa, pb)), _dot(d, _cross(pb, pc)), _dot(d, _cross(pc, pa))
    return across & (((u >= 0.0) & (v >= 0.0) & (w >= 0.0)) | ((u <= 0.0) & (v <= 0.0) & (w <= 0.0)))


def _corners(tri):
    """[...,3,3] -> three vectors."""
    return [tuple(tri[..., k, c].copy() for c in range(3)) for k in range(3)]       # (strided views are slow)


def feature_distances2(A, B):
    """[15, ...]: the six vertex-triangle and nine edge-edge squared distances of triangles A, B [...,3,3] (broadcasting)."""
    a, b = _corners(A), _corners(B)
    out = [point_triangle(a[k], *b) for k in range(3)] + [point_triangle(b[k], *a) for k in range(3)]
    out += [segment_segment(a[i], a[(i + 1) % 3], b[j], b[(j + 1) % 3]) for i in range(3) for j in range(3)]
    return np.stack(np.broadcast_arrays(*out))


def pierced(A, B):
    a, b = _corners(A), _corners(B)
    hit = False
    for k in range(3):
        hit = hit | pierces(a[k], a[(k + 1) % 3], *b) | pierces(b[k], b[(k + 1) % 3], *a)
    return hit


def triangle_triangle(A, B):
    """Squared distance of triangles A, B [...,3,3] in one frame: 0 where an edge pierces, else the least of the 15 features."""
    with np.errstate(all="ignore"):
        return np.where(pierced(A, B), 0.0, feature_distances2(A, B).min(axis=0))


# ---- one configuration ----------------------------------------------------------------------------------------------------------
def world_triangles(pose, triangles, tri_link):
    """[T,3,3]: link-frame corners [T,9] at one configuration's poses [L,16] (float32 values), by the kernel's expression."""
    Tm = np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(-1, 4, 4)
    R = Tm[tri_link][:, None]                                             # [T,1,4,4]
    q = np.asarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
    x, y, z = q[..., 0], q[..., 1], q[..., 2]
    out = np.empty(q.shape, dtype=np.float64)
    for k in range(3):
        out[..., k] = ((R[..., k, 0] * x + R[..., k, 1] * y) + R[..., k, 2] * z) + R[..., k, 3]
    return out


def _min_pairs(W, ia, ib, chunk=1 << 14):
    """(least squared distance, ta, tb) over the triangle pairs (ia[k], ib[k]) of world triangles W; (inf, -1, -1) if none.
    Nothing comes below 0: the search ends there."""
    best, ta, tb = np.inf, -1, -1
    for k in range(0, ia.shape[0], chunk):
        if best == 0.0:
            break
        a, b = ia[k:k + chunk], ib[k:k + chunk]
        d2 = triangle_triangle(W[a], W[b])
        m = int(np.argmin(d2))
        if d2[m] < best:
            best, ta, tb = float(d2[m]), int(a[m]), int(b[m])
    return best, ta, tb


def _environment(W, env_tri, planes, obstacles, cutoff):
    ec = float(cutoff)
    E = W[env_tri]
    if E.shape[0] and planes.shape[0]:
        n = planes[:, None, None, :]
        ec = min(ec, float((((n[..., 0] * E[None, ..., 0] + n[..., 1] * E[None, ..., 1]) + n[..., 2] * E[None, ..., 2]) + n[..., 3]).min()))
    if E.shape[0] and obstacles.shape[0]:
        a, b, c = _corners(E[None])
        o = obstacles[:, None, :]
        with np.errstate(all="ignore"):
            d = np.sqrt(point_triangle((o[..., 0], o[..., 1], o[..., 2]), a, b, c)) - o[..., 3]
        ec = min(ec, float(d.min()))
    return ec


def _clearance(link_poses, spheres, offsets, pair_enable, triangles, tri_offsets, planes, obstacles, env_links, cutoff, culled, per_pair=None):
    lp = np.asarray(link_poses, dtype=np.float32)
    n, L = lp.shape[0], lp.shape[1]
    lp = lp.reshape(n, L, 16)
    offsets, tri_offsets = np.asarray(offsets, dtype=np.int64), np.asarray(tri_offsets, dtype=np.int64)
    S = int(offsets[-1])
    spheres = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)[:S]
    triangles = np.asarray(triangles, dtype=np.float64).reshape(-1, 9)
    assert offsets.shape == (L + 1,) and offsets[0] == 0 and (np.diff(offsets) >= 0).all()
    assert tri_offsets.shape[0] >= S + 1 and tri_offsets[0] == 0 and (np.diff(tri_offsets[:S + 1]) >= 0).all()
    T = int(tri_offsets[S])
    triangles = triangles[:T]
    tri_leaf = np.repeat(np.arange(S), np.diff(tri_offsets[:S + 1]))
    leaf_link = np.repeat(np.arange(L), np.diff(offsets))
    tri_link = leaf_link[tri_leaf]
    link_tri = [np.arange(tri_offsets[offsets[l]], tri_offsets[offsets[l + 1]]) for l in range(L)]
    pairs = FR.pairs_of(pair_enable, L)
    planes = np.zeros((0, 4)) if planes is None else np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    obstacles = np.zeros((0, 4)) if obstacles is None else np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
    env_tri = np.concatenate([link_tri[l] for l in range(L) if (int(env_links) >> l) & 1] + [np.zeros(0, dtype=np.int64)])
    mc, ec = np.full(n, float(cutoff)), np.full(n, float(cutoff))
    mp, mt = np.full(n, -1, dtype=np.int32), np.full((n, 2), -1, dtype=np.int32)
    for b in range(n):
        if not np.isfinite(lp[b]).all():
            mc[b] = ec[b] = NAN
            continue
        W = world_triangles(lp[b], triangles, tri_link)
        if culled:
            WS = FR.world_spheres(lp[b], spheres, offsets)
            ctr = ((W[:, 0] + W[:, 1]) + W[:, 2]) * (1.0 / 3.0)
            rad = np.sqrt(((W - ctr[:, None]) ** 2).sum(axis=2).max(axis=1))
        best, found = (np.inf, -1, -1, -1), {}
        for i, j in pairs:
            if not (link_tri[i].shape[0] and link_tri[j].shape[0]):
                continue
            if culled:
                g = FR.gap(WS[offsets[i]:offsets[i + 1]], WS[offsets[j]:offsets[j + 1]])
                sa, sb = np.nonzero(~(g > cutoff + SLACK))
                ia, ib, order = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0)]
                for a, c in zip(sa + offsets[i], sb + offsets[j]):
                    ta, tb = np.arange(tri_offsets[a], tri_offsets[a + 1]), np.arange(tri_offsets[c], tri_offsets[c + 1])
                    # ... first against the other leaf's sphere (the proxies' bound, with the same slack)
                    ta = ta[~(np.sqrt(((ctr[ta] - WS[c, :3]) ** 2).sum(axis=1)) - (rad[ta] + WS[c, 3]) > cutoff + SLACK)]
                    tb = tb[~(np.sqrt(((ctr[tb] - WS[a, :3]) ** 2).sum(axis=1)) - (rad[tb] + WS[a, 3]) > cutoff + SLACK)]
                    # the triangles' own spheres: a bound from the world corners, with 1e-6 to spare for its rounding
                    bound = np.sqrt(((ctr[ta][:, None] - ctr[tb][None]) ** 2).sum(axis=2)) - (rad[ta][:, None] + rad[tb][None])
                    ka, kb = np.nonzero(~(bound > cutoff + SLACK))
                    ia.append(ta[ka])
                    ib.append(tb[kb])
                    order.append(bound[ka, kb])
                near = np.argsort(np.concatenate(order), kind="stable")    # the closest spheres first: a 0 ends the search
                ia, ib = np.concatenate(ia)[near], np.concatenate(ib)[near]
            else:
                ia, ib = np.repeat(link_tri[i], link_tri[j].shape[0]), np.tile(link_tri[j], link_tri[i].shape[0])
            d2, ta, tb = _min_pairs(W, ia, ib)
            found[32 * i + j] = d2
            if d2 < best[0]:
                best = (d2, 32 * i + j, ta, tb)
        d = np.sqrt(best[0])
        if d < cutoff:
            mc[b], mp[b], mt[b] = d, best[1], best[2:]
        ec[b] = _environment(W, env_tri, planes, obstacles, cutoff)
        if per_pair is not None:
            per_pair.append(found)
    return mc, mp, mt, ec


def clearance(link_poses, spheres, offsets, pair_enable, triangles, tri_offsets, planes=None, obstacles=None, env_links=0,
              cutoff=0.02):
    """(mesh_clear [n], mesh_pair [n] int32, mesh_tri [n,2] int32, env_clear [n]) of link_poses [n,L,16] or [n,L,4,4], brute
    force.  The witnesses are SOME pair at the minimum (of the first link pair, by its code, that attains it); the kernel may
    report another one."""
    return _clearance(link_poses, spheres, offsets, pair_enable, triangles, tri_offsets, planes, obstacles, env_links, cutoff, False)


def clearance_culled(link_poses, spheres, offsets, pair_enable, triangles, tri_offsets, planes=None, obstacles=None, env_links=0,
                     cutoff=0.02, per_pair=None):
    """As :func:`clearance`, skipping what the spheres put above ``cutoff + 1e-6`` (the environment is brute force in both).
    ``per_pair``: a list that receives, per configuration that could be judged, {pair code: the least squared distance found for
    that link pair (inf: everything culled)}."""
    return _clearance(link_poses, spheres, offsets, pair_enable, triangles, tri_offsets, planes, obstacles, env_links, cutoff, True,
                      per_pair)


def witness_distance(pose, triangles, tri_offsets, offsets, ta, tb):
    """sqrt of the squared distance of triangles ta, tb (rows of ``triangles``) at one configuration's poses."""
    offsets, tri_offsets = np.asarray(offsets, dtype=np.int64), np.asarray(tri_offsets, dtype=np.int64)
    S = int(offsets[-1])
    tri_link = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))[np.repeat(np.arange(S), np.diff(tri_offsets[:S + 1]))]
    sel = np.array([ta, tb])
    W = world_triangles(pose, np.asarray(triangles).reshape(-1, 9)[sel], tri_link[sel])
    return float(np.sqrt(triangle_triangle(W[0], W[1])))


# ---- synthetic cases of the GPU tests -----------------------------------------------------------------------------------------
def soup(rng, count, extent=0.15, size=0.04):
    """(vertices [3 count, 3], faces [count, 3]): ``count`` separate triangles with corners within ``size`` of an anchor that
    lies within ``extent`` of the link's origin."""
    anchor = rng.uniform(-extent, extent, (count, 1, 3))
    v = (anchor + rng.uniform(-size, size, (count, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * count).reshape(count, 3)


def proxies_of(meshes, leaf_triangles):
    """Spheres, offsets, bounds, triangles and their offsets of links given as (vertices, faces), as the package builds them."""
    from easyhec_amd.feasibility import leaf_mesh, link_bound
    per = [leaf_mesh(v, f, leaf_triangles) for v, f in meshes]
    offsets = np.zeros(len(per) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([s.shape[0] for s, _, _ in per])
    counts = np.concatenate([c for _, _, c in per] + [np.zeros(0, dtype=np.int64)])
    tri_offsets = np.zeros(counts.shape[0] + 1, dtype=np.int32)
    tri_offsets[1:] = np.cumsum(counts)
    return {"spheres": np.concatenate([s for s, _, _ in per]), "offsets": offsets,
            "bounds": np.stack([link_bound(v, s) for (v, _), (s, _, _) in zip(meshes, per)]),
            "triangles": np.concatenate([t for _, t, _ in per]), "tri_offsets": tri_offsets}


def make_case(seed, counts, n, leaf_triangles=64, n_planes=0, n_obstacles=0, pairs="all", spread=0.35, cutoff=0.05):
    """One synthetic problem: links of ``counts`` separate triangles each, n random configurations, planes through the
    neighbourhood and obstacles among the links."""
    rng = np.random.default_rng(seed)
    L = len(counts)
    case = proxies_of([soup(rng, c) for c in counts], leaf_triangles)
    pe = np.zeros(L, dtype=np.uint32)
    for i in range(L):
        for j in range(i + 1, L):
            if pairs == "all" or (pairs == "random" and rng.uniform() < 0.6):
                pe[i] |= np.uint32(1) << np.uint32(j)
        if pairs == "random":
            pe[i] |= np.uint32(rng.integers(0, 1 << (i + 1)))              # bits j <= i mean nothing and must be ignored
    planes = None
    if n_planes:
        nrm = rng.normal(size=(n_planes, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        planes = np.concatenate([nrm, rng.uniform(0.1, spread + 0.2, (n_planes, 1))], axis=1)
    obstacles = None
    if n_obstacles:
        obstacles = np.concatenate([rng.uniform(-spread - 0.3, spread + 0.3, (n_obstacles, 3)),
                                    rng.uniform(0.01, 0.08, (n_obstacles, 1))], axis=1)
    env = int(rng.integers(1, 1 << L)) if (n_planes or n_obstacles) else 0
    case.update(link_poses=FR.rigid_poses(rng, n, L, spread), pair_enable=pe, planes=planes, obstacles=obstacles, env_links=env,
                cutoff=cutoff)
    return case


def reference_of(case, culled=False, cutoff=None):
    fn = clearance_culled if culled else clearance
    return fn(case["link_poses"], case["spheres"], case["offsets"], case["pair_enable"], case["triangles"], case["tri_offsets"],
              case["planes"], case["obstacles"], case["env_links"], case["cutoff"] if cutoff is None else cutoff)
