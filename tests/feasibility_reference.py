"""Brute-force float64 restatement of ``ehr_config_clearance`` (include/ehr.h, csrc/ehr_feasible.hip): every sphere pair of
every enabled link pair, every sphere against every plane and obstacle, no culling, the contract's expressions operation by
operation (numpy rounds every product and sum on its own, as the library built with -ffp-contract=off does).  A minimum is exact
in any order, so the kernel is compared bit for bit.  CPU only, numpy; tests/test_feasibility_reference.py pins it on analytic
cases, tests/test_gpu_feasibility.py compares the kernel against it.

Also here: the synthetic cases of the GPU tests (``make_case``), built once per shape and shared."""
import numpy as np

NAN = float("nan")


def world_spheres(pose, spheres, offsets):
    """[S,4]: link-frame spheres at one configuration's poses [L,16] (float32 values): c_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k."""
    T = np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(-1, 4, 4)
    link = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    R = T[link]
    x, y, z = spheres[:, 0], spheres[:, 1], spheres[:, 2]
    out = np.empty((spheres.shape[0], 4), dtype=np.float64)
    for k in range(3):
        out[:, k] = ((R[:, k, 0] * x + R[:, k, 1] * y) + R[:, k, 2] * z) + R[:, k, 3]
    out[:, 3] = spheres[:, 3]
    return out


def gap(A, B):
    """[Na,Nb]: sqrt((dx dx + dy dy) + dz dz) - (r_a + r_b) of spheres A [Na,4] against B [Nb,4]."""
    dx = A[:, None, 0] - B[None, :, 0]
    dy = A[:, None, 1] - B[None, :, 1]
    dz = A[:, None, 2] - B[None, :, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz) - (A[:, None, 3] + B[None, :, 3])


def plane_value(planes, W):
    """[Np,S]: (((n_x c_x + n_y c_y) + n_z c_z) + d) - r."""
    n = planes[:, None, :]
    return (((n[..., 0] * W[None, :, 0] + n[..., 1] * W[None, :, 1]) + n[..., 2] * W[None, :, 2]) + n[..., 3]) - W[None, :, 3]


def reach_value(reach, W):
    """[S]: R - (sqrt(|c - o|^2) + r)."""
    dx, dy, dz = W[:, 0] - reach[0], W[:, 1] - reach[1], W[:, 2] - reach[2]
    return reach[3] - (np.sqrt((dx * dx + dy * dy) + dz * dz) + W[:, 3])


def pairs_of(pair_enable, L):
    """The enabled pairs (i, j), j > i, in the order of their code 32 i + j."""
    return [(i, j) for i in range(L) for j in range(i + 1, L) if (int(pair_enable[i]) >> j) & 1]


def clearance(link_poses, spheres, offsets, pair_enable, planes=None, obstacles=None, env_links=0, reach=None, cutoff=0.25):
    """(self_clear [n], self_pair [n] int32, env_clear [n], reach_clear [n]) of link_poses [n,L,16] or [n,L,4,4]."""
    lp = np.asarray(link_poses, dtype=np.float32)
    n, L = lp.shape[0], lp.shape[1]
    lp = lp.reshape(n, L, 16)
    spheres = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    offsets = np.asarray(offsets, dtype=np.int64)
    assert offsets.shape == (L + 1,) and offsets[0] == 0 and (np.diff(offsets) >= 0).all() and offsets[-1] <= spheres.shape[0]
    spheres = spheres[:offsets[-1]]
    pairs = pairs_of(pair_enable, L)
    planes = np.zeros((0, 4)) if planes is None else np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    obstacles = np.zeros((0, 4)) if obstacles is None else np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
    env = np.concatenate([np.arange(offsets[l], offsets[l + 1]) for l in range(L) if (int(env_links) >> l) & 1] + [np.zeros(0, dtype=np.int64)])
    sc, ec, rc = np.full(n, float(cutoff)), np.full(n, float(cutoff)), np.full(n, float(cutoff))
    sp = np.full(n, -1, dtype=np.int32)
    for b in range(n):
        if not np.isfinite(lp[b]).all():
            sc[b] = ec[b] = rc[b] = NAN
            continue
        W = world_spheres(lp[b], spheres, offsets)
        for i, j in pairs:
            A, B = W[offsets[i]:offsets[i + 1]], W[offsets[j]:offsets[j + 1]]
            if A.shape[0] and B.shape[0]:
                m = gap(A, B).min()
                if m < sc[b]:
                    sc[b], sp[b] = m, 32 * i + j
        E = W[env]
        if E.shape[0] and planes.shape[0]:
            ec[b] = min(ec[b], plane_value(planes, E).min())
        if E.shape[0] and obstacles.shape[0]:
            ec[b] = min(ec[b], gap(E, obstacles).min())
        if reach is not None and W.shape[0]:
            rc[b] = min(rc[b], reach_value(np.asarray(reach, dtype=np.float64), W).min())
    return sc, sp, ec, rc


def validity(sc, ec, rc, margin):
    """What the filter accepts: NaN compares false."""
    with np.errstate(invalid="ignore"):
        return (sc > margin) & (ec > margin) & (rc >= 0)


def reduce_steps(sc, sp, ec, rc, steps, margin):
    """The reduction of FeasibilityFilter.check over [Q * steps] -> dict of [Q] arrays."""
    sc, sp, ec, rc = (np.asarray(a).reshape(-1, steps) for a in (sc, sp, ec, rc))
    with np.errstate(invalid="ignore"):
        self_ok, env_ok, reach_ok = (sc > margin).all(axis=1), (ec > margin).all(axis=1), (rc >= 0).all(axis=1)
    low = lambda x: np.where(np.isnan(x), -np.inf, x).argmin(axis=1)     # (numpy: the first among equals)
    slack = np.minimum(np.minimum(sc - margin, ec - margin), rc)
    rows = np.arange(sc.shape[0])
    return {"valid": self_ok & env_ok & reach_ok, "self_ok": self_ok, "env_ok": env_ok, "reach_ok": reach_ok,
            "self_clear": sc.min(axis=1), "env_clear": ec.min(axis=1), "reach_clear": rc.min(axis=1),
            "self_pair": sp[rows, low(sc)], "worst_step": low(slack)}


# ---- synthetic cases of the GPU tests -----------------------------------------------------------------------------------------
def rigid_poses(rng, n, L, spread):
    """[n,L,4,4] float32: random rotations (a QR factor, so orthonormal to float64 rounding, then rounded once) and translations
    ~ U(-spread, spread)."""
    out = np.zeros((n, L, 4, 4), dtype=np.float64)
    for b in range(n):
        for l in range(L):
            q, r = np.linalg.qr(rng.normal(size=(3, 3)))
            q = q * np.sign(np.diag(r))[None]
            if np.linalg.det(q) < 0:
                q[:, 0] = -q[:, 0]
            out[b, l, :3, :3] = q
            out[b, l, :3, 3] = rng.uniform(-spread, spread, 3)
            out[b, l, 3, 3] = 1.0
    return out.astype(np.float32)


def bounds_of(spheres, offsets):
    """[L,4]: per link a sphere about the mean of its spheres' centres that contains them all (the kernel's bound must CONTAIN the
    link's spheres; that a float32 pose is no exact rotation moves distances by parts in 1e7, which the kernel's culling slack of
    1e-6 m covers at these sizes)."""
    L = len(offsets) - 1
    out = np.zeros((L, 4))
    for l in range(L):
        s = spheres[offsets[l]:offsets[l + 1]]
        if s.shape[0]:
            c = s[:, :3].mean(axis=0)
            out[l, :3] = c
            out[l, 3] = (np.linalg.norm(s[:, :3] - c, axis=1) + s[:, 3]).max() * (1 + 1e-9) + 1e-12
    return out


def make_case(seed, counts, n, n_planes=0, n_obstacles=0, with_reach=False, pairs="all", spread=0.6, cutoff=0.25):
    """One synthetic problem: links with ``counts`` spheres each (radius 5..40 mm, within 0.15 m of the link's origin), n random
    configurations, planes through the neighbourhood, obstacles among the links, a reach ball that some spheres leave."""
    rng = np.random.default_rng(seed)
    L = len(counts)
    offsets = np.zeros(L + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    S = int(offsets[-1])
    spheres = np.concatenate([rng.uniform(-0.15, 0.15, (S, 3)), rng.uniform(0.005, 0.04, (S, 1))], axis=1)
    pe = np.zeros(L, dtype=np.uint32)
    if pairs == "all":
        for i in range(L):
            for j in range(i + 1, L):
                pe[i] |= np.uint32(1) << np.uint32(j)
    elif pairs == "random":
        for i in range(L):
            for j in range(i + 1, L):
                if rng.uniform() < 0.5:
                    pe[i] |= np.uint32(1) << np.uint32(j)
            pe[i] |= np.uint32(rng.integers(0, 1 << (i + 1)))          # bits j <= i mean nothing and must be ignored
    planes = None
    if n_planes:
        nrm = rng.normal(size=(n_planes, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        planes = np.concatenate([nrm, rng.uniform(0.2, spread + 0.3, (n_planes, 1))], axis=1)
    obstacles = None
    if n_obstacles:
        obstacles = np.concatenate([rng.uniform(-spread - 0.5, spread + 0.5, (n_obstacles, 3)),
                                    rng.uniform(0.01, 0.08, (n_obstacles, 1))], axis=1)
    reach = np.array([0.02, -0.01, 0.03, spread * 1.2]) if with_reach else None
    env = int(rng.integers(1, 1 << L)) if L < 32 else 0xfffffffe
    return {"link_poses": rigid_poses(rng, n, L, spread), "spheres": spheres, "offsets": offsets,
            "bounds": bounds_of(spheres, offsets), "pair_enable": pe, "planes": planes, "obstacles": obstacles,
            "env_links": env, "reach": reach, "cutoff": cutoff}


def reference_of(case):
    return clearance(case["link_poses"], case["spheres"], case["offsets"], case["pair_enable"], case["planes"],
                     case["obstacles"], case["env_links"], case["reach"], case["cutoff"])
