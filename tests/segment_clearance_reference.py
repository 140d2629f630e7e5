"""Numpy restatement of ``ehr_segment_clearance`` (include/ehr.h, csrc/ehr_segment_clearance.hip), operation by operation:
brute force over every sphere pair, plane and obstacle, no culling, every product and sum rounded on its own as the library
built with -ffp-contract=off rounds them.  Minima are exact in any order and every sum runs over ascending j from 0.0, so the
kernel is compared bit for bit.

``evaluate`` is a pure function of one evaluation's float32 ``link_poses`` and ``joint_frames`` (what ``ehr_joint_forward``
writes at the interval's centre), the tables, ``|d|`` and the half-width ``h``; ``search`` is the depth-first walk and takes a
callback ``kin(t) -> (link_poses [L,16], joint_frames [J,6])``, so the same text runs on the host's kinematics
(tests/test_segment_clearance_reference.py) and on the kernel's (tests/test_gpu_segment_clearance.py).  CPU only, numpy."""
import numpy as np

import feasibility_reference as F

NAN = float("nan")
SLACK = 1e-6     # FEAS_CULL_SLACK, subtracted once from each certified value


def joint_kinds(table, J):
    out = np.zeros(J, dtype=np.int32)
    for k, c in zip(table["kind"], table["qidx"]):
        if 0 <= c < J:
            out[c] = k
    return out


def make_tables(table, spheres, offsets, pair_enable, W, below, planes=None, obstacles=None, env_links=0, reach=None,
                cutoff=0.25):
    """What ``evaluate`` and ``search`` read, as one dict."""
    J = int(np.asarray(W).shape[0])
    f = lambda a: None if a is None else np.asarray(a, dtype=np.float64).reshape(-1, 4)
    return {"spheres": np.asarray(spheres, dtype=np.float64).reshape(-1, 4), "offsets": np.asarray(offsets, dtype=np.int64),
            "pair_enable": np.asarray(pair_enable).astype(np.uint32), "planes": f(planes), "obstacles": f(obstacles),
            "env_links": int(env_links), "reach": None if reach is None else np.asarray(reach, dtype=np.float64).reshape(4),
            "cutoff": float(cutoff), "upstream": [int(u) for u in np.asarray(table["upstream"]).astype(np.uint32)],
            "below": [int(u) for u in np.asarray(below).astype(np.uint32)], "W": np.asarray(W, dtype=np.float64),
            "jkind": joint_kinds(table, J)}


def chain_rates(tab, dabs):
    """G [J,L]: G[j,l] = sum over k in up(l) with k below j of |d_k| W[k,l], k ascending."""
    W = tab["W"]
    J, L = W.shape
    G = np.zeros((J, L))
    for j in range(J):
        for l in range(L):
            m, acc = tab["upstream"][l] & tab["below"][j], 0.0
            for k in range(J):
                if (m >> k) & 1:
                    acc = acc + dabs[k] * W[k, l]
            G[j, l] = acc
    return G


def masked_sum(M, dabs, column):
    """sum over j in M of |d_j| column[j], j ascending from 0.0: C(l,M) on G[:,l], Ebar's first-order part on W[:,l]."""
    acc = 0.0
    for j in range(len(dabs)):
        if (M >> j) & 1:
            acc = acc + dabs[j] * column[j]
    return acc


def inflate(h, first, C):
    return h * first + ((0.5 * h) * h) * C


def lever_sums(M, tab, dabs, jf, Ws):
    """[n]: sum over j in M of |d_j| rho[j,s] for the world spheres Ws [n,4]; rho = |(c - p_j) x a_j| + r (revolute), else 1."""
    acc = np.zeros(Ws.shape[0])
    a, p = jf[:, :3].astype(np.float64), jf[:, 3:].astype(np.float64)
    for j in range(len(dabs)):
        if not (M >> j) & 1:
            continue
        if tab["jkind"][j] == 1:
            vx, vy, vz = Ws[:, 0] - p[j, 0], Ws[:, 1] - p[j, 1], Ws[:, 2] - p[j, 2]
            ux, uy, uz = vy * a[j, 2] - vz * a[j, 1], vz * a[j, 0] - vx * a[j, 2], vx * a[j, 1] - vy * a[j, 0]
            rho = np.sqrt((ux * ux + uy * uy) + uz * uz) + Ws[:, 3]
        else:
            rho = np.ones(Ws.shape[0])
        acc = acc + dabs[j] * rho
    return acc


def evaluate(link_poses, joint_frames, tab, dabs, h, G=None):
    """One evaluation -> (raw self, raw pair code, raw env, raw reach, cert self, cert env, cert reach); the certified values
    with SLACK subtracted.  link_poses [L,16] and joint_frames [J,6] are float32 VALUES."""
    lp = np.asarray(link_poses, dtype=np.float32).reshape(-1, 16)
    jf = np.asarray(joint_frames, dtype=np.float32).reshape(-1, 6)
    off, cutoff, up, Wt = tab["offsets"], tab["cutoff"], tab["upstream"], tab["W"]
    L = lp.shape[0]
    dabs = np.asarray(dabs, dtype=np.float64)
    G = chain_rates(tab, dabs) if G is None else G
    Wd = F.world_spheres(lp, tab["spheres"][:off[-1]], off)
    rs, rp, re, rr, cs, ce, cr = cutoff, -1, cutoff, cutoff, cutoff, cutoff, cutoff

    def fold(values, infl, raw, cert):
        """raw = min(raw, values); cert = min(cert, values - infl where values < cutoff)."""
        raw = min(raw, float(values.min()))
        gate = values < cutoff
        if gate.any():
            cert = min(cert, float((values - infl)[gate].min()))
        return raw, cert

    env = tab["planes"] is not None or tab["obstacles"] is not None
    for l in range(L):
        s0, s1 = off[l], off[l + 1]
        is_env = env and (tab["env_links"] >> l) & 1
        if s0 == s1 or not (is_env or tab["reach"] is not None):
            continue
        M, A = up[l], Wd[s0:s1]
        C = masked_sum(M, dabs, G[:, l])
        far = cutoff - inflate(h, masked_sum(M, dabs, Wt[:, l]), C)
        e = inflate(h, lever_sums(M, tab, dabs, jf, A), C)
        if tab["reach"] is not None:
            cr = min(cr, far)
            rr, cr = fold(F.reach_value(tab["reach"], A), e, rr, cr)
        if is_env:
            ce = min(ce, far)
            if tab["planes"] is not None:
                re, ce = fold(F.plane_value(tab["planes"], A), e[None, :], re, ce)
            if tab["obstacles"] is not None:
                re, ce = fold(F.gap(A, tab["obstacles"]), e[:, None], re, ce)
    for i, j in F.pairs_of(tab["pair_enable"], L):
        A, B = Wd[off[i]:off[i + 1]], Wd[off[j]:off[j + 1]]
        if not (A.shape[0] and B.shape[0]):
            continue
        Mi, Mj = up[i] & ~up[j], up[j] & ~up[i]
        Ci, Cj = masked_sum(Mi, dabs, G[:, i]), masked_sum(Mj, dabs, G[:, j])
        cs = min(cs, cutoff - (inflate(h, masked_sum(Mi, dabs, Wt[:, i]), Ci) + inflate(h, masked_sum(Mj, dabs, Wt[:, j]), Cj)))
        ea, eb = inflate(h, lever_sums(Mi, tab, dabs, jf, A), Ci), inflate(h, lever_sums(Mj, tab, dabs, jf, B), Cj)
        g = F.gap(A, B)
        if g.min() < rs:
            rs, rp = float(g.min()), 32 * i + j
        gate = g < cutoff
        if gate.any():
            cs = min(cs, float((g - (ea[:, None] + eb[None, :]))[gate].min()))
    return rs, rp, re, rr, cs - SLACK, ce - SLACK, cr - SLACK


def search(kin, tab, d, margin, min_depth, max_depth, max_evals):
    """The depth-first walk of ``ehr_segment_clearance`` for one candidate.  kin(t) -> (link_poses, joint_frames) float32; d
    [J] = q1 - q0 (float64; the caller has checked q0 and q1 finite: status 3 with evals 0 otherwise).  Returns a dict of the
    kernel's outputs and ``trace_t`` / ``trace_val`` lists."""
    cutoff = tab["cutoff"]
    dabs = np.abs(np.asarray(d, dtype=np.float64))
    out = {"status": -1, "t_free": 0.0, "evals": 0, "cert_self": cutoff, "cert_env": cutoff, "cert_reach": cutoff,
           "stop_self": NAN, "stop_env": NAN, "stop_reach": NAN, "stop_pair": -1, "trace_t": [], "trace_val": []}
    if not np.isfinite(dabs).all():
        out["status"] = 3
        return out
    G = chain_rates(tab, dabs)
    k, i = min_depth, 0
    while True:
        h = 2.0 ** -(k + 1)
        a, c = (2 * i) * h, (2 * i + 1) * h
        out["t_free"] = a
        if out["evals"] >= max_evals:
            out["status"] = 2
            return out
        lp, jf = kin(c)
        out["trace_t"].append(c)
        out["evals"] += 1
        if not np.isfinite(np.asarray(lp, dtype=np.float32)).all():
            out["trace_val"].append([NAN] * 6)
            out["status"] = 3
            return out
        rs, rp, re, rr, cs, ce, cr = evaluate(lp, jf, tab, dabs, h, G)
        out["trace_val"].append([rs, re, rr, cs, ce, cr])
        if not rs > margin or not re > margin or not rr >= 0:
            act = 1
        elif cs > margin and ce > margin and cr >= 0:
            act = 0
            out["cert_self"], out["cert_env"], out["cert_reach"] = min(out["cert_self"], cs), min(out["cert_env"], ce), \
                min(out["cert_reach"], cr)
        elif k < max_depth and out["evals"] < max_evals:
            k, i = k + 1, 2 * i
            continue
        else:
            act = 2
        if act:
            out.update(status=act, stop_self=rs, stop_env=re, stop_reach=rr, stop_pair=rp)
            return out
        while k > min_depth and i & 1:
            k, i = k - 1, i >> 1
        i += 1
        if k == min_depth and i == 1 << min_depth:
            out.update(status=0, t_free=1.0)
            return out


# ---- host kinematics and cases --------------------------------------------------------------------------------------------------
def host_kin(table, q0, q1, offset=None):
    """kin(t) on the host: tests/joint_reference.py's float64 forward kinematics at q0 + t (q1 - q0), rounded once to float32."""
    import joint_reference as JR
    q0, d = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64) - np.asarray(q0, dtype=np.float64)

    def kin(t):
        _, lp, jf = JR.fk(table, (q0 + t * d)[None], offset)
        return lp[0].astype(np.float32).reshape(-1, 16), jf[0].astype(np.float32)
    return kin


def robot_case(robot, planes=None, obstacles=None, reach=None, cutoff=0.25, margin=0.01, leaf_triangles=64, travel=None,
               pairs="auto"):
    """A robot's tables as the filter builds them, host only: (table, tab, parts)."""
    from easyhec_amd import feasibility as fz
    table = robot.joint_table()
    spheres, offsets, bounds = fz.robot_proxies(robot, leaf_triangles)
    L = len(offsets) - 1
    if pairs == "auto":
        pairs, _ = fz.enabled_pairs(robot, spheres, offsets, margin)
    pe = fz.pair_words(pairs, L)
    env = sum(1 << l for l in range(L) if int(table["upstream"][l]) != 0)
    W = fz.reach_radii(robot, bounds, travel)
    below = fz.joint_below(table)
    tab = make_tables(table, spheres, offsets, pe, W, below, planes, obstacles, env, reach, cutoff)
    return table, tab, {"spheres": spheres, "offsets": offsets, "bounds": bounds, "pair_enable": pe, "env_links": env, "W": W,
                        "below": below, "pairs": pairs}


# ---- synthetic cases of the GPU tests ---------------------------------------------------------------------------------------------
def make_case(tree, use, counts, seed, n=3, scales=(0.3, 2.0, 5.0), n_planes=0, n_obstacles=0, with_reach=False, cutoff=0.25,
              margin=0.01, depth=(1, 6), max_evals=40):
    """One synthetic problem on tests/joint_table_cases.py's tree ``tree`` with the rendered links ``use`` (None: the case's own):
    ``counts`` small spheres per link (radius 4..12 mm within 4 cm of the link's origin), the link pairs that keep 3 cm at q0
    enabled, planes and a reach ball that q0 respects, obstacles away from q0, and n candidates at ``scales`` times a random
    direction (prismatic joints a tenth of it): near ones come out clear, far ones split, hit or stay undecided."""
    import joint_reference as JR
    import joint_table_cases as TC
    from easyhec_amd import feasibility as fz
    rng = np.random.default_rng(seed)
    c = TC.case(tree)
    table = c.table if use is None else c.chain.joint_table(use)
    J, L = c.chain.dof, len(table["use"])
    assert len(counts) == L
    kinds = TC.kinds(tree)
    offsets = np.zeros(L + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    S = int(offsets[-1])
    spheres = np.concatenate([rng.uniform(-0.04, 0.04, (S, 3)), rng.uniform(0.004, 0.012, (S, 1))], axis=1)
    bounds = F.bounds_of(spheres, offsets)
    q0 = TC.qpos(tree, 1, seed=seed)[0]
    offset = TC.offsets(tree, seed=seed)
    step = rng.normal(size=(n, J)) * np.where(kinds == 2, 0.1, 1.0)[None]
    q1 = q0[None] + step / np.linalg.norm(step, axis=1, keepdims=True) * np.asarray(scales, dtype=np.float64)[:n, None]
    _, lp0, _ = JR.fk(table, q0[None], offset)
    W0 = F.world_spheres(lp0[0].astype(np.float32).reshape(-1, 16), spheres, offsets)
    pe = np.zeros(L, dtype=np.uint32)
    for i in range(L):
        for j in range(i + 1, L):
            A, B = W0[offsets[i]:offsets[i + 1]], W0[offsets[j]:offsets[j + 1]]
            if A.shape[0] and B.shape[0] and F.gap(A, B).min() > 0.03:
                pe[i] |= np.uint32(1) << np.uint32(j)
    planes = obstacles = reach = None
    far = np.abs(W0[:, :3]).max() + 0.05 if S else 1.0
    if n_planes:
        nrm = rng.normal(size=(n_planes, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        planes = np.concatenate([nrm, np.full((n_planes, 1), far * np.sqrt(3.0))], axis=1)
        planes[0, 3] = (-(W0[:, :3] @ nrm[0]) + W0[:, 3]).max() + 0.02                   # 2 cm behind the nearest sphere at q0
    if n_obstacles:
        obstacles = np.concatenate([rng.uniform(-far, far, (n_obstacles, 3)), rng.uniform(0.01, 0.03, (n_obstacles, 1))], axis=1)
        near = F.gap(W0, obstacles).min(axis=0) < 0.05
        obstacles[near, :3] += 3.0 * far                                                 # those that touch q0: out of the way
    if with_reach:
        reach = np.array([0.0, 0.0, 0.0, np.linalg.norm(W0[:, :3], axis=1).max() + 0.08])
    travel = np.where(kinds == 2, np.abs(np.concatenate([q1, q0[None]])).max(axis=0) + 0.2, 0.0)
    Wr, below = fz.reach_radii(table, bounds, travel), fz.joint_below(table)
    env = (1 << L) - 1
    return {"table": table, "q0": q0, "q1": q1, "offset": offset, "spheres": spheres, "offsets": offsets, "bounds": bounds,
            "pair_enable": pe, "planes": planes, "obstacles": obstacles, "env_links": env, "reach": reach, "cutoff": cutoff,
            "margin": margin, "depth": depth, "max_evals": max_evals, "W": Wr, "below": below,
            "tab": make_tables(table, spheres, offsets, pe, Wr, below, planes, obstacles, env, reach, cutoff)}


def run_case(case, kin_of):
    """The mirror on every candidate of a case; kin_of(b) -> kin(t).  A candidate that is not finite: status 3 with no evaluation."""
    outs = []
    for b in range(case["q1"].shape[0]):
        d = case["q1"][b] - case["q0"]
        outs.append(search(kin_of(b), case["tab"], d, case["margin"], case["depth"][0], case["depth"][1], case["max_evals"]))
    return outs
