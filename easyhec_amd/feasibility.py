"""Feasibility of candidate joint configurations, on the device (``ehr_config_clearance`` in include/ehr.h,
csrc/ehr_feasible.hip).

The explorers score thousands of candidate joint configurations and the arm moves to the best one; whether it CAN go there
the reference decides with three filters in front of its scoring (space_explorer.py:105-137 of the reference: self-collision,
a maximum-distance constraint over the links, a workspace-boundary point cloud).  This module is their stand-in:

    link_spheres      a link's mesh -> proxy spheres (a median-split tree over the triangles; every triangle of a leaf lies
                      inside the leaf's sphere, so clear spheres mean clear meshes: the filter is conservative)
    config_clearance  one ``ehr_config_clearance`` launch on device tensors
    FeasibilityFilter the robot's proxies, the link pairs worth checking, the environment (half-spaces, obstacle spheres, a
                      ball of allowed reach) and ``check``: candidates (and the straight joint-space segment from the current
                      configuration to each) -> ``valid`` and the clearances, device tensors, with no host synchronisation
    robot_triangles   the triangles every proxy sphere stands for, in the spheres' order
    mesh_clearance    one ``ehr_mesh_clearance`` launch (csrc/ehr_mesh_clearance.hip; DESIGN.md section 6t, INTEGRATION.md
                      4a-14): the exact distance between the meshes behind the proxies, and of the meshes to planes and
                      obstacles.  ``FeasibilityFilter(exact=True)`` judges self and environment clearance with it.
    segment_clearance one ``ehr_segment_clearance`` launch (csrc/ehr_segment_clearance.hip; DESIGN.md section 6u, INTEGRATION.md
                      4a-15): a certificate that the proxies keep ``margin`` on the WHOLE segment to a candidate, or how far
                      the move is certified and what stopped it.  ``FeasibilityFilter(swept=True).check_swept`` calls it;
                      ``joint_below`` and ``reach_radii`` are its host tables.
    edge_clearance    one ``ehr_edge_clearance`` launch: the same certificate for the edges of a roadmap, each between its own
                      two nodes; roadmap_edges builds the edge list and its adjacency on the device, roadmap_paths is one
                      ``ehr_roadmap_paths`` launch (csrc/ehr_roadmap.hip): shortest
                      paths of at most H certified moves.  ``FeasibilityFilter(swept=True, detour_hops=H).plan`` calls the three.

What it is NOT: a motion planner with smoothing or timing -- the straight segment is sampled at ``path_steps`` configurations
(``check``) or certified as a whole on the proxies (``check_swept``), ``plan`` chains such certified segments over the round's
own candidates, and nothing is shortcut or timed; and, without ``exact=True``, a mesh-exact collision test.  Links that are not rendered (a gripper whose meshes are not packaged) have no proxies and are
not covered.  HIP only; no fallback."""
import ctypes
import types

import numpy as np
import torch

from . import _lib, dr

__all__ = ["link_spheres", "link_bound", "box_planes", "robot_proxies", "enabled_pairs", "config_clearance",
           "leaf_mesh", "robot_triangles", "mesh_clearance", "joint_below", "reach_radii", "segment_clearance",
           "edge_clearance", "roadmap_paths", "roadmap_edges", "FeasibilityFilter", "REFERENCE_WORKSPACE"]

REFERENCE_WORKSPACE = ((-0.2, -0.5, -0.5), (1.0, 0.5, 1.0))  # the reference's workspace box (workspace_boundary.py:9)


def _missing():
    raise RuntimeError("this libehr_hip.so has no feasibility kernel (ehr_config_clearance): rebuild it")


def _missing_mesh():
    raise RuntimeError("this libehr_hip.so has no mesh clearance kernel (ehr_mesh_clearance): rebuild it")


# ---- proxy geometry (host, once per robot) --------------------------------------------------------------------------------
def _enclosing(points):
    """(centre, radius): the midpoint of the points' bounding box and the largest computed distance to them, moved up by one
    ``np.nextafter``."""
    c = 0.5 * (points.min(axis=0) + points.max(axis=0))
    d = points - c
    r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max()
    return c, np.nextafter(r, np.inf)


def link_spheres(vertices, faces, leaf_triangles=64, return_leaves=False):
    """[S,4] float64 (centre, radius) proxy spheres of one link's mesh.  The triangles are split recursively at the median
    of their centroids along the axis on which the centroids extend furthest (stable argsort, ``n // 2`` to the first half)
    until a leaf holds ``<= leaf_triangles``; a leaf's sphere is :func:`_enclosing` of its triangles' vertices.  Deterministic;
    every triangle of a leaf lies inside its sphere.  A link without triangles has no spheres.  ``return_leaves``: also the list of
    every leaf's triangle indices, in the spheres' order."""
    leaf_triangles = int(leaf_triangles)
    if leaf_triangles < 1:
        raise ValueError("leaf_triangles must be >= 1")
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return (np.zeros((0, 4), dtype=np.float64), []) if return_leaves else np.zeros((0, 4), dtype=np.float64)
    if f.min() < 0 or f.max() >= v.shape[0]:
        raise ValueError("link_spheres: a face indexes past the vertices")
    tri = v[f]                                            # [T,3,3]
    cent = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / 3.0
    out, leaves, stack = [], [], [np.arange(f.shape[0])]
    while stack:                                          # depth first, the first half first
        idx = stack.pop()
        n = idx.shape[0]
        if n <= leaf_triangles:
            c, r = _enclosing(tri[idx].reshape(-1, 3))
            out.append([c[0], c[1], c[2], r])
            leaves.append(idx)
            continue
        ci = cent[idx]
        axis = int(np.argmax(ci.max(axis=0) - ci.min(axis=0)))
        order = np.argsort(ci[:, axis], kind="stable")
        stack.append(idx[order[n // 2:]])
        stack.append(idx[order[:n // 2]])
    out = np.asarray(out, dtype=np.float64)
    return (out, leaves) if return_leaves else out


def link_bound(vertices, spheres):
    """[4] float64: the link's one bounding sphere, which the kernel culls with.  Its centre is the midpoint of the bounding box
    of ALL the link's vertices, as a leaf's; its radius reaches every vertex AND every proxy sphere (a leaf's sphere may stick
    out of the sphere around the vertices, and a bound that culls must contain what it stands for), moved up by one
    ``np.nextafter``."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    s = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    if v.shape[0] == 0 and s.shape[0] == 0:
        return np.zeros(4, dtype=np.float64)
    pts = v if v.shape[0] else s[:, :3]
    c, r = _enclosing(pts)
    if s.shape[0]:
        d = s[:, :3] - c
        r = max(r, np.nextafter((np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + s[:, 3]).max(), np.inf))
    return np.array([c[0], c[1], c[2], r], dtype=np.float64)


def box_planes(lo, hi):
    """[6,4] float64: the six inward half-spaces (n, d), ``n.x + d >= 0`` inside, of the box lo..hi."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"box_planes: need finite lo < hi, got {lo.tolist()} .. {hi.tolist()}")
    out = np.zeros((6, 4), dtype=np.float64)
    for k in range(3):
        out[2 * k, k], out[2 * k, 3] = 1.0, -lo[k]
        out[2 * k + 1, k], out[2 * k + 1, 3] = -1.0, hi[k]
    return out


def robot_proxies(robot, leaf_triangles=64):
    """(spheres [S,4], sphere_offsets [L+1] int32, link_bounds [L,4]) of the robot's rendered links, concatenated."""
    per_link = [link_spheres(v, f, leaf_triangles) for v, f in robot.meshes]
    offsets = np.zeros(len(per_link) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([s.shape[0] for s in per_link])
    spheres = np.concatenate(per_link) if per_link else np.zeros((0, 4))
    bounds = np.stack([link_bound(v, s) for (v, _), s in zip(robot.meshes, per_link)])
    return np.ascontiguousarray(spheres, dtype=np.float64), offsets, bounds


def leaf_mesh(vertices, faces, leaf_triangles=64):
    """(spheres [S,4], triangles [T,9] float64, counts [S] int64) of one link: :func:`link_spheres` and the link-frame corner
    coordinates of the triangles, reordered so that those of sphere s follow those of sphere s - 1 (``counts`` of them each)."""
    spheres, leaves = link_spheres(vertices, faces, leaf_triangles, return_leaves=True)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    order = np.concatenate(leaves) if leaves else np.zeros(0, dtype=np.int64)
    return spheres, np.ascontiguousarray(v[f[order]].reshape(-1, 9)), np.array([len(i) for i in leaves], dtype=np.int64)


def robot_triangles(robot, leaf_triangles=64):
    """(triangles [T,9] float64, tri_offsets [S+1] int32) of the robot's rendered links: the triangles of proxy sphere s of
    :func:`robot_proxies` (same ``leaf_triangles``) are ``tri_offsets[s] .. tri_offsets[s+1]``."""
    per_link = [leaf_mesh(v, f, leaf_triangles) for v, f in robot.meshes]
    counts = np.concatenate([c for _, _, c in per_link] + [np.zeros(0, dtype=np.int64)])
    offsets = np.zeros(counts.shape[0] + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(counts)
    tri = np.concatenate([t for _, t, _ in per_link]) if per_link else np.zeros((0, 9))
    return np.ascontiguousarray(tri, dtype=np.float64), offsets


def _world_spheres(link_poses, spheres, offsets):
    """[n,S,4] float64: the spheres in the base frame at link_poses [n,L,4,4] (float32 values), by the kernel's expression."""
    T = np.asarray(link_poses, dtype=np.float32).astype(np.float64)
    link = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    R = T[:, link]                                                       # [n,S,4,4]
    x, y, z = spheres[None, :, 0], spheres[None, :, 1], spheres[None, :, 2]
    out = np.empty((T.shape[0], spheres.shape[0], 4), dtype=np.float64)
    for k in range(3):
        out[..., k] = ((R[..., k, 0] * x + R[..., k, 1] * y) + R[..., k, 2] * z) + R[..., k, 3]
    out[..., 3] = spheres[None, :, 3]
    return out


def pair_clearances(link_poses, spheres, offsets):
    """{(i, j): proxy clearance of link pair i < j, the minimum over the configurations of link_poses [n,L,4,4]} on the host
    (numpy): what the automatic pair list is decided on, once per robot.  Pairs with a link that has no spheres: +inf."""
    W = _world_spheres(link_poses, spheres, offsets)
    L = len(offsets) - 1
    out = {}
    for i in range(L):
        for j in range(i + 1, L):
            A, B = W[:, offsets[i]:offsets[i + 1]], W[:, offsets[j]:offsets[j + 1]]
            if A.shape[1] == 0 or B.shape[1] == 0:
                out[(i, j)] = np.inf
                continue
            d = A[:, :, None, :3] - B[:, None, :, :3]
            gap = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) - \
                (A[:, :, None, 3] + B[:, None, :, 3])
            out[(i, j)] = float(gap.min())
    return out


def _tree_relations(table):
    """(adjacent, rigid): sets of rendered-link pairs (i < j).  adjacent: one is the other's nearest rendered ancestor; rigid:
    no active joint lies on the tree path between them."""
    parent, qidx, use = np.asarray(table["parent"]), np.asarray(table["qidx"]), np.asarray(table["use"])
    link_of = {int(n): l for l, n in enumerate(use)}
    chains = []
    for n in use:
        chain, i = [], int(n)
        while i >= 0:
            chain.append(i)
            i = int(parent[i])
        chains.append(chain)
    adjacent, rigid = set(), set()
    for l, chain in enumerate(chains):
        for n in chain[1:]:
            if n in link_of:
                if link_of[n] != l:
                    adjacent.add((min(l, link_of[n]), max(l, link_of[n])))
                break
    L = len(use)
    for i in range(L):
        for j in range(i + 1, L):
            a, b = chains[i], chains[j]
            common = set(a) & set(b)
            between = [n for n in a if n not in common] + [n for n in b if n not in common]
            if all(qidx[n] < 0 for n in between):
                rigid.add((i, j))
    return adjacent, rigid


def enabled_pairs(robot, spheres, offsets, margin=0.01, ignore_pairs="auto", settle_qpos=None):
    """(pairs, ignored) of the robot's rendered links.  Every pair i < j is enabled but: a link and its nearest rendered
    ancestor ("adjacent"); pairs with only fixed joints between them ("rigid"); and, with ``ignore_pairs="auto"``, pairs whose
    proxy clearance at ``settle_qpos`` (default: the zero configuration; may be several) is ``<= margin`` ("settle": proxies
    that touch where the arm is known to be free tell nothing) -- or, with a list of pairs, exactly those ("listed").
    ``ignored``: a list of ``{"pair", "reason", "clearance"}`` with the settle clearance of each."""
    table = robot.joint_table()
    L = len(offsets) - 1
    adjacent, rigid = _tree_relations(table)
    q0 = np.zeros((1, robot.chain.dof)) if settle_qpos is None else np.atleast_2d(np.asarray(settle_qpos, dtype=np.float64))
    settle = pair_clearances(robot.link_poses_batch(q0).astype(np.float32), spheres, offsets)
    listed = None
    if not (isinstance(ignore_pairs, str) and ignore_pairs == "auto"):
        listed = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in ignore_pairs}
        if any(a == b or a < 0 or b >= L for a, b in listed):
            raise ValueError(f"ignore_pairs {sorted(listed)}: pairs of two different links out of 0..{L - 1}")
    pairs, ignored = [], []
    for i in range(L):
        for j in range(i + 1, L):
            p, c = (i, j), settle[(i, j)]
            if p in adjacent:
                why = "adjacent"
            elif p in rigid:
                why = "rigid"
            elif listed is not None:
                why = "listed" if p in listed else None
            else:
                why = "settle" if c <= margin else None
            if why is None:
                pairs.append(p)
            else:
                ignored.append({"pair": p, "reason": why, "clearance": c})
    return pairs, ignored


def pair_words(pairs, L):
    """[L] uint32: bit j of word i (j > i) = pair (i, j) is checked."""
    w = np.zeros(L, dtype=np.uint32)
    for i, j in pairs:
        i, j = (int(i), int(j)) if i < j else (int(j), int(i))
        if not 0 <= i < j < L:
            raise ValueError(f"pair ({i}, {j}): two different links out of 0..{L - 1}")
        w[i] |= np.uint32(1) << np.uint32(j)
    return w


# ---- the kernel -------------------------------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def config_clearance(link_poses, spheres, sphere_offsets, link_bounds, pair_enable, planes=None, obstacles=None, env_links=0,
                     reach=None, cutoff=0.25):
    """One ``ehr_config_clearance`` launch (include/ehr.h).  Device tensors: link_poses [n,L,4,4] float32, spheres [S,4],
    link_bounds [L,4], planes [Np,4], obstacles [No,4], reach [4] float64, pair_enable [L] int32 (the uint32 words' bits);
    ``sphere_offsets`` [L+1]: a HOST array.  Returns a namespace of device tensors [n]: ``self_clear``, ``env_clear``,
    ``reach_clear`` float64 and ``self_pair`` int32.  Never synchronises; the sizes' limits are the library's to refuse."""
    if not _lib.has_feasibility():
        _missing()
    dr._check_dev("link_poses", link_poses, torch.float32)
    dev = link_poses.device
    dr._require(link_poses.dim() == 4 and tuple(link_poses.shape[2:]) == (4, 4), "link_poses must have shape [n, L, 4, 4]")
    n, L = int(link_poses.shape[0]), int(link_poses.shape[1])
    off = np.ascontiguousarray(np.asarray(sphere_offsets), dtype=np.int32)
    dr._require(off.shape == (L + 1,), "sphere_offsets must be a host array of L + 1 entries")

    def f64(name, t, rows):
        if t is None:
            return None
        dr._check_dev(name, t, torch.float64)
        dr._require(t.device == dev and t.dim() == 2 and t.shape[1] == 4 and t.shape[0] >= rows, f"{name} must have shape [{rows}, 4]")
        return t.contiguous()

    spheres = f64("spheres", spheres, max(int(off[-1]), 0))
    link_bounds = f64("link_bounds", link_bounds, L)
    planes, obstacles = f64("planes", planes, 0), f64("obstacles", obstacles, 0)
    if reach is not None:
        dr._check_dev("reach", reach, torch.float64)
        dr._require(reach.device == dev and reach.numel() == 4, "reach must have 4 entries")
        reach = reach.contiguous()
    dr._check_dev("pair_enable", pair_enable, torch.int32)
    dr._require(pair_enable.device == dev and pair_enable.shape == (L,), "pair_enable must have shape [L]")
    out = types.SimpleNamespace(self_clear=torch.empty((n,), dtype=torch.float64, device=dev),
                                self_pair=torch.empty((n,), dtype=torch.int32, device=dev),
                                env_clear=torch.empty((n,), dtype=torch.float64, device=dev),
                                reach_clear=torch.empty((n,), dtype=torch.float64, device=dev))
    Np = 0 if planes is None else int(planes.shape[0])
    No = 0 if obstacles is None else int(obstacles.shape[0])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ehr_config_clearance(
            _lib.ptr(link_poses.contiguous()), _lib.ptr(spheres), off.ctypes.data_as(ctypes.c_void_p), _lib.ptr(link_bounds),
            _lib.ptr(pair_enable.contiguous()), _lib.ptr(planes) if Np else None, Np, _lib.ptr(obstacles) if No else None, No,
            int(env_links) & 0xffffffff, _lib.ptr(reach), float(cutoff), n, L, _lib.ptr(out.self_clear), _lib.ptr(out.self_pair),
            _lib.ptr(out.env_clear), _lib.ptr(out.reach_clear), _stream()), "ehr_config_clearance")
    return out


def mesh_clearance(link_poses, spheres, sphere_offsets, link_bounds, pair_enable, triangles, tri_offsets, planes=None,
                   obstacles=None, env_links=0, cutoff=0.02):
    """One ``ehr_mesh_clearance`` launch (include/ehr.h).  Device tensors as :func:`config_clearance`'s, and triangles [T,9]
    float64, tri_offsets [S+1] int32 (:func:`robot_triangles`); ``sphere_offsets`` [L+1]: a HOST array.  Returns a namespace of
    device tensors: ``mesh_clear``, ``env_clear`` float64 [n], ``mesh_pair`` int32 [n], ``mesh_tri`` int32 [n,2].  Never
    synchronises; the sizes' limits are the library's to refuse."""
    if not _lib.has_mesh_clearance():
        _missing_mesh()
    dr._check_dev("link_poses", link_poses, torch.float32)
    dev = link_poses.device
    dr._require(link_poses.dim() == 4 and tuple(link_poses.shape[2:]) == (4, 4), "link_poses must have shape [n, L, 4, 4]")
    n, L = int(link_poses.shape[0]), int(link_poses.shape[1])
    off = np.ascontiguousarray(np.asarray(sphere_offsets), dtype=np.int32)
    dr._require(off.shape == (L + 1,), "sphere_offsets must be a host array of L + 1 entries")
    S = max(int(off[-1]), 0)

    def f64(name, t, rows, cols=4):
        if t is None:
            return None
        dr._check_dev(name, t, torch.float64)
        dr._require(t.device == dev and t.dim() == 2 and t.shape[1] == cols and t.shape[0] >= rows,
                    f"{name} must have shape [{rows}, {cols}]")
        return t.contiguous()

    spheres, link_bounds = f64("spheres", spheres, S), f64("link_bounds", link_bounds, L)
    planes, obstacles = f64("planes", planes, 0), f64("obstacles", obstacles, 0)
    triangles = f64("triangles", triangles, 0, 9)
    dr._check_dev("pair_enable", pair_enable, torch.int32)
    dr._require(pair_enable.device == dev and pair_enable.shape == (L,), "pair_enable must have shape [L]")
    dr._check_dev("tri_offsets", tri_offsets, torch.int32)
    dr._require(tri_offsets.device == dev and tri_offsets.dim() == 1 and tri_offsets.shape[0] >= S + 1,
                "tri_offsets must have S + 1 entries")
    out = types.SimpleNamespace(mesh_clear=torch.empty((n,), dtype=torch.float64, device=dev),
                                mesh_pair=torch.empty((n,), dtype=torch.int32, device=dev),
                                mesh_tri=torch.empty((n, 2), dtype=torch.int32, device=dev),
                                env_clear=torch.empty((n,), dtype=torch.float64, device=dev))
    Np = 0 if planes is None else int(planes.shape[0])
    No = 0 if obstacles is None else int(obstacles.shape[0])
    T = int(triangles.shape[0])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ehr_mesh_clearance(
            _lib.ptr(link_poses.contiguous()), _lib.ptr(spheres), off.ctypes.data_as(ctypes.c_void_p), _lib.ptr(link_bounds),
            _lib.ptr(pair_enable.contiguous()), _lib.ptr(planes) if Np else None, Np, _lib.ptr(obstacles) if No else None, No,
            int(env_links) & 0xffffffff, float(cutoff), n, L, _lib.ptr(triangles) if T else None, _lib.ptr(tri_offsets.contiguous()),
            T, _lib.ptr(out.mesh_clear), _lib.ptr(out.mesh_pair), _lib.ptr(out.mesh_tri), _lib.ptr(out.env_clear), _stream()),
            "ehr_mesh_clearance")
    return out


def _missing_segment():
    raise RuntimeError("this libehr_hip.so has no segment clearance kernel (ehr_segment_clearance): rebuild it")


def joint_below(table):
    """[J] uint32: bit k of word j = active joint k lies strictly below active joint j (the link k moves hangs from the link
    j moves), so j moves k's axis."""
    parent, qidx = np.asarray(table["parent"]), np.asarray(table["qidx"])
    J = int(qidx.max()) + 1 if qidx.size else 0
    out = np.zeros(J, dtype=np.uint32)
    for n in range(parent.shape[0]):
        k = int(qidx[n])
        if k < 0:
            continue
        i = int(parent[n])
        while i >= 0:
            if qidx[i] >= 0:
                out[int(qidx[i])] |= np.uint32(1) << np.uint32(k)
            i = int(parent[i])
    return out


def reach_radii(robot, link_bounds, travel=None):
    """W [J,L] float64 of ``ehr_segment_clearance``: a bound, at ANY configuration, on the distance of any point of any proxy of
    rendered link l from the axis of active joint j.  0 where j is not upstream of l and 1 for a prismatic j.  For a revolute j
    the axis passes through the origin of the link j moves; from there down the chain to link l every joint origin adds the
    norm of its translation and every prismatic joint on the way its ``travel`` (the largest ``|q + offset|`` it may take, [J];
    None: 0), and the link's own bound adds ``|centre| + radius``.  ``robot``: a Robot, or a joint table."""
    table = robot if isinstance(robot, dict) else robot.joint_table()
    parent, kind, qidx, use = (np.asarray(table[k]) for k in ("parent", "kind", "qidx", "use"))
    origin = np.asarray(table["origin"], dtype=np.float64).reshape(-1, 4, 4)
    bounds = np.asarray(link_bounds, dtype=np.float64).reshape(-1, 4)
    J, L = int(qidx.max()) + 1, use.shape[0]
    travel = np.zeros(J) if travel is None else np.abs(np.asarray(travel, dtype=np.float64).reshape(J))
    W = np.zeros((J, L), dtype=np.float64)
    for l in range(L):
        c = bounds[l]
        far = float(np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + c[3])    # from link l's origin
        i = int(use[l])
        while i >= 0:
            j = int(qidx[i])
            if j >= 0:
                W[j, l] = far if kind[i] == 1 else 1.0
            t = origin[i, :3, 3]
            far += float(np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))
            if j >= 0 and kind[i] == 2:
                far += float(travel[j])
            i = int(parent[i])
    return W


def _segment_common(table, J, dev, offset, spheres, sphere_offsets, link_bounds, pair_enable, upstream, below, reach_radius,
                    planes, obstacles, reach, n, max_evals, trace):
    """What :func:`segment_clearance` and :func:`edge_clearance` share: the checked tensors as the argument groups the library
    takes around the segments' own (table and sizes, offset, proxies, reach, host tables), the pre-filled outputs [n] and the
    tensors those pointers belong to."""
    parent, origin, kind, axis, qidx, use = table
    N, L = int(parent.shape[0]), int(use.shape[0])
    off = np.ascontiguousarray(np.asarray(sphere_offsets), dtype=np.int32)
    dr._require(off.shape == (L + 1,), "sphere_offsets must be a host array of L + 1 entries")

    def dev_t(name, t, dtype, shape):
        dr._check_dev(name, t, dtype)
        dr._require(t.device == dev and tuple(t.shape) == tuple(shape), f"{name} must have shape {list(shape)}")
        return t.contiguous()

    def f64(name, t, rows):
        if t is None:
            return None
        dr._check_dev(name, t, torch.float64)
        dr._require(t.device == dev and t.dim() == 2 and t.shape[1] == 4 and t.shape[0] >= rows, f"{name} must have shape [{rows}, 4]")
        return t.contiguous()

    parent, kind, qidx = (dev_t(k, t, torch.int32, (N,)) for k, t in (("parent", parent), ("kind", kind), ("qidx", qidx)))
    use = dev_t("use", use, torch.int32, (L,))
    origin, axis = dev_t("origin", origin.reshape(N, 16), torch.float64, (N, 16)), dev_t("axis", axis, torch.float64, (N, 3))
    offset = dev_t("offset", offset, torch.float32, (J,))
    upstream, below = dev_t("upstream", upstream, torch.int32, (L,)), dev_t("below", below, torch.int32, (J,))
    reach_radius = dev_t("reach_radius", reach_radius, torch.float64, (J, L))
    pair_enable = dev_t("pair_enable", pair_enable, torch.int32, (L,))
    spheres, link_bounds = f64("spheres", spheres, max(int(off[-1]), 0)), f64("link_bounds", link_bounds, L)
    planes, obstacles = f64("planes", planes, 0), f64("obstacles", obstacles, 0)
    if reach is not None:
        reach = dev_t("reach", reach.reshape(-1), torch.float64, (4,))
    Np = 0 if planes is None else int(planes.shape[0])
    No = 0 if obstacles is None else int(obstacles.shape[0])
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    ints = lambda: torch.full((n,), -1, dtype=torch.int32, device=dev)
    out = types.SimpleNamespace(status=ints(), t_free=nan(n), evals=ints(), cert_self=nan(n), cert_env=nan(n), cert_reach=nan(n),
                                stop_self=nan(n), stop_env=nan(n), stop_reach=nan(n), stop_pair=ints())
    if trace:
        out.trace_t, out.trace_val = nan(n, max(max_evals, 1)), nan(n, max(max_evals, 1), 6)
    head = [_lib.ptr(t) for t in (parent, origin, kind, axis, qidx, use)] + [N, J, L]
    proxies = [_lib.ptr(spheres), off.ctypes.data_as(ctypes.c_void_p), _lib.ptr(link_bounds), _lib.ptr(pair_enable),
               _lib.ptr(planes) if Np else None, Np, _lib.ptr(obstacles) if No else None, No]
    tables = [_lib.ptr(upstream), _lib.ptr(below), _lib.ptr(reach_radius)]
    keep = (parent, origin, kind, axis, qidx, use, offset, spheres, off, link_bounds, pair_enable, planes, obstacles, reach,
            upstream, below, reach_radius)               # (alive until the launch is queued)
    return head, _lib.ptr(offset), proxies, _lib.ptr(reach), tables, out, keep


def _segment_outputs(out, trace):
    return [_lib.ptr(getattr(out, k)) for k in ("status", "t_free", "evals", "cert_self", "cert_env", "cert_reach", "stop_self",
                                                "stop_env", "stop_reach", "stop_pair")], \
        [_lib.ptr(out.trace_t) if trace else None, _lib.ptr(out.trace_val) if trace else None]


def segment_clearance(table, q0, q1, offset, spheres, sphere_offsets, link_bounds, pair_enable, upstream, below, reach_radius,
                      planes=None, obstacles=None, env_links=0, reach=None, cutoff=0.25, margin=0.01, depth=(3, 9), max_evals=96,
                      trace=False):
    """One ``ehr_segment_clearance`` launch (include/ehr.h).  Device tensors: ``table`` = (parent, origin, kind, axis, qidx, use)
    of the joint table (int32 / float64), q0 [J], q1 [n,J] float64, offset [J] float32, the proxy arguments of
    :func:`config_clearance` (``sphere_offsets`` [L+1]: a HOST array), upstream [L] and below [J] int32 (the uint32 words'
    bits), reach_radius [J,L] float64.  Returns a namespace of device tensors [n]: ``status``, ``evals``, ``stop_pair`` int32,
    ``t_free``, ``cert_self``, ``cert_env``, ``cert_reach``, ``stop_self``, ``stop_env``, ``stop_reach`` float64, pre-filled
    with NaN / -1; with ``trace``, ``trace_t`` [n,max_evals] and ``trace_val`` [n,max_evals,6] (NaN past ``evals``).  Never
    synchronises; the sizes' limits are the library's to refuse."""
    if not _lib.has_segment_clearance():
        _missing_segment()
    dr._check_dev("q1", q1, torch.float64)
    dev = q1.device
    dr._require(q1.dim() == 2, "q1 must have shape [n, J]")
    n, J = int(q1.shape[0]), int(q1.shape[1])
    max_evals = int(max_evals)
    head, offset, proxies, reach, tables, out, keep = _segment_common(
        table, J, dev, offset, spheres, sphere_offsets, link_bounds, pair_enable, upstream, below, reach_radius, planes, obstacles,
        reach, n, max_evals, trace)
    dr._check_dev("q0", q0, torch.float64)
    dr._require(q0.device == dev and tuple(q0.shape) == (J,), f"q0 must have shape {[J]}")
    q0, q1 = q0.contiguous(), q1.contiguous()
    outs, traces = _segment_outputs(out, trace)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ehr_segment_clearance(
            *head, _lib.ptr(q0), _lib.ptr(q1), offset, n, *proxies, int(env_links) & 0xffffffff, reach, float(cutoff), *tables,
            float(margin), int(depth[0]), int(depth[1]), max_evals, *outs, *traces, _stream()), "ehr_segment_clearance")
    return out


def _missing_roadmap():
    raise RuntimeError("this libehr_hip.so has no roadmap kernels (ehr_edge_clearance, ehr_roadmap_paths): rebuild it")


def edge_clearance(table, nodes, edge_a, edge_b, offset, spheres, sphere_offsets, link_bounds, pair_enable, upstream, below,
                   reach_radius, planes=None, obstacles=None, env_links=0, reach=None, cutoff=0.25, margin=0.01, depth=(3, 9),
                   max_evals=96, trace=False):
    """One ``ehr_edge_clearance`` launch (include/ehr.h): :func:`segment_clearance` for the edges of a roadmap.  Device tensors
    as there, but nodes [V,J] float64 and edge_a, edge_b [n] int32 take the place of q0 and q1: edge e runs from node
    ``edge_a[e]`` to node ``edge_b[e]``, and an index outside ``0..V-1`` marks an edge that is skipped (status 3, evals 0).
    Returns :func:`segment_clearance`'s namespace [n] and ``length`` [n] float64, pre-filled with NaN / -1.  Never synchronises;
    the sizes' limits are the library's to refuse."""
    if not _lib.has_roadmap():
        _missing_roadmap()
    dr._check_dev("nodes", nodes, torch.float64)
    dev = nodes.device
    dr._require(nodes.dim() == 2, "nodes must have shape [V, J]")
    V, J = int(nodes.shape[0]), int(nodes.shape[1])
    dr._check_dev("edge_a", edge_a, torch.int32)
    dr._check_dev("edge_b", edge_b, torch.int32)
    dr._require(edge_a.device == dev and edge_b.device == dev and edge_a.dim() == 1 and edge_a.shape == edge_b.shape,
                "edge_a and edge_b must have shape [n]")
    n, max_evals = int(edge_a.shape[0]), int(max_evals)
    head, offset, proxies, reach, tables, out, keep = _segment_common(
        table, J, dev, offset, spheres, sphere_offsets, link_bounds, pair_enable, upstream, below, reach_radius, planes, obstacles,
        reach, n, max_evals, trace)
    out.length = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    nodes, edge_a, edge_b = nodes.contiguous(), edge_a.contiguous(), edge_b.contiguous()
    outs, traces = _segment_outputs(out, trace)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ehr_edge_clearance(
            *head, _lib.ptr(nodes), V, _lib.ptr(edge_a), _lib.ptr(edge_b), offset, n, *proxies, int(env_links) & 0xffffffff, reach,
            float(cutoff), *tables, float(margin), int(depth[0]), int(depth[1]), max_evals, *outs, _lib.ptr(out.length), *traces,
            _stream()), "ehr_edge_clearance")
    return out


def roadmap_paths(adj_start, adj_node, adj_edge, edge_status, edge_length, source=0, hops=4):
    """One ``ehr_roadmap_paths`` launch (include/ehr.h): shortest paths of at most ``hops`` usable edges from ``source``.  Device
    tensors: the CSR adjacency adj_start [V+1], adj_node [A], adj_edge [A] int32 (:func:`roadmap_edges`), edge_status [E] int32
    and edge_length [E] float64 (:func:`edge_clearance`).  Returns a namespace of device tensors, pre-filled with NaN / -1:
    ``dist`` [H+1,V] float64, ``pred_node``, ``pred_edge`` [H,V], ``hops`` [V], ``path`` [V,H+1], ``path_edge`` [V,H] and
    ``changed`` [H] int32.  Never synchronises; the sizes' limits are the library's to refuse."""
    if not _lib.has_roadmap():
        _missing_roadmap()
    dr._check_dev("adj_start", adj_start, torch.int32)
    dev = adj_start.device
    dr._require(adj_start.dim() == 1 and adj_start.shape[0] >= 1, "adj_start must have shape [V + 1]")
    V, H = int(adj_start.shape[0]) - 1, int(hops)
    for name, t, dtype in (("adj_node", adj_node, torch.int32), ("adj_edge", adj_edge, torch.int32),
                           ("edge_status", edge_status, torch.int32), ("edge_length", edge_length, torch.float64)):
        dr._check_dev(name, t, dtype)
        dr._require(t.device == dev and t.dim() == 1, f"{name} must have one dimension")
    dr._require(adj_node.shape == adj_edge.shape, "adj_node and adj_edge must have shape [A]")
    dr._require(edge_status.shape == edge_length.shape, "edge_status and edge_length must have shape [E]")
    A, E = int(adj_node.shape[0]), int(edge_status.shape[0])
    adj_start, adj_node, adj_edge = adj_start.contiguous(), adj_node.contiguous(), adj_edge.contiguous()
    edge_status, edge_length = edge_status.contiguous(), edge_length.contiguous()
    Hs, Vs = max(H, 0), max(V, 0)
    ints = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)
    out = types.SimpleNamespace(dist=torch.full((Hs + 1, Vs), float("nan"), dtype=torch.float64, device=dev),
                                pred_node=ints(Hs, Vs), pred_edge=ints(Hs, Vs), hops=ints(Vs), path=ints(Vs, Hs + 1),
                                path_edge=ints(Vs, Hs), changed=ints(Hs))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ehr_roadmap_paths(
            _lib.ptr(adj_start), _lib.ptr(adj_node) if A else None, _lib.ptr(adj_edge) if A else None, A,
            _lib.ptr(edge_status) if E else None, _lib.ptr(edge_length) if E else None, V, E, int(source), H, _lib.ptr(out.dist),
            _lib.ptr(out.pred_node), _lib.ptr(out.pred_edge), _lib.ptr(out.hops), _lib.ptr(out.path), _lib.ptr(out.path_edge),
            _lib.ptr(out.changed), _stream()), "ehr_roadmap_paths")
    return out


def roadmap_edges(nodes, ok, neighbours):
    """The edge list and the adjacency of one round's roadmap, on the device, with fixed shapes and no synchronisation.
    nodes [V,J] float64 (node 0: where the arm is), ok [V] bool (the node may be an end point), ``neighbours`` = K >= 0.

    Edges ``0 .. V-2`` are the direct moves ``(0, v)``, v = 1..V-1.  Edge ``V - 1 + (v - 1) K + k`` is node v's k-th nearest
    OTHER node u >= 1, written ``(min(u, v), max(u, v))``: nearness by the squared joint-space distance, accumulated ``acc = acc +
    d_j * d_j`` over ascending j from 0.0, each operation rounded on its own; a stable sort, so ties go to the lower index, and
    a second stable sort that puts the nodes with ``ok`` before the others (a slot is not spent on a node that cannot be an
    end point while one that can is left).  It is written ``(-1, -1)`` -- skipped -- where either end has no ``ok``, where
    u < v lists v among its own K (the lower index's copy stands), and where v has fewer than k + 1 other nodes.

    Returns (edge_a [E], edge_b [E], adj_start [V+1], adj_node [2E], adj_edge [2E]) int32, E = (V - 1)(1 + K): the CSR
    adjacency over all E edges, both directions, each node's slots in ascending edge index; the slots of skipped edges lie
    past ``adj_start[V]`` with node -1.

    Memory: dense [V,V] transients -- two float64 and three int64 matrices and one of bool, about 41 V^2 bytes: 0.7 GB at the
    4096 nodes a roadmap may have, 41 MB at 1000."""
    dr._check_dev("nodes", nodes, torch.float64)
    dev = nodes.device
    dr._require(nodes.dim() == 2 and nodes.shape[0] >= 1, "nodes must have shape [V, J]")
    V, J, K = int(nodes.shape[0]), int(nodes.shape[1]), int(neighbours)
    dr._require(K >= 0, "neighbours must be >= 0")
    dr._require(ok.device == dev and ok.dtype == torch.bool and tuple(ok.shape) == (V,), "ok must be a bool tensor [V]")
    M = V - 1                                            # the nodes that have neighbours: 1..V-1
    ar = torch.arange(1, V, device=dev, dtype=torch.int64)
    da, db = torch.zeros_like(ar), ar.clone()            # the direct moves
    if K > 0 and M > 0:
        O = max(M - 1, 0)                                # the others of each node
        rows = torch.arange(M, device=dev)[:, None]
        cols = torch.arange(O, device=dev)[None, :]
        other = cols + (cols >= rows)                    # [M,O]: 0..M-1 without the row itself, ascending
        x = nodes[1:]
        acc = torch.zeros((M, M), dtype=torch.float64, device=dev)   # every pair once, the diagonal dropped below
        for j in range(J):
            d = x[None, :, j] - x[:, None, j]
            acc = acc + d * d
        acc = torch.gather(acc, 1, other)
        order = torch.argsort(acc, dim=1, stable=True)               # (NaN sorts last, as numpy's)
        near = torch.gather(other, 1, order)                         # 0-based among nodes 1.., nearest first
        first = torch.argsort((~ok[1:][near]).to(torch.int8), dim=1, stable=True)[:, :K]
        near = torch.gather(near, 1, first)                          # [M,min(K,O)]: those with ok before the others
        lists = torch.zeros((M, M), dtype=torch.bool, device=dev)
        lists.scatter_(1, near, True)                                # lists[v,u]: v lists u
        v0 = rows.expand_as(near)
        good = ok[1:][v0] & ok[1:][near] & ~((near < v0) & lists[near, v0])
        na = torch.where(good, torch.minimum(near, v0) + 1, -1)
        nb = torch.where(good, torch.maximum(near, v0) + 1, -1)
        pad = torch.full((M, K - near.shape[1]), -1, dtype=torch.int64, device=dev)
        na, nb = torch.cat([na, pad], dim=1).reshape(-1), torch.cat([nb, pad], dim=1).reshape(-1)
    else:
        na = nb = torch.full((M * K,), -1, dtype=torch.int64, device=dev)
    ea, eb = torch.cat([da, na]), torch.cat([db, nb])
    E = int(ea.shape[0])
    eidx = torch.arange(E, device=dev, dtype=torch.int64)
    owner, partner = torch.cat([ea, eb]), torch.cat([eb, ea])
    owner = torch.where(owner < 0, V, owner)                         # skipped edges: past every node
    # (the keys of kept edges differ; the two slots of a skipped edge tie, and both read (-1, e): their order does not show)
    at = torch.argsort(owner * max(E, 1) + torch.cat([eidx, eidx]))
    start = torch.searchsorted(owner[at].contiguous(), torch.arange(V + 1, device=dev, dtype=torch.int64))
    i32 = lambda t: t.to(torch.int32).contiguous()
    return i32(ea), i32(eb), i32(start), i32(partner[at]), i32(torch.cat([eidx, eidx])[at])


# ---- the filter -------------------------------------------------------------------------------------------------------------
def _joint_kinds(table, J):
    """[J]: the kind of the link each active joint moves."""
    out = np.zeros(J, dtype=np.int32)
    for k, c in zip(np.asarray(table["kind"]), np.asarray(table["qidx"])):
        if 0 <= c < J:
            out[c] = k
    return out


def _rows4(a, name, limit):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, 4))
    if a.shape[0] > limit or not np.isfinite(a).all():
        raise ValueError(f"{name}: at most {limit} finite rows of 4, got {a.shape[0]}")
    return a if a.shape[0] else None


class FeasibilityFilter:
    """Which candidate joint configurations the arm can take: sphere proxies of the rendered links against each other, against
    half-spaces and obstacle spheres, and inside a ball of allowed reach.

    robot: :class:`easyhec_amd.robot.Robot`.  leaf_triangles: see :func:`link_spheres`.  margin: the clearance [m] a valid
    configuration keeps to itself and to the environment.  ignore_pairs / settle_qpos: see :func:`enabled_pairs`.  planes
    [Np,4] (n, d), ``n.x + d >= 0`` inside (normalised here to unit n; :func:`box_planes` makes a workspace box); obstacles
    [No,4] spheres in the base frame; env_links: the rendered links tested against both (default: every link an active joint
    moves -- the base stands on the table).  reach: (centre, radius) of the ball every proxy must stay inside, or None.
    cutoff: clearances are reported up to this value [m].  offsets: joint zero offsets [J] for the kinematics -- None (zeros),
    an array, or a solve step's current offsets tensor (read on every call).  path_steps: what an online loop passes to
    :meth:`check` (None: 1).

    exact: judge the arm against itself and against planes and obstacles on the MESHES behind the proxies
    (:func:`mesh_clearance`); reach stays on the proxies.  The proxies remain the broad phase, so nothing they clear is looked
    at again.  exact_cutoff: mesh clearances are reported up to this value [m] (default ``max(2 margin, 0.02)``: only "above
    margin or not" is needed, and a short cutoff is what lets the kernel skip most of the meshes).

    swept: :meth:`check_swept` is what an online loop calls: a certificate for the whole segment instead of ``path_steps``
    samples of it, with a search budget of ``swept_depth`` = (min, max) bisection depth and ``swept_evals`` evaluations per
    candidate; offset_bound: the largest joint offset [rad or m] the certificate allows for.  Not with ``exact``.

    detour_hops: 0, or 2..8 (with ``swept``): :meth:`plan` is what an online loop calls -- a candidate whose straight move is
    turned down is kept if a path of at most ``detour_hops`` certified straight moves over the other candidates leads to it.
    detour_neighbours: the nearest candidates each candidate is joined to; detour_via: extra nodes per :meth:`plan`, drawn with
    ``robot.sample_qpos`` from a generator seeded with ``detour_seed`` at construction.

    ``pairs``: the enabled link pairs; ``ignored``: the others with reason and settle clearance.  With ``exact``, ``mesh_pairs``
    is what the mesh kernel checks: ``pairs`` and every "settle"-ignored pair whose MESHES keep more than ``margin`` at the
    settle configuration (the proxies touched there, the links do not); ``ignored`` then holds the rest, the "settle" entries
    with their ``mesh_clearance``."""

    def __init__(self, robot, leaf_triangles=64, margin=0.01, ignore_pairs="auto", settle_qpos=None, planes=None,
                 obstacles=None, env_links=None, reach=None, cutoff=0.25, offsets=None, device="cuda:0", path_steps=None,
                 exact=False, exact_cutoff=None, swept=False, swept_depth=(3, 9), swept_evals=96, offset_bound=0.2,
                 detour_hops=0, detour_neighbours=8, detour_via=0, detour_seed=0):
        from .joint_calib import _check_table
        if getattr(robot, "mount_link", None) is not None:
            raise ValueError(f"FeasibilityFilter: the robot is a view mounted on link {robot.mount_link!r}; clearance to planes, "
                             "obstacles and the reach ball is a base-frame question: pass the robot's .base")
        if not _lib.has_feasibility():
            _missing()
        self.exact, self.swept = bool(exact), bool(swept)
        if self.swept and self.exact:
            raise ValueError("FeasibilityFilter: swept=True certifies the sphere proxies; a mesh-exact certificate (exact=True) "
                             "does not exist")
        if self.swept and not _lib.has_segment_clearance():
            _missing_segment()
        self.detour_hops, self.detour_neighbours, self.detour_via = int(detour_hops), int(detour_neighbours), int(detour_via)
        if self.detour_hops != 0 and not 2 <= self.detour_hops <= _lib.ROADMAP_MAX_HOPS:
            raise ValueError(f"FeasibilityFilter: detour_hops {detour_hops} must be 0 (no detours) or 2..{_lib.ROADMAP_MAX_HOPS}")
        if self.detour_hops and not self.swept:
            raise ValueError("FeasibilityFilter: detour_hops needs swept=True (a roadmap's edges are certified segments)")
        if self.detour_neighbours < 0 or self.detour_via < 0:
            raise ValueError(f"FeasibilityFilter: detour_neighbours {detour_neighbours} and detour_via {detour_via} must be >= 0")
        if self.detour_hops and not _lib.has_roadmap():
            _missing_roadmap()
        self._via_rng = np.random.default_rng(detour_seed)             # seeded once: every plan() draws on from it
        self.swept_depth, self.swept_evals = (int(swept_depth[0]), int(swept_depth[1])), int(swept_evals)
        self.offset_bound = float(offset_bound)
        if not (0 <= self.swept_depth[0] <= self.swept_depth[1] <= _lib.SEG_MAX_DEPTH and
                1 <= self.swept_evals <= _lib.SEG_MAX_EVALS and np.isfinite(self.offset_bound) and self.offset_bound >= 0):
            raise ValueError(f"FeasibilityFilter: swept_depth {swept_depth} must be 0 <= min <= max <= {_lib.SEG_MAX_DEPTH}, "
                             f"swept_evals {swept_evals} 1..{_lib.SEG_MAX_EVALS}, offset_bound {offset_bound} >= 0")
        if self.exact and not _lib.has_mesh_clearance():
            _missing_mesh()
        if not (np.isfinite(cutoff) and cutoff > 0 and np.isfinite(margin) and 0 <= margin < cutoff):
            raise ValueError(f"FeasibilityFilter: need 0 <= margin < cutoff, finite (margin {margin}, cutoff {cutoff})")
        self.robot, self.margin, self.cutoff = robot, float(margin), float(cutoff)
        self.path_steps = None if path_steps is None else int(path_steps)
        self.dev = dev = torch.device(device)
        table = robot.joint_table()
        self.J, self.L = int(robot.chain.dof), int(robot.num_links)
        _check_table(table, self.J)
        if not 1 <= self.L <= _lib.FEAS_MAX_LINKS:
            raise ValueError(f"FeasibilityFilter: {self.L} rendered links; the kernel takes 1..{_lib.FEAS_MAX_LINKS}")
        self.spheres, self.sphere_offsets, self.link_bounds = robot_proxies(robot, leaf_triangles)
        if self.spheres.shape[0] > _lib.FEAS_MAX_SPHERES:
            raise ValueError(f"FeasibilityFilter: {self.spheres.shape[0]} proxy spheres; the kernel takes {_lib.FEAS_MAX_SPHERES} "
                             "(raise leaf_triangles)")
        self.pairs, self.ignored = enabled_pairs(robot, self.spheres, self.sphere_offsets, self.margin, ignore_pairs, settle_qpos)
        moved = [l for l in range(self.L) if int(table["upstream"][l]) != 0]
        self.env_links = moved if env_links is None else sorted({int(l) for l in env_links})
        if any(l < 0 or l >= self.L for l in self.env_links):
            raise ValueError(f"env_links {self.env_links}: rendered links are 0..{self.L - 1}")
        self.env_mask = sum(1 << l for l in self.env_links)
        planes = _rows4(planes, "planes", _lib.FEAS_MAX_PLANES)
        if planes is not None:
            norm = np.sqrt((planes[:, :3] ** 2).sum(axis=1))
            if not (norm > 0).all():
                raise ValueError("planes: a normal of length 0")
            planes = planes / norm[:, None]
        self.planes, self.obstacles = planes, _rows4(obstacles, "obstacles", _lib.FEAS_MAX_OBSTACLES)
        if reach is not None:
            reach = np.asarray(reach, dtype=np.float64).reshape(-1)
            if reach.shape != (4,) or not np.isfinite(reach).all() or reach[3] <= 0:
                raise ValueError("reach: (cx, cy, cz, radius > 0)")
        self.reach = reach
        up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt)).to(dev)
        self._t = [up(table[k], dt) for k, dt in (("parent", np.int32), ("origin", np.float64), ("kind", np.int32),
                                                  ("axis", np.float64), ("qidx", np.int32), ("use", np.int32))]
        self._N = int(table["parent"].shape[0])
        self._spheres, self._bounds = up(self.spheres, np.float64), up(self.link_bounds, np.float64)
        self._pair_enable = up(pair_words(self.pairs, self.L).view(np.int32), np.int32)
        self._planes, self._obstacles, self._reach = up(self.planes, np.float64), up(self.obstacles, np.float64), up(reach, np.float64)
        if offsets is None:
            self.offsets = torch.zeros((self.J,), dtype=torch.float32, device=dev)
        elif torch.is_tensor(offsets) and offsets.device == dev and offsets.dtype == torch.float32:
            self.offsets = offsets                      # a step's own tensor: its current values on every call
        else:
            self.offsets = torch.as_tensor(np.asarray(offsets.detach().cpu() if torch.is_tensor(offsets) else offsets,
                                                      dtype=np.float32)).to(dev)
        if tuple(self.offsets.shape) != (self.J,) or not self.offsets.is_contiguous():
            raise ValueError(f"offsets must be a contiguous [{self.J}] tensor")
        if self.exact:
            self._init_exact(leaf_triangles, exact_cutoff, settle_qpos)
        if self.swept and self.spheres.shape[0] > _lib.SEG_MAX_SPHERES:
            raise ValueError(f"FeasibilityFilter: {self.spheres.shape[0]} proxy spheres; the swept kernel takes "
                             f"{_lib.SEG_MAX_SPHERES} (raise leaf_triangles)")
        self._table = table
        self._upstream = up(np.asarray(table["upstream"], dtype=np.uint32).view(np.int32), np.int32)
        self._below = up(joint_below(table).view(np.int32), np.int32)
        self._prismatic = np.array([int(k) == 2 for k in _joint_kinds(table, self.J)])

    def _init_exact(self, leaf_triangles, exact_cutoff, settle_qpos):
        """The triangles behind the proxies and ``mesh_pairs``: one launch per "settle"-ignored pair, that pair alone enabled,
        at the settle configuration(s) (the host's kinematics, as :func:`enabled_pairs` uses)."""
        self.exact_cutoff = max(2.0 * self.margin, 0.02) if exact_cutoff is None else float(exact_cutoff)
        if not (np.isfinite(self.exact_cutoff) and self.margin < self.exact_cutoff):
            raise ValueError(f"FeasibilityFilter: need margin < exact_cutoff, finite (margin {self.margin}, exact_cutoff "
                             f"{self.exact_cutoff})")
        self.triangles, self.tri_offsets = robot_triangles(self.robot, leaf_triangles)
        if self.triangles.shape[0] > _lib.MESH_MAX_TRIANGLES:
            raise ValueError(f"FeasibilityFilter: {self.triangles.shape[0]} triangles; the kernel takes {_lib.MESH_MAX_TRIANGLES}")
        dev = self.dev
        self._triangles = torch.from_numpy(self.triangles).to(dev)
        self._tri_offsets = torch.from_numpy(self.tri_offsets).to(dev)
        self._pair_none = torch.zeros((self.L,), dtype=torch.int32, device=dev)
        q0 = np.zeros((1, self.J)) if settle_qpos is None else np.atleast_2d(np.asarray(settle_qpos, dtype=np.float64))
        lp = torch.from_numpy(np.ascontiguousarray(self.robot.link_poses_batch(q0), dtype=np.float32)).to(dev)
        self.mesh_pairs, rest = list(self.pairs), []
        for d in self.ignored:
            if d["reason"] == "settle":
                words = torch.from_numpy(pair_words([d["pair"]], self.L).view(np.int32)).to(dev)
                clear = float(mesh_clearance(lp, self._spheres, self.sphere_offsets, self._bounds, words, self._triangles,
                                             self._tri_offsets, cutoff=self.exact_cutoff).mesh_clear.min().cpu())
                if clear > self.margin:
                    self.mesh_pairs.append(d["pair"])
                    continue
                d = dict(d, mesh_clearance=clear)
            rest.append(d)
        self.mesh_pairs.sort()
        self.ignored = rest
        self._mesh_enable = torch.from_numpy(pair_words(self.mesh_pairs, self.L).view(np.int32)).to(dev)

    # -- the parts ----------------------------------------------------------------------------------------------------------
    def path_table(self, qposes, current_qpos=None, path_steps=1):
        """[Q * path_steps, J] float64 (host): per candidate the configurations ``current + (s + 1) / path_steps * (candidate -
        current)``, s = 0..path_steps - 1 -- the last is the candidate itself; without ``current_qpos``, the candidates."""
        q = np.atleast_2d(np.asarray(qposes.detach().cpu() if torch.is_tensor(qposes) else qposes, dtype=np.float64))
        qp = np.zeros((q.shape[0], self.J))
        qp[:, :min(self.J, q.shape[1])] = q[:, :self.J]
        path_steps = int(path_steps)
        if current_qpos is None:
            if path_steps != 1:
                raise ValueError("check: path_steps > 1 needs current_qpos")
            return qp, 1
        if path_steps < 1:
            raise ValueError("check: path_steps must be >= 1")
        c = np.asarray(current_qpos, dtype=np.float64).reshape(-1)
        cur = np.zeros(self.J)
        cur[:min(self.J, c.shape[0])] = c[:self.J]
        frac = (np.arange(path_steps, dtype=np.float64) + 1.0) / path_steps
        tab = cur[None, None, :] + frac[None, :, None] * (qp[:, None, :] - cur[None, None, :])
        tab[:, -1] = qp                                  # (the candidate itself, not current + 1.0 * difference)
        return np.ascontiguousarray(tab.reshape(-1, self.J)), path_steps

    def kinematics(self, qpos_table):
        """link_poses [n,L,4,4] float32 on the device of a host table [n,J]: one ``ehr_joint_forward`` at ``offsets``."""
        dev, n = self.dev, int(qpos_table.shape[0])
        qd = torch.from_numpy(np.ascontiguousarray(qpos_table, dtype=np.float64)).to(dev)
        lp = torch.empty((n, self.L, 4, 4), device=dev)
        jf = torch.empty((n, self.J, 6), device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ehr_joint_forward(*[_lib.ptr(t) for t in self._t], self._N, self.J, self.L, _lib.ptr(qd),
                                                    _lib.ptr(self.offsets), n, _lib.ptr(lp), _lib.ptr(jf), _stream()),
                       "ehr_joint_forward")
        return lp

    def clearance(self, link_poses):
        """The kernel on link poses [n,L,4,4]: a namespace of ``self_clear``, ``self_pair``, ``env_clear``, ``reach_clear`` [n]."""
        return config_clearance(link_poses, self._spheres, self.sphere_offsets, self._bounds, self._pair_enable, self._planes,
                                self._obstacles, self.env_mask, self._reach, self.cutoff)

    def check_swept(self, qposes, current_qpos, trace=False):
        """Judges the WHOLE straight joint-space segment from ``current_qpos`` to each candidate [Q, <= dof] on the sphere
        proxies: one ``ehr_segment_clearance`` launch with the budget ``swept_depth`` / ``swept_evals``; nothing synchronises.
        The prismatic joints' travel in ``reach_radii`` is their largest ``|q|`` over ``current_qpos`` and the candidates plus
        ``offset_bound``, which the joint offsets must stay within.  Returns a namespace of device tensors [Q]:

        ``valid`` bool: ``status == 0``, more than ``margin`` is kept on all of the segment; ``status`` int32 (0 clear, 1 hit,
        2 undecided within the budget, 3 cannot judge: a value that is not finite), ``t_free`` (the move is certified on
        ``[0, t_free]``), ``evals``; ``self_ok`` / ``env_ok`` / ``reach_ok``: what stopped it -- for a hit the tests the
        stopping configuration passes, for status 2 and 3 none (the kernel does not say which certificate fell short, so
        none counts as passed); ``cert_self`` / ``cert_env`` / ``cert_reach``: the least certified values, and
        ``stop_self`` / ``stop_env`` / ``stop_reach`` / ``stop_pair``: the raw values where the search stopped (NaN, -1 when
        clear).  ``trace``: also ``trace_t`` and ``trace_val`` of :func:`segment_clearance`."""
        qp, _ = self.path_table(qposes)
        cur, _ = self.path_table(np.asarray(current_qpos, dtype=np.float64).reshape(1, -1))
        travel = np.where(self._prismatic, np.abs(np.concatenate([qp, cur])).max(axis=0) + self.offset_bound, 0.0)
        W = reach_radii(self._table, self.link_bounds, travel)
        dev = self.dev
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        out = segment_clearance(self._t, to(cur[0]), to(qp), self.offsets, self._spheres, self.sphere_offsets, self._bounds,
                                self._pair_enable, self._upstream, self._below, to(W), self._planes, self._obstacles,
                                self.env_mask, self._reach, self.cutoff, self.margin, self.swept_depth, self.swept_evals,
                                trace=trace)
        hit = out.status == 1
        out.valid = out.status == 0
        out.self_ok = out.valid | (hit & (out.stop_self > self.margin))
        out.env_ok = out.valid | (hit & (out.stop_env > self.margin))
        out.reach_ok = out.valid | (hit & (out.stop_reach >= 0))
        return out

    def plan(self, qposes, current_qpos, via=None):
        """A roadmap over one round's candidates: which of them [Q, <= dof] the arm can reach from ``current_qpos`` by at most
        ``detour_hops`` straight joint-space moves, each certified on the
        sphere proxies as :meth:`check_swept` certifies the direct one.  The nodes are ``[current] + candidates + via``
        (``via`` [., <= dof]: extra configurations to pass through; None: ``detour_via`` samples of ``robot.sample_qpos``), at
        most 4096.  End-point validity comes from :meth:`check` of all nodes but the first (one kinematics and one
        ``ehr_config_clearance`` launch), the edges from :func:`roadmap_edges` (every direct move and each valid node's
        ``detour_neighbours`` nearest), their certificates from one ``ehr_edge_clearance`` launch, the paths from one
        ``ehr_roadmap_paths`` launch.  ``reach_radii`` takes the prismatic joints' travel over ALL nodes plus ``offset_bound``.
        Nothing synchronises.  Returns a namespace of device tensors:

        ``direct``: the fields of :meth:`check_swept` [Q] for the direct moves (the same bits as ``check_swept`` when there are
        no via nodes or no prismatic joints; otherwise :func:`segment_clearance` at this roadmap's ``reach_radii``);
        ``reachable`` bool [Q]; ``hops`` int32 [Q] (-1: not reachable); ``length`` float64 [Q]: the path's joint-space length
        (inf: not reachable); ``detour`` bool [Q] = ``reachable & ~direct.valid``; ``path_nodes`` int32 [Q,H+1]: node indices,
        0 (the current configuration) first, -1 past the end; ``waypoints`` float64 [Q,H+1,J]: those nodes' rows, NaN past the
        end; ``path_cert`` float64 [Q]: the least ``cert_self`` / ``cert_env`` over the path's edges (NaN: not reachable);
        ``nodes`` [V,J], ``end_valid`` bool [V], ``edges`` int32 [E,2] ((-1, -1): skipped), ``edge_status``, ``edge_evals`` int32
        [E], ``edge_length`` float64 [E], ``changed`` int32 [H] (``changed[-1] == 0``: more hops reach nothing more),
        ``paths``, the whole of :func:`roadmap_paths`, and ``edge_clearance``, the whole of :func:`edge_clearance`.

        What it is NOT: a time parameterisation or a smoother.  The waypoints are the corners of a polyline in joint space;
        nothing is shortcut, blended or timed (the reference's TOPP pass has no counterpart here)."""
        if not self.detour_hops:
            raise RuntimeError("FeasibilityFilter.plan: the filter was built with detour_hops=0")
        H, K = self.detour_hops, self.detour_neighbours
        qp, _ = self.path_table(qposes)
        cur, _ = self.path_table(np.asarray(current_qpos, dtype=np.float64).reshape(1, -1))
        if via is None:
            via = self.robot.sample_qpos(self.detour_via, self._via_rng) if self.detour_via else np.zeros((0, self.J))
        via = np.asarray(via, dtype=np.float64)
        vp = self.path_table(via)[0] if via.size else np.zeros((0, self.J))
        nodes = np.ascontiguousarray(np.concatenate([cur, qp, vp]))
        Q, V = qp.shape[0], nodes.shape[0]
        if V > _lib.ROADMAP_MAX_NODES:
            raise ValueError(f"FeasibilityFilter.plan: {V} nodes (1 + {Q} candidates + {vp.shape[0]} via); the roadmap takes "
                             f"{_lib.ROADMAP_MAX_NODES}")
        dev = self.dev
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        end_valid = torch.cat([torch.ones((1,), dtype=torch.bool, device=dev), self.check(nodes[1:]).valid]) if V > 1 else \
            torch.ones((1,), dtype=torch.bool, device=dev)
        travel = np.where(self._prismatic, np.abs(nodes).max(axis=0) + self.offset_bound, 0.0)
        W = reach_radii(self._table, self.link_bounds, travel)
        nd = to(nodes)
        ea, eb, adj_start, adj_node, adj_edge = roadmap_edges(nd, end_valid, K)
        ec = edge_clearance(self._t, nd, ea, eb, self.offsets, self._spheres, self.sphere_offsets, self._bounds, self._pair_enable,
                            self._upstream, self._below, to(W), self._planes, self._obstacles, self.env_mask, self._reach,
                            self.cutoff, self.margin, self.swept_depth, self.swept_evals)
        paths = roadmap_paths(adj_start, adj_node, adj_edge, ec.status, ec.length, 0, H)
        direct = types.SimpleNamespace(**{k: getattr(ec, k)[:Q] for k in (
            "status", "t_free", "evals", "cert_self", "cert_env", "cert_reach", "stop_self", "stop_env", "stop_reach", "stop_pair")})
        hit = direct.status == 1
        direct.valid = direct.status == 0
        direct.self_ok = direct.valid | (hit & (direct.stop_self > self.margin))
        direct.env_ok = direct.valid | (hit & (direct.stop_env > self.margin))
        direct.reach_ok = direct.valid | (hit & (direct.stop_reach >= 0))
        hops_q = paths.hops[1:Q + 1]
        path_nodes, path_edge = paths.path[1:Q + 1], paths.path_edge[1:Q + 1].to(torch.int64)
        reachable = hops_q >= 0
        cert = torch.minimum(ec.cert_self, ec.cert_env)[path_edge.clamp(min=0)]
        cert = torch.where(path_edge >= 0, cert, torch.full_like(cert, float("inf"))).amin(dim=1)
        way = nd[path_nodes.to(torch.int64).clamp(min=0)]
        out = types.SimpleNamespace(
            direct=direct, reachable=reachable, hops=hops_q, length=paths.dist[H, 1:Q + 1], detour=reachable & ~direct.valid,
            path_nodes=path_nodes, waypoints=torch.where((path_nodes >= 0)[:, :, None], way, torch.full_like(way, float("nan"))),
            path_cert=torch.where(reachable, cert, torch.full_like(cert, float("nan"))), nodes=nd, end_valid=end_valid,
            edges=torch.stack([ea, eb], dim=1), edge_status=ec.status, edge_evals=ec.evals, edge_length=ec.length,
            changed=paths.changed, paths=paths, edge_clearance=ec)
        return out

    def mesh_clearance(self, link_poses):
        """The mesh kernel on link poses [n,L,4,4] (``exact=True`` only): a namespace of ``mesh_clear``, ``mesh_pair``,
        ``mesh_tri``, ``env_clear``, over ``mesh_pairs`` and up to ``exact_cutoff``."""
        if not self.exact:
            raise RuntimeError("FeasibilityFilter.mesh_clearance: the filter was built with exact=False")
        return mesh_clearance(link_poses, self._spheres, self.sphere_offsets, self._bounds, self._mesh_enable, self._triangles,
                              self._tri_offsets, self._planes, self._obstacles, self.env_mask, self.exact_cutoff)

    def check(self, qposes, current_qpos=None, path_steps=1):
        """Judges candidates [Q, <= dof]; with ``current_qpos`` each at the ``path_steps`` configurations of the straight
        joint-space segment towards it (:meth:`path_table`).  Kinematics, one clearance launch and a reduction over the steps
        with torch on the device: nothing synchronises.  Returns a namespace of device tensors [Q]:

        ``valid`` bool: ``self_clear > margin``, ``env_clear > margin`` and ``reach_clear >= 0`` at EVERY step (a NaN -- a
        configuration the kernel could not judge -- is not valid); ``self_ok`` / ``env_ok`` / ``reach_ok``: the three parts;
        ``self_clear`` / ``env_clear`` / ``reach_clear`` float64: the minimum over the steps (NaN if any step's is);
        ``self_pair`` int32: the pair at the first step that attains ``self_clear`` (-1: none below cutoff, or NaN);
        ``worst_step`` int64: the first step with the least slack ``min(self_clear - margin, env_clear - margin, reach_clear)``,
        a NaN counting as the least.

        With ``exact=True`` the kinematics run once, the proxy kernel gives ``reach_clear`` and the mesh kernel the other two:
        ``self_clear`` and ``env_clear`` are then distances of the meshes, reported up to ``exact_cutoff``, ``self_pair`` a
        pair of ``mesh_pairs`` that attains ``self_clear``, and the result gains ``mesh_pair`` (the same) and ``mesh_tri``
        int32 [Q,2], a triangle pair (rows of ``triangles``) that attains it, of the same step."""
        table, steps = self.path_table(qposes, current_qpos, path_steps)
        Q = table.shape[0] // steps
        lp = self.kinematics(table)
        if self.exact:
            mesh = self.mesh_clearance(lp)
            raw = config_clearance(lp, self._spheres, self.sphere_offsets, self._bounds, self._pair_none, None, None, 0,
                                   self._reach, self.cutoff)
            raw.self_clear, raw.self_pair, raw.env_clear = mesh.mesh_clear, mesh.mesh_pair, mesh.env_clear
        else:
            raw = self.clearance(lp)
        sc, ec, rc = (t.view(Q, steps) for t in (raw.self_clear, raw.env_clear, raw.reach_clear))
        self_ok, env_ok, reach_ok = (sc > self.margin).all(dim=1), (ec > self.margin).all(dim=1), (rc >= 0).all(dim=1)
        ar = torch.arange(steps, device=self.dev)[None].expand(Q, steps)

        def first_min(x):                                # NaN counts as the least; the lowest step among equals
            x = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x)
            return torch.where(x == x.amin(dim=1, keepdim=True), ar, steps).amin(dim=1)

        slack = torch.minimum(torch.minimum(sc - self.margin, ec - self.margin), rc)   # (torch.minimum hands a NaN on)
        at = first_min(sc)
        pair = raw.self_pair.view(Q, steps).gather(1, at[:, None])[:, 0]
        out = types.SimpleNamespace(valid=self_ok & env_ok & reach_ok, self_ok=self_ok, env_ok=env_ok, reach_ok=reach_ok,
                                    self_clear=sc.amin(dim=1), env_clear=ec.amin(dim=1), reach_clear=rc.amin(dim=1),
                                    self_pair=pair, worst_step=first_min(slack))
        if self.exact:
            out.mesh_pair = pair
            out.mesh_tri = mesh.mesh_tri.view(Q, steps, 2).gather(1, at[:, None, None].expand(Q, 1, 2))[:, 0]
        return out
