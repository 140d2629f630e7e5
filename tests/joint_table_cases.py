"""Synthetic kinematic trees for the joint-offset kernels (csrc/ehr_joint.hip, the joint branch of csrc/ehr_lm.hip): seeded
URDF-style specs that go through ``UrdfChain(spec=...)`` and ``joint_table`` like a robot's, at the table shapes the two
packaged arms never reach.  CPU only, numpy; not collected by pytest (tests/test_joint_table_cases.py pins every case, the GPU
tests are tests/test_gpu_joint_table_shapes.py).

Every axis is given NON-UNIT (|a| drawn from [0.3, 3]; ``joint_table`` normalises), in a general direction; every origin is a
general rotation and a translation within +-0.15 m; some fixed joints carry the axis ``0 0 0`` a URDF may give them.

    one            root + one revolute link                                                       N=2   J=1   L=1
    skew_serial    8 links in series, all joints revolute, every axis component >= 0.2 of |a|     N=8   J=7   L=7
    prismatic_mid  serial: revolute, prismatic, revolute, revolute, prismatic, revolute;          N=7   J=6   L=7
                   every link rendered (the root too)
    tree           branches at the root (three) and at mid-depth, active joints on four branches,  N=11  J=8   L=7
                   the root rendered, an active joint (behind a fixed one) with no rendered link
    full           a random tree, revolute and prismatic mixed, the kernels' limits               N=64  J=32  L=32
    serial64       64 links in series, revolute alternating with fixed, the last 32 rendered      N=64  J=32  L=32

``case(name)`` -> Case(name, spec, chain, use, table); ``qpos`` / ``offsets`` are the joint vectors the tests walk."""
import functools
from collections import namedtuple

import numpy as np

NAMES = ("one", "skew_serial", "prismatic_mid", "tree", "full", "serial64")
Case = namedtuple("Case", "name spec chain use table")

REV_RANGE, PRIS_RANGE = 3.5, 0.05      # revolute joints cross +-pi; prismatic joints move +-5 cm
_SEED = {n: 4100 + 17 * i for i, n in enumerate(NAMES)}


def _rotation(rng):
    """A general rotation: Rodrigues of a random direction and an angle in +-pi."""
    w = rng.normal(size=3)
    w /= np.linalg.norm(w)
    th = rng.uniform(-np.pi, np.pi)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _origin(rng):
    T = np.eye(4)
    T[:3, :3] = _rotation(rng)
    T[:3, 3] = rng.uniform(-0.15, 0.15, size=3)
    return T


def _axis(rng, least=0.0):
    """A non-unit axis: a direction whose components are all at least ``least`` in magnitude, times a length in [0.3, 3]."""
    while True:
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        if np.abs(a).min() >= least:
            return (a * rng.uniform(0.3, 3.0)).tolist()


def _joint(rng, typ, parent, child, least=0.0, zero_axis=False):
    lim = {"revolute": REV_RANGE, "prismatic": PRIS_RANGE, "fixed": 0.0}[typ]
    axis = _axis(rng, least)
    return {"name": f"{parent}_{child}", "type": typ, "parent": parent, "child": child, "origin": _origin(rng).tolist(),
            "axis": [0.0, 0.0, 0.0] if zero_axis else axis, "lower": -lim, "upper": lim}


def _serial(rng, types, least=0.0):
    links = [f"l{i}" for i in range(len(types) + 1)]
    return {"links": links, "joints": [_joint(rng, t, links[i], links[i + 1], least) for i, t in enumerate(types)]}


def _spec_one(rng):
    return _serial(rng, ["revolute"]), [1]


def _spec_skew_serial(rng):
    return _serial(rng, ["revolute"] * 7, least=0.2), list(range(1, 8))


def _spec_prismatic_mid(rng):
    return _serial(rng, ["revolute", "prismatic", "revolute", "revolute", "prismatic", "revolute"]), list(range(7))


def _spec_tree(rng):
    """                 b
              a1        c1      f1 (fixed, axis 0 0 0)
              a2        c2      e1 (revolute, not rendered: an active joint nothing rendered hangs from)
          a3 (pris.)  d1
          a4          d2 (fixed, axis 0 0 0)
    Articulation order (breadth first): b a1 c1 f1 a2 c2 e1 a3 d1 a4 d2; active joints in that order:
    a1 c1 a2 c2 e1 a3 d1 a4 = 0..7."""
    J = lambda typ, p, c, z=False: _joint(rng, typ, p, c, zero_axis=z)
    joints = [J("revolute", "b", "a1"), J("revolute", "b", "c1"), J("fixed", "b", "f1", True),
              J("revolute", "a1", "a2"), J("revolute", "c1", "c2"), J("revolute", "f1", "e1"),
              J("prismatic", "a2", "a3"), J("revolute", "a2", "d1"), J("revolute", "a3", "a4"), J("fixed", "d1", "d2", True)]
    links = ["b", "a1", "a2", "a3", "a4", "c1", "c2", "d1", "d2", "f1", "e1"]      # (document order is not articulation order)
    order = ["b", "a1", "c1", "f1", "a2", "c2", "e1", "a3", "d1", "a4", "d2"]
    use = [order.index(l) for l in ("b", "a1", "a2", "a3", "a4", "c2", "d2")]
    return {"links": links, "joints": joints}, use


def _spec_full(rng):
    """63 joints under a root: link i hangs from one of the six links before it (so the tree is deep) or, one time in four,
    from any earlier link (so it branches); 32 of the joints are active, 24 revolute and 8 prismatic, the rest fixed, every
    third fixed one with the axis 0 0 0.  Rendered: the links moved by the first and the last active joint, the first link
    that shares no active joint with the latter, and 29 more drawn at random."""
    n = 64
    kinds = np.array(["revolute"] * 24 + ["prismatic"] * 8 + ["fixed"] * 31)
    rng.shuffle(kinds)
    links = [f"l{i}" for i in range(n)]
    joints, nfixed = [], 0
    for i in range(1, n):
        p = int(rng.integers(0, i)) if rng.uniform() < 0.25 else int(rng.integers(max(0, i - 6), i))
        zero = kinds[i - 1] == "fixed" and nfixed % 3 == 0
        nfixed += kinds[i - 1] == "fixed"
        joints.append(_joint(rng, str(kinds[i - 1]), links[p], links[i], zero_axis=bool(zero)))
    spec = {"links": links, "joints": joints}
    from easyhec_amd.kinematics import UrdfChain
    every = UrdfChain(spec=spec).joint_table(range(n))
    up, qidx = every["upstream"].astype(np.uint64), every["qidx"]
    first, last = int(np.flatnonzero(qidx == 0)[0]), int(np.flatnonzero(qidx == 31)[0])
    apart = int(np.flatnonzero(((up & up[last]) == 0) & (up != 0))[0])           # (not a link with an empty mask)
    must = [first, last, apart]
    rest = [i for i in rng.permutation(n).tolist() if i not in must]
    return spec, sorted(must + rest[:32 - len(must)])


def _spec_serial64(rng):
    return _serial(rng, ["revolute", "fixed"] * 31 + ["revolute"]), list(range(32, 64))


@functools.lru_cache(maxsize=None)
def case(name):
    from easyhec_amd.kinematics import UrdfChain
    spec, use = globals()["_spec_" + name](np.random.default_rng(_SEED[name]))
    chain = UrdfChain(spec=spec)
    return Case(name, spec, chain, list(use), chain.joint_table(use))


def kinds(name):
    """[J] kind of every active joint (1 revolute, 2 prismatic), from the SPEC (not from the table)."""
    return np.array([1 if j["type"] == "revolute" else 2 for j in case(name).chain.active], dtype=np.int32)


def qpos(name, B, seed=0):
    """[B,J] float64 joint vectors: revolute U(-3.5, 3.5), prismatic U(-0.05, 0.05)."""
    k = kinds(name)
    rng = np.random.default_rng(_SEED[name] + 1000 + 31 * B + seed)
    return np.where(k == 2, rng.uniform(-PRIS_RANGE, PRIS_RANGE, (B, k.size)), rng.uniform(-REV_RANGE, REV_RANGE, (B, k.size)))


def offsets(name, seed=0):
    """[J] float32 zero offsets, as tests/test_gpu_joint_offsets.py draws them: revolute +-0.1 rad, prismatic +-5 mm."""
    k = kinds(name)
    rng = np.random.default_rng(_SEED[name] + 2000 + seed)
    return np.where(k == 2, rng.uniform(-0.005, 0.005, k.size), rng.uniform(-0.1, 0.1, k.size)).astype(np.float32)


def ancestors(name):
    """{link name: [active-joint column, ...] between the root and the link}, walked on the SPEC's names."""
    c = case(name)
    col = {j["name"]: i for i, j in enumerate(c.chain.active)}
    of_child = {j["child"]: j for j in c.spec["joints"]}
    out = {}
    for l in c.spec["links"]:
        cols, at = [], l
        while at in of_child:
            j = of_child[at]
            if j["name"] in col:
                cols.append(col[j["name"]])
            at = j["parent"]
        out[l] = sorted(cols)
    return out


# ---- what the backward kernels are given -------------------------------------------------------------------------------------
def free_mask(name, pattern):
    """[J] int32.  "all": every joint free; "frozen": the last joint (joint 31 of the two 32-joint cases) and every joint
    j = 2 (mod 5) are not free."""
    J = case(name).chain.dof
    free = np.ones(J, np.int32)
    if pattern == "frozen":
        free[[j for j in range(J) if j % 5 == 2] + [J - 1]] = 0
    else:
        assert pattern == "all", pattern
    return free


def bwd_case(name, B, draw, pattern="all"):
    """The inputs of one backward call on case ``name``, with the keys of tests/test_gpu_joint_offsets.py's ``_bwd_case``:
    B joint vectors, offsets, a grad_mvp with a fifth of the (view, link) pairs a million times the others, one of
    pose_reference's cameras and depth-plane pairs, a random camera pose and the free mask of ``pattern``."""
    import pose_reference as R
    c = case(name)
    J, L = c.chain.dof, len(c.use)
    rng = np.random.default_rng(_SEED[name] + 3000 + 100 * B + draw)
    g = rng.normal(size=(B, L, 4, 4))
    g *= np.where(rng.uniform(size=(B, L, 1, 1)) < 0.2, 1e6, 1.0)
    K, H, W = R.CAMERAS[draw % 2]
    near, far = R.NEAR_FAR[(draw + B) % 2]
    return dict(t=c.table, J=J, L=L, B=B, q=qpos(name, B, seed=30 + draw), off=offsets(name, seed=1 + draw), g=g.astype(np.float32),
                K=K, H=H, W=W, near=near, far=far, Tc=R.random_rigid(rng, 1)[0], free=free_mask(name, pattern))


# ---- the branched arm as a robot -----------------------------------------------------------------------------------------------
def box_mesh(sides):
    """A closed box about the origin: (vertices float32 [8,3], faces int32 [12,3]), outward winding."""
    h = np.asarray(sides, np.float64) / 2
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * h    # index = 4 x + 2 y + z
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    return v.astype(np.float32), np.array(f, np.int32)


@functools.lru_cache(maxsize=None)
def tree_robot():
    """``tree`` as an easyhec_amd.robot.Robot: one box of 12 triangles per rendered link, sides drawn from 8..15 cm."""
    from easyhec_amd.robot import Robot
    c = case("tree")
    rng = np.random.default_rng(_SEED["tree"] + 4000)
    meshes = [box_mesh(rng.uniform(0.08, 0.15, size=3)) for _ in c.use]
    return Robot("tree", meshes, c.chain, c.use, [f"box{k}" for k in range(len(c.use))])
