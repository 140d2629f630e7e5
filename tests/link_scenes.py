"""Scenes that vary what the robots' scenes never do: the NUMBER of links (1 .. 32, primes, views x links at and one above
the 512 (view, link) units a pass of the chain plans for), the number of triangles per link (0, 1, around every multiple
of 64 up to 257, more than 64 clusters), shared against unshared vertices (the eager and the lazy vertex form), and images
smaller than one 32 x 8 tile.  CPU only, numpy, not collected by pytest.  tests/test_link_scenes.py pins every case against
the oracle and the float64 block reference; tests/test_gpu_link_scenes.py runs the kernels on them."""
import math
import types

import numpy as np

import fused_loss_reference as R
import helpers


def patch(n, rng, unshared=False):
    """A link of exactly ``n`` triangles: the first n faces of a jittered k x k grid over [-0.5, 0.5]^2, k = ceil(sqrt(n / 2)),
    without the vertices they leave unused, bent out of plane (z = 0.1 (x^2 - y^2)).  unshared: every triangle gets its own
    three vertices (V = 3 T)."""
    if n == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    k = int(math.ceil(math.sqrt(n / 2.0)))
    pos, tri = helpers.grid_mesh(k, lo=-0.5, hi=0.5, jitter=0.15 / k, rng=rng)
    tri = tri[:n]
    assert tri.shape[0] == n
    used, inv = np.unique(tri.ravel(), return_inverse=True)
    v = pos[used, :3].astype(np.float64)
    f = inv.reshape(-1, 3).astype(np.int32)
    v[:, 2] = 0.1 * (v[:, 0] ** 2 - v[:, 1] ** 2)
    if unshared:
        v = v[f.ravel()]
        f = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    return v.astype(np.float32), f


def _rotation(a):
    cx, cy, cz = np.cos(a)
    sx, sy, sz = np.sin(a)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rx @ ry @ rz


def scene(counts, H, W, B, seed, cols, pitch, size, f, unshared=False, name=None):
    """Link l (a ``patch`` of counts[l] triangles scaled by ``size``) at column l % cols, row l // cols of a lattice of spacing
    ``pitch`` centred on the optical axis, at depth 1 + 0.05 l / L in front of an identity camera of focal length ``f`` pixels;
    every link turned by up to +-0.5 rad about each axis, drawn anew per view.  -> a fused_loss_reference._scene that also
    carries link_poses [B,L,4,4] and K [3,3] (float64), for the cases that start from the pose."""
    rng = np.random.default_rng(seed)
    L = len(counts)
    meshes = []
    for n in counts:
        v, fc = patch(n, rng, unshared)
        meshes.append((v * np.float32(size), fc))
    rows = (L + cols - 1) // cols
    lp = np.tile(np.eye(4)[None, None], (B, L, 1, 1))
    for b in range(B):
        for l in range(L):
            lp[b, l, :3, :3] = _rotation(rng.uniform(-0.5, 0.5, 3))
            lp[b, l, :3, 3] = [(l % cols - 0.5 * (min(cols, L) - 1)) * pitch, (l // cols - 0.5 * (rows - 1)) * pitch,
                               1.0 + 0.05 * l / L]
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    s = R._scene(name or f"links{L}_{H}x{W}x{B}", meshes, helpers.mvp_numpy(K, H, W, np.eye(4), lp), H, W)
    s.link_poses, s.K, s.counts = lp, K, list(counts)
    return s


C32 = [1, 2, 3, 0, 31, 32, 33, 63, 64, 65, 0, 127, 128, 129, 191, 192, 193, 255, 256, 257, 500, 1000, 0, 4095, 4096, 4097, 5, 7,
       11, 13, 17, 4161]
assert len(C32) == 32 and sum(C32) == 20024

SUBTILE_COUNTS = [65, 0, 3, 129, 1]
SUBTILE_SHAPES = [(1, 1), (1, 40), (3, 5), (7, 31), (8, 32), (9, 33), (5, 70), (40, 4)]
# 1 x 1: no neighbouring pixel, so no antialiased pair and no gradient: a mask-and-loss case.  (1 x 40 has horizontal pairs at
# the patches' left and right silhouettes under every seed tried, so it is held to the gradient bars like the others.)
MASK_ONLY = ("sub_1x1",)


def _link_counts(L):
    return [65, 0, 129][:L] if L <= 3 else C32[:L]


# name -> keyword arguments of scene().  Placements (cols, pitch, size, f) are chosen so that the conditions asserted in
# tests/test_link_scenes.py hold: links overlap their neighbours (three links on one pixel) and almost every link with a
# triangle has a silhouette pixel in every view.
CASES = {
    "full32": dict(counts=C32, H=72, W=104, B=2, seed=1, cols=8, pitch=0.22, size=0.25, f=55.0),
    "full32_lazy": dict(counts=C32, H=72, W=104, B=2, seed=1, cols=8, pitch=0.22, size=0.25, f=55.0, unshared=True),
    "units512": dict(counts=C32, H=128, W=160, B=16, seed=2, cols=8, pitch=0.2, size=0.26, f=100.0),
    "units513": dict(counts=C32, H=128, W=160, B=17, seed=3, cols=8, pitch=0.2, size=0.26, f=100.0),
    "prime7": dict(counts=C32[4:11], H=64, W=96, B=74, seed=4, cols=4, pitch=0.22, size=0.3, f=60.0),
    "first_empty": dict(counts=[0, 65, 3], H=40, W=56, B=2, seed=5, cols=3, pitch=0.2, size=0.3, f=45.0),
    "last_empty": dict(counts=[65, 3, 0], H=40, W=56, B=2, seed=6, cols=3, pitch=0.2, size=0.3, f=45.0),
    "only_one_live": dict(counts=[0, 0, 1, 0], H=40, W=56, B=2, seed=7, cols=4, pitch=0.2, size=0.3, f=45.0),
    "L13x5": dict(counts=C32[:13], H=64, W=96, B=5, seed=8, cols=5, pitch=0.22, size=0.3, f=60.0),   # U = 65
}
for _L in (2, 3, 5, 13, 17, 31):
    CASES[f"L{_L}"] = dict(counts=_link_counts(_L), H=64, W=96, B=3, seed=10 + _L, cols=min(_L, 7), pitch=0.22, size=0.3,
                           f=60.0 if _L <= 17 else 48.0)
for _H, _W in SUBTILE_SHAPES:
    CASES[f"sub_{_H}x{_W}"] = dict(counts=SUBTILE_COUNTS, H=_H, W=_W, B=2, seed=100 + _H, cols=5, pitch=0.12, size=0.5,
                                   f=0.9 * max(_H, _W))

SUBTILE = [k for k in CASES if k.startswith("sub_")]
# (case, kind of reference mask): one seeded soft reference per case; full32 also with a binary and an out-of-range one
RUNS = [(k, "uniform") for k in CASES] + [("full32", "binary"), ("full32", "wide")]
RUN_IDS = [f"{k}-{kind}" for k, kind in RUNS]

_CACHE = {}


def scene_of(case):
    if case not in _CACHE:
        _CACHE[case] = scene(name=case, **CASES[case])
    return _CACHE[case]


def expected_of(oracle, case, kind="uniform"):
    """``fused_loss_reference.expected()`` of (case, reference kind), computed once per process and never written to."""
    k = (case, kind)
    if k not in _CACHE:
        s = scene_of(case)
        _CACHE[k] = R.expected(oracle, s, R.reference_mask(oracle, s, kind))
    return _CACHE[k]


def empty_links(s):
    return np.array([f.shape[0] == 0 for _, f in s.meshes])


def n_tiles(s):
    return ((s.W + 31) // 32) * ((s.H + 7) // 8)
