"""ehr_mask_information on the scenes of tests/link_scenes.py and on the flagged stack of tests/depth_plane_scenes.py: the
tangents, the cases and the float64 expectations (tests/information_reference.py) that tests/test_gpu_information_scenes.py
and tests/test_gpu_lm_tangent_shapes.py hold the kernels against.  CPU only, numpy, not collected by pytest;
tests/test_info_scene_cases.py pins the conditions the GPU cases rely on.

vb_info_kernel (csrc/ehr_vbuf.hip) re-reads the job slots behind the composite launch and indexes them on its own: a binary
search over jbase, the ballot for the first link that owns a tile, one lane per link in tmask / bmask, b0 / B_all into dmvp,
(view0 + b) % nviews into the weights, and a dynamic-LDS layout whose waves per workgroup follow from N and the number of
(view, link) units U.  The robots' scenes show it 8 links and U <= 24; these cases show it 1 .. 32 links, empty links first,
last and in between, U = 512 in one chunk and 513 in two, 74 views in chunks of 73 + 1, images smaller than a tile, and a
tile that a second call hands to a whole workgroup.

Tangents: the six generators of information_reference.se3_generators() on clip space, G_k @ mvp (the scenes' camera is the
identity: this is the tie scene's recipe), cut to N or filled up to N with seeded normal matrices of the same per-(view, link)
amplitude -- information_reference.tangents_for's recipe.  The translation along z moves only the z row, which the kernel
must ignore: its row and column of info and its entry of grad have no scale and must be exactly zero (25 of 36 entries have
one at N = 6).

No bar is introduced here: every comparison is information_reference.check (2 C_J(L) u S, (C_J(L) + 1) u Sg, exact count),
bit equality or exact zero.
"""
import types

import numpy as np

import depth_plane_scenes as DP
import fused_loss_reference as R
import information_reference as IR
import link_scenes as S

LINK_CASES = ["full32", "full32_lazy", "units512", "units513", "prime7", "first_empty", "last_empty", "only_one_live", "L13x5",
              "L2", "L3", "L5", "L17", "L31"] + S.SUBTILE
STACK_CASES = ["stack_base", "stack_heavy"]
CASES = LINK_CASES + STACK_CASES
# Left out: depth_plane_scenes.robot_cut_by_far at 100 x 150 -- the reference counts 0 and 4 pixels there: nothing to see.

ALL_ZERO = ("sub_1x1",)               # no neighbouring pixel: no blended pair, so info, grad and count are all zero
MANY_N = ("full32", "units513", "prime7")                              # the cases that also run N = 1 and N = 32
# N at which vb_info_launch drops from 4 to 2 to 1 waves per workgroup: the largest nw of 4, 2, 1 with
# (2 U + 1) * 4 + nw * 1024 (N + 3) <= 65536 bytes of dynamic LDS
THRESHOLDS = {"full32": [12, 13, 28, 29], "units512": [11, 12, 26, 27, 28]}

# The reference's count per view at N = 6 on a uniform reference mask (tests/test_info_scene_cases.py asserts them)
COUNTS = {"full32": [468, 440], "only_one_live": [37, 41], "sub_1x40": [2, 1], "sub_9x33": [11, 19], "stack_base": [139, 135],
          "stack_heavy": [145, 113]}
COUNT_RANGES = {"units512": (574, 706), "units513": (585, 708), "prime7": (137, 173)}     # (smallest, largest) over the views
# (view, link) units with a triangle but no probed pixel, of the units with a triangle
UNPROBED = {"full32": (1, 58), "units513": (0, 493), "prime7": (0, 444)}


def waves_per_workgroup(N, U):
    """vb_info_launch's choice, restated: what THRESHOLDS is derived from."""
    nw = 4
    while nw > 1 and (2 * U + 1) * 4 + nw * 1024 * (N + 3) > 65536:
        nw >>= 1
    return nw


# Worst (|info - info_ref| / (2^-24 S), |grad - grad_ref| / (2^-24 Sg)) over the entries of each case, MI355X, 2026-10-20,
# printed by the cases themselves under
#     pytest -m gpu tests/test_gpu_information_scenes.py tests/test_gpu_lm_tangent_shapes.py -s
# (bars: 2 C_J(L) and C_J(L) + 1 with C_J(L) = 31 + 4 L: 318 and 160 at 32 links, 78 and 40 at two).  The kernel stays within
# three units where the derivation allows 78 to 318: the largest figures belong to the images smaller than a tile, whose two to
# twenty counted pixels leave S little to average over.  The wave-count cases repeat their scene's N = 6 figures because the
# six generators carry the worst entries.  A figure above the bar is a finding to explain by recomputing that pixel from the
# oracle's pairs, not a reason to widen the bar.
MEASURED = {
    "parity full32 N=6": (0.346, 0.105),
    "parity full32_lazy N=6": (0.170, 0.093),
    "parity units512 N=6": (0.466, 0.129),
    "parity units513 N=6": (0.417, 0.138),
    "parity prime7 N=6": (0.819, 0.316),
    "parity first_empty N=6": (0.892, 0.266),
    "parity last_empty N=6": (0.915, 0.383),
    "parity only_one_live N=6": (1.253, 0.337),
    "parity L13x5 N=6": (0.495, 0.195),
    "parity L2 N=6": (0.991, 0.302),
    "parity L3 N=6": (0.513, 0.203),
    "parity L5 N=6": (0.455, 0.178),
    "parity L17 N=6": (0.395, 0.132),
    "parity L31 N=6": (0.297, 0.194),
    "parity sub_1x1 N=6": (0.0, 0.0),
    "parity sub_1x40 N=6": (2.166, 1.172),
    "parity sub_3x5 N=6": (2.011, 1.220),
    "parity sub_7x31 N=6": (1.082, 0.696),
    "parity sub_8x32 N=6": (1.427, 0.535),
    "parity sub_9x33 N=6": (1.166, 0.660),
    "parity sub_5x70 N=6": (2.596, 0.392),
    "parity sub_40x4 N=6": (0.902, 0.607),
    "parity stack_base N=6": (0.371, 0.136),
    "parity stack_heavy N=6": (0.424, 0.095),
    "parity full32 N=1": (0.188, 0.046),
    "parity full32 N=32": (0.346, 0.135),
    "parity units513 N=1": (0.374, 0.109),
    "parity units513 N=32": (0.417, 0.138),
    "parity prime7 N=1": (0.819, 0.313),
    "parity prime7 N=32": (0.836, 0.316),
    "waves full32 N=12 (4 per workgroup)": (0.346, 0.105),
    "waves full32 N=13 (2 per workgroup)": (0.346, 0.105),
    "waves full32 N=28 (2 per workgroup)": (0.346, 0.111),
    "waves full32 N=29 (1 per workgroup)": (0.346, 0.111),
    "waves units512 N=11 (4 per workgroup)": (0.466, 0.129),
    "waves units512 N=12 (2 per workgroup)": (0.466, 0.129),
    "waves units512 N=26 (2 per workgroup)": (0.466, 0.129),
    "waves units512 N=27 (1 per workgroup)": (0.466, 0.129),
    "waves units512 N=28 (1 per workgroup)": (0.466, 0.129),
    "weights real units513": (0.379, 0.186),
    "weights shared units513": (0.461, 0.120),
    "weights real prime7": (0.896, 0.451),
    "weights shared prime7": (0.813, 0.385),
    "weights pair prime7": (0.916, 0.348),
    "linearize -> information full32 identity": (0.165, 0.074),
    "linearize -> information full32 w0.3": (0.149, 0.067),
}
# ehr_lm_linearize, the same run: worst |dmvp - ref| / bar (lm_reference.tangent_ratio, bar 1).  A pose or intrinsics tangent is
# one float32 rounding of a float64 value, so its figure is the worst rounding met, just under 1; the joints' bar allows three.
MEASURED_TANGENTS = {
    "full32 identity": 0.967, "full32 w1e-3": 0.992, "full32 below_clamp": 0.985, "full32 above_clamp": 0.963, "full32 w0.3": 0.961,
    "units513 identity": 0.986, "units513 w1e-3": 0.991, "units513 below_clamp": 0.995, "units513 above_clamp": 0.991,
    "units513 w0.3": 0.992,
    "xarm7 every link, joints": 0.575, "xarm7 every link, prismatic blocks": 0.270,
    "franka every link, joints": 0.578, "franka every link, prismatic blocks": 0.195,
    "L5 intrinsics, worst of the eight masks": 0.941,
}

_CACHE = {}


def scene_of(case):
    if case.startswith("stack_"):
        if case not in _CACHE:
            _CACHE[case] = R._scene(case, *DP.flagged_stack(case[6:]))
        return _CACHE[case]
    return S.scene_of(case)


def expected0(oracle, case):
    """``fused_loss_reference.expected()`` of the case on its uniform reference mask (link scenes: link_scenes.expected_of's,
    shared with tests/test_gpu_link_scenes.py); once per process, never written to."""
    if not case.startswith("stack_"):
        return S.expected_of(oracle, case)
    k = (case, "expected")
    if k not in _CACHE:
        s = scene_of(case)
        _CACHE[k] = R.expected(oracle, s, R.reference_mask(oracle, s, "uniform"))
    return _CACHE[k]


def empty_links(s):
    return np.array([f.shape[0] == 0 for _, f in s.meshes])


def tangents(s, N, seed=0):
    """[N,B,L,4,4] float32 for scene ``s``: G_k @ mvp for the six generators, cut to N or filled up to N with seeded normal
    matrices of the generators' size per (view, link), z row included (the kernel must ignore it)."""
    D = np.stack([G @ s.mvp.astype(np.float64) for G in IR.se3_generators()]).astype(np.float32)
    if N <= 6:
        return np.ascontiguousarray(D[:N])
    rng = np.random.default_rng(100 * N + seed)
    amp = np.abs(D).max(axis=(0, 3, 4))                                          # [B,L]
    extra = rng.normal(size=(N - 6,) + D.shape[1:]) * amp[None, :, :, None, None]
    return np.ascontiguousarray(np.concatenate([D, extra.astype(np.float32)]))


def rendered(oracle, case):
    """information_reference.rendered of the case: shared by every N, weight and tangent set of the process."""
    k = (case, "rendered")
    if k not in _CACHE:
        s = scene_of(case)
        _CACHE[k] = IR.rendered(oracle, s.meshes, s.mvp, s.H, s.W)
    return _CACHE[k]


def reference(oracle, case, D, w=None):
    """information_reference of the case for the tangents ``D`` (any array [N,B,L,4,4]) and weights ``w``; not cached."""
    e0 = expected0(oracle, case)
    return IR.information_reference(oracle, e0.s.meshes, e0.s.mvp, D, e0.ref, w, rd=rendered(oracle, case))


def weight_of(case, kind):
    """None | "real": [B,H,W] uniform in [0, 2] | "shared": [1,H,W] | "pair": [2,H,W] (B even) | "ones" | "zeros"."""
    import weighted_loss_reference as WR
    s = scene_of(case)
    if kind is None:
        return None
    if kind in ("ones", "zeros"):
        return np.full((s.B, s.H, s.W), 1.0 if kind == "ones" else 0.0, np.float32)
    Bv = {"real": s.B, "shared": 1, "pair": 2}[kind]
    assert s.B % Bv == 0
    return WR.real_weight((Bv, s.H, s.W), seed=Bv)


def expected(oracle, case, N, weight=None):
    """(D, w, information_reference) of (case, N tangents of ``tangents``, weight kind); once per process, never written to."""
    k = (case, N, weight)
    if k not in _CACHE:
        D, w = tangents(scene_of(case), N), weight_of(case, weight)
        _CACHE[k] = (D, w, reference(oracle, case, D, w))
    return _CACHE[k]


def nested(oracle, case, Ns):
    """One set of max(Ns) tangents and, for every n of Ns, the reference of its first n: the calls of the wave-count cases,
    whose n x n blocks must also agree bit for bit.  -> (D, {n: reference}); once per process."""
    k = (case, "nested", tuple(Ns))
    if k not in _CACHE:
        D = tangents(scene_of(case), max(Ns))
        _CACHE[k] = (D, {n: reference(oracle, case, D[:n]) for n in Ns})
    return _CACHE[k]


# ---- the camera poses of tests/test_gpu_lm_tangent_shapes.py -----------------------------------------------------------------
LM_AXIS = np.array([0.2, -0.1, 0.97]) / np.linalg.norm([0.2, -0.1, 0.97])   # mostly about the optical axis: the links stay in frame
LM_TRANSLATION = np.array([0.02, -0.01, 0.03], np.float32)
LM_DOFS = ("identity", "w1e-3", "below_clamp", "above_clamp", "w0.3")


def squared_angle(dof):
    """|w|^2 in float64 of the float32 rotation part: what se3_exp_f64 (csrc/ehr_lm.hip) and the reference compare with 1e-4."""
    w = np.asarray(dof, np.float32)[-3:].astype(np.float64)
    return float(w @ w)


def clamp_neighbours():
    """(w_below, w_above) float32 [3]: rotation vectors one float32 step of one component apart whose squared angle lies
    below, and at or above, the exponential map's clamp."""
    w = (LM_AXIS * 0.01 * (1.0 - 1e-6)).astype(np.float32)
    assert squared_angle(w) < 1e-4
    for _ in range(100000):
        up = w.copy()
        up[2] = np.nextafter(up[2], np.float32(1.0))
        if squared_angle(up) >= 1e-4:
            return w, up
        w = up
    raise AssertionError("the clamp was not reached")


def lm_dofs():
    """name -> dof [6] float32: the scenes' identity camera, and four rotations with a translation: well under the clamp
    (|w| = 1e-3), one float32 step below and above |w|^2 = 1e-4, and 0.3 rad."""
    lo, hi = clamp_neighbours()
    out = {"identity": np.zeros(6, np.float32)}
    for name, w in (("w1e-3", (LM_AXIS * 1e-3).astype(np.float32)), ("below_clamp", lo), ("above_clamp", hi),
                    ("w0.3", (LM_AXIS * 0.3).astype(np.float32))):
        out[name] = np.concatenate([LM_TRANSLATION, w]).astype(np.float32)
    assert tuple(out) == LM_DOFS
    return out


def unprobed_units(s, rd):
    """(units with a triangle but no probed pixel, units with a triangle) over the (view, link) units of the scene."""
    live = ~empty_links(s)
    return int((rd.nprobe[:, live] == 0).sum()), int(live.sum()) * s.B


def summary(e):
    return types.SimpleNamespace(count=e.count.tolist(), share=float((e.S > 0).mean()), nprobe=int(e.nprobe.sum()))
