"""The mesh clearance kernel (csrc/ehr_mesh_clearance.hip) and ``FeasibilityFilter(exact=True)`` on the GPU, against the numpy
restatement of tests/mesh_clearance_reference.py: both clearances bit for bit, the reported witnesses evaluated by the reference,
over triangle counts 0..130 per link, leaves of 4 and 64 triangles, 1..70 configurations, planes, obstacles, masks, degenerate and
piercing triangles, a NaN pose, culling and the refusals; proxies and meshes disagreeing in both directions; the packaged xArm7
on sampled configurations.  tests/test_mesh_clearance_reference.py pins the reference on the CPU.  Every figure is printed
before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import feasibility_reference as FR
import mesh_clearance_reference as MR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, feasibility
    assert _lib.has_mesh_clearance()
    return feasibility


def dev64(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run(F, case, link_poses=None, cutoff=None):
    lp = case["link_poses"] if link_poses is None else link_poses
    out = F.mesh_clearance(torch.tensor(lp, device=DEV), dev64(case["spheres"]), case["offsets"], dev64(case["bounds"]),
                           torch.tensor(case["pair_enable"].view(np.int32), device=DEV), dev64(case["triangles"].reshape(-1, 9)),
                           torch.tensor(case["tri_offsets"], device=DEV), dev64(case["planes"]), dev64(case["obstacles"]),
                           case["env_links"], case["cutoff"] if cutoff is None else cutoff)
    return host(out.mesh_clear), host(out.mesh_pair), host(out.mesh_tri), host(out.env_clear)


def same_bits(g, r):
    return (bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r))


def assert_same(what, got, ref, case, link_poses=None):
    """The clearances bit for bit (NaN against NaN); the witnesses -1 exactly where the reference's are, a pair that is enabled
    and triangles of its two links, and their distance, evaluated by the reference, equal to mesh_clear."""
    lp = case["link_poses"] if link_poses is None else link_poses
    bad = []
    for name, g, r in (("mesh_clear", got[0], ref[0]), ("env_clear", got[3], ref[3])):
        same = same_bits(g, r)
        print(f"[mesh clearance] {what}: {name} differs in {int((~same).sum())} of {same.size}"
              + ("" if same.all() else f" (first: got {g[~same][0]!r}, reference {r[~same][0]!r})"))
        bad += [] if same.all() else [name]
    none = ref[1] < 0
    if not ((got[1] < 0) == none).all() or not ((got[2] < 0).all(axis=1) == none).all():
        bad.append("witnesses present")
    else:
        L = len(case["offsets"]) - 1
        first = np.asarray(case["tri_offsets"])[np.asarray(case["offsets"])]     # the links' first triangles
        for b in np.nonzero(~none)[0]:
            i, j = divmod(int(got[1][b]), 32)
            ta, tb = (int(t) for t in got[2][b])
            ok = 0 <= i < j < L and (int(case["pair_enable"][i]) >> j) & 1 and first[i] <= ta < first[i + 1] and \
                first[j] <= tb < first[j + 1]
            d = MR.witness_distance(lp[b], case["triangles"], case["tri_offsets"], case["offsets"], ta, tb) if ok else None
            if not ok or d != got[0][b]:
                print(f"[mesh clearance] {what}: configuration {b}: witness pair ({i}, {j}) triangles ({ta}, {tb}) at {d!r}, "
                      f"mesh_clear {got[0][b]!r}")
                bad.append(f"witness {b}")
    assert not bad, (what, bad)


# triangles per link, n, leaf size, planes, obstacles, pairs
CASES = {
    "[1,1]": dict(counts=[1, 1], n=3, spread=0.2, cutoff=1.0),
    "[5,3]-leaf4": dict(counts=[5, 3], n=3, leaf_triangles=4, n_planes=1, n_obstacles=2, spread=0.2, cutoff=0.25),
    "ragged": dict(counts=[0, 1, 63, 64, 65, 130, 1], n=3, leaf_triangles=64, n_planes=6, n_obstacles=40, pairs="random"),
    "n70": dict(counts=[20, 9], n=70, leaf_triangles=8, n_planes=1, n_obstacles=1, spread=0.3),
    "n1": dict(counts=[12, 7, 5], n=1, leaf_triangles=4, spread=0.2),
}
_BUILT = {}


def degenerate(case):
    """Some triangles of a built case made degenerate IN PLACE of their leaves (the corners stay inside the leaf's sphere): a
    repeated corner, three corners on a line, a point."""
    t = case["triangles"].reshape(-1, 3, 3)
    t[0, 2] = t[0, 1]
    t[1, 2] = t[1, 0] + 0.5 * (t[1, 1] - t[1, 0])
    t[2, 1] = t[2, 2] = t[2, 0]
    t[-1, 0] = t[-1, 2]
    t[-2, 1] = t[-2, 0] + 0.25 * (t[-2, 2] - t[-2, 0])
    return case


def built(name):
    """A case and its reference, computed once and shared (never written to)."""
    if name not in _BUILT:
        if name == "degenerate":
            case = degenerate(MR.make_case(7, counts=[5, 3], n=6, leaf_triangles=4, n_planes=1, n_obstacles=4, spread=0.15, cutoff=0.5))
        else:
            case = MR.make_case(list(CASES).index(name) + 21, **CASES[name])
        _BUILT[name] = (case, MR.reference_of(case))
    return _BUILT[name]


@pytest.mark.parametrize("name", list(CASES) + ["degenerate"])
def test_kernel_against_the_reference(F, name):
    case, ref = built(name)
    mc, mp, mt, ec = ref
    cut = case["cutoff"]
    print(f"[mesh clearance] {name}: T = {case['triangles'].shape[0]}, S = {int(case['offsets'][-1])}, reference mesh_clear "
          f"{mc.min():.5f}..{mc.max():.5f} ({int((mc == 0).sum())} at 0, {int((mc < cut).sum())} of {mc.size} below cutoff), env "
          f"{ec.min():.5f}..{ec.max():.5f}")
    got = run(F, case)
    assert_same(name, got, ref, case)
    again = run(F, case)                                                              # two runs: the same bits
    assert same_bits(again[0], got[0]).all() and same_bits(again[3], got[3]).all()
    assert_same(name + " again", again, ref, case)


def test_a_piercing_pair(F):
    """One triangle each: an edge through the middle of a large triangle.  All 15 feature distances exceed 0.1, only the
    piercing test finds the intersection."""
    A = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    B = np.array([[0.0, 0.0, -0.5], [0.0, 0.0, 0.5], [0.25, 0.0, 0.5]])
    assert MR.feature_distances2(A, B).min() > 0.1 ** 2
    case = MR.proxies_of([(A, np.arange(3)[None]), (B, np.arange(3)[None])], 64)
    lp = np.zeros((2, 2, 4, 4), dtype=np.float32)
    lp[:, :, range(4), range(4)] = 1.0
    lp[1, 1, 2, 3] = 1.0                                                              # ... and lifted clear of it: 0.5
    case.update(link_poses=lp, pair_enable=np.array([2, 0], dtype=np.uint32), planes=None, obstacles=None, env_links=0, cutoff=2.0)
    ref = MR.reference_of(case)
    assert ref[0].tolist() == [0.0, 0.5] and ref[1].tolist() == [1, 1]
    got = run(F, case)
    assert_same("piercing", got, ref, case)
    assert got[0][0] == 0.0 and got[2][0].tolist() == [0, 1]
    assert MR.witness_distance(lp[0], case["triangles"], case["tri_offsets"], case["offsets"], *got[2][0]) == 0.0


def test_a_nan_pose_leaves_its_neighbours_alone(F):
    case, ref = built("ragged")
    lp = case["link_poses"].copy()
    lp[1, 4, 1, 2] = np.nan
    got = run(F, case, lp)
    assert np.isnan([got[0][1], got[3][1]]).all() and got[1][1] == -1 and got[2][1].tolist() == [-1, -1]
    for k in (0, 2):                                                                  # the neighbours: what they were
        assert bits(got[0])[k] == bits(ref[0])[k] and bits(got[3])[k] == bits(ref[3])[k]
    lp[1, 4, 1, 2], lp[1, 6, 3, 0] = case["link_poses"][1, 4, 1, 2], np.inf           # ... and an infinite entry, in the last row
    got = run(F, case, lp)
    assert np.isnan([got[0][1], got[3][1]]).all() and got[1][1] == -1


@pytest.mark.parametrize("name", ["ragged", "n70"])
def test_culling_changes_nothing(F, name):
    """The same problem with a cutoff so large that no sphere culls anything, and with a short one: below the short cutoff
    the same bits, above it the cutoff."""
    case, _ = built(name)
    wide = run(F, case, cutoff=10.0)
    assert_same(name + " unculled", wide, MR.reference_of(case, cutoff=10.0), case)
    for short in (0.02, case["cutoff"]):
        got = run(F, case, cutoff=short)
        below = wide[0] < short
        print(f"[mesh clearance] culling {name} at {short}: {int(below.sum())} of {below.size} below the short cutoff")
        assert (bits(got[0]) == bits(np.where(below, wide[0], short))).all()
        assert (bits(got[3]) == bits(np.where(wide[3] < short, wide[3], short))).all()
        assert ((got[1] >= 0) == below).all()
        assert_same(f"{name} at {short}", got, (np.where(below, wide[0], short), np.where(below, wide[1], -1), None,
                                                np.where(wide[3] < short, wide[3], short)), case)


def test_sizes_outside_the_limits_are_refused(F):
    from easyhec_amd import _lib
    case, _ = built("[1,1]")
    sph, bnd, tri = dev64(case["spheres"]), dev64(np.zeros((33, 4))), dev64(case["triangles"].reshape(-1, 9))
    pe = lambda L: torch.zeros((L,), dtype=torch.int32, device=DEV)
    lp = lambda n, L: torch.zeros((n, L, 4, 4), device=DEV)
    to = lambda k: torch.zeros((k,), dtype=torch.int32, device=DEV)
    big = dev64(np.zeros((4097, 4)))
    call = lambda *a, **k: (lambda: F.mesh_clearance(*a, **k))
    for match, fn in (
            ("1 <= L <= 32", call(lp(1, 33), sph, np.zeros(34, dtype=np.int32), bnd, pe(33), tri, to(3))),
            ("n 0 >= 1", call(lp(0, 2), sph, case["offsets"], bnd, pe(2), tri, to(3))),
            ("S 4097 <= 4096", call(lp(1, 1), big, np.array([0, 4097], dtype=np.int32), bnd, pe(1), tri, to(4098))),
            ("ascend from 0", call(lp(1, 2), sph, np.array([0, 2, 1], dtype=np.int32), bnd, pe(2), tri, to(3))),
            ("planes <= 16", call(lp(1, 2), sph, case["offsets"], bnd, pe(2), tri, to(3), planes=dev64(np.zeros((17, 4))))),
            ("obstacles <= 1024", call(lp(1, 2), sph, case["offsets"], bnd, pe(2), tri, to(3), obstacles=dev64(np.zeros((1025, 4))))),
            ("finite and > 0", call(lp(1, 2), sph, case["offsets"], bnd, pe(2), tri, to(3), cutoff=0.0)),
            ("finite and > 0", call(lp(1, 2), sph, case["offsets"], bnd, pe(2), tri, to(3), cutoff=float("nan"))),
            ("T 1048577 <= 1048576", call(lp(1, 2), sph, case["offsets"], bnd, pe(2),
                                          torch.zeros((_lib.MESH_MAX_TRIANGLES + 1, 9), dtype=torch.float64, device=DEV), to(3))),
            ("CUDA/HIP tensor", call(torch.zeros((1, 2, 4, 4)), sph, case["offsets"], bnd, pe(2), tri, to(3)))):
        with pytest.raises(RuntimeError, match=match):
            fn()
    # a NULL tensor, which the wrapper cannot produce: the entry point itself
    p, out = _lib.ptr, torch.zeros((8,), dtype=torch.float64, device=DEV)
    off = np.ascontiguousarray(case["offsets"], dtype=np.int32)
    rc = _lib.lib().ehr_mesh_clearance(p(lp(1, 2)), p(sph), off.ctypes.data_as(ctypes.c_void_p), p(bnd), p(pe(2)), None, 0, None, 0,
                                       0, 0.1, 1, 2, p(tri), None, 2, p(out), p(out), p(out), p(out), None)
    assert rc != 0 and b"NULL tensor" in _lib.lib().ehr_last_error()
    # tri_offsets that do not ascend or leave 0..T (device memory nobody reads back) are clamped: the launch stays in bounds
    case2 = dict(case, tri_offsets=np.array([5, -3, 9], dtype=np.int32))
    got = run(F, case2)
    assert np.isfinite(got[0]).all()
    # the limits themselves pass: 16 planes and 1024 obstacles
    c = MR.make_case(3, [5, 4], 2, leaf_triangles=4, n_planes=16, n_obstacles=1024)
    assert_same("at the limits", run(F, c), MR.reference_of(c), c)


# ---- proxies and meshes disagree, in both directions ------------------------------------------------------------------------
def plate(z):
    """A thin 0.4 m square plate of 8 triangles at height z (link frame)."""
    xs = np.linspace(-0.2, 0.2, 3)
    v = np.array([[x, y, z] for x in xs for y in xs])
    f = [[3 * i + j, 3 * i + j + 1, 3 * (i + 1) + j] for i in range(2) for j in range(2)] + \
        [[3 * i + j + 1, 3 * (i + 1) + j + 1, 3 * (i + 1) + j] for i in range(2) for j in range(2)]
    return v, np.array(f)


def verdicts(F, case, proxy_pairs, mesh_pairs, margin):
    from easyhec_amd.feasibility import pair_words
    L = len(case["offsets"]) - 1
    lp = torch.tensor(case["link_poses"], device=DEV)
    args = (lp, dev64(case["spheres"]), case["offsets"], dev64(case["bounds"]))
    prox = F.config_clearance(*args, torch.tensor(pair_words(proxy_pairs, L).view(np.int32), device=DEV), cutoff=0.25)
    mesh = F.mesh_clearance(*args, torch.tensor(pair_words(mesh_pairs, L).view(np.int32), device=DEV),
                            dev64(case["triangles"]), torch.tensor(case["tri_offsets"], device=DEV), cutoff=0.05)
    return host(prox.self_clear), host(mesh.mesh_clear), host(prox.self_clear) > margin, host(mesh.mesh_clear) > margin


def test_the_proxies_reject_and_the_meshes_accept(F):
    """Two thin plates 3 cm apart: their leaf spheres (0.1 m and more across) overlap, the meshes keep 3 cm."""
    case = MR.proxies_of([plate(0.0), plate(0.03)], 2)
    lp = np.zeros((1, 2, 4, 4), dtype=np.float32)
    lp[:, :, range(4), range(4)] = 1.0
    case.update(link_poses=lp, pair_enable=np.array([2, 0], dtype=np.uint32), planes=None, obstacles=None, env_links=0, cutoff=0.05)
    ref = MR.reference_of(case)
    proxy_ref = FR.clearance(lp, case["spheres"], case["offsets"], case["pair_enable"])[0]
    print(f"[mesh clearance] plates: reference proxies {proxy_ref.tolist()}, meshes {ref[0].tolist()}")
    assert proxy_ref[0] < 0 and ref[0][0] == 0.03                                     # (on the reference alone)
    sc, mc, proxy_ok, exact_ok = verdicts(F, case, [(0, 1)], [(0, 1)], 0.01)
    assert bits(sc)[0] == bits(proxy_ref)[0] and bits(mc)[0] == bits(ref[0])[0]
    assert not proxy_ok[0] and exact_ok[0]


def test_the_proxies_accept_and_the_meshes_reject(F):
    """A pair the proxy list leaves out (as a "settle" pair is) and the mesh list carries: the plates cross."""
    case = MR.proxies_of([plate(0.0), plate(0.0)], 2)
    lp = np.zeros((1, 2, 4, 4), dtype=np.float32)
    lp[:, :, range(4), range(4)] = 1.0
    lp[0, 1, :3, :3] = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])  # the second plate on edge, through the first
    case.update(link_poses=lp, pair_enable=np.array([2, 0], dtype=np.uint32), planes=None, obstacles=None, env_links=0, cutoff=0.05)
    ref = MR.reference_of(case)
    assert ref[0][0] == 0.0                                                            # (on the reference alone)
    sc, mc, proxy_ok, exact_ok = verdicts(F, case, [], [(0, 1)], 0.01)
    assert sc[0] == 0.25 and proxy_ok[0] and mc[0] == 0.0 and not exact_ok[0]


# ---- the packaged arm -------------------------------------------------------------------------------------------------------
_ARM = {}


def arm(F, xarm7):
    """The exact filter, 32 sampled configurations, their device kinematics and the culled reference with the least squared
    distance of every enabled pair: built once, shared, never written to."""
    if not _ARM:
        from easyhec_amd.feasibility import pair_words
        flt = F.FeasibilityFilter(xarm7, leaf_triangles=64, margin=0.01, planes=[[0.0, 0.0, 1.0, 0.0]], exact=True)
        q = xarm7.sample_qpos(32, np.random.default_rng(1), scale=1.0)
        table, _ = flt.path_table(q)
        lp = host(flt.kinematics(table))
        per_pair = []
        ref = MR.clearance_culled(lp, flt.spheres, flt.sphere_offsets, pair_words(flt.mesh_pairs, flt.L), flt.triangles,
                                  flt.tri_offsets, flt.planes, flt.obstacles, flt.env_mask, flt.exact_cutoff, per_pair=per_pair)
        _ARM.update(flt=flt, q=q, lp=lp, ref=ref, per_pair=per_pair)
    return _ARM


def test_xarm7_pair_lists(F, xarm7):
    flt = arm(F, xarm7)["flt"]
    plain = F.FeasibilityFilter(xarm7, leaf_triangles=64, margin=0.01)
    settle = {d["pair"]: d for d in plain.ignored if d["reason"] == "settle"}
    print(f"[mesh clearance xarm7] pairs {len(flt.pairs)}, mesh_pairs {len(flt.mesh_pairs)}; settle pairs of the proxies "
          f"{sorted(settle)}; still ignored {[(d['pair'], d['reason'], d.get('mesh_clearance')) for d in flt.ignored if d['reason'] == 'settle']}")
    assert flt.exact_cutoff == 0.02 and flt.pairs == plain.pairs and not hasattr(plain, "mesh_pairs")
    assert set(flt.mesh_pairs) >= set(flt.pairs) and flt.mesh_pairs == sorted(flt.mesh_pairs)
    kept = {d["pair"]: d for d in flt.ignored if d["reason"] == "settle"}
    assert set(flt.mesh_pairs) - set(flt.pairs) == set(settle) - set(kept)             # every settle pair is in one of the two
    assert all(d["mesh_clearance"] <= flt.margin for d in kept.values())
    assert [d for d in flt.ignored if d["reason"] != "settle"] == [d for d in plain.ignored if d["reason"] != "settle"]
    # the decision, on the reference: each settle pair alone, at the settle configuration
    from easyhec_amd.feasibility import pair_words
    lp0 = xarm7.link_poses_batch(np.zeros((1, flt.J))).astype(np.float32)
    for pr in sorted(settle):
        d = MR.clearance_culled(lp0, flt.spheres, flt.sphere_offsets, pair_words([pr], flt.L), flt.triangles, flt.tri_offsets,
                                cutoff=flt.exact_cutoff)[0][0]
        print(f"[mesh clearance xarm7] settle pair {pr}: proxies {settle[pr]['clearance']:.4f}, meshes {d:.4f} (reported up to 0.02)")
        assert (pr in flt.mesh_pairs) == (d > flt.margin)
        assert pr in flt.mesh_pairs or bits(kept[pr]["mesh_clearance"]) == bits(d)


def test_xarm7_sampled_configurations(F, xarm7):
    A = arm(F, xarm7)
    flt, q, lp, ref = A["flt"], A["q"], A["lp"], A["ref"]
    mc, mp, mt, ec = ref
    case = {"link_poses": lp, "offsets": flt.sphere_offsets, "tri_offsets": flt.tri_offsets, "triangles": flt.triangles,
            "pair_enable": FR_words(flt.mesh_pairs, flt.L)}
    ok = (mc > flt.margin) & (ec > flt.margin)
    near = min(np.abs(mc - flt.margin).min(), np.abs(ec - flt.margin).min())
    print(f"[mesh clearance xarm7] the reference accepts {int(ok.sum())} of 32 (self {int((mc > flt.margin).sum())}, env "
          f"{int((ec > flt.margin).sum())}); {int((mc == 0).sum())} intersect; nearest clearance to its threshold {near:.2e} m")
    out = flt.check(q)
    got = (host(out.self_clear), host(out.mesh_pair), host(out.mesh_tri), host(out.env_clear))
    assert_same("xarm7", got, ref, case)
    assert (host(out.self_pair) == got[1]).all() and (host(out.reach_clear) == flt.cutoff).all() and host(out.reach_ok).all()
    if near > 1e-9:
        assert (host(out.valid) == ok).all() and (host(out.self_ok) == (mc > flt.margin)).all()
    # on the reference alone: over the pairs both lists hold, the meshes accept every configuration the proxies accept
    sc = FR.clearance(lp, flt.spheres, flt.sphere_offsets, FR_words(flt.pairs, flt.L), cutoff=flt.cutoff)[0]
    shared = {32 * i + j for i, j in flt.pairs}
    mesh_shared = np.array([np.sqrt(min([d2 for code, d2 in pp.items() if code in shared] + [np.inf])) for pp in A["per_pair"]])
    print(f"[mesh clearance xarm7] proxies accept {int((sc > flt.margin).sum())} of 32 on self clearance, the meshes over the same "
          f"pairs {int((mesh_shared > flt.margin).sum())}, over mesh_pairs {int((mc > flt.margin).sum())}")
    assert ((mesh_shared > flt.margin) | ~(sc > flt.margin)).all()
    assert (sc <= np.minimum(mesh_shared, flt.cutoff) + 1e-6).all()


def FR_words(pairs, L):
    from easyhec_amd.feasibility import pair_words
    return pair_words(pairs, L)


def test_xarm7_check_over_a_path(F, xarm7):
    """``check`` with path steps reduces the mesh kernel's outputs as it reduces the proxies': against the same reduction of the
    kernel's own per-step outputs (which the test above holds to the reference)."""
    flt = arm(F, xarm7)["flt"]
    cur = np.array([0.0, 0.3, 0.0, 1.2, 0.0, 0.9, 0.0])
    cand = xarm7.sample_qpos(6, np.random.default_rng(4), scale=1.0)
    table, steps = flt.path_table(cand, cur, 3)
    lp = flt.kinematics(table)
    raw = flt.mesh_clearance(lp)
    rc = host(flt.clearance(lp).reach_clear)
    mtri = host(raw.mesh_tri).reshape(6, 3, 2)
    ref = FR.reduce_steps(host(raw.mesh_clear), host(raw.mesh_pair), host(raw.env_clear), rc, 3, flt.margin)
    out = flt.check(cand, current_qpos=cur, path_steps=3)
    for k in ("valid", "self_ok", "env_ok", "reach_ok", "self_pair", "worst_step"):
        assert (host(getattr(out, k)) == ref[k]).all(), k
    for k in ("self_clear", "env_clear", "reach_clear"):
        assert (bits(host(getattr(out, k))) == bits(ref[k])).all(), k
    at = np.where(np.isnan(host(raw.mesh_clear).reshape(6, 3)), -np.inf, host(raw.mesh_clear).reshape(6, 3)).argmin(axis=1)
    assert (host(out.mesh_tri) == mtri[np.arange(6), at]).all() and (host(out.mesh_pair) == ref["self_pair"]).all()


# ---- the online loop --------------------------------------------------------------------------------------------------------
def test_online_loop_with_an_exact_filter(F, xarm7):
    """``OnlineCalibration(feasible=)`` with an exact filter: the log carries the filter's own counts and says which mode turned
    the candidates down; the configuration asked for is one the filter accepts."""
    from easyhec_amd import render_api
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.online import OnlineCalibration
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    H, W = 120, 160
    K = np.array(scaled_K(XARM7_K_1280x720, 0.125, W, H, True), dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    flt = F.FeasibilityFilter(xarm7, margin=0.01, planes=[[0.0, 0.0, 1.0, 0.0]], path_steps=2, exact=True)
    under = np.array([[0.0, 2.0, 0.0, 0.3, 0.0, 0.0, 0.0], [1.0, 1.9, 0.0, 0.2, 0.0, 0.3, 0.0]])   # folded below the table
    cand = np.concatenate([xarm7.sample_qpos(10, np.random.default_rng(1), scale=0.6), under])
    first = np.zeros(7)
    fc = flt.check(cand, current_qpos=first, path_steps=2)
    valid = host(fc.valid)
    print(f"[mesh clearance online] the exact filter accepts {valid.astype(int).tolist()}")
    assert not valid[10:].any() and valid[:10].sum() >= 2
    asked = []

    def capture(qpos):
        asked.append(np.array(qpos))
        return render_api.nvdiffrast_render_xarm_api(None, Tc_gt, qpos, H, W, K)

    loop = OnlineCalibration(xarm7, K, H, W, perturb_pose(Tc_gt), capture, lambda _r: (cand, None), num_epochs=60, explore_iters=2,
                             explore="information", feasible=flt)
    loop.fit(first)
    r = loop.log[0]
    print(f"[mesh clearance online] {r}")
    assert r["rejected_mode"] == "exact"
    assert (r["rejected_self"], r["rejected_env"], r["rejected_reach"]) == (
        int((~host(fc.self_ok)).sum()), int((~host(fc.env_ok)).sum()), int((~host(fc.reach_ok)).sum()))
    hit = [i for i in range(12) if (cand[i] == asked[1]).all()]
    assert len(hit) == 1 and valid[hit[0]]
