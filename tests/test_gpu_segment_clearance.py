"""The swept feasibility kernel (csrc/ehr_segment_clearance.hip) and ``FeasibilityFilter.check_swept`` on the GPU, held against
the numpy mirror of tests/segment_clearance_reference.py BIT FOR BIT through the trace: q(trace_t) is rebuilt on the host,
``ehr_joint_forward`` gives its poses and joint frames, the mirror walks the search on them, and every traced value, the t
sequence and all outputs must be equal; the raw values must also be ``ehr_config_clearance``'s on those poses.
tests/test_segment_clearance_reference.py pins the mirror on the CPU.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import feasibility_reference as FR
import segment_clearance_reference as SR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FLOATS = ("t_free", "cert_self", "cert_env", "cert_reach", "stop_self", "stop_env", "stop_reach")
INTS = ("status", "evals", "stop_pair")


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, feasibility
    assert _lib.has_segment_clearance()
    return feasibility


@pytest.fixture(scope="module")
def xarm7():
    from easyhec_amd.robot import load_robot
    return load_robot("xarm7")


def dev(a, dtype=np.float64):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=dtype), device=DEV)


def words(a):
    return dev(np.asarray(a).astype(np.uint32).view(np.int32), np.int32)


def same(a, b):
    """Equal bits, NaN against NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def table_tensors(table):
    N = table["parent"].shape[0]
    return [dev(table["parent"], np.int32), dev(table["origin"].reshape(N, 16)), dev(table["kind"], np.int32), dev(table["axis"]),
            dev(table["qidx"], np.int32), dev(table["use"], np.int32)]


def joint_forward(tensors, q, offset):
    """(link_poses [m,L,16], joint_frames [m,J,6]) float32 of ``ehr_joint_forward`` at the host table q [m,J]."""
    from easyhec_amd import _lib
    q = np.atleast_2d(np.ascontiguousarray(q, dtype=np.float64))
    m, J = q.shape
    N, L = int(tensors[0].shape[0]), int(tensors[5].shape[0])
    lp, jf = torch.empty((m, L, 16), device=DEV), torch.empty((m, J, 6), device=DEV)
    _lib.check(_lib.lib().ehr_joint_forward(*[_lib.ptr(t) for t in tensors], N, J, L, _lib.ptr(dev(q)), _lib.ptr(offset), m,
                                            _lib.ptr(lp), _lib.ptr(jf), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "ehr_joint_forward")
    torch.cuda.synchronize()
    return lp.cpu().numpy(), jf.cpu().numpy()


def launch(F, case, **over):
    """One launch on a case of SR.make_case (``over``: q1, cutoff, margin, depth, max_evals) -> dict of numpy arrays."""
    c = dict(case, **over)
    tensors = table_tensors(c["table"])
    out = F.segment_clearance(tensors, dev(c["q0"]), dev(np.atleast_2d(c["q1"])), dev(c["offset"], np.float32), dev(c["spheres"]),
                              c["offsets"], dev(c["bounds"]), words(c["pair_enable"]), words(c["table"]["upstream"]),
                              words(c["below"]), dev(c["W"]), dev(c["planes"]), dev(c["obstacles"]), c["env_links"],
                              dev(c["reach"]), c["cutoff"], c["margin"], c["depth"], c["max_evals"], trace=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(out).items()}


def mirror(F, case, got, **over):
    """The mirror on the KERNEL's kinematics: ``ehr_joint_forward`` at q0 + t d for the t of the kernel's trace (one launch), and
    for any other t the mirror asks for (one launch each: then the t sequences differ, and the comparison says so)."""
    c = dict(case, **over)
    c["tab"] = dict(c["tab"], cutoff=c["cutoff"])
    tensors, offset = table_tensors(c["table"]), dev(c["offset"], np.float32)
    q1 = np.atleast_2d(c["q1"])
    refs = []
    for b in range(q1.shape[0]):
        d = q1[b] - c["q0"]
        ts = got["trace_t"][b, :max(int(got["evals"][b]), 0)]
        cache = {}
        if ts.size and np.isfinite(d).all():
            lp, jf = joint_forward(tensors, c["q0"][None] + ts[:, None] * d[None], offset)
            cache = {float(t): (lp[k], jf[k]) for k, t in enumerate(ts)}
            # the raw values are ehr_config_clearance's on those poses
            raw = F.config_clearance(torch.tensor(lp.reshape(len(ts), -1, 4, 4), device=DEV), dev(c["spheres"]), c["offsets"],
                                     dev(c["bounds"]), words(c["pair_enable"]), dev(c["planes"]), dev(c["obstacles"]),
                                     c["env_links"], dev(c["reach"]), c["cutoff"])
            torch.cuda.synchronize()
            for k, name in enumerate(("self_clear", "env_clear", "reach_clear")):
                assert same(got["trace_val"][b, :len(ts), k], getattr(raw, name).cpu().numpy()).all(), (b, name)
            if int(got["status"][b]) in (1, 2) and not np.isnan(got["stop_self"][b]):
                assert got["stop_pair"][b] == raw.self_pair.cpu().numpy()[-1]

        def kin(t, cache=cache, d=d):
            if float(t) not in cache:
                lp, jf = joint_forward(tensors, (c["q0"] + t * d)[None], offset)
                cache[float(t)] = (lp[0], jf[0])
            return cache[float(t)]
        refs.append(SR.search(kin, c["tab"], d, c["margin"], c["depth"][0], c["depth"][1], c["max_evals"]))
    return refs


def assert_same(what, got, refs):
    bad = []
    for b, ref in enumerate(refs):
        e = ref["evals"]
        print(f"[segment] {what} candidate {b}: mirror status {ref['status']} after {e} evaluations, t_free {ref['t_free']}, "
              f"certified {ref['cert_self']:.5f} {ref['cert_env']:.5f} {ref['cert_reach']:.5f}; kernel status "
              f"{int(got['status'][b])} after {int(got['evals'][b])}, t_free {got['t_free'][b]}")
        bad += [(b, k) for k in INTS if int(got[k][b]) != ref[k]]
        bad += [(b, k) for k in FLOATS if not same(got[k][b], ref[k]).all()]
        n = min(e, int(got["evals"][b]))
        if not same(got["trace_t"][b, :n], ref["trace_t"][:n]).all():
            bad.append((b, "trace_t"))
        elif n and not same(got["trace_val"][b, :n], np.array(ref["trace_val"][:n]).reshape(n, 6)).all():
            diff = ~same(got["trace_val"][b, :n], np.array(ref["trace_val"][:n]).reshape(n, 6))
            k = np.argwhere(diff)[0]
            print(f"[segment]   trace_val differs first at evaluation {k[0]} value {k[1]}: kernel {got['trace_val'][b, k[0], k[1]]!r}, "
                  f"mirror {ref['trace_val'][k[0]][k[1]]!r}")
            bad.append((b, "trace_val"))
        if not np.isnan(got["trace_t"][b, max(int(got["evals"][b]), 0):]).all():
            bad.append((b, "trace written past evals"))
    assert not bad, (what, bad)


# tree, rendered links, spheres per link, ...: SR.make_case
CASES = {
    "L1": dict(tree="one", use=None, counts=[65], seed=21, n_planes=2, n_obstacles=3, with_reach=True),           # no pairs
    "L2-J1": dict(tree="one", use=[0, 1], counts=[33, 7], seed=22, n_planes=1),
    "prismatic-empty-link": dict(tree="prismatic_mid", use=None, counts=[5, 0, 64, 1, 63, 3, 17], seed=23, n_planes=3,
                                 n_obstacles=40, with_reach=True),                                                 # S = 153
    "tree": dict(tree="tree", use=None, counts=[9, 20, 11, 13, 70, 31, 7], seed=24, n_planes=6, n_obstacles=5, with_reach=True),
}
_BUILT = {}


def built(name):
    if name not in _BUILT:
        _BUILT[name] = SR.make_case(**CASES[name])
    return _BUILT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_mirror(F, name):
    case = built(name)
    got = launch(F, case)
    refs = mirror(F, case, got)
    assert_same(name, got, refs)
    again = launch(F, case)
    assert all(same(got[k], again[k]).all() for k in FLOATS + ("trace_t", "trace_val")) and \
        all((got[k] == again[k]).all() for k in INTS), "two runs: the same bits"
    up = case["tab"]["upstream"]
    if name == "tree":       # a pair on two branches: both masks non-empty
        assert any(up[i] & ~up[j] and up[j] & ~up[i] for i, j in FR.pairs_of(case["pair_enable"], len(up)))
    if name == "prismatic-empty-link":
        assert 2 in case["tab"]["jkind"].tolist() and int(case["offsets"][-1]) % 2 == 1
    if name != "L2-J1":
        assert max(r["evals"] for r in refs) > 2, "the case must split an interval"


def test_a_nan_candidate_leaves_its_neighbours_alone(F):
    case = built("tree")
    whole = launch(F, case)
    q1 = case["q1"].copy()
    q1[1, 2] = np.nan
    got = launch(F, case, q1=q1)
    assert (got["status"][1], got["evals"][1], got["stop_pair"][1], got["t_free"][1]) == (3, 0, -1, 0.0)
    assert np.isnan([got["stop_self"][1], got["stop_env"][1], got["stop_reach"][1]]).all() and np.isnan(got["trace_t"][1]).all()
    assert got["cert_self"][1] == got["cert_env"][1] == got["cert_reach"][1] == case["cutoff"]
    for b in (0, 2):
        assert all(same(got[k][b], whole[k][b]).all() for k in FLOATS + ("trace_t", "trace_val"))
        assert all(got[k][b] == whole[k][b] for k in INTS)
    alone = launch(F, case, q1=case["q1"][1:2])                                        # n = 1: what it is among three
    assert all(same(alone[k][0], whole[k][1]).all() for k in FLOATS + ("trace_t", "trace_val"))
    assert all(alone[k][0] == whole[k][1] for k in INTS)
    inf = case["q1"].copy()
    inf[1, 0] = np.inf
    assert launch(F, case, q1=inf)["status"].tolist() == [int(whole["status"][0]), 3, int(whole["status"][2])]


def test_one_evaluation_and_no_splitting(F):
    case = built("prismatic-empty-link")
    one = launch(F, case, max_evals=1)
    assert_same("max_evals = 1", one, mirror(F, case, one, max_evals=1))
    # (depth 1: an undecided first interval stops at 0, a certified one leaves the budget spent at 1/2)
    assert (one["evals"] == 1).all() and set(one["status"].tolist()) <= {1, 2} and np.isin(one["t_free"], (0.0, 0.5)).all()
    flat = launch(F, case, depth=(3, 3))
    refs = mirror(F, case, flat, depth=(3, 3))
    assert_same("min_depth = max_depth", flat, refs)
    assert all(r["trace_t"] == [(2 * i + 1) / 16 for i in range(r["evals"])] for r in refs)
    deep = launch(F, case, depth=(0, 20), max_evals=64)                                # the limits of the depth
    assert_same("depth 0..20", deep, mirror(F, case, deep, depth=(0, 20), max_evals=64))


def test_a_long_cutoff_changes_only_what_the_short_one_caps(F):
    """A 3 cm and a 10 m cutoff, both against the mirror; and at the first evaluation (the same t under both) the raw values below the short cutoff
    have the same bits, the others are capped, and no certified value grows when the cutoff shrinks: the far values stand for
    what lies beyond it."""
    case = built("tree")
    short, far = launch(F, case, cutoff=0.03, depth=(2, 6)), launch(F, case, cutoff=10.0, depth=(2, 6))
    assert_same("cutoff 0.03", short, mirror(F, case, short, cutoff=0.03, depth=(2, 6)))
    assert_same("cutoff 10", far, mirror(F, case, far, cutoff=10.0, depth=(2, 6)))
    a, b = short["trace_val"][:, 0], far["trace_val"][:, 0]
    print(f"[segment] first evaluations, cutoff 0.03: {a.tolist()}, cutoff 10: {b.tolist()}")
    below = b[:, :3] < 0.03
    assert same(a[:, :3][below], b[:, :3][below]).all() and (a[:, :3][~below] == 0.03).all() and below.any() and (~below).any()
    assert (a[:, 3:] <= b[:, 3:]).all()


def test_refused_sizes_and_nulls(F):
    from easyhec_amd import _lib
    case = built("L2-J1")
    for over, msg in ((dict(depth=(5, 3)), "bad budget"), (dict(depth=(0, 21)), "bad budget"), (dict(max_evals=0), "bad budget"),
                      (dict(max_evals=4097), "bad budget"), (dict(margin=0.3), "margin"), (dict(margin=-0.1), "margin"),
                      (dict(cutoff=float("inf")), "cutoff")):
        with pytest.raises(RuntimeError, match=msg):
            launch(F, case, **over)
    big = dict(case, offsets=np.array([0, 33, _lib.SEG_MAX_SPHERES + 1], np.int32),
               spheres=np.zeros((_lib.SEG_MAX_SPHERES + 1, 4)))
    with pytest.raises(RuntimeError, match="spheres"):
        launch(F, big)
    with pytest.raises(RuntimeError, match="ascend"):
        launch(F, dict(case, offsets=np.array([0, 33, 20], np.int32)))
    t = table_tensors(case["table"])
    p = _lib.ptr
    z = torch.zeros(64, dtype=torch.float64, device=DEV)
    args = [p(x) for x in t] + [2, 1, 2, p(z), p(z), p(z), 1, p(z), case["offsets"].ctypes.data_as(ctypes.c_void_p), p(z), p(z), None, 0,
                                None, 0, 0, None, 0.25, p(z), p(z), p(z), 0.01, 3, 9, 96] + [p(z)] * 10 + [None, None, None]
    for k in (0, 9, 15, 26, 31, 40):
        bad = list(args)
        bad[k] = None
        assert _lib.lib().ehr_segment_clearance(*bad) != 0 and b"NULL" in _lib.lib().ehr_last_error()
    bad = list(args)
    bad[41] = p(z)                                                                     # trace_t without trace_val
    assert _lib.lib().ehr_segment_clearance(*bad) != 0 and b"NULL" in _lib.lib().ehr_last_error()
    with pytest.raises(ValueError, match="swept"):
        from easyhec_amd.robot import load_robot
        F.FeasibilityFilter(load_robot("xarm7"), swept=True, exact=True)


# ---- the packaged arm -------------------------------------------------------------------------------------------------------------
def filter_case(flt, cur, cand):
    """A filter's own tensors as a case of the mirror."""
    qp, _ = flt.path_table(cand)
    c0, _ = flt.path_table(np.asarray(cur, dtype=np.float64).reshape(1, -1))
    travel = np.where(flt._prismatic, np.abs(np.concatenate([qp, c0])).max(axis=0) + flt.offset_bound, 0.0)
    from easyhec_amd import feasibility as fz
    W, below = fz.reach_radii(flt._table, flt.link_bounds, travel), fz.joint_below(flt._table)
    pe = fz.pair_words(flt.pairs, flt.L)
    return {"table": flt._table, "q0": c0[0], "q1": qp, "offset": flt.offsets.cpu().numpy(), "spheres": flt.spheres,
            "offsets": flt.sphere_offsets, "bounds": flt.link_bounds, "pair_enable": pe, "planes": flt.planes,
            "obstacles": flt.obstacles, "env_links": flt.env_mask, "reach": flt.reach, "cutoff": flt.cutoff, "margin": flt.margin,
            "depth": flt.swept_depth, "max_evals": flt.swept_evals, "W": W, "below": below,
            "tab": SR.make_tables(flt._table, flt.spheres, flt.sphere_offsets, pe, W, below, flt.planes, flt.obstacles, flt.env_mask,
                                  flt.reach, flt.cutoff)}


def swept_outputs(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(out).items()}


BENT = np.array([0, 0.3, 0, 0.9, 0, 0.6, 0.0])


def test_xarm7_eight_candidates(F, xarm7):
    flt = F.FeasibilityFilter(xarm7, margin=0.01, planes=F.box_planes(*F.REFERENCE_WORKSPACE), swept=True, swept_evals=48)
    cand = xarm7.sample_qpos(40, np.random.default_rng(0), scale=0.5)[[0, 1, 2, 3, 5, 8, 13, 21]]
    got = swept_outputs(flt.check_swept(cand, BENT, trace=True))
    case = filter_case(flt, BENT, cand)
    refs = mirror(F, case, got)
    assert_same("xarm7", got, refs)
    status = np.array([r["status"] for r in refs])
    assert (got["valid"] == (status == 0)).all()
    hit = status == 1
    for k, bar in (("self", flt.margin), ("env", flt.margin)):
        assert (got[k + "_ok"] == ((status == 0) | (hit & (got["stop_" + k] > bar)))).all()
    assert (got["reach_ok"] == ((status == 0) | hit)).all()                          # (no reach ball: nothing to fail)
    assert int(flt.spheres.shape[0]) == 960


def test_franka_fits_the_lds(F):
    """2944 spheres: 40 bytes each beside the kinematics' frames, inside the 160 KiB of a compute unit."""
    from easyhec_amd.robot import load_robot
    franka = load_robot("franka")
    flt = F.FeasibilityFilter(franka, margin=0.01, swept=True, swept_depth=(1, 4), swept_evals=6)
    assert int(flt.spheres.shape[0]) == 2944
    cur = np.array([0.0, -0.4, 0.0, -1.8, 0.0, 1.6, 0.8])
    cand = cur[None] + np.array([[0.02, 0.02, 0.0, 0.02, 0.0, 0.0, 0.0], [0.6, 0.3, -0.4, 0.5, 0.3, -0.2, 0.4]])
    got = swept_outputs(flt.check_swept(cand, cur, trace=True))
    assert_same("franka", got, mirror(F, filter_case(flt, cur, cand), got))


def test_the_move_four_samples_step_over(F, xarm7):
    q0, q1 = np.array([-1.5, 0.8, 0, 1.6, 0, 0, 0.0]), np.array([1.5, 0.8, 0, 1.6, 0, 0, 0.0])
    probe = F.FeasibilityFilter(xarm7, margin=0.01)
    lp, _ = joint_forward(probe._t, probe.path_table((q0 + 9 / 16 * (q1 - q0))[None])[0], probe.offsets)
    last = FR.world_spheres(lp[0], probe.spheres, probe.sphere_offsets)[probe.sphere_offsets[-2]:]
    far = int(np.argmax(np.hypot(last[:, 0], last[:, 1])))
    flt = F.FeasibilityFilter(xarm7, margin=0.01, obstacles=[[last[far, 0], last[far, 1], last[far, 2], 0.01]], swept=True)
    sampled = swept_outputs(flt.check(q1[None], current_qpos=q0, path_steps=4))
    print(f"[segment] four samples: valid {sampled['valid'].tolist()}, env_clear {sampled['env_clear'].tolist()}")
    assert sampled["valid"].all(), "the sampled check accepts the move"
    got = swept_outputs(flt.check_swept(q1[None], q0, trace=True))
    print(f"[segment] swept: status {got['status'].tolist()}, t_free {got['t_free'].tolist()}, stop_env {got['stop_env'].tolist()}")
    stop_t = got["trace_t"][0, got["evals"][0] - 1]
    assert got["status"][0] == 1 and 0.5 <= got["t_free"][0] and 0.5 < stop_t < 0.625
    assert not got["valid"][0] and not got["env_ok"][0] and got["self_ok"][0] and got["reach_ok"][0]
    assert_same("tunnelling", got, mirror(F, filter_case(flt, q0, q1[None]), got))


def test_online_loop_with_a_swept_filter(F, xarm7):
    from easyhec_amd import render_api
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.online import OnlineCalibration
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    H, W = 120, 160
    K = np.array(scaled_K(XARM7_K_1280x720, 0.125, W, H, True), dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    flt = F.FeasibilityFilter(xarm7, margin=0.01, planes=[[0.0, 0.0, 1.0, 0.0]], swept=True, swept_depth=(3, 7), swept_evals=40)
    under = np.array([[0.0, 2.0, 0.0, 0.3, 0.0, 0.0, 0.0]])                             # folded below the table
    cand = np.concatenate([xarm7.sample_qpos(7, np.random.default_rng(1), scale=0.6), under])
    first = BENT
    got = swept_outputs(flt.check_swept(cand, first, trace=True))
    refs = mirror(F, filter_case(flt, first, cand), got)
    assert_same("online", got, refs)
    status = np.array([r["status"] for r in refs])
    print(f"[segment online] the mirror's statuses {status.tolist()}")
    assert status[-1] != 0 and (status == 0).any()
    asked = []

    def capture(qpos):
        asked.append(np.array(qpos))
        return render_api.nvdiffrast_render_xarm_api(None, Tc_gt, qpos, H, W, K)

    loop = OnlineCalibration(xarm7, K, H, W, perturb_pose(Tc_gt), capture, lambda _r: (cand, None), num_epochs=60, explore_iters=2,
                             explore="information", feasible=flt)
    loop.fit(first)
    r = loop.log[0]
    print(f"[segment online] {loop.log}")
    hit = [i for i in range(len(cand)) if (cand[i] == asked[1]).all()]
    assert len(hit) == 1 and status[hit[0]] == 0
    assert r["rejected_mode"] == "swept" and r["undecided"] == int((status >= 2).sum())
    for k in ("self", "env", "reach"):
        assert r["rejected_" + k] == int((~got[k + "_ok"]).sum())
    assert "rejected_mode" not in loop.log[1]
