"""The numpy mirror of ``ehr_segment_clearance`` (tests/segment_clearance_reference.py) on the host's kinematics: that its
certified values are sound against dense sampling, an analytic case in closed form, the move that the sampled check steps over,
the budget's edges, and the share of sample-valid moves it decides.  CPU only."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import feasibility_reference as F
import joint_reference as JR
import joint_table_cases as TC
import segment_clearance_reference as SR
from easyhec_amd import feasibility as fz
from easyhec_amd.robot import load_robot

MARGIN, CUTOFF = 0.01, 0.25
BENT = (0, 0.3, 0, 0.9, 0, 0.6, 0)


@functools.lru_cache(maxsize=None)
def arm(name, reach=False):
    """(robot, table, tab, parts) with the reference's workspace box (and a ball of allowed reach); the tree's prismatic joints
    travel 5 cm + 0.2."""
    if name == "tree":
        robot = TC.tree_robot()
        travel = np.where(TC.kinds("tree") == 2, TC.PRIS_RANGE + 0.2, 0.0)
        return (robot,) + SR.robot_case(robot, planes=fz.box_planes((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)),
                                        reach=(0.0, 0.0, 0.0, 0.9) if reach else None, travel=travel, leaf_triangles=4)
    robot = load_robot(name)
    return (robot,) + SR.robot_case(robot, planes=fz.box_planes(*fz.REFERENCE_WORKSPACE),
                                    reach=(0.0, 0.0, 0.3, 1.3) if reach else None)


def padded(robot, q):
    out = np.zeros(robot.chain.dof)
    out[:len(q)] = q
    return out


def segments(name, n, seed):
    robot = arm(name)[0]
    rng = np.random.default_rng(seed)
    if name == "tree":
        q = TC.qpos("tree", 2 * n, seed=seed)
        return [(q[2 * k], q[2 * k + 1]) for k in range(n)]
    q = robot.sample_qpos(2 * n, rng, scale=0.5)
    return [(padded(robot, q[2 * k]), padded(robot, q[2 * k + 1])) for k in range(n)]


# ---- soundness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,count", [("xarm7", 4), ("franka", 2), ("tree", 4)])
def test_certified_values_lie_below_dense_samples(name, count):
    """For random segments and intervals at depths 3, 5 and 7: each certified value of the interval is <= the least raw
    clearance over 21 dense samples of it (the certified values are lower bounds of the clearance on the whole interval)."""
    robot, table, tab, parts = arm(name, reach=True)
    rng = np.random.default_rng(7)
    checked = 0
    for q0, q1 in segments(name, count, seed=3):
        kin, dabs = SR.host_kin(table, q0, q1), np.abs(q1 - q0)
        for depth in (3, 5, 7):
            i = int(rng.integers(0, 1 << depth))
            h = 2.0 ** -(depth + 1)
            c = (2 * i + 1) * h
            cert = SR.evaluate(*kin(c), tab, dabs, h)[4:]
            dense = np.array([[v for k, v in enumerate(SR.evaluate(*kin(t), tab, dabs, h)[:4]) if k != 1]
                              for t in np.linspace(c - h, c + h, 21)]).min(axis=0)
            for what, lo, raw in zip(("self", "env", "reach"), cert, dense):
                assert lo <= raw, f"{name} depth {depth} interval {i} {what}: certified {lo} above the dense minimum {raw}"
                checked += 1
    assert checked == count * 9


def test_tree_has_pairs_with_two_masks_and_a_prismatic_joint():
    """The synthetic tree exercises what the two arms do not: pairs on different branches (both masks non-empty) and a
    prismatic joint with rate 1."""
    robot, table, tab, parts = arm("tree")
    up = tab["upstream"]
    assert any(up[i] & ~up[j] and up[j] & ~up[i] for i, j in parts["pairs"])
    assert 2 in tab["jkind"].tolist()
    J = robot.chain.dof
    pris = [j for j in range(J) if tab["jkind"][j] == 2]
    assert all(tab["W"][j, l] == 1.0 for j in pris for l in range(len(up)) if (up[l] >> j) & 1)
    assert all(tab["W"][j, l] == 0.0 for j in range(J) for l in range(len(up)) if not (up[l] >> j) & 1)


# ---- one link, one revolute joint, one sphere, one plane -------------------------------------------------------------------------
def one_joint_case(xmax):
    """A sphere of radius r at distance R0 from the z axis it turns about; the half-space x <= xmax."""
    R0, r = 0.5, 0.05
    table = {"parent": np.array([-1, 0], np.int32), "origin": np.tile(np.eye(4).reshape(16), (2, 1)),
             "kind": np.array([0, 1], np.int32), "axis": np.array([[1.0, 0, 0], [0, 0, 1.0]]), "qidx": np.array([-1, 0], np.int32),
             "use": np.array([1], np.int32), "upstream": np.array([1], np.uint32)}
    spheres = np.array([[R0, 0.0, 0.0, r]])
    W = fz.reach_radii(table, spheres)                      # the sphere is its own bound
    tab = SR.make_tables(table, spheres, [0, 1], np.zeros(1, np.uint32), W, fz.joint_below(table),
                         planes=np.array([[-1.0, 0.0, 0.0, xmax]]), env_links=1, cutoff=CUTOFF)
    return table, tab, R0, r


def test_one_joint_against_a_plane_in_closed_form():
    """rho = R0 + r = W, G = 0, so E = h |d| (R0 + r); the plane's value at q is xmax - R0 cos q - r.  From q = pi/3 to 2 pi/3
    the value grows with t, so the first interval of a depth decides it: depth k certifies iff
    xmax - R0 cos(pi/3 + h d) - r - h d (R0 + r) - 1e-6 > margin with h = 2^-(k+1).  With xmax such that the start keeps
    margin + 2 mm that is depth 5 and no depth before it."""
    R0, r = 0.5, 0.05
    xmax = R0 * math.cos(math.pi / 3) + r + MARGIN + 0.002
    table, tab, R0, r = one_joint_case(xmax)
    q0, q1 = np.array([math.pi / 3]), np.array([2 * math.pi / 3])
    d = float(q1[0] - q0[0])
    assert tab["W"][0, 0] == pytest.approx(R0 + r, abs=1e-15)
    kin = SR.host_kin(table, q0, q1)

    def closed(k):
        h = 2.0 ** -(k + 1)
        return xmax - R0 * math.cos(q0[0] + h * d) - r - h * d * (R0 + r) - SR.SLACK

    first = next(k for k in range(12) if closed(k) > MARGIN)
    assert first == 5
    for k in (3, 4, 5):                                       # (shallower centres lie beyond cutoff)
        h = 2.0 ** -(k + 1)
        rs, rp, re, rr, cs, ce, cr = SR.evaluate(*kin(h), tab, np.abs(q1 - q0), h)
        assert (rs, rp, rr, cs, cr) == (CUTOFF, -1, CUTOFF, CUTOFF - SR.SLACK, CUTOFF - SR.SLACK)
        assert re == pytest.approx(xmax - R0 * math.cos(q0[0] + h * d) - r, abs=2e-7)    # (float32 poses)
        assert re - ce - SR.SLACK == pytest.approx(h * d * (R0 + r), abs=2e-7)
        assert ce == pytest.approx(closed(k), abs=4e-7)
    out = SR.search(kin, tab, q1 - q0, MARGIN, 0, first, 4096)
    assert (out["status"], out["t_free"]) == (0, 1.0)
    assert max(Fraction(t).denominator for t in out["trace_t"]) == 2 ** (first + 1)   # centres of depth k are odd / 2^(k+1)
    short = SR.search(kin, tab, q1 - q0, MARGIN, 0, first - 1, 4096)
    assert (short["status"], short["t_free"]) == (2, 0.0) and short["stop_env"] > MARGIN


# ---- the move the sampled check steps over ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tunnelling_case():
    """The xArm7, stretched out, turns 3 rad about its base; a 1 cm obstacle sits where the outermost sphere of the last link
    is at t = 9/16.  (robot, table, q0, q1, obstacle [1,4])."""
    robot = load_robot("xarm7")
    table = robot.joint_table()
    q0 = padded(robot, (-1.5, 0.8, 0, 1.6, 0, 0, 0))
    q1 = padded(robot, (1.5, 0.8, 0, 1.6, 0, 0, 0))
    spheres, offsets, _ = fz.robot_proxies(robot)
    lp, _ = SR.host_kin(table, q0, q1)(9 / 16)
    last = F.world_spheres(lp, spheres, offsets)[offsets[-2]:offsets[-1]]
    far = int(np.argmax(np.hypot(last[:, 0], last[:, 1])))
    return robot, table, q0, q1, np.array([[last[far, 0], last[far, 1], last[far, 2], 0.01]])


def test_swept_search_finds_what_four_samples_step_over():
    robot, table, q0, q1, obstacle = tunnelling_case()
    _, tab, parts = SR.robot_case(robot, obstacles=obstacle)
    steps = 4
    frac = (np.arange(steps) + 1.0) / steps
    _, lp, _ = JR.fk(table, q0[None] + frac[:, None] * (q1 - q0)[None])
    sampled = F.clearance(lp.astype(np.float32), parts["spheres"], parts["offsets"], parts["pair_enable"], None, obstacle,
                          parts["env_links"], None, CUTOFF)
    assert F.reduce_steps(*sampled, steps, MARGIN)["valid"].all(), "the sampled check must accept this move"
    out = SR.search(SR.host_kin(table, q0, q1), tab, q1 - q0, MARGIN, 3, 9, 96)
    assert out["status"] == 1
    assert 0.5 <= out["t_free"] and 0.5 < out["trace_t"][-1] < 0.625
    assert out["stop_env"] <= MARGIN < out["stop_self"]


# ---- budgets ----------------------------------------------------------------------------------------------------------------------
def test_budget_edges():
    robot, table, tab, parts = arm("xarm7")
    q0 = padded(robot, BENT)
    for c in robot.sample_qpos(40, np.random.default_rng(0), scale=0.5):      # the first clear move that needs splits
        q1 = padded(robot, c)
        kin = SR.host_kin(table, q0, q1)
        full = SR.search(kin, tab, q1 - q0, MARGIN, 3, 9, 96)
        if full["status"] == 0 and full["evals"] > 16:
            break
    else:
        raise AssertionError("the draw must hold a clear move that needs splits")
    # one evaluation: the first interval's centre, undecided at its left end
    one = SR.search(kin, tab, q1 - q0, MARGIN, 3, 9, 1)
    assert (one["status"], one["evals"], one["t_free"], one["trace_t"]) == (2, 1, 0.0, [1 / 16])
    assert one["stop_self"] == full["trace_val"][0][0]
    # no splitting allowed: stops at the first interval of depth 3 that does not certify
    flat = SR.search(kin, tab, q1 - q0, MARGIN, 3, 3, 96)
    assert flat["status"] == 2 and flat["t_free"] == flat["trace_t"][-1] - 1 / 16 and flat["evals"] == len(flat["trace_t"])
    assert flat["trace_t"] == [(2 * i + 1) / 16 for i in range(flat["evals"])]
    # the budget runs out between two intervals: everything so far is certified, no evaluation stopped the search
    k = next(n for n in range(2, full["evals"]) if SR.search(kin, tab, q1 - q0, MARGIN, 3, 9, n)["status"] == 2
             and math.isnan(SR.search(kin, tab, q1 - q0, MARGIN, 3, 9, n)["stop_self"]))
    cut = SR.search(kin, tab, q1 - q0, MARGIN, 3, 9, k)
    assert cut["evals"] == k and 0 < cut["t_free"] < 1 and cut["stop_pair"] == -1 and cut["trace_t"] == full["trace_t"][:k]
    # a candidate that is not finite cannot be judged
    bad = q1.copy()
    bad[2] = np.nan
    nan = SR.search(SR.host_kin(table, q0, bad), tab, bad - q0, MARGIN, 3, 9, 96)
    assert (nan["status"], nan["evals"]) == (3, 0) and math.isnan(nan["stop_self"]) and nan["cert_self"] == CUTOFF


# ---- decided share ------------------------------------------------------------------------------------------------------------------
def test_sample_valid_moves_from_the_bent_start_come_out_clear():
    """40 candidates of sample_qpos(scale=0.5) from the bent start, depth 3..9, 96 evaluations: every candidate the 8-step sampled
    check accepts is certified clear, and nothing certified clear is sample-invalid."""
    robot, table, tab, parts = arm("xarm7")
    q0 = padded(robot, BENT)
    frac = (np.arange(8) + 1.0) / 8
    accepted = 0
    for c in robot.sample_qpos(40, np.random.default_rng(0), scale=0.5):
        q1 = padded(robot, c)
        _, lp, _ = JR.fk(table, q0[None] + frac[:, None] * (q1 - q0)[None])
        sampled = F.clearance(lp.astype(np.float32), parts["spheres"], parts["offsets"], parts["pair_enable"], tab["planes"], None,
                              parts["env_links"], tab["reach"], CUTOFF)
        ok = bool(F.reduce_steps(*sampled, 8, MARGIN)["valid"][0])
        out = SR.search(SR.host_kin(table, q0, q1), tab, q1 - q0, MARGIN, 3, 9, 96)
        assert (out["status"] == 0) == ok, f"sampled check {ok}, swept status {out['status']} after {out['evals']} evaluations"
        accepted += ok
    assert accepted >= 4, "the draw must hold accepted moves"
