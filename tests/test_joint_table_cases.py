"""The synthetic kinematic trees of tests/joint_table_cases.py, pinned on the CPU the way tests/test_joint_reference.py pins the
packaged robots: every case has the table shape it is named for; FK from the table alone (tests/joint_reference.py) is
``UrdfChain.link_poses_batch`` and an FK that never uses Rodrigues' formula (``torch.linalg.matrix_exp`` of the joint's twist,
walked on the spec's names); ``upstream`` is an ancestor walk; the analytic derivative is a central difference; the offset
gradient is the chain rule through FK.

Sensitivity pins: a deliberately wrong copy of the reference -- one per mistake a kernel could make that neither packaged robot
would show -- misses the true reference on its designated case by at least 100 times the bar tests/test_gpu_joint_table_shapes.py
applies to that quantity on that case (the bar is computed as there: from the reference's own float32 run)."""
import numpy as np
import pytest
import torch

import joint_reference as JR
import joint_table_cases as C
import pose_reference as R

F64, F32 = torch.float64, torch.float32
U = R.U


def _links(c):
    return list(range(len(c.chain.link_order)))


# ---- the shapes --------------------------------------------------------------------------------------------------------------
SHAPES = {"one": (2, 1, 1), "skew_serial": (8, 7, 7), "prismatic_mid": (7, 6, 7), "tree": (11, 8, 7), "full": (64, 32, 32),
          "serial64": (64, 32, 32)}


@pytest.mark.parametrize("name", C.NAMES)
def test_table_shape_and_the_spec_s_axes(name):
    c = C.case(name)
    t = c.table
    N, J, L = SHAPES[name]
    assert (t["parent"].shape[0], c.chain.dof, t["use"].shape[0]) == (N, J, L)
    assert t["upstream"].dtype == np.uint32 and t["use"].tolist() == c.use
    assert t["parent"][0] == -1 and (t["parent"][1:] >= 0).all() and (t["parent"][1:] < np.arange(1, N)).all()
    assert sorted(t["qidx"][t["qidx"] >= 0].tolist()) == list(range(J)) and ((t["kind"] == 0) == (t["qidx"] < 0)).all()
    assert np.array_equal(JR.joint_kinds(t), C.kinds(name))
    # the spec's axes are non-unit (or 0 0 0 on a fixed joint); the table's are unit, the same direction
    assert np.allclose(np.linalg.norm(t["axis"], axis=1), 1.0, atol=1e-15)
    for j in c.spec["joints"]:
        n = float(np.linalg.norm(j["axis"]))
        assert (j["type"] == "fixed" and n == 0.0) or 0.3 <= n <= 3.0, j
        if j["type"] != "fixed":
            assert abs(n - 1.0) > 1e-4
            i = c.chain.link_order.index(j["child"])
            assert np.abs(t["axis"][i] - np.asarray(j["axis"]) / n).max() <= 1e-15
        T = np.asarray(j["origin"])
        assert np.abs(T[:3, 3]).max() <= 0.15 and np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-14
        assert np.abs(T[:3, :3] - np.eye(3)).max() > 1e-4                      # a rotation of its own, not the identity
    from easyhec_amd.joint_calib import _check_table, free_joint_list
    _check_table(t, J)                                                           # what the solves refuse a table by
    assert free_joint_list(t, J, range(J)) == list(range(J))


def test_properties_the_cases_are_named_for():
    t = C.case("skew_serial").table
    assert (t["kind"][1:] == 1).all() and (np.abs(t["axis"][1:]) >= 0.2).all() and (t["parent"] == np.arange(-1, 7)).all()
    c = C.case("prismatic_mid")
    assert C.kinds("prismatic_mid").tolist() == [1, 2, 1, 1, 2, 1] and c.use == list(range(7))
    assert [int(u) for u in c.table["upstream"]] == [0, 1, 3, 7, 15, 31, 63]     # revolute joints downstream of a prismatic one
    # tree: the articulation order interleaves the branches
    c = C.case("tree")
    t = c.table
    assert c.chain.link_order == ["b", "a1", "c1", "f1", "a2", "c2", "e1", "a3", "d1", "a4", "d2"]
    assert (t["parent"][1:] != np.arange(10)).sum() >= 9 and (t["parent"] == 0).sum() == 3 and (t["parent"] == 4).sum() == 2
    up = [int(u) for u in t["upstream"]]
    assert c.use[0] == 0 and up[0] == 0                                          # the rendered root: an empty mask
    seen = 0
    for u in up:
        seen |= u
    idle = [j for j in range(8) if not (seen >> j) & 1]
    assert idle == [4] and C.kinds("tree")[4] == 1                               # an active joint nothing rendered hangs from
    assert any(a and b and not a & b for a in up for b in up)                    # rendered links on different branches
    assert sum(1 for j in c.spec["joints"] if j["type"] == "fixed" and j["axis"] == [0.0, 0.0, 0.0]) == 2
    assert C.kinds("tree")[5] == 2 and up[4] == 0xa5                             # a4: behind the prismatic a3 and three revolutes
    # full: the limits of the kernels, both ends of the mask
    c = C.case("full")
    up = [int(u) for u in c.table["upstream"]]
    k = C.kinds("full")
    assert (k == 1).sum() == 24 and (k == 2).sum() == 8
    assert any(u >> 31 for u in up) and any(u & 1 for u in up) and any(u >> 31 and u & 0xffff for u in up)
    assert any(a and b and not a & b for a in up for b in up)
    assert any(np.asarray(c.table["upstream"]).view(np.int32) < 0)               # the sign bit of the view the host uploads
    assert any(j["type"] == "fixed" and j["axis"] == [0.0, 0.0, 0.0] for j in c.spec["joints"])
    pris_up = [j for j in range(32) if k[j] == 2]
    assert any(u >> j & 1 and any(u >> r & 1 for r in range(j + 1, 32) if k[r] == 1) for u in up for j in pris_up)
    # serial64: the longest walk, the full mask
    c = C.case("serial64")
    assert (c.table["parent"] == np.arange(-1, 63)).all() and c.table["kind"][1:].tolist() == [1, 0] * 31 + [1]
    assert c.use == list(range(32, 64)) and int(c.table["upstream"][-1]) == 0xFFFFFFFF and int(c.table["upstream"][0]) == 0xFFFF
    assert (C.free_mask("full", "frozen")[[2, 7, 31]] == 0).all() and C.free_mask("full", "frozen").sum() == 25


def test_joint_vectors_cross_pi():
    for name in C.NAMES:
        k = C.kinds(name)
        q = np.concatenate([C.qpos(name, B) for B in (1, 5, 9)])
        assert (np.abs(q[:, k == 1]) <= 3.5).all() and (np.abs(q[:, k == 2]) <= 0.05).all()
        off = C.offsets(name)
        assert off.dtype == np.float32 and (np.abs(off[k == 2]) <= 0.005).all() and (np.abs(off) <= 0.1).all()
    q = C.qpos("full", 9)
    assert (np.abs(q[:, C.kinds("full") == 1]) > np.pi).any()


# ---- forward kinematics --------------------------------------------------------------------------------------------------------
def expm_fk(c, q):
    """[B,N,4,4] float64 in articulation order, walked on the spec's NAMES: pose(child) = pose(parent) @ origin @ exp(q xi),
    xi the joint's twist about / along its normalised axis -- ``torch.linalg.matrix_exp``, no Rodrigues formula."""
    col = {j["name"]: i for i, j in enumerate(c.chain.active)}
    of_child = {j["child"]: j for j in c.spec["joints"]}
    q = torch.as_tensor(np.atleast_2d(q), dtype=F64)
    B = q.shape[0]
    memo = {}

    def pose(l):
        if l not in memo:
            if l not in of_child:
                memo[l] = torch.eye(4, dtype=F64).expand(B, 4, 4)
            else:
                j = of_child[l]
                T = pose(j["parent"]) @ torch.tensor(j["origin"], dtype=F64)
                if j["type"] != "fixed":
                    a = torch.tensor(j["axis"], dtype=F64)
                    a = a / torch.sqrt((a * a).sum())
                    xi = torch.zeros((4, 4), dtype=F64)
                    if j["type"] == "revolute":
                        xi[0, 1], xi[0, 2], xi[1, 2] = -a[2], a[1], -a[0]
                        xi[1, 0], xi[2, 0], xi[2, 1] = a[2], -a[1], a[0]
                    else:
                        xi[:3, 3] = a
                    T = T @ torch.linalg.matrix_exp(q[:, col[j["name"]], None, None] * xi)
                memo[l] = T
        return memo[l]

    return torch.stack([pose(l) for l in c.chain.link_order], dim=1).numpy()


@pytest.mark.parametrize("name", C.NAMES)
def test_fk_from_the_table_is_the_host_s_and_the_matrix_exponential_s(name):
    c = C.case(name)
    q, off = C.qpos(name, 5), C.offsets(name).astype(np.float64)
    frames, lp, jf = JR.fk(c.table, q, off)
    host = c.chain.link_poses_batch(q + off, _links(c))
    d_host = float(np.abs(frames - host).max())
    d_exp = float(np.abs(frames - expm_fk(c, q + off)).max())
    print(f"{name}: |fk - link_poses_batch| {d_host:.2e} | |fk - matrix_exp fk| {d_exp:.2e}")
    assert d_host <= 1e-12 and d_exp <= 1e-12
    assert np.array_equal(lp, frames[:, c.use])
    # joint frames: the world axis and the moved link's origin, from the independent FK
    E = expm_fk(c, q + off)
    for i, l in enumerate(c.chain.link_order):
        col = int(c.table["qidx"][i])
        if col >= 0:
            a = np.asarray(c.chain._joint_of_child[l]["axis"])
            want = np.concatenate([E[:, i, :3, :3] @ (a / np.linalg.norm(a)), E[:, i, :3, 3]], axis=1)
            assert np.abs(jf[:, col] - want).max() <= 1e-12


@pytest.mark.parametrize("name", C.NAMES)
def test_upstream_bits_are_an_ancestor_walk(name):
    c = C.case(name)
    anc = C.ancestors(name)
    for k, li in enumerate(c.use):
        assert int(c.table["upstream"][k]) == sum(1 << j for j in anc[c.chain.link_order[li]]), (k, li)


@pytest.mark.parametrize("name", C.NAMES)
def test_analytic_derivative_is_the_central_difference(name):
    """Every link x every active joint of the case, against a central difference of the HOST's kinematics."""
    c = C.case(name)
    every = _links(c)
    t = c.chain.joint_table(every)
    J = c.chain.dof
    q, off = C.qpos(name, 2), C.offsets(name).astype(np.float64)
    _, lp, jf = JR.fk(t, q, off)
    D = JR.pose_derivatives(t, lp, jf)
    h, worst = 1e-6, 0.0
    for j in range(J):
        e = np.zeros(J)
        e[j] = h
        num = (c.chain.link_poses_batch(q + off + e, every) - c.chain.link_poses_batch(q + off - e, every)) / (2 * h)
        worst = max(worst, float(np.abs(D[:, :, j] - num).max()))
        up = np.array([(int(u) >> j) & 1 for u in t["upstream"]], dtype=bool)
        assert np.abs(num[:, ~up]).max(initial=0.0) == 0.0, j
        assert up.any() and np.abs(num[:, up]).max() > 0.0
    print(f"{name}: worst |D - central difference| = {worst:.2e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("name", C.NAMES)
def test_offset_gradient_is_the_chain_rule_through_fk(name):
    c = C.bwd_case(name, 2, 0)
    t, J = c["t"], c["J"]
    q, off, Tc = c["q"], c["off"].astype(np.float64), c["Tc"].astype(np.float64)
    g = np.random.default_rng(4).normal(size=c["g"].shape)      # (pairs of one size: a difference quotient has no digits to spare)
    cam = (c["K"], c["H"], c["W"], c["near"], c["far"])
    _, lp, jf = JR.fk(t, q, off)
    s, scale = JR.offset_gradient(t, g, Tc, *cam, lp, jf)
    f = lambda o: float((g * R.mvp(Tc, *cam, JR.fk(t, q, o)[1])).sum())
    for j in range(J):
        e = np.zeros(J)
        e[j] = 1e-6
        num = (f(off + e) - f(off - e)) / 2e-6
        assert abs(s[j] - num) <= 1e-7 * scale[j], (j, s[j], num)
    assert (scale >= np.abs(s)).all()
    if name == "tree":
        assert scale[4] == 0 and s[4] == 0 and (scale[[0, 1, 2, 3, 5, 6, 7]] > 0).all()


def test_the_boxes_of_the_branched_arm_are_closed():
    rb = C.tree_robot()
    assert rb.use_links == C.case("tree").use and rb.num_links == 7 and rb.num_tris == 84
    assert np.array_equal(rb.joint_table()["upstream"], C.case("tree").table["upstream"])
    for v, f in rb.meshes:
        assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == (8, 3) and f.shape == (12, 3)
        side = v.max(axis=0) - v.min(axis=0)
        assert (side >= 0.08 - 1e-6).all() and (side <= 0.15 + 1e-6).all()
        edges = {(int(a), int(b)) for tri in f for a, b in zip(tri, np.roll(tri, -1))}
        assert len(edges) == 36 and all((b, a) in edges for a, b in edges)       # every edge once in each direction
        vol = sum(float(np.linalg.det(v[tri].astype(np.float64))) for tri in f) / 6
        assert abs(vol - float(np.prod(side))) <= 1e-6 * vol                     # outward winding


# ---- sensitivity pins ----------------------------------------------------------------------------------------------------------
def wrong_fk(table, qpos, offset, mistake):
    """A copy of ``joint_reference.fk`` (float64) with ONE mistake:
      "hat_sign"    [a]x[2][1] = -ax instead of +ax in the sine term (an entry the packaged robots multiply by zero)
      "drop_axa"    the products ax * a_c and a_m * ax of [a]x^2 = a a^T - |a|^2 I left out
      "prismatic"   a prismatic joint moves its own link, but the links below hang from where the link was
      "parent"      every link hangs from the link before it"""
    q = np.atleast_2d(np.asarray(qpos, np.float64)) + np.asarray(offset, np.float64)[None]
    B, J = q.shape
    N = table["parent"].shape[0]
    origin, axis = table["origin"].reshape(N, 4, 4), table["axis"]
    frames, below = np.zeros((B, N, 4, 4)), np.zeros((B, N, 4, 4))
    jf = np.zeros((B, J, 6))
    for b in range(B):
        for i in range(N):
            p, k, c = int(table["parent"][i]), int(table["kind"][i]), int(table["qidx"][i])
            if mistake == "parent":
                p = i - 1
            Tp = np.eye(4) if p < 0 else below[b, p]
            M = np.eye(4)
            if c >= 0 and k == 1:
                a = axis[i]
                Kx = JR._hat(a, np.float64)
                K2 = Kx @ Kx
                if mistake == "hat_sign":
                    Kx = Kx.copy()
                    Kx[2, 1] = -Kx[2, 1]
                if mistake == "drop_axa":
                    aa = np.outer(a, a)
                    aa[0, :] = 0.0
                    aa[:, 0] = 0.0
                    K2 = aa - (a @ a) * np.eye(3)
                M[:3, :3] = np.eye(3) + np.sin(q[b, c]) * Kx + (1.0 - np.cos(q[b, c])) * K2
            elif c >= 0 and k == 2:
                M[:3, 3] = axis[i] * q[b, c]
            frames[b, i] = Tp @ origin[i] @ M
            below[b, i] = Tp @ origin[i] if (mistake == "prismatic" and k == 2) else frames[b, i]
            if c >= 0:
                jf[b, c, :3] = frames[b, i, :3, :3] @ axis[i]
                jf[b, c, 3:] = frames[b, i, :3, 3]
    return frames, frames[:, table["use"]], jf


def test_the_wrong_copy_with_no_mistake_is_the_reference():
    for name in ("skew_serial", "prismatic_mid", "tree"):
        c = C.case(name)
        q, off = C.qpos(name, 5), C.offsets(name)
        for a, b in zip(JR.fk(c.table, q, off), wrong_fk(c.table, q, off, None)):
            assert np.abs(a - b).max() <= 1e-14


def forward_misses(name, mistake):
    """(miss of link_poses / its bar, miss of joint_frames / its bar) of the wrong copy, measured as the GPU forward test
    measures the kernel, over its views (B = 1 and 5)."""
    c = C.case(name)
    r_lp, r_jf = 0.0, 0.0
    for B in (1, 5):
        q, off = C.qpos(name, B), C.offsets(name)
        _, lp64, jf64 = JR.fk(c.table, q, off)
        _, _, jf32 = JR.fk(c.table, q, off, dtype=F32)
        _, lpw, jfw = wrong_fk(c.table, q, off, mistake)
        want = lp64.astype(np.float32)
        d_lp = float((np.abs(lpw.astype(np.float32).astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
        s = float(np.abs(jf64).max())
        e32, ew = R.rel_err(jf32, jf64, s), R.rel_err(jfw.astype(np.float32), jf64, s)
        r_lp, r_jf = max(r_lp, d_lp / U), max(r_jf, ew / R.bound(e32))
    return r_lp, r_jf


@pytest.mark.parametrize("name,mistake", [("skew_serial", "hat_sign"), ("skew_serial", "drop_axa"), ("prismatic_mid", "prismatic"),
                                          ("tree", "parent")])
def test_a_wrong_forward_kernel_would_miss_the_bar_a_hundredfold(name, mistake):
    r_lp, r_jf = forward_misses(name, mistake)
    print(f"{name} with {mistake}: link_poses miss {r_lp:.3g} x its bar, joint_frames miss {r_jf:.3g} x its bar")
    assert r_lp >= 100.0 and r_jf >= 100.0
    # ... and neither packaged robot's table would have shown the first two: no revolute axis there has an x component
    if mistake in ("hat_sign", "drop_axa"):
        from easyhec_amd.robot import load_robot
        for rb in ("xarm7", "franka"):
            t = load_robot(rb).joint_table()
            q = np.random.default_rng(0).uniform(-1, 1, size=(3, int(t["qidx"].max()) + 1))
            for a, b in zip(JR.fk(t, q), wrong_fk(t, q, np.zeros(q.shape[1]), mistake)):
                assert np.abs(a - b).max() <= 1e-14


def wrong_upstream(table, mistake):
    """The table with ``upstream`` read wrongly:
      "low16"      only the low 16 bits are kept (a mask held in a half word)
      "smear"      the mask is a SIGNED int shifted right arithmetically: bit 31 smears over the word, and a link with
                   joint 31 upstream has every joint upstream.  (A read that keeps ONE bit of a shift by j <= 31 is the same
                   for either shift; the smear shows where more than that bit is kept, and this is its full extent.)
      "prismatic"  a prismatic joint is upstream of the link it moves only, not of the links below"""
    t = dict(table)
    up = np.asarray(table["upstream"]).astype(np.uint32)
    if mistake == "low16":
        t["upstream"] = up & np.uint32(0xFFFF)
    elif mistake == "smear":
        t["upstream"] = up | (up.view(np.int32) >> 31).view(np.uint32)
    elif mistake == "prismatic":
        out = up.copy()
        for k, li in enumerate(table["use"]):
            for i in range(table["parent"].shape[0]):
                if table["kind"][i] == 2 and table["qidx"][i] >= 0 and i != li:
                    out[k] &= ~np.uint32(1 << int(table["qidx"][i]))
        t["upstream"] = out
    else:
        raise ValueError(mistake)
    return t


def gradient_miss(name, mistake, B, pattern="all"):
    """The wrong copy's offset gradient against the true one, over the bar of the GPU gradient test on that case."""
    worst = 0.0
    for draw in range(2):
        c = C.bwd_case(name, B, draw, pattern)
        _, lp64, jf64 = JR.fk(c["t"], c["q"], c["off"])
        lp, jf = lp64.astype(np.float32), jf64.astype(np.float32)              # what the forward kernel hands on
        args = (c["g"], c["Tc"], c["K"], c["H"], c["W"], c["near"], c["far"], lp, jf)
        s64, scale = JR.offset_gradient(c["t"], *args)
        s32, _ = JR.offset_gradient(c["t"], *args, dtype=F32)
        sw, _ = JR.offset_gradient(wrong_upstream(c["t"], mistake), *args)
        live = c["free"].astype(bool) & (scale > 0)
        e32 = R.rel_err(s32[live], s64[live], scale[live])
        worst = max(worst, R.rel_err(sw[live], s64[live], scale[live]) / R.bound(e32))
    return worst


@pytest.mark.parametrize("name,mistake,B", [("full", "low16", 9), ("full", "smear", 9), ("prismatic_mid", "prismatic", 5)])
def test_a_wrong_upstream_mask_would_miss_the_gradient_s_bar_a_hundredfold(name, mistake, B):
    r = gradient_miss(name, mistake, B)
    print(f"{name} with {mistake}: offset gradient miss {r:.3g} x its bar")
    assert r >= 100.0
    t = C.case(name).table
    assert not np.array_equal(wrong_upstream(t, mistake)["upstream"], t["upstream"])
    from easyhec_amd.robot import load_robot
    for rb in ("xarm7", "franka"):                                               # the packaged tables: no such mask to get wrong
        t = load_robot(rb).joint_table()
        assert np.array_equal(wrong_upstream(t, mistake)["upstream"], t["upstream"])
