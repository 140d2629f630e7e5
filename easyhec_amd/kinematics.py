"""Forward kinematics of a URDF serial chain -- the producer of the hot path's ``link_poses`` input.

The reference obtains link poses from SAPIEN/Pinocchio
(/root/reference/easyhec/structures/sapien_kin.py:26-30, called per frame and link in
/root/reference/easyhec/data/datasets/xarm_real.py:42-56).  Only revolute/prismatic/fixed joints of a tree whose
root is fixed at the identity are needed for the xArm7 and Franka URDFs, so that is what is implemented.
Link indices follow SAPIEN's articulation order, which for these URDFs is the order in which <link> elements are
reached by a breadth-first walk from the root (== document order for the arm links).
"""
import xml.etree.ElementTree as ET

import numpy as np

__all__ = ["UrdfChain", "rpy_to_matrix"]


def rpy_to_matrix(rpy):
    r, p, y = [float(v) for v in rpy]
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], dtype=np.float64)


def _origin(elem):
    T = np.eye(4)
    if elem is not None:
        T[:3, :3] = rpy_to_matrix((elem.get("rpy") or "0 0 0").split())
        T[:3, 3] = [float(v) for v in (elem.get("xyz") or "0 0 0").split()]
    return T


def _axis_angle(axis, q):
    a = np.asarray(axis, dtype=np.float64)
    a = a / (np.linalg.norm(a) + 1e-30)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(4)
    R[:3, :3] = np.eye(3) + np.sin(q) * K + (1 - np.cos(q)) * (K @ K)
    return R


class UrdfChain:
    """Minimal URDF kinematic tree: ``compute_forward_kinematics(qpos) -> {link_name: 4x4}``."""

    def __init__(self, urdf_path=None, spec=None):
        if spec is None:
            spec = self.parse(urdf_path)
        self.links = list(spec["links"])
        self.joints = [dict(j) for j in spec["joints"]]
        for j in self.joints:
            j["origin"] = np.asarray(j["origin"], dtype=np.float64).reshape(4, 4)
            j["axis"] = np.asarray(j["axis"], dtype=np.float64)
        children = {j["child"] for j in self.joints}
        roots = [l for l in self.links if l not in children]
        self.root = roots[0]
        # articulation order: BFS from the root, joints in document order
        order, queue = [], [self.root]
        self._joint_of_child = {j["child"]: j for j in self.joints}
        while queue:
            l = queue.pop(0)
            order.append(l)
            queue.extend(j["child"] for j in self.joints if j["parent"] == l)
        self.link_order = order
        self.active = [self._joint_of_child[l] for l in order if l in self._joint_of_child and
                       self._joint_of_child[l]["type"] in ("revolute", "continuous", "prismatic")]
        self.dof = len(self.active)

    @staticmethod
    def parse(urdf_path):
        root = ET.parse(urdf_path).getroot()
        links = [l.get("name") for l in root.findall("link")]
        joints = []
        for j in root.findall("joint"):
            ax = j.find("axis")
            lim = j.find("limit")
            joints.append({
                "name": j.get("name"), "type": j.get("type"),
                "parent": j.find("parent").get("link"), "child": j.find("child").get("link"),
                "origin": _origin(j.find("origin")).tolist(),
                "axis": [float(v) for v in (ax.get("xyz") if ax is not None else "1 0 0").split()],
                "lower": float(lim.get("lower", "0")) if lim is not None else 0.0,
                "upper": float(lim.get("upper", "0")) if lim is not None else 0.0,
            })
        return {"links": links, "joints": joints}

    def spec(self):
        return {"links": self.links,
                "joints": [{**{k: v for k, v in j.items() if k not in ("origin", "axis")},
                            "origin": j["origin"].tolist(), "axis": j["axis"].tolist()} for j in self.joints]}

    def limits(self):
        return np.array([[j["lower"], j["upper"]] for j in self.active], dtype=np.float64)

    def compute_forward_kinematics(self, qpos):
        """qpos: ``dof`` joint values in articulation order (shorter vectors are zero-padded, as
        xarm_real.py:47-48 does).  Returns {link name: base<-link 4x4 float64}."""
        q = np.zeros(self.dof)
        qpos = np.asarray(qpos, dtype=np.float64).reshape(-1)
        q[:min(self.dof, qpos.size)] = qpos[:self.dof]
        qmap = {id(j): q[i] for i, j in enumerate(self.active)}
        poses = {self.root: np.eye(4)}
        for l in self.link_order[1:]:
            j = self._joint_of_child[l]
            T = poses[j["parent"]] @ j["origin"]
            if j["type"] in ("revolute", "continuous"):
                T = T @ _axis_angle(j["axis"], qmap[id(j)])
            elif j["type"] == "prismatic":
                P = np.eye(4)
                P[:3, 3] = j["axis"] / (np.linalg.norm(j["axis"]) + 1e-30) * qmap[id(j)]
                T = T @ P
            poses[l] = T
        return poses

    def mount_index(self, mount):
        """The node (articulation index) of a mount given as one, or as a link name."""
        if isinstance(mount, str):
            if mount not in self.link_order:
                raise ValueError(f"mount {mount!r} is not a link of this chain")
            return self.link_order.index(mount)
        m = int(mount)
        if not 0 <= m < len(self.link_order):
            raise ValueError(f"mount {mount} is not a link index of this chain (0..{len(self.link_order) - 1})")
        return m

    @staticmethod
    def in_mount_frame(Fm, Fl):
        """inv(Fm) @ Fl for rigid [...,4,4] float64 frames by the formula of the mounted forward kernel
        (csrc/ehr_joint_core.h): R = R_m^T R_l, t = R_m^T (t_l - t_m), the difference first."""
        out = np.array(Fl, dtype=np.float64, copy=True)
        RmT = np.swapaxes(Fm[..., :3, :3], -1, -2)
        out[..., :3, :3] = RmT @ Fl[..., :3, :3]
        out[..., :3, 3] = (RmT @ (Fl[..., :3, 3] - Fm[..., :3, 3])[..., None])[..., 0]
        return out

    def link_poses_batch(self, qposes, link_indices, mount=None):
        """[N, len(link_indices), 4, 4] float64 for N joint vectors at once (same arithmetic as
        :meth:`compute_forward_kinematics`, vectorised over the batch: the space explorer needs FK of ~1000 candidate
        configurations per round, space_explorer.py:98-150).  mount (a link index or name; default None: the base frame):
        the poses are mount<-link, ``inv(F_mount) @ F_link``, for a camera that rides on that link."""
        Q = np.atleast_2d(np.asarray(qposes, dtype=np.float64))
        N = Q.shape[0]
        q = np.zeros((N, self.dof))
        q[:, :min(self.dof, Q.shape[1])] = Q[:, :self.dof]
        col = {id(j): i for i, j in enumerate(self.active)}
        eye = np.broadcast_to(np.eye(4), (N, 4, 4))
        poses = {self.root: eye}
        for l in self.link_order[1:]:
            j = self._joint_of_child[l]
            T = poses[j["parent"]] @ j["origin"]
            if j["type"] in ("revolute", "continuous"):
                a = j["axis"] / (np.linalg.norm(j["axis"]) + 1e-30)
                Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                ang = q[:, col[id(j)]]
                R = np.tile(np.eye(4), (N, 1, 1))
                R[:, :3, :3] = np.eye(3) + np.sin(ang)[:, None, None] * Kx + (1 - np.cos(ang))[:, None, None] * (Kx @ Kx)
                T = T @ R
            elif j["type"] == "prismatic":
                P = np.tile(np.eye(4), (N, 1, 1))
                P[:, :3, 3] = (j["axis"] / (np.linalg.norm(j["axis"]) + 1e-30))[None] * q[:, col[id(j)], None]
                T = T @ P
            poses[l] = T
        out = np.stack([poses[self.link_order[i]] for i in link_indices], axis=1).astype(np.float64)
        if mount is not None:
            out = self.in_mount_frame(np.asarray(poses[self.link_order[self.mount_index(mount)]], np.float64)[:, None], out)
        return out

    def joint_table(self, link_indices, mount=None):
        """The tree as flat arrays in articulation order (N = ``len(link_order)``, J = ``dof``, L = ``len(link_indices)``):
        what the joint-offset kernels (csrc/ehr_joint.hip) and tests/joint_reference.py walk instead of this object.

        ``parent [N] int32`` (-1 for the root; a parent precedes its child), ``origin [N,16] float64`` (row-major joint
        origin; identity for the root), ``kind [N] int32`` (0 fixed, 1 revolute / continuous, 2 prismatic), ``axis [N,3]
        float64`` (unit), ``qidx [N] int32`` (column of the active joint that moves the link, or -1), ``use [L] int32``
        (the rendered links), ``upstream [L] uint32`` (bit j: active joint j lies between the root and rendered link l).
        With these, ``T_child = T_parent @ origin @ motion(q[qidx])`` is :meth:`compute_forward_kinematics`.

        mount (a link index or name; default None: exactly the table above, no further keys): the table of a camera that
        rides on that link.  It adds ``mount`` (the node), ``mount_upstream`` (uint32, bit j: active joint j lies between
        the root and the mount) and ``upstream_base`` (the mask above), and ``upstream`` becomes the RELATIVE mask
        ``upstream_base ^ mount_upstream``: the joints on exactly one side of the pair (mount, link), which are the ones
        that move the link in the mount's frame.  Every reader of ``table["upstream"]`` gets the right one."""
        N, J = len(self.link_order), self.dof
        if N > 64 or J > 32:
            raise ValueError(f"joint_table: {N} links / {J} active joints exceed the limits of 64 links and 32 joints")
        index = {l: i for i, l in enumerate(self.link_order)}
        col = {id(j): i for i, j in enumerate(self.active)}
        kinds = {"fixed": 0, "revolute": 1, "continuous": 1, "prismatic": 2}
        parent = np.full(N, -1, dtype=np.int32)
        origin = np.tile(np.eye(4).reshape(16), (N, 1))
        kind = np.zeros(N, dtype=np.int32)
        axis = np.tile(np.array([1.0, 0.0, 0.0]), (N, 1))
        qidx = np.full(N, -1, dtype=np.int32)
        for i, l in enumerate(self.link_order[1:], start=1):
            j = self._joint_of_child[l]
            if j["type"] not in kinds:
                raise ValueError(f"joint_table: joint {j['name']!r} has unsupported type {j['type']!r}")
            parent[i] = index[j["parent"]]
            assert parent[i] < i
            origin[i] = j["origin"].reshape(16)
            kind[i] = kinds[j["type"]]
            if kind[i]:  # (a fixed joint keeps the placeholder: its axis is never used, and a URDF may give it as 0 0 0)
                axis[i] = j["axis"] / (np.linalg.norm(j["axis"]) + 1e-30)
            qidx[i] = col.get(id(j), -1)
        use = np.asarray(list(link_indices), dtype=np.int32)
        if use.size and (use.min() < 0 or use.max() >= N):
            raise ValueError("joint_table: link index out of range")
        upstream = np.zeros(use.size, dtype=np.uint32)
        for k, i in enumerate(use):
            while i >= 0:
                if qidx[i] >= 0:
                    upstream[k] |= np.uint32(1) << np.uint32(qidx[i])
                i = parent[i]
        table = {"parent": parent, "origin": origin, "kind": kind, "axis": axis, "qidx": qidx, "use": use,
                 "upstream": upstream}
        if mount is not None:
            m = self.mount_index(mount)
            mu, i = np.uint32(0), m
            while i >= 0:
                if qidx[i] >= 0:
                    mu |= np.uint32(1) << np.uint32(qidx[i])
                i = parent[i]
            table.update(mount=m, mount_upstream=mu, upstream_base=upstream, upstream=upstream ^ mu)
        return table

    def link_poses(self, qpos, link_indices, mount=None):
        """[len(link_indices),4,4] poses for SAPIEN-style link indices (``use_links`` in the reference configs); mount<-link
        with ``mount`` (see :meth:`link_poses_batch`)."""
        poses = self.compute_forward_kinematics(qpos)
        out = np.stack([poses[self.link_order[i]] for i in link_indices]).astype(np.float64)
        if mount is not None:
            out = self.in_mount_frame(poses[self.link_order[self.mount_index(mount)]][None], out)
        return out
