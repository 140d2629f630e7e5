"""Launches the forward kinematics kernels on xArm7 at B views, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/mounted_forward_trace.py [--lib PATH]

``joint_forward_kernel`` (the camera in the base frame) and, where the library has it, ``joint_forward_mounted_kernel`` (the
camera on link7) are each launched ``--launches`` times after a warm-up on the same inputs; the per-kernel figures are the
trace's.  ``--lib``: another build of the same ABI (the parent commit's, which has the base kernel only).  Binds the two
entries itself: ``easyhec_amd._lib`` would refuse a library that lacks a symbol the header declares."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "easyhec_amd", "libehr_hip.so"))
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    from easyhec_amd.robot import load_robot
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    so = ctypes.CDLL(a.lib)
    rb = load_robot("xarm7")
    t = rb.mounted("link7").joint_table()
    J, N, L, B = int(rb.chain.dof), int(t["parent"].shape[0]), len(t["use"]), a.views
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    tab = [up(t[k], dt) for k, dt in (("parent", np.int32), ("origin", np.float64), ("kind", np.int32), ("axis", np.float64),
                                      ("qidx", np.int32), ("use", np.int32))]
    q = np.zeros((B, J))
    q[:, :7] = rb.sample_qpos(B, np.random.default_rng(0))
    qd, od = up(q, np.float64), torch.zeros(J, device=dev)
    lp, jf = torch.empty((B, L, 4, 4), device=dev), torch.empty((B, J, 6), device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    I, V, U32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32
    so.ehr_joint_forward.argtypes = [V] * 6 + [I] * 3 + [V, V, I, V, V, V]
    calls = [lambda: so.ehr_joint_forward(*[p(x) for x in tab], N, J, L, p(qd), p(od), B, p(lp), p(jf), stream)]
    if hasattr(so, "ehr_joint_forward_mounted"):
        so.ehr_joint_forward_mounted.argtypes = [V] * 6 + [I] * 4 + [U32, V, V, I, V, V, V]
        m, um = int(t["mount"]), int(t["mount_upstream"])
        calls.append(lambda: so.ehr_joint_forward_mounted(*[p(x) for x in tab], N, J, L, m, um, p(qd), p(od), B, p(lp), p(jf),
                                                          stream))
    for call in calls:
        for _ in range(20 + a.launches):
            assert call() == 0
        torch.cuda.synchronize()
    print(f"{len(calls)} kernels x {a.launches} launches after 20 of warm-up, B = {B}, N = {N}, J = {J}, L = {L}")


if __name__ == "__main__":
    main()
