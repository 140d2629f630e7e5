"""What the job kernel's walkers walk, counted on the CPU: a numpy restatement of the job stage of csrc/ehr_vbuf.hip on a
bench workload's own inputs (make_views(seed=0), the perturbed initial pose), with and without the box trim (the staging
block of vb_raster_round).
    python tools/box_trim_count.py [workload] [views, e.g. 0,3]
It models the plan's clusters (vb_kd_order), the cluster-box and triangle-box culls, rounds of 64 survivors, the interior
skip and the all-interior exit, and prices a job the way the kernel's hint does as if every box took the unit walker:
units walked + 256 per round.  It does not model the span walker, the depth tests, unsafe (kind 2) triangles or the
general-triangle pass (a robot in front of the camera has none of the last two).  Every trimmed box is checked: no covered
pixel may lie outside it.  Needs no GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
from easyhec_amd.robot import load_robot  # noqa: E402
from easyhec_amd.synthetic import WORKLOADS, camera_Tc_c2b, make_views, perturb_pose  # noqa: E402

TW, TH, RW, RH, SMALL = 32, 8, 34, 10, 3


def kd_order(cen, idx):
    """vb_kd_order: median split along the longest axis, the left part a multiple of 64, ties by index."""
    n = len(idx)
    if n <= 64:
        return idx
    c = cen[idx]
    ax = 0
    ext = c.max(0) - c.min(0)
    if ext[1] > ext[ax]:
        ax = 1
    if ext[2] > ext[ax]:
        ax = 2
    half = min(max(((n // 2 + 63) // 64) * 64, 64), n - 1)
    o = np.lexsort((idx, c[:, ax]))
    return np.concatenate([kd_order(cen, np.sort(idx[o[:half]])), kd_order(cen, np.sort(idx[o[half:]]))])


def clusters(v, f):
    """-> [nc, 64] triangle ids of one link (-1 = padding), in the plan's order."""
    v = v.astype(np.float32)
    cen = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) * np.float32(1.0 / 3.0)
    order = kd_order(cen, np.arange(len(f)))
    pad = (-len(order)) % 64
    return np.concatenate([order, np.full(pad, -1, order.dtype)]).reshape(-1, 64)


def records(v, f, M, W, H):
    """Per triangle of one (view, link): box [n,4] (x0 > x1: none) and the edge values at the box's first pixel with their
    steps (e [n,3], sx [n,3], sy [n,3]), as setup_coverage / vb_edges make them."""
    p = np.concatenate([v.astype(np.float32), np.ones((len(v), 1), np.float32)], 1) @ M.astype(np.float32).T
    X = np.rint((p[:, 0] / p[:, 3]) * np.float32(W * 8)).astype(np.int64)
    Y = np.rint((p[:, 1] / p[:, 3]) * np.float32(H * 8)).astype(np.int64)
    X, Y = X[f], Y[f]
    area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    sw = area2 < 0
    X[sw, 1], X[sw, 2] = X[sw, 2].copy(), X[sw, 1].copy()
    Y[sw, 1], Y[sw, 2] = Y[sw, 2].copy(), Y[sw, 1].copy()
    cx, cy = 8 - 8 * W, 8 - 8 * H
    x0 = np.maximum((X.min(1) - cx + 15) >> 4, 0)
    x1 = np.minimum((X.max(1) - cx) >> 4, W - 1)
    y0 = np.maximum((Y.min(1) - cy + 15) >> 4, 0)
    y1 = np.minimum((Y.max(1) - cy) >> 4, H - 1)
    valid = (area2 != 0) & (x0 <= x1) & (y0 <= y1) & (p[f, 3] > 0).all(1)
    Px, Py = 16 * x0 + cx, 16 * y0 + cy
    e, sx, sy = [np.zeros((len(f), 3), np.int64) for _ in range(3)]
    for k in range(3):
        j = (k + 1) % 3
        dX, dY = X[:, j] - X[:, k], Y[:, j] - Y[:, k]
        tl = (dY < 0) | ((dY == 0) & (dX < 0))
        e[:, k] = dX * (Py - Y[:, k]) - dY * (Px - X[:, k]) - np.where(tl, 0, 1)
        sx[:, k], sy[:, k] = -16 * dY, 16 * dX
    # the vertex kernel's exact test of the small boxes
    small = valid & (x1 - x0 < SMALL) & (y1 - y0 < SMALL)
    any_px = np.zeros(len(f), bool)
    for j in range(SMALL):
        for i in range(SMALL):
            inside = ((e + i * sx + j * sy) >= 0).all(1) & (i <= x1 - x0) & (j <= y1 - y0)
            any_px |= inside
    valid &= ~small | any_px
    box = np.stack([np.where(valid, x0, 65535), np.where(valid, y0, 65535), np.where(valid, x1, 0), np.where(valid, y1, 0)], 1)
    return box, e, sx, sy


def trim(e, sx, sy, bw, bh):
    """The trim rule on one box: -> (i0, j0, bw', bh'), empty if a size is <= 0.  Exact integer bounds."""
    def rng(m, s, n):
        lo, hi = 0, n - 1
        for mk, sk in zip(m, s):
            if sk > 0:
                lo = max(lo, -(mk // sk))            # ceil(-m / s)
            elif sk < 0:
                hi = min(hi, mk // -sk)              # floor(m / |s|); negative when m < 0
            elif mk < 0:
                hi = -1
        return lo, hi
    j0, j1 = rng([int(ek + max(0, sk * (bw - 1))) for ek, sk in zip(e, sx)], [int(s) for s in sy], bh)
    if j0 > j1:
        return 0, 0, 0, 0
    e = [int(ek + j0 * sk) for ek, sk in zip(e, sy)]
    i0, i1 = rng([ek + max(0, int(sk) * (j1 - j0)) for ek, sk in zip(e, sy)], [int(s) for s in sx], bw)
    return i0, j0, i1 - i0 + 1, j1 - j0 + 1


def interior(cov):
    c = np.pad(cov, 1, constant_values=True)   # past the region's edge counts as covered
    return cov & c[1:-1, :-2] & c[1:-1, 2:] & c[:-2, 1:-1] & c[2:, 1:-1]


def job(surv, box, e, sx, sy, rg, st, do_trim):
    """One job: `surv` = the triangles that passed the box culls, in order; rg = (x0, y0, x1, y1) of the region inside the
    image.  -> cost.  Counts go to the dict `st`."""
    rx0, ry0 = rg[4], rg[5]
    cov = np.zeros((RH, RW), bool)
    cost = 0
    for r0 in range(0, len(surv), 64):
        intr = interior(cov)
        if intr.all():
            break
        st["rounds"] += 1
        cost += 256
        new = []
        for t in surv[r0:r0 + 64]:
            cx0, cy0 = max(box[t, 0], rg[0]), max(box[t, 1], rg[1])
            bw, bh = min(box[t, 2], rg[2]) - cx0 + 1, min(box[t, 3], rg[3]) - cy0 + 1
            ek = e[t] + (cx0 - box[t, 0]) * sx[t] + (cy0 - box[t, 1]) * sy[t]
            ii, jj = np.meshgrid(np.arange(bw), np.arange(bh))
            ins = ((ek[None, None, :] + ii[..., None] * sx[t] + jj[..., None] * sy[t]) >= 0).all(2)
            if do_trim:
                i0, j0, tw, th = trim(ek, sx[t], sy[t], bw, bh)
                keep = np.zeros_like(ins)
                keep[j0:j0 + max(th, 0), i0:i0 + max(tw, 0)] = True
                assert not (ins & ~keep).any(), "the trim dropped a covered pixel"
                if tw <= 0 or th <= 0:
                    st["empty"] += 1
                    continue
                ins = ins[j0:j0 + th, i0:i0 + tw]
                cx0, cy0, bw, bh = cx0 + i0, cy0 + j0, tw, th
            x, y = cx0 - rx0, cy0 - ry0
            if intr[y:y + bh, x:x + bw].all():
                st["hidden"] += 1
                continue
            gw = (bw + 3) // 4
            st["tris"] += 1
            st["tris_no_pixel"] += not ins.any()
            st["units"] += gw * bh
            st["units_no_pixel_tri"] += 0 if ins.any() else gw * bh
            st["rows"] += bh
            st["rows_covered"] += int(ins.any(1).sum())
            padded = np.zeros((bh, gw * 4), bool)
            padded[:, :bw] = ins
            st["units_covered"] += int(padded.reshape(bh, gw, 4).any(2).sum())
            if gw >= 4:
                st["wide_rows"] += bh
                st["wide_rows_covered"] += int(ins.any(1).sum())
            cost += gw * bh
            new.append((y, x, ins))
        for y, x, ins in new:
            cov[y:y + ins.shape[0], x:x + ins.shape[1]] |= ins
    return cost


def count(workload, views, do_trim):
    wl = WORKLOADS[workload]
    rb = load_robot(wl["robot"])
    H, W = wl["H"], wl["W"]
    _, lp = make_views(rb, wl["views"], seed=0)
    Tc = perturb_pose(camera_Tc_c2b(radius=wl["radius"], lift=wl["lift"]))
    mvp = helpers.mvp_numpy(np.asarray(wl["K"], np.float64), H, W, Tc, lp)
    cl = [clusters(v, f) for v, f in rb.meshes]
    st = dict.fromkeys(["rounds", "tris", "tris_no_pixel", "units", "units_no_pixel_tri", "units_covered", "rows", "rows_covered",
                        "wide_rows", "wide_rows_covered", "hidden", "empty", "pairs", "jobs"], 0)
    costs = []
    for b in views:
        for l, (v, f) in enumerate(rb.meshes):
            box, e, sx, sy = records(v, f, mvp[b, l], W, H)
            ok = box[:, 0] <= box[:, 2]
            if not ok.any():
                continue
            cb = []
            for c in cl[l]:
                t = c[c >= 0]
                t = t[ok[t]]
                cb.append((box[t, 0].min(), box[t, 1].min(), box[t, 2].max(), box[t, 3].max()) if len(t) else (65535, 65535, 0, 0))
            lb = (box[ok, 0].min(), box[ok, 1].min(), box[ok, 2].max(), box[ok, 3].max())
            for ty in range(max(lb[1] - 1, 0) // TH, min(lb[3] + 1, H - 1) // TH + 1):
                for tx in range(max(lb[0] - 1, 0) // TW, min(lb[2] + 1, W - 1) // TW + 1):
                    rx0, ry0 = tx * TW - 1, ty * TH - 1
                    rg = (max(rx0, 0), max(ry0, 0), min(rx0 + RW - 1, W - 1), min(ry0 + RH - 1, H - 1), rx0, ry0)
                    surv = []
                    for c, bx in zip(cl[l], cb):
                        if bx[0] <= rg[2] and bx[2] >= rg[0] and bx[1] <= rg[3] and bx[3] >= rg[1]:
                            st["pairs"] += 1
                            t = c[c >= 0]
                            m = (box[t, 0] <= rg[2]) & (box[t, 2] >= rg[0]) & (box[t, 1] <= rg[3]) & (box[t, 3] >= rg[1])
                            surv.extend(t[m].tolist())
                    st["jobs"] += 1
                    if surv:
                        costs.append(job(surv, box, e, sx, sy, rg, st, do_trim))
    return st, np.sort(np.asarray(costs))[::-1]


if __name__ == "__main__":
    workload = sys.argv[1] if len(sys.argv) > 1 else "xarm7_1280x720_8view"
    views = [int(s) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [0, 3]
    print(f"{workload}, views {views}")
    for do_trim in (False, True):
        st, costs = count(workload, views, do_trim)
        print("--- with the trim" if do_trim else "--- clamped boxes (no trim)")
        print(f"cluster-tile pairs per view {st['pairs'] / len(views):.0f}, jobs per view {st['jobs'] / len(views):.0f}, rounds {st['rounds']}")
        print(f"triangles walked {st['tris']} (cover no pixel of the region: {st['tris_no_pixel']}, their units {st['units_no_pixel_tri']}); "
              f"hidden {st['hidden']}, trimmed to nothing {st['empty']}")
        print(f"box rows walked {st['rows']} (with a covered pixel {st['rows_covered']}); of boxes >= 4 units wide {st['wide_rows']} ({st['wide_rows_covered']})")
        print(f"units walked {st['units']} (with a covered pixel {st['units_covered']})")
        print(f"summed job cost {costs.sum()}, the 100 most expensive {costs[:100].sum()}, largest {costs[0]}, "
              f"jobs >= 1500: {(costs >= 1500).sum()}, >= 2500: {(costs >= 2500).sum()}")
