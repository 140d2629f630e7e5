"""ehr_mask_information (vb_info_kernel and its two reduction kernels, csrc/ehr_vbuf.hip) through
easyhec_amd.information.mask_information on the cases of tests/info_scene_cases.py: 1 .. 32 links, empty links, U = 512 in
one chunk and 513 in two, 74 views in chunks of 73 + 1, images smaller than a tile, the flagged stack, the N at which the
launch drops from 4 to 2 to 1 waves per workgroup, weights across a chunk border, the eager and the lazy vertex form, the
heavy-job hint and the refusals.  Every value is held against the float64 reference under information_reference.check
(2 C_J(L) u S, (C_J(L) + 1) u Sg, exact count); everything else is bit equality or exact zero.  No tolerance of its own.
tests/test_info_scene_cases.py pins the cases on the CPU.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import info_scene_cases as C
import information_reference as IR
from test_gpu_fused_loss import link_scene, stateless
from test_gpu_information import call, same
from test_gpu_link_scenes import tiny_scene

pytestmark = pytest.mark.gpu

_SCENES = {}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused, information
    return fused, information, dr, torch.device("cuda:0")


def device_scene(fused, case, dev):
    if case not in _SCENES:
        _SCENES[case] = link_scene(fused, C.scene_of(case), dev)
    return _SCENES[case]


def run(env, oracle, case, D, ctx=None, weight=None, want_loss=False, views=None):
    """One mask_information of the case (``views``: a slice of them) -> numpy namespace."""
    fused, I, dr, dev = env
    e0 = C.expected0(oracle, case)
    sl = slice(None) if views is None else views
    return call(I, dr.RasterizeCudaContext() if ctx is None else ctx, device_scene(fused, case, dev), e0.s.mvp[sl], D[:, sl],
                e0.ref[sl], dev, weight=weight, want_loss=want_loss)


def check_zero_rows_of_empty_links(env, oracle, case, D, out, ctx):
    """Tangent 1 kept on the empty links alone (and made large there): its row, column and gradient entry are exact zeros,
    every other entry keeps its bits."""
    dead = C.empty_links(C.scene_of(case))
    if not dead.any():
        return
    Dz = D.copy()
    Dz[1][:, ~dead] = 0
    Dz[1][:, dead] *= 1e6
    z = run(env, oracle, case, Dz, ctx)
    keep = [k for k in range(D.shape[0]) if k != 1]
    assert (z.info[:, 1] == 0).all() and (z.info[:, :, 1] == 0).all() and (z.grad[:, 1] == 0).all(), case
    assert (z.info[:, keep][:, :, keep] == out.info[:, keep][:, :, keep]).all() and (z.grad[:, keep] == out.grad[:, keep]).all(), case


# ---- a. parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES)
def test_parity_at_six_tangents(env, oracle, case):
    """count exact, every info and grad entry within its derived bar, the z translation's row and column exactly zero (no
    scale), sub_1x1 all zero, and exact zeros where only empty links could contribute."""
    fused, I, dr, dev = env
    D, _, e = C.expected(oracle, case, 6)
    assert (e.count == e.count_max).all()
    ctx = dr.RasterizeCudaContext()
    out = run(env, oracle, case, D, ctx)
    IR.check(out.info, out.grad, out.count, e, f"parity {case} N=6")
    assert (out.count == e.count).all()
    assert (out.info[:, 2] == 0).all() and (out.info[:, :, 2] == 0).all() and (out.grad[:, 2] == 0).all()
    assert (out.info == out.info.transpose(0, 2, 1)).all()
    if case in C.ALL_ZERO:
        assert (out.info == 0).all() and (out.grad == 0).all() and (out.count == 0).all()
    else:
        assert (e.count > 0).all() and (out.info[:, 0, 0] > 0).all()
    check_zero_rows_of_empty_links(env, oracle, case, D, out, ctx)


@pytest.mark.parametrize("N", [1, 32])
@pytest.mark.parametrize("case", C.MANY_N)
def test_parity_at_one_and_thirty_two_tangents(env, oracle, case, N):
    D, _, e = C.expected(oracle, case, N)
    out = run(env, oracle, case, D)
    IR.check(out.info, out.grad, out.count, e, f"parity {case} N={N}")
    assert (e.count > 0).all() and (e.S > 0).any()
    if N == 32:
        assert (out.info[:, 2] == 0).all() and (out.info[:, :, 2] == 0).all() and (out.grad[:, 2] == 0).all()


# ---- b. the wave counts of the launch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.THRESHOLDS))
def test_wave_count_thresholds(env, oracle, case):
    """The N on both sides of every drop of the waves per workgroup (4 -> 2 -> 1), each against the reference of its own
    tangents; and the call with N tangents reproduces, bit for bit, the n x n block, the first n gradient entries and the
    count of the call with its first n (the extra tangents add only pixels that contribute an exact zero to those entries;
    the six generators already reach every pixel with a pair, so count does not move: asserted on the reference)."""
    fused, I, dr, dev = env
    Ns = C.THRESHOLDS[case]
    s = C.scene_of(case)
    D, refs = C.nested(oracle, case, Ns)
    ctx, prev, pn = dr.RasterizeCudaContext(), None, 0
    for n in Ns:
        nw = C.waves_per_workgroup(n, s.B * s.L)
        out = run(env, oracle, case, D[:n], ctx)
        IR.check(out.info, out.grad, out.count, refs[n], f"waves {case} N={n} ({nw} per workgroup)")
        assert (refs[n].count == refs[n].count_max).all() and (out.count == refs[n].count).all()
        if prev is not None:
            assert (refs[n].count == refs[pn].count).all()
            assert (out.info[:, :pn, :pn] == prev.info).all() and (out.grad[:, :pn] == prev.grad).all(), (case, pn, n)
            assert (out.count == prev.count).all(), (case, pn, n)
        prev, pn = out, n


# ---- c. chunk borders --------------------------------------------------------------------------------------------------------
BORDERS = [("units513", [(0, 3), (13, 16), (14, 17), (16, 17)]), ("prime7", [(0, 10), (63, 73), (64, 74), (73, 74)])]


@pytest.mark.parametrize("case,slices", BORDERS)
def test_chunk_borders(env, oracle, case, slices):
    """units513 goes through in chunks of 16 + 1 views, prime7 in 73 + 1: the call is held against the reference, and every
    view equals, bit for bit (loss included), the same view of single-chunk calls on a second context -- slices that end at
    the border, lie across it, and hold the last chunk's one view alone."""
    fused, I, dr, dev = env
    s = C.scene_of(case)
    bc = 512 // s.L
    assert bc < s.B <= 2 * bc and s.B - bc == 1
    assert any(hi == bc for _, hi in slices) and any(lo < bc < hi for lo, hi in slices) and (bc, s.B) in slices
    D, _, e = C.expected(oracle, case, 6)
    a = run(env, oracle, case, D, want_loss=True)
    IR.check(a.info, a.grad, a.count, e, f"chunks {case} N=6")
    small = dr.RasterizeCudaContext()
    for lo, hi in slices:
        sl = slice(lo, hi)
        p = run(env, oracle, case, D, small, want_loss=True, views=sl)
        assert (p.info == a.info[sl]).all() and (p.grad == a.grad[sl]).all() and (p.count == a.count[sl]).all(), (case, lo, hi)
        assert (p.loss == a.loss[sl]).all(), (case, lo, hi)


# ---- d. weights across the border --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kinds", [("units513", ("real", "shared")), ("prime7", ("real", "shared", "pair"))])
def test_weights_across_the_border(env, oracle, case, kinds):
    """A real-valued weight per view, one shared by every view and (prime7: 74 = 2 x 37) a pair of them, each against the
    reference with that weight; all-ones weights change no bit, all-zero weights leave nothing."""
    fused, I, dr, dev = env
    D, _, e = C.expected(oracle, case, 6)
    ctx = dr.RasterizeCudaContext()
    a = run(env, oracle, case, D, ctx, want_loss=True)
    IR.check(a.info, a.grad, a.count, e, f"weights none {case}")
    for kind in kinds:
        Dw, w, ew = C.expected(oracle, case, 6, weight=kind)
        out = run(env, oracle, case, Dw, ctx, weight=w)
        IR.check(out.info, out.grad, out.count, ew, f"weights {kind} {case}")
        assert (ew.count > 0).all() and not same(out, a)
    ones = run(env, oracle, case, D, ctx, weight=C.weight_of(case, "ones"), want_loss=True)
    assert same(a, ones) and (a.loss == ones.loss).all()
    zero = run(env, oracle, case, D, ctx, weight=C.weight_of(case, "zeros"))
    assert (zero.info == 0).all() and (zero.grad == 0).all() and (zero.count == 0).all()
    again = run(env, oracle, case, D, ctx, want_loss=True)                      # (and without weights again)
    assert same(a, again) and (a.loss == again.loss).all()


# ---- e. plans and repeated calls ---------------------------------------------------------------------------------------------
def test_eager_and_lazy_form_on_one_context(env, oracle):
    """full32 (shared vertices: the eager vertex form) and full32_lazy (three vertices per triangle: the lazy one) in turn on
    one context: each agrees with its own reference, and with itself from call to call."""
    fused, I, dr, dev = env
    ctx, first = dr.RasterizeCudaContext(), {}
    for case in ("full32", "full32_lazy", "full32", "full32_lazy"):
        D, _, e = C.expected(oracle, case, 6)
        out = run(env, oracle, case, D, ctx)
        IR.check(out.info, out.grad, out.count, e, f"forms {case} on a shared context")
        assert case not in first or same(first[case], out)
        first.setdefault(case, out)
    assert not same(first["full32"], first["full32_lazy"])


def test_heavy_job_hint_is_put_back(env, oracle):
    """flagged_stack("heavy"): the tile under the stack costs more than the heavy bar, so a second chain on a context hands
    it to a whole workgroup.  Three information calls with a render_mask_loss after each of the first two: the information
    results are bit-identical and the reference's; the fused results are those of a context that never ran the information
    op (which copies the hint aside and puts it back)."""
    fused, I, dr, dev = env
    case = "stack_heavy"
    e0 = C.expected0(oracle, case)
    D, _, e = C.expected(oracle, case, 6)
    scene = device_scene(fused, case, dev)
    ctx, plain = dr.RasterizeCudaContext(), dr.RasterizeCudaContext()
    infos, mine, theirs = [], [], []
    for i in range(3):
        infos.append(run(env, oracle, case, D, ctx, want_loss=True))
        if i < 2:
            mine.append(stateless(fused, ctx, scene, e0.s.mvp, e0.ref, dev))
            theirs.append(stateless(fused, plain, scene, e0.s.mvp, e0.ref, dev))
    IR.check(infos[0].info, infos[0].grad, infos[0].count, e, f"heavy {case} first call")
    for o in infos[1:]:
        assert same(infos[0], o) and (infos[0].loss == o.loss).all()
    for a, b in zip(mine, theirs):
        assert all((x == y).all() for x, y in zip(a, b))
    assert (infos[0].loss == mine[0][1]).all()
    assert (mine[0][0] == e0.m_ref).all()


# ---- f. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(env, oracle):
    fused, I, dr, dev = env
    D, _, e = C.expected(oracle, "full32", 6)
    e0 = C.expected0(oracle, "full32")
    ctx = dr.RasterizeCudaContext()
    base = run(env, oracle, "full32", D, ctx)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    scene, mvp, ref = device_scene(fused, "full32", dev), t(e0.s.mvp), t(e0.ref)

    def still_good(what):
        fused.check_status(ctx)
        out = run(env, oracle, "full32", D, ctx)
        IR.check(out.info, out.grad, out.count, e, f"refusals full32 after {what}")
        assert same(base, out)

    s33 = tiny_scene(33)
    sc33 = link_scene(fused, s33, dev)
    D33 = C.tangents(s33, 6)
    with pytest.raises(RuntimeError, match=r"1 <= L <= 32"):
        I.mask_information(ctx, sc33, t(s33.mvp), t(D33), torch.zeros((1, s33.H, s33.W), device=dev))
    still_good("33 links")
    with pytest.raises(RuntimeError, match="dmvp must have shape"):
        I.mask_information(ctx, scene, mvp, t(D[:, :1]), ref)                     # the wrong B
    still_good("dmvp of one view")
    with pytest.raises(RuntimeError, match="dmvp must have shape"):
        I.mask_information(ctx, scene, mvp, t(D[:, :, :31]), ref)                 # the wrong L
    still_good("dmvp of 31 links")
