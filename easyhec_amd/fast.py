"""``FusedPoseStep`` -- one optimisation step of /root/reference/easyhec/trainer/rbsolver.py:29-43 as a fixed chain of
three HIP launches with no host round trip: [pose forward + vertices + raster records] -> jobs (coverage, depth where the
silhouette analysis will look, and the resolve of every job by the wave that drew it) -> composite [+ in its last
workgroup: loss, gradients, pose backward, Adam]; data-parallel: the composite launch stops before Adam and ONE more
launch exchanges the 8 floats with the peers and applies Adam (peer-memory mailboxes; or an all-reduce followed by Adam).

It operates IN PLACE on an :class:`easyhec_amd.rb_solver.RBSolver`'s ``dof`` parameter and ``history_ops`` buffer and
keeps torch.optim.Adam-compatible state (exp_avg, exp_avg_sq, step), so it is interchangeable with the autograd path
of :class:`easyhec_amd.trainer.RBSolverTrainer` step for step (tests/test_gpu_fast.py).  Stepping, graph capture and the
recovery from a reported step are :class:`easyhec_amd.chain_step._ChainStep`'s, shared with the multi-start step; this
module adds the solo chain's launches and, for data-parallel solves, the choice and set-up of the exchange
(:func:`choose_exchange`)."""
import ctypes
import os
import sys
from typing import NamedTuple

import torch
import torch.distributed as dist

from . import _lib
from .chain_step import _ChainStep
from .param_group import AdamGroup

__all__ = ["FusedPoseStep", "choose_exchange"]

POSE_LR, POSE_WEIGHT_DECAY = 0.003, 0.0005  # Adam's defaults for the pose, and for every group that is not given its own


def _f(x):
    return ctypes.c_float(float(x))


def ranks_agree(ok, pg, dev):
    """True iff EVERY rank of the process group passes ``ok`` = True (one all-reduce(min) of a flag; collective: every
    rank must call it)."""
    on_dev = dist.get_backend(pg) == "nccl"
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev if on_dev else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=pg)
    return bool(int(flag.item()) == 1)


class Exchange(NamedTuple):
    """Which exchanges of the 8-float vector a data-parallel step attempts, in this order, and which of them must come up."""
    try_p2p: bool
    p2p_required: bool
    try_rccl: bool
    rccl_required: bool
    agree_on_rccl: bool  # the ranks settle together whether the RCCL exchange is used

    def after_p2p(self, ok):
        """``(p2p, rccl)`` once the peer-memory attempt is over (``ok``: made, and good on every rank): it replaces the
        all-reduce; otherwise the RCCL attempt, if any, is still to come."""
        return (True, False) if ok else (False, self.try_rccl)


def choose_exchange(rccl, p2p, comm_env, try_rccl, distributed, backend):
    """How the ranks exchange the 8-float vector.  ``rccl`` / ``p2p``: the constructor's arguments (None = default);
    ``comm_env`` / ``try_rccl``: the values of EHR_COMM ("" if unset) and EHR_TRY_RCCL; ``backend``: the process group's,
    looked at only where ``distributed``.

    "rccl" = ncclAllReduce on the library's own communicator, enqueued on the chain's stream between the solver step and
    Adam (default for the nccl backend, i.e. one process per GPU); otherwise torch.distributed.all_reduce (gloo: the CPU
    tests, two ranks sharing one GPU).  rccl=True without a process group makes a single-rank communicator (the same launch
    sequence on one GPU).  (EHR_TRY_RCCL=1, test hook: attempt the library-owned exchange under any backend, so that the
    agreement / fall-back branches run where RCCL cannot come up -- two ranks on one device.)

    "p2p" (EHR_COMM=p2p, or p2p=True): the one-shot exchange over peer memory (ehr_comm_p2p_*: every rank stores its 8
    floats into every peer's mailbox, sums in rank order and runs Adam in the SAME kernel -- one launch instead of an
    all-reduce plus ehr_pose_adam).  Needs a process group with the ranks on GPUs of one node (or, for tests, on one GPU).
    Default under the nccl backend (one process per GPU of a node) unless ``rccl`` is given: tried first, the RCCL
    all-reduce is the fall-back.  EHR_COMM = p2p / rccl / torch forces the choice (p2p: under any backend)."""
    nccl = distributed and backend == "nccl"
    if rccl is not None:
        want_rccl = bool(rccl)
    else:
        want_rccl = comm_env != "torch" and distributed and (nccl or try_rccl == "1")
    want_p2p = p2p if p2p is not None else (comm_env == "p2p" or (comm_env == "" and rccl is None and nccl))
    try_p2p = bool(want_p2p) and distributed
    return Exchange(try_p2p, try_p2p and bool(p2p), want_rccl, bool(rccl), distributed and rccl is None)


def _private_weight(batch, dev):
    """``batch["weight"]`` as a private contiguous float32 clone on ``dev`` (the sums ``bind_ref`` caches depend on it), or
    None."""
    w = batch.get("weight")
    return None if w is None else w.to(dev, torch.float32).contiguous().clone()


def _hip_device(who, model, batch):
    """The model's device, after the one check of everything that takes a model and a batch without a step object: the
    model and ``batch['mask' | 'link_poses' | 'K']`` on a HIP device, else raise in ``who``'s name."""
    dev = model.dof.device
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs on a HIP device only: move the model with .cuda() first (there is no CPU path)")
    for k in ("mask", "link_poses", "K"):
        if not torch.is_tensor(batch[k]) or batch[k].device.type != "cuda":
            raise RuntimeError(f"{who}: batch['{k}'] must be a tensor on the HIP device")
    return dev


def refuse_unsupported(kw, available, starts, data_parallel, missing):
    """The refusals every solve built on ``FusedPoseStep`` makes before it constructs one, each raised with the caller's
    own reason: ``starts=`` among the keywords ``kw`` (a call ported from ``MultiStartPoseStep`` gets the reason, not a
    TypeError about a keyword), a data-parallel job, and a library without the solve's kernels (``available()`` false)."""
    if "starts" in kw:
        raise ValueError(starts)
    pg = kw.get("process_group")
    if kw.get("rccl") or kw.get("p2p") or (dist.is_available() and dist.is_initialized() and dist.get_world_size(pg) > 1):
        raise ValueError(data_parallel)
    if not available():
        raise RuntimeError(missing)


class FusedPoseStep(_ChainStep):
    def __init__(self, model, batch, lr=POSE_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=POSE_WEIGHT_DECAY, near=0.001,
                 far=10.0, process_group=None, rccl=None, slack=None, p2p=None, *, loss=None, defer_adam=False):
        """loss: the [1] device tensor the step's loss goes to (default: one of its own; a camera of a rig gets its element
        of the rig's).  defer_adam: the chain stops after ``red`` (no Adam, ``loss`` not written) although the solve is not
        data-parallel -- the caller finishes the step with a launch of its own (easyhec_amd/rig_calib.py).

        A calibration solve is this class built with more launches around the chain, each a part the step holds:
        ``_before`` (``launch(step, stream)``) runs ahead of the chain, ``_after`` behind it, in order; a part of ``_after``
        also adds its parameter group to the state dict (``add_state`` / ``check_state`` / ``load_state``) and says whether
        its launch ``rewrites_K``."""
        self.model = model
        self.renderer = model._ensure_renderer()
        self.scene = model._ensure_scene()
        self.glctx = self.renderer.glctx
        dev = model.dof.device
        self.dev = dev
        self.H, self.W = model.H, model.W
        # a private copy, always (``.to`` / ``.contiguous`` return the caller's own tensor when nothing has to change, and
        # the sums cached by ``bind_ref`` must not go stale under an in-place edit of ``batch["mask"]``)
        self.ref = batch["mask"].to(dev, torch.float32).contiguous().clone()
        # optional per-pixel weights of the loss (batch["weight"], 0 = an occluded or unreliable pixel): private like ref
        self.weight = _private_weight(batch, dev)
        self.link_poses = batch["link_poses"].to(dev, torch.float32).contiguous()
        self.K = batch["K"][0].to(dev, torch.float32).contiguous()
        self.B, self.L = self.link_poses.shape[0], self.link_poses.shape[1]
        assert self.L == self.scene.num_links and self.ref.shape == (self.B, self.H, self.W)
        assert self.weight is None or self.weight.shape == self.ref.shape
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.near, self.far = near, far
        self.pg, self.defer_adam = process_group, bool(defer_adam)
        self._before, self._after = (), ()
        self.distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.pg) > 1
        ex = choose_exchange(rccl, p2p, os.environ.get("EHR_COMM", ""), os.environ.get("EHR_TRY_RCCL"), self.distributed,
                             dist.get_backend(self.pg) if self.distributed else None)
        ok = False
        if ex.try_p2p:
            # set up over the process group, checked against it, and dropped by ALL ranks together if any rank cannot
            ok, why = True, ""
            try:
                self._init_p2p()
            except RuntimeError as e:
                ok, why = False, str(e)
            if not ranks_agree(ok, self.pg, self.dev):
                if ok:
                    ok, why = False, "another rank could not set it up"
                    with torch.cuda.device(self.dev):
                        _lib.lib().ehr_comm_p2p_close(self.glctx.handle)
                if ex.p2p_required:
                    raise RuntimeError(f"peer-memory exchange unavailable: {why}")
                print(f"[easyhec_amd] peer-memory exchange unavailable ({why}); using the all-reduce", file=sys.stderr)
        self.p2p, self.rccl = ex.after_p2p(ok)
        if self.rccl:
            ok, why = True, ""
            try:
                self._init_comm()
            except RuntimeError as e:
                if ex.rccl_required:  # asked for explicitly: fail loudly
                    raise
                ok, why = False, str(e)
            if ex.agree_on_rccl:
                # the ranks must agree on the exchange they use: one rank on torch.distributed and the others on the
                # library's communicator would wait for each other for ever
                if ok and not ranks_agree(ok, self.pg, self.dev):
                    ok, why = False, "another rank could not set it up"
                    with torch.cuda.device(self.dev):
                        _lib.lib().ehr_comm_destroy(self.glctx.handle)
                elif not ok:
                    ranks_agree(False, self.pg, self.dev)
            if not ok:
                print(f"[easyhec_amd] library-owned RCCL exchange unavailable ({why}); using torch.distributed.all_reduce",
                      file=sys.stderr)
                self.rccl = False
        # optimiser state (torch.optim.Adam names): a fresh Adam (step 0, zero moments) unless load_state_dict restores
        # one -- like the reference's load_model path.  The row of ``history_ops`` the next step records its pose in is a
        # counter of its own (the reference's first all-zero row, rb_solver.py:50-51): it starts at the model's history
        # cursor, so a solver built on a loaded checkpoint appends whatever the optimiser's step count is.
        self.pose_group = g = AdamGroup(6, dev, lr, weight_decay)   # (the parameter is the model's ``dof``)
        self.exp_avg, self.exp_avg_sq, self.step_t, self.grad = g.exp_avg, g.exp_avg_sq, g.step_t, g.grad
        self.hist_row = torch.full((1,), int(model.history_cursor()), dtype=torch.int32, device=dev)
        # work buffers, allocated once
        self.mvp = torch.empty((self.B, self.L, 4, 4), device=dev)
        self.grad_mvp = torch.empty((self.B, self.L, 4, 4), device=dev)
        self.tc_jac = torch.empty((7, 16), device=dev)
        self.loss_b = torch.empty((self.B,), device=dev)
        self.red = torch.empty((8,), device=dev)
        self.loss = torch.zeros((1,), device=dev) if loss is None else loss
        self.mask = torch.empty((self.B, self.H, self.W), device=dev)
        self._init_chain(slack)

    def _init_comm(self):
        """ncclCommInitRank through the C ABI (``ehr_comm_*``): rank 0's ncclUniqueId travels over the process group that
        is already up (the only use torch.distributed has on this path)."""
        lib = _lib.lib()
        world = dist.get_world_size(self.pg) if self.distributed else 1
        rank = dist.get_rank(self.pg) if self.distributed else 0
        idbuf = (ctypes.c_ubyte * 128)()
        err = None
        if rank == 0:
            try:
                _lib.check(lib.ehr_comm_unique_id(idbuf), "ehr_comm_unique_id")
            except RuntimeError as e:   # the other ranks are waiting in the broadcast below: they get an all-zero id
                err, idbuf = e, (ctypes.c_ubyte * 128)()
        if world > 1:
            on_dev = dist.get_backend(self.pg) == "nccl"
            t = torch.tensor(list(idbuf), dtype=torch.uint8, device=self.dev if on_dev else "cpu")
            dist.broadcast(t, src=dist.get_global_rank(self.pg, 0) if self.pg is not None else 0, group=self.pg)
            idbuf = (ctypes.c_ubyte * 128)(*t.cpu().tolist())
        if err is not None or not any(idbuf):
            raise RuntimeError(f"no ncclUniqueId from rank 0 ({err})")
        with torch.cuda.device(self.dev):
            _lib.check(lib.ehr_comm_init(self.glctx.handle, idbuf, world, rank), "ehr_comm_init")
            # self-check before the solve depends on it: one all-reduce of a known vector on the new communicator must
            # give what the process group gives (the N > 1 form of this exchange has never run on hardware in the build
            # container; a mismatch here raises, and the default selection above falls back to torch.distributed)
            probe = torch.full((8,), float(rank + 1), device=self.dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.ehr_comm_allreduce(self.glctx.handle, _lib.ptr(probe), 8, stream), "ehr_comm_allreduce")
            torch.cuda.synchronize()
            want = world * (world + 1) / 2.0
            if not bool((probe == want).all()):
                raise RuntimeError(f"ehr_comm_allreduce self-check: got {probe.tolist()}, expected {want}")

    def _init_p2p(self):
        """Mailboxes of the one-shot exchange (``ehr_comm_p2p_*``): every rank exports its mailbox's 64-byte IPC handle, the
        handles travel over the process group that is already up, every rank opens its peers', and one exchange of a known
        vector must give what it should before the solve depends on it.  Every rank makes the same collective calls whatever
        fails locally (a rank that cannot export ships an all-zero handle; the open phase ends on an agreement)."""
        lib = _lib.lib()
        world, rank = dist.get_world_size(self.pg), dist.get_rank(self.pg)
        hbuf, err = (ctypes.c_ubyte * 64)(), None
        try:
            with torch.cuda.device(self.dev):
                _lib.check(lib.ehr_comm_p2p_export(self.glctx.handle, hbuf), "ehr_comm_p2p_export")
        except RuntimeError as e:
            hbuf, err = (ctypes.c_ubyte * 64)(), e
        on_dev = dist.get_backend(self.pg) == "nccl"
        mine = torch.tensor(list(hbuf), dtype=torch.uint8, device=self.dev if on_dev else "cpu")
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine, group=self.pg)          # (also the barrier "every rank has exported")
        flat = torch.stack(every).cpu().contiguous()
        if err is None and not bool((flat != 0).any(dim=1).all()):
            err = RuntimeError("a rank exported no mailbox")
        if err is None:
            try:
                allh = (ctypes.c_ubyte * (64 * world))(*flat.view(-1).tolist())
                with torch.cuda.device(self.dev):
                    _lib.check(lib.ehr_comm_p2p_open(self.glctx.handle, allh, world, rank), "ehr_comm_p2p_open")
            except RuntimeError as e:
                err = e
        if not ranks_agree(err is None, self.pg, self.dev):   # every rank has opened (or nobody goes on): stores may begin
            raise err if err is not None else RuntimeError("another rank could not open the mailboxes")
        with torch.cuda.device(self.dev):
            probe = torch.full((8,), float(rank + 1), device=self.dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.ehr_comm_p2p_step(self.glctx.handle, _lib.ptr(probe), None, None, None, None, _f(0), _f(0), _f(0),
                                             _f(0), _f(0), None, None, stream), "ehr_comm_p2p_step")
            torch.cuda.synchronize()
        want = world * (world + 1) / 2.0
        if not bool((probe == want).all()):
            raise RuntimeError(f"ehr_comm_p2p_step self-check: got {probe.tolist()}, expected {want}")

    # -- one step -------------------------------------------------------------------------------------------------
    def _enqueue(self, want_mask, stream=None):
        lib = _lib.lib()
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        m, sc = self.model, self.scene
        dof = m.dof.data
        hist = m.history_ops
        for part in self._before:
            part.launch(self, stream)
        # one C call = 3 launches: [pose fwd + vertices + raster records] -> jobs, resolved by the waves that drew them
        # [-> general-triangle jobs, resolved likewise, once a step has needed them] -> composite [+ in its last workgroup:
        # accumulators + pose bwd (+ Adam)]
        _lib.check(lib.ehr_solver_step(
            self.glctx.handle, _lib.ptr(sc.verts), _lib.ptr(sc.tris), _lib.ptr(sc.tri_link), _lib.ptr(sc.vert_link),
            _lib.ptr(sc.opp), _lib.ptr(self.K), _lib.ptr(self.link_poses), _lib.ptr(self.ref), self.B, self.L,
            sc.num_verts, sc.num_tris, self.H, self.W, _f(self.near), _f(self.far), _lib.ptr(dof),
            _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(self.step_t), _lib.ptr(hist), hist.shape[0],
            _lib.ptr(self.hist_row), _f(self.lr), _f(self.betas[0]), _f(self.betas[1]), _f(self.eps), _f(self.wd), _lib.ptr(self.mvp),
            _lib.ptr(self.tc_jac), _lib.ptr(self.mask if want_mask else None), _lib.ptr(self.loss_b),
            _lib.ptr(self.grad_mvp), _lib.ptr(self.red), _lib.ptr(self.loss), _lib.ptr(self.grad),
            int(self.distributed or self.rccl or self.defer_adam), stream), "ehr_solver_step")
        if self.p2p:
            # the exchange and Adam in ONE launch: stores into the peers' mailboxes, a wait on the own one, sums in rank order
            _lib.check(lib.ehr_comm_p2p_step(self.glctx.handle, _lib.ptr(self.red), _lib.ptr(dof), _lib.ptr(self.exp_avg),
                                             _lib.ptr(self.exp_avg_sq), _lib.ptr(self.step_t), _f(self.lr), _f(self.betas[0]),
                                             _f(self.betas[1]), _f(self.eps), _f(self.wd), _lib.ptr(self.loss),
                                             _lib.ptr(self.grad), stream), "ehr_comm_p2p_step")
        elif self.distributed or self.rccl:
            # the ONE collective of a step (32 bytes), between the chain and Adam
            if self.rccl:
                _lib.check(lib.ehr_comm_allreduce(self.glctx.handle, _lib.ptr(self.red), 8, stream), "ehr_comm_allreduce")
            else:
                dist.all_reduce(self.red, op=dist.ReduceOp.SUM, group=self.pg)
            _lib.check(lib.ehr_pose_adam(_lib.ptr(dof), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                         _lib.ptr(self.step_t), _lib.ptr(self.red), _f(self.lr), _f(self.betas[0]),
                                         _f(self.betas[1]), _f(self.eps), _f(self.wd), _lib.ptr(self.loss),
                                         _lib.ptr(self.grad), stream), "ehr_pose_adam")
        # the parts' finish launches.  The ORDER is a contract, stated and checked here once: every finish launch reads what
        # the chain left as it was rendered, K included, so the one that rewrites K for the next step runs last.
        if any(part.rewrites_K for part in self._after[:-1]):
            raise RuntimeError("a finish launch that rewrites K must be the last one: the others read K as rendered")
        for part in self._after:
            part.launch(self, stream)

    def _host_copies_stale(self):
        self.model._hist_n = None  # the chain writes history_ops rows itself: the host cursor is stale from here on

    def _check_capturable(self):
        """The chain is 3 kernels on one stream.  The data-parallel step (4-5) is captured too when its exchange is the
        library's own -- the peer-memory one (``p2p``: [solver step, exchange + Adam]) or ncclAllReduce (``rccl``: [solver
        step, all-reduce, Adam]) -- on one stream; with the torch.distributed exchange (gloo) it cannot be."""
        if self.distributed and not (self.rccl or self.p2p):
            raise RuntimeError("capture(): not available with the torch.distributed exchange (use the RCCL or the peer-memory one)")

    @property
    def steps_done(self):
        return int(self.step_t.item())

    def _group0(self):
        """The pose's ``param_groups`` entry, which every other group's is built from."""
        return {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.wd, "amsgrad": False,
                "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                "decoupled_weight_decay": False, "params": [0]}

    def state_dict(self):
        """torch.optim.Adam-shaped state for checkpoints (trainer/rbsolver.py:95-114): group 0 is the pose; every part
        with a parameter group of its own adds it, with the parameters that no model holds."""
        sd = {"state": {0: self.pose_group.state_entry()}, "param_groups": [self._group0()]}
        for part in self._after:
            part.add_state(self, sd)
        return sd

    def load_state_dict(self, sd):
        """Inverse of :meth:`state_dict`; also accepts a ``torch.optim.Adam.state_dict()`` of the same parameter.  A part
        whose group the state does not hold keeps its own; one whose group was saved for another problem (another free set,
        other settings) raises before anything is loaded."""
        for part in self._after:
            part.check_state(self, sd)
        st = sd.get("state", {})
        if len(st):  # (none: a fresh optimiser)
            self.pose_group.load_state(st[sorted(st.keys())[0]])
        for part in self._after:
            part.load_state(self, sd)
