"""``_PlannedContext`` and ``_ChainStep``.

``_PlannedContext`` -- what everything that renders through a plan of its own has in common
(:class:`easyhec_amd.fast.FusedPoseStep`, :class:`easyhec_amd.multistart.MultiStartPoseStep`,
:class:`easyhec_amd.lm_multi.MultiStartLM`): the job-slot policy, the plan on a rasterizer context with the weights and the
reference masks bound to it, and what the context's status says after a REPORTED call (NaN loss, parameters untouched: the
slot-limited plan overflowed, or the view needs the general-triangle pass).  A user sets ``glctx``, ``scene``, ``H``, ``W``,
``B`` (the views the plan holds), ``ref`` (the masks, shared by ``B / ref.shape[0]`` poses) and ``weight`` (per-pixel weights
of the loss shaped like ``ref``, or None), and calls :meth:`_PlannedContext._init_plan`.

``_ChainStep`` -- the two Adam steppers on top of it: a launch chain that is enqueued or replayed from the context's
hipGraph, and the protocol around a reported step -- the non-blocking look at the loss, the recovery with its graph
handling, and the loop that takes an exact number of effective steps.  A subclass also sets ``dev`` and ``loss`` (one element
per pose), provides ``_enqueue(want_mask, stream=None)`` and
``steps_done`` (Adam's own counter, which only advances on real steps; reading it synchronises), and ends its constructor
with :meth:`_init_chain`."""
import ctypes
import os

import torch

from . import _lib, fused


def check_solver_settings(cfg, what="the launch chain"):
    """The one check of ``cfg.solver`` for everything that steps a launch chain (``what``: the caller's name for it in the
    message); returns the constructors' ``lr`` / ``weight_decay`` keywords from it."""
    if cfg.solver.do_grad_clip or cfg.solver.optimizer != "Adam":
        raise ValueError(f"{what} implements the reference's default solver only (Adam, no gradient clipping)")
    return {"lr": cfg.solver.max_lr, "weight_decay": cfg.solver.weight_decay}


class _ReportedStepProtocol:
    """The protocol around a REPORTED step, in one place for every stepper (``_ChainStep``; the camera rig of
    easyhec_amd/rig_calib.py, which drives several chains): the non-blocking look at the loss and the loop that takes an
    exact number of effective steps.  A user sets ``dev`` and ``loss`` (all NaN for a reported step) and provides
    ``steps_done``, ``_recover_and_note()`` and ``_check_status()`` (raises with the status of the context(s))."""

    def _init_protocol(self):
        # A reported step loses nothing but time -- unless nobody looks.  step() therefore looks itself, without ever
        # waiting: every `check_every` steps the loss goes to pinned host memory behind an event, the copy that was started
        # `check_every` steps earlier is inspected, and a NaN there triggers the recovery.
        self.check_every = 16
        self._calls = 0
        self._probe = torch.zeros(self.loss.numel(), dtype=torch.float32)
        if self.dev.type == "cuda":
            self._probe = self._probe.pin_memory()
        self._probe_ev = None
        self.recoveries = []  # what the recovery did, in order

    def _poll(self):
        """Non-blocking look at the loss of the step taken `check_every` steps ago (a report is step-wide: every element
        NaN); starts the next look."""
        if self._probe_ev is not None:
            if not self._probe_ev.query():
                return  # (still in flight: look again next time; never wait here)
            self._probe_ev = None
            if bool(torch.isnan(self._probe).all()):
                self._recover_and_note()
        self._probe.copy_(self.loss, non_blocking=True)
        self._probe_ev = torch.cuda.Event()
        self._probe_ev.record()

    def effective_rounds(self, n, who):
        """The loop that takes exactly ``n`` EFFECTIVE steps: yields ``(steps still to take, effective steps so far)``; the
        caller takes that many steps and comes back.  While steps were reported, the chain is recovered and the rest is
        asked for again -- at most 4 times, then raises with the context's status (``who``: the caller's name, for the
        message).  ``steps_done`` is read once per round."""
        start, done, rounds = self.steps_done, 0, 0
        while done < n:
            yield n - done, done
            done = self.steps_done - start
            if done < n:
                rounds += 1
                if rounds > 4:
                    self._check_status()
                    raise RuntimeError(f"{who}: {n - done} of {n} steps keep being reported as not taken (NaN loss)")
                self._recover_and_note()

    def take_effective_steps(self, n, who):
        """Takes exactly ``n`` EFFECTIVE steps with :meth:`effective_rounds` and returns ``[>= n, loss.numel()]`` (CPU): the
        ``loss`` of every step that was not reported, in order.  One device log per round, filled by copies on the stream;
        the first wait is the copy to the host at the end."""
        logs = []
        for remaining, _ in self.effective_rounds(n, who):
            log = torch.empty((remaining, self.loss.numel()), device=self.dev)
            for it in range(remaining):
                log[it].copy_(self.step())
            logs.append(log)
        hist = torch.cat(logs).cpu() if logs else torch.zeros((0, self.loss.numel()))
        return hist[~torch.isnan(hist).all(dim=1)]  # (reported steps: NaN in every element, taken by nobody)


class _PlannedContext:
    def _init_plan(self, slack):
        # job slots: `slack` per view tile (default: half as many slots as a view has tiles) instead of one per (view,
        # link, tile) -- 30 MB instead of 0.48 GB of scratch at 8 views 720p x 8 links; the workloads here use a tenth of
        # that (a robot's links touch ~5 % of a frame's tiles).  A view that needs more (every pixel under more than
        # `slack` link boxes on average: a close-up) is REPORTED -- NaN loss, parameters untouched -- and
        # :meth:`recover_from_overflow` plans again with a slot for every (view, link, tile).  EHR_VB_SLACK overrides (0 = all).
        # (Small images: at least 256 slots per view -- a link's box touches a few tiles however small the frame is.)
        if slack is None and "EHR_VB_SLACK" not in os.environ:
            ntiles = ((self.W + 31) // 32) * ((self.H + 7) // 8)
            self.slack = max(0.5, 256.0 / ntiles)
        else:
            self.slack = float(os.environ["EHR_VB_SLACK"]) if slack is None else float(slack)
        self._plan_and_bind()

    def _plan_and_bind(self):
        fused._ensure_plan(self.glctx, self.scene, self.B, self.H, self.W, slack=self.slack)
        # the reference masks are constants of the solve: the loss of the tiles no link touches is cached once
        # (bit-identical results).  self.ref is this object's private copy, never written to.  The weights, if any, first:
        # binding them unbinds the reference, whose cached sums are sums of w ref^2.
        weight = getattr(self, "weight", None)
        if weight is not None or getattr(self.glctx, "_bound_weight", None) is not None:
            fused.bind_weight(self.glctx, self.scene, weight, views=self.B)
        fused.bind_ref(self.glctx, self.scene, self.ref, views=self.B)

    def _overflow_status(self):
        """What the context reports (``ehr_fused_status``; synchronises): False (nothing), "general-triangle pass"
        (EHR_ERR_RETRY: the call met triangles for that pass, and the context launches it from now on) or "job slots" (the
        slot-limited plan overflowed).  Raises on an overflow of a plan that already has every slot."""
        with torch.cuda.device(self.glctx.device):
            rc = _lib.lib().ehr_fused_status(self.glctx.handle)
        if rc == 0:
            return False
        if rc == _lib.EHR_ERR_RETRY:
            return "general-triangle pass"
        if self.slack == 0.0:
            _lib.check(rc, "fused render")
        return "job slots"

    def _plan_every_slot(self):
        self.slack = 0.0
        self._plan_and_bind()

    def recover_from_overflow(self):
        """Call when calls were reported (NaN loss).  Synchronises.  Returns what :meth:`_overflow_status` found; after
        "job slots" the context is planned again with a slot for every (view, link, tile), the weights and the reference
        bound again.  The reported calls changed nothing, so the caller simply goes on."""
        what = self._overflow_status()
        if what == "job slots":
            self._plan_every_slot()
        return what


class _ChainStep(_PlannedContext, _ReportedStepProtocol):
    def _init_chain(self, slack):
        self._init_plan(slack)
        self._graph = None
        self._init_protocol()  # (a NaN seen there triggers recover_from_overflow(); `recoveries` notes what it did)

    def _host_copies_stale(self):
        """Called where the chain has written, or is about to write, device state that the host may hold a copy of."""

    def step(self, want_mask=False):
        """Enqueue one optimisation step.  Returns the (device) mean mask loss of every pose, evaluated BEFORE the update
        like ``loss`` in trainer/rbsolver.py:33-41; all NaN for a reported step.  Never synchronises."""
        self._host_copies_stale()
        if getattr(self.glctx, "_bound_weight", None) is not getattr(self, "weight", None):
            # the weights are state of the CONTEXT, and somebody else used it since (the model's forward with other
            # weights, or none): bind this solve's again -- never step on weights that are not its own
            had_graph = bool(self._graph)
            self.release_graph()
            self._plan_and_bind()
            if had_graph:
                self.capture()
        with torch.cuda.device(self.dev):
            if self._graph and not want_mask:
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                _lib.check(_lib.lib().ehr_graph_launch(self.glctx.handle, stream), "ehr_graph_launch")
            else:
                self._enqueue(want_mask)
            self._calls += 1
            if self._calls % self.check_every == 0:
                self._poll()
        return self.loss

    def _check_capturable(self):
        """Raises if this step's chain cannot be recorded."""

    def capture(self):
        """Record the step's launch chain into a hipGraph owned by the rasterizer context (``ehr_graph_*`` in
        include/ehr.h); ``step()`` then replays it with one host call.  Iteration state lives on the device, so replays are
        ordinary optimisation steps.  The chain is GPU-bound, so this saves host time, not step time."""
        if self._graph:
            return
        self._check_capturable()
        lib = _lib.lib()
        with torch.cuda.device(self.dev):
            torch.cuda.synchronize()
            cap = ctypes.c_void_p()
            _lib.check(lib.ehr_graph_begin(self.glctx.handle, ctypes.byref(cap)), "ehr_graph_begin")
            try:
                self._enqueue(False, stream=cap)
            except Exception:
                lib.ehr_graph_release(self.glctx.handle)
                raise
            _lib.check(lib.ehr_graph_end(self.glctx.handle), "ehr_graph_end")
        self._graph = True

    def release_graph(self):
        if self._graph:
            _lib.check(_lib.lib().ehr_graph_release(self.glctx.handle), "ehr_graph_release")
            self._graph = None

    def recover_from_overflow(self):
        """Call when a step's loss came back NaN (for every pose).  Synchronises.  If the context reports that the step
        needed the general-triangle pass (EHR_ERR_RETRY: the context launches it from now on) the graph, if any, is
        re-captured; if it reports an overflow and the plan was slot-limited, plans again with a slot for every (view, link,
        tile), re-binds the weights and the reference masks and re-captures.  Returns what it did (a non-empty string) in both cases, False
        if the context reports nothing: the steps since the report changed nothing (dof, Adam moments and step counter stay
        untouched on a NaN, and the chain's head writes the unchanged pose to the SAME history row again: include/ehr.h,
        ehr_solver_step), so the caller simply goes on stepping.  Raises on any other overflow."""
        # (on every rank of a data-parallel job alike, whichever rank's views caused the report: the reduced loss was NaN for
        #  all of them, none of them stepped, and each of them kept recording the unchanged pose in one and the same row)
        self._host_copies_stale()
        what = self._overflow_status()
        if what:
            # "general-triangle pass": the chain had not been launching it, so a captured chain is recorded again with it;
            # "job slots": the graph is released before the plan it was recorded on is replaced
            had_graph = bool(self._graph)
            self.release_graph()
            if what == "job slots":
                self._plan_every_slot()
            if had_graph:
                self.capture()
        return what

    def _recover_and_note(self):
        what = self.recover_from_overflow()
        if what:
            self.recoveries.append(what)
        return what

    def _check_status(self):
        fused.check_status(self.glctx)
