"""``AdamGroup`` -- one Adam parameter group of a launch chain, as the kernels see it and as a checkpoint holds it.

The kernels update a group in place: ``n`` float32 parameters, the moments ``exp_avg`` / ``exp_avg_sq``, an int32 counter that
advances on real steps only, and the gradient they report.  A checkpoint holds it in ``torch.optim.Adam.state_dict()``'s
shape: ``state[i] = {step, exp_avg, exp_avg_sq}`` and ``param_groups[i]``, a copy of group 0 with this group's ``lr``,
``weight_decay`` and ``params=[i]``.  The users are the pose of :class:`easyhec_amd.fast.FusedPoseStep` (whose parameter is the
model's ``dof``: ``param`` is None), the joint offsets (``joint_calib``; one group shared by the cameras of ``rig_calib``) and
the intrinsics' ``theta`` (``intrinsics_calib``)."""
import torch


class AdamGroup:
    def __init__(self, n, dev, lr, weight_decay, init=None):
        """A fresh group (step 0, zero moments) of ``n`` parameters on ``dev``; ``init``: where the parameters start, or
        None where somebody else (the model) owns them."""
        self.n, self.lr, self.wd = n, lr, weight_decay
        self.param = None if init is None else torch.as_tensor(init, dtype=torch.float32).reshape(n).clone().to(dev)
        self.exp_avg = torch.zeros(n, device=dev)
        self.exp_avg_sq = torch.zeros(n, device=dev)
        self.step_t = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.grad = torch.zeros(n, device=dev)

    def state_entry(self):
        """The group's entry of ``state_dict()["state"]`` (CPU copies)."""
        return {"step": self.step_t.float().cpu().reshape(()), "exp_avg": self.exp_avg.cpu().clone(),
                "exp_avg_sq": self.exp_avg_sq.cpu().clone()}

    def param_group(self, group0, index):
        """The group's entry of ``state_dict()["param_groups"]``: ``group0`` with this group's settings."""
        return dict(group0, lr=self.lr, weight_decay=self.wd, params=[index])

    def check_saved(self, saved, what, owner):
        """Raises where a saved ``param_groups`` entry has another lr or weight decay: its moments belong to another
        problem.  ``what`` / ``owner``: the caller's words for the group and for itself."""
        if float(saved.get("lr", self.lr)) != self.lr or float(saved.get("weight_decay", self.wd)) != self.wd:
            raise ValueError(f"load_state_dict: {what} was saved with lr {saved.get('lr')} / weight decay "
                             f"{saved.get('weight_decay')}, this {owner} has {self.lr} / {self.wd}")

    def load_state(self, entry, param=None):
        """Inverse of :meth:`state_entry` (``entry`` None: the moments and the counter stay), in place; ``param``: the
        parameters' saved values, if the group owns them and they were saved."""
        if entry is not None:
            self.exp_avg.copy_(torch.as_tensor(entry["exp_avg"], dtype=torch.float32).reshape(self.n))
            self.exp_avg_sq.copy_(torch.as_tensor(entry["exp_avg_sq"], dtype=torch.float32).reshape(self.n))
            self.step_t.fill_(int(round(float(torch.as_tensor(entry["step"]).reshape(-1)[0]))))
        if param is not None:
            self.param.copy_(torch.as_tensor(param, dtype=torch.float32).reshape(self.n))
