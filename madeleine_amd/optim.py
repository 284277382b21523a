"""madeleine_amd.AdamW -- torch.optim.AdamW's update on this package's own HIP kernels (csrc/adamw.hip), with the two guards a training
loop otherwise pays a host synchronisation for: a step whose gradients hold an inf or a NaN is skipped on the device, and the gradients
are clipped by their global norm inside the update.  Replaces optim.AdamW(ssl_model.parameters(), lr=args.lr) of the reference
(setup_components.py:196)."""
import math

import torch

from . import functional as MF

MAX_TENSORS = MF.ADAMW_MAX_TENSORS      # tensors per launch set (MDL_ADAMW_MAX_TENSORS)


class AdamW(torch.optim.Optimizer):
    """AdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None, skip_nonfinite=True)

    The update of torch.optim.AdamW (decoupled weight decay, no amsgrad, no maximize) for dense fp32 parameters on a ROCm device, as a
    fixed sequence of HIP launches per step: per set of up to MAX_TENSORS parameters of a group one gradient-statistics launch (only
    with skip_nonfinite or max_grad_norm), one update launch and one commit launch -- 3 launches for a model of up to 48 parameter
    tensors, whatever the step's outcome.  step() reads nothing back to the host, copies nothing to the device and, after the first
    step, allocates nothing.  There is no CPU or eager fallback: step() raises for a parameter that is not on a ROCm device.

    skip_nonfinite: if any element of any gradient (all parameter groups) is inf or NaN, the step is void: no parameter, no moment and
        no `step` count changes, and a device-side counter of skipped steps goes up by one.  skipped_steps() reads that counter; it is
        a host read (a synchronisation), meant for the end of an epoch.
    max_grad_norm: the gradients enter the update scaled by clip_grad_norm_'s coefficient min(1, max_grad_norm / (norm + 1e-6)), the
        norm being the global 2-norm over all groups.  Unlike clip_grad_norm_, clipping does NOT modify .grad.
    grad_norm: 0-d device tensor, the global gradient norm of the last step that computed statistics (inf or NaN on a void step).
        Reading it as a tensor does not synchronise.
    With skip_nonfinite=False and max_grad_norm=None the update runs alone, with no statistics pass.

    A learning-rate scheduler still advances on a skipped step, as it does under torch.amp.GradScaler: the host does not know the
    verdict.  lr is read from param_groups at each step as a Python float (LinearLR, CosineAnnealingLR drive it unchanged); a tensor
    lr raises ValueError.
    Under data parallelism the verdict is the same on every rank, because it is taken after the gradient mean (FlatGradSync /
    DistributedDataParallel have all-reduced the gradients before step() reads them).

    State is laid out as by torch.optim.AdamW(fused=True): per parameter `step` (0-d float32 device tensor), `exp_avg`, `exp_avg_sq`;
    state dicts load in both directions between this class and torch.optim.AdamW.  A parameter whose .grad is None is left entirely
    alone, its `step` included.  The skipped-step counter and grad_norm are not part of the state dict.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None, skip_nonfinite=True):
        if isinstance(lr, torch.Tensor):
            raise ValueError("madeleine_amd.AdamW: lr must be a Python float (a tensor lr would be a host read per step)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("madeleine_amd.AdamW: betas must be Python floats")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not (isinstance(max_grad_norm, (int, float)) and max_grad_norm > 0.0 and math.isfinite(max_grad_norm)):
            raise ValueError(f"Invalid max_grad_norm value: {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        # the keys of torch.optim.AdamW's groups, so that a state dict of this class loads into it and back; `fused` describes the state layout
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=True, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        dev = self.param_groups[0]["params"][0].device
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
        self._skipped = torch.zeros((), dtype=torch.int64, device=dev)
        self._scratch = None          # (statistics launches it holds, tensor)

    # ---- argument checks: construction where knowable, else step() ----
    @staticmethod
    def _name(group, gi, pi):
        names = group.get("param_names")
        return "parameter %r" % names[pi] if names else "parameter %d of group %d" % (pi, gi)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        gi = len(self.param_groups) - 1
        group = self.param_groups[gi]
        for pi, p in enumerate(group["params"]):
            if p.dtype != torch.float32:
                raise ValueError("madeleine_amd.AdamW: %s is %s; only float32 parameters are supported" % (self._name(group, gi, pi), p.dtype))
            if p.is_sparse or p.layout != torch.strided or not p.is_contiguous():
                raise ValueError("madeleine_amd.AdamW: %s is not a dense contiguous tensor" % self._name(group, gi, pi))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # torch.optim.AdamW without fused / capturable keeps `step` on the CPU: bring every one to the fused layout
        for group in self.param_groups:
            group["fused"] = True
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    st["step"] = torch.as_tensor(st["step"]).detach().to(device=p.device, dtype=torch.float32).reshape(()).clone()

    def skipped_steps(self) -> int:
        """Steps skipped so far because of a non-finite gradient.  A host read: synchronises with the device."""
        return int(self._skipped.item())

    def _hyper(self, group, gi):
        lr, (beta1, beta2) = group["lr"], group["betas"]
        if isinstance(lr, torch.Tensor) or isinstance(beta1, torch.Tensor) or isinstance(beta2, torch.Tensor):
            raise ValueError("madeleine_amd.AdamW: lr and betas of group %d must be Python floats, not tensors" % gi)
        if group.get("amsgrad") or group.get("maximize") or not group.get("decoupled_weight_decay", True):
            raise ValueError("madeleine_amd.AdamW: group %d asks for amsgrad, maximize or coupled weight decay; none is supported" % gi)
        return float(lr), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"])

    def _gather(self):
        """[(hyperparameters, parameters, gradients, states)] per launch set: the parameters that have a gradient, group by group, at
        most MAX_TENSORS each.  Creates missing state."""
        sets, dev = [], None
        for gi, group in enumerate(self.param_groups):
            hyper = self._hyper(group, gi)
            ps, gs, sts = [], [], []
            for pi, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or g.layout != torch.strided:
                    raise RuntimeError("madeleine_amd.AdamW: %s has a sparse gradient; only dense gradients are supported"
                                       % self._name(group, gi, pi))
                if not p.is_cuda:
                    raise RuntimeError("madeleine_amd.AdamW: %s lives on %s; the HIP kernels are the only backend (no CPU fallback)"
                                       % (self._name(group, gi, pi), p.device))
                if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("madeleine_amd.AdamW: %s and its gradient must be float32 and the parameter contiguous (got %s, %s)"
                                       % (self._name(group, gi, pi), p.dtype, g.dtype))
                if g.device != p.device or (dev is not None and p.device != dev):
                    raise RuntimeError("madeleine_amd.AdamW: %s is not on the device of the other parameters / of its gradient"
                                       % self._name(group, gi, pi))
                dev = p.device
                if not g.is_contiguous():
                    g = g.contiguous()          # rare; a torch copy, the gradient itself stays as it is
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                ps.append(p)
                gs.append(g)
                sts.append(st)
            for o in range(0, len(ps), MAX_TENSORS):
                sets.append((hyper, ps[o:o + MAX_TENSORS], gs[o:o + MAX_TENSORS], sts[o:o + MAX_TENSORS]))
        return sets, dev

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sets, dev = self._gather()
        if not sets:
            return loss
        flags = (MF.ADAMW_GUARD if self.skip_nonfinite else 0) | (MF.ADAMW_CLIP if self.max_grad_norm is not None else 0)
        n_stat = len(sets) if flags else 0
        ws = None
        if n_stat:
            if self._scratch is None or self._scratch[0] < n_stat or self._scratch[1].device != dev:
                self._scratch = (n_stat, MF.adamw_workspace(n_stat, dev))
            ws = self._scratch[1]
        if self.grad_norm.device != dev:      # the model moved after construction
            self.grad_norm, self._skipped = self.grad_norm.to(dev), self._skipped.to(dev)
        max_norm = self.max_grad_norm if self.max_grad_norm is not None else 0.0
        with torch.cuda.device(dev):
            tables = []
            for i, (hyper, ps, gs, sts) in enumerate(sets):
                g_ptrs, numels = MF.adamw_ptrs(gs), MF.adamw_sizes(ps)
                tables.append((g_ptrs, numels))
                if n_stat:
                    MF.adamw_grad_stats(len(ps), g_ptrs, numels, ws, i, n_stat)
            for i, (hyper, ps, gs, sts) in enumerate(sets):
                g_ptrs, numels = tables[i]
                step_ptrs = MF.adamw_ptrs([st["step"] for st in sts])
                MF.adamw_update(len(ps), MF.adamw_ptrs(ps), g_ptrs, MF.adamw_ptrs([st["exp_avg"] for st in sts]),
                                MF.adamw_ptrs([st["exp_avg_sq"] for st in sts]), step_ptrs, numels, *hyper, max_norm, flags, ws, n_stat)
                MF.adamw_commit(len(ps), step_ptrs, flags | (MF.ADAMW_FINAL if i == len(sets) - 1 else 0), ws, n_stat, self.grad_norm,
                                self._skipped)
        return loss
