"""The solver's per-step tail on the HIP path.

The reference's training loop (solver.py:91-94) is
    loss = self.criterion(logits, a); self.optimizer.zero_grad(); loss.backward(); self.optimizer.step()
with `criterion` = nn.KLDivLoss() for mhb/mhb_coAtt and nn.CrossEntropyLoss() otherwise
(solver.py:25-28) and `optimizer` = torch.optim.Adam(model.parameters(), lr=cfg.lr) (solver.py:29).
The classes below keep those names, constructor defaults and call signatures, so the solver only
has to import them from here; their arithmetic runs in libvqa_fusion.so (csrc/train.hip).
"""
import torch
from torch import nn

from . import ops
from .lib import VqfError


def _times(d, g):
    """d (N,A) * g, g = the scalar gradient arriving at the loss (loss.backward(): a one-element GPU tensor)"""
    if g.is_cuda and g.dtype == torch.float32 and g.numel() == 1 and d.dim() == 2 and d.is_contiguous():
        return ops.scale_by_device_scalar(d, g.reshape(1))
    return d * g


class _CeLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss, d = ops.ce_loss(logits.contiguous(), target, want_grad=logits.requires_grad)
        ctx.save_for_backward(d)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return _times(d, g), None


class _KlDivLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target):
        loss, d = ops.kldiv_loss(logp.contiguous(), target.contiguous(), want_grad=logp.requires_grad)
        ctx.save_for_backward(d)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return _times(d, g), None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() as constructed at solver.py:28: mean over rows, ignore_index -100, no
    class weights / label smoothing.  forward(logits (N,A) fp32, target (N,) int64) -> scalar."""

    def forward(self, logits, target):
        return _CeLossFn.apply(logits, target)


class KLDivLoss(nn.Module):
    """nn.KLDivLoss() as constructed at solver.py:26: default reduction, i.e. the mean over all N*A
    elements of target * (log target - input).  forward(log-probs (N,A), target (N,A)) -> scalar."""

    def forward(self, logp, target):
        return _KlDivLossFn.apply(logp, target)


class _BceLossFn(torch.autograd.Function):
    """target: a (N, A) fp32 tensor or a SoftAnswers (not a tensor: autograd passes it through); never differentiated"""

    @staticmethod
    def forward(ctx, logits, target, per_row):
        want_grad = logits.requires_grad      # of the incoming tensor: grad mode is off here, a contiguous copy would say False
        logits = logits.contiguous()
        loss, d, _, _ = ops.bce_logits_loss(logits, _bce_target(target), _bce_scale(logits, per_row), want_grad=want_grad,
                                            want_pred=False)
        ctx.save_for_backward(d)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        return _times(d, g), None, None


def _bce_target(target):
    """a dense target is made contiguous, as _KlDivLossFn does; a SoftAnswers goes through as it is"""
    return target.contiguous() if torch.is_tensor(target) else target


def _bce_scale(logits, per_row):
    """c of the criterion: 1 / N ("batchmean") or 1 / (N A) ("mean"), formed in double"""
    if logits.dim() != 2 or logits.numel() < 1:
        raise VqfError("BCEWithLogitsLoss: non-empty logits (N,A) expected")
    return 1.0 / (logits.shape[0] if per_row else logits.numel())


class BCEWithLogitsLoss(nn.Module):
    """Binary cross-entropy with logits on soft answers, the criterion of models trained on detector-box features.
    reduction "mean": nn.BCEWithLogitsLoss()'s default, the mean over all N*A elements; "batchmean": the sum over answers and
    the mean over questions.  No weight, pos_weight or other reduction.  forward(logits (N,A) fp32, target) -> scalar, target
    a (N,A) fp32 tensor of soft scores or a SoftAnswers (by definition the call on target.dense(A))."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "batchmean"):
            raise ValueError("BCEWithLogitsLoss: reduction must be 'mean' or 'batchmean', got %r" % (reduction,))
        self.reduction = reduction

    def forward(self, logits, target):
        return _BceLossFn.apply(logits, target, self.reduction == "batchmean")


def criterion_for(model_name):
    """solver.py:25-28."""
    return KLDivLoss() if model_name in ("mhb_coAtt", "mhb") else CrossEntropyLoss()


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_(parameters, max_norm) on the HIP path: the 2-norm over the gradients of every
    parameter that has one, then each gradient scaled in place by min(1, max_norm / (norm + 1e-6)) -- two kinds of launches
    (norm, scale) and a one-workgroup finish, whatever the number of tensors up to 32 per launch.  Returns the total norm
    as a 0-d GPU tensor; nothing is read back to the host and nothing synchronises.  A NaN / Inf gradient gives what torch
    gives with error_if_nonfinite=False (norm NaN -> every gradient NaN; norm Inf -> every gradient times 0);
    `error_if_nonfinite` itself is not offered: raising needs the norm on the host.  norm_type other than 2 raises
    ValueError; CPU, non-fp32 or non-contiguous gradients raise VqfError."""
    if float(norm_type) != 2.0:
        raise ValueError("clip_grad_norm_: only norm_type=2 is built, got %r" % (norm_type,))
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("clip_grad_norm_: max_norm must be > 0, got %r" % (max_norm,))
    if torch.is_tensor(parameters):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.zeros(())
    with torch.no_grad():
        norm, coef = ops.grad_norm_clip(grads, max_norm)
        ops.grad_scale_(grads, coef)
    return norm


class _MultiTensorOptimizer(torch.optim.Optimizer):
    """The step both optimizers share: per param group one multi-tensor call (one launch per 32 tensors) on the parameters
    that have a gradient.  With max_grad_norm the norm over the gradients of ALL groups is taken first, once, and every
    update reads the clip coefficient from the device (ops.grad_norm_clip); p.grad is left as it is."""
    _second = None      # the state key beside 'exp_avg'
    _op = None

    def _check_and_init(self, params, lr, betas, eps, weight_decay, max_grad_norm):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if eps < 0.0:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("Invalid max_grad_norm value: {}".format(max_grad_norm))
        self.grad_norm = None
        self.clip_coef = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        if max_grad_norm is not None:       # a group default only when asked for: without it the groups are torch's, key for key
            defaults["max_grad_norm"] = max_grad_norm
        torch.optim.Optimizer.__init__(self, params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        if "max_grad_norm" in self.defaults:        # a state_dict written by the torch optimizer has no such key
            for group in self.param_groups:
                group.setdefault("max_grad_norm", self.defaults["max_grad_norm"])
        self.__dict__.setdefault("grad_norm", None)
        self.__dict__.setdefault("clip_coef", None)

    def _clip_coef(self):
        """None without max_grad_norm; else the device coefficient of this step (the norm over every group's gradients)"""
        limits = {g.get("max_grad_norm") for g in self.param_groups}
        if limits == {None}:
            return None
        if len(limits) != 1:
            raise ValueError("max_grad_norm: one value for all param groups expected (the norm is global), got %r"
                             % sorted(limits, key=repr))
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not grads:
            return None
        if any(g.is_sparse for g in grads):
            raise RuntimeError("%s does not support sparse gradients" % type(self).__name__)
        grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
        self.grad_norm, self.clip_coef = ops.grad_norm_clip(grads, limits.pop())
        return self.clip_coef

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        coef = self._clip_coef()
        kw = {} if coef is None else {"grad_scale": coef}
        for group in self.param_groups:
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("%s does not support sparse gradients" % type(self).__name__)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st[self._second] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_step.setdefault(int(st["step"].item()), []).append((p, g, st["exp_avg"], st[self._second]))
            beta1, beta2 = group["betas"]
            for step, items in by_step.items():
                type(self)._op([i[0] for i in items], [i[1] for i in items], [i[2] for i in items],
                               [i[3] for i in items], step, group["lr"], beta1, beta2, group["eps"],
                               group["weight_decay"], **kw)
        return loss


class Adam(_MultiTensorOptimizer):
    """torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0) (solver.py:29)
    with every parameter of a group updated by one vqf_adam_step call.  State layout
    ('step', 'exp_avg', 'exp_avg_sq') and param_groups match torch's, so `param_group['lr'] = ...`
    (solver.py:47-50) and optimizer state_dicts interchange with torch.optim.Adam.

    max_grad_norm=None is that optimizer, launch for launch.  With a value, step() is
    torch.nn.utils.clip_grad_norm_(all parameters, max_grad_norm) followed by the update, in two kinds of launches: the
    norm over every gradient of every group, then the update kernel reading the clip coefficient from the device.  The
    gradients in memory are NOT scaled (p.grad after step() is p.grad before it); parameters and state have the bits of
    clip_grad_norm_ + the plain step.  After step(), `grad_norm` and `clip_coef` are the 0-d GPU tensors of that step
    (None before the first one).  The value is a group default ('max_grad_norm', one value for all groups)."""
    _second = "exp_avg_sq"
    _op = staticmethod(ops.adam_step)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None):
        self._check_and_init(params, lr, betas, eps, weight_decay, max_grad_norm)


class Adamax(_MultiTensorOptimizer):
    """torch.optim.Adamax(params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0), the optimizer of
    bottom-up-attention style training, with every parameter of a group updated by one vqf_adamax_step call in the order
    of torch's single-tensor path.  State layout ('step', 'exp_avg', 'exp_inf') and param_groups match torch's:
    state_dicts interchange with torch.optim.Adamax both ways.  max_grad_norm: as in Adam."""
    _second = "exp_inf"
    _op = staticmethod(ops.adamax_step)

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None):
        self._check_and_init(params, lr, betas, eps, weight_decay, max_grad_norm)
