"""fp64 restatements of the optimizer tail (csrc/train.hip: gradient-norm clipping, Adam and Adamax reading the clip
coefficient): the total norm, the coefficient with its fp32 formation, clip-then-Adam, clip-then-Adamax, and the error
bound of the norm kernel counted from its code.  Shared by test_optim_tail_ref_cpu.py (which holds these against torch in
fp64) and test_gpu_optim_tail.py."""
import math

import numpy as np
import torch

import recipe

# the case of tests/test_gpu_train_step.py::_adam_case
P_AMP, G_AMP, LR0 = 0.5, 0.1, 7e-4
# one element, the scalar tail, exactly / one under / one over a block of 4096 elements, several blocks
SHAPES = [(1,), (3,), (7,), (33, 5), (4095,), (4096,), (4097,), (3, 5000)]
# three launches of 32 tensors, ragged
MANY_SHAPES = [(i % 7 + 1, 3 + i) for i in range(70)]


def sym(name, shape, amp):
    return torch.from_numpy(recipe.sym_tensor(tuple(shape), amp, recipe.name_seed(name, 0)))


def case_params(shapes):
    return [sym("adam.p%d" % i, s, P_AMP) for i, s in enumerate(shapes)]


def case_grads(shapes, step):
    return [sym("adam.g%d.%d" % (i, step), s, G_AMP) for i, s in enumerate(shapes)]


def case_lr(step):
    return LR0 * (0.5 if step >= 3 else 1.0)      # halved after step 3


def total_norm(grads):
    """sqrt of the sum of squares over every tensor, in fp64 -> python float"""
    s = 0.0
    for g in grads:
        s += float((g.detach().double().cpu() ** 2).sum())
    return math.sqrt(s)


def clip_coef(norm, max_norm):
    """The coefficient from an fp32 norm, formed in fp32 as torch.nn.utils.clip_grad_norm_ forms it:
    `max_norm / (norm + 1e-6)` is (norm + 1e-6).reciprocal() * max_norm, then clamp(max=1), which keeps a NaN -> np.float32"""
    with np.errstate(all="ignore"):
        n = np.float32(norm)
        c = (np.float32(1.0) / (n + np.float32(1e-6))) * np.float32(max_norm)
        return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def clip_scale(grads, max_norm):
    """-> (norm, coef, the clipped gradients in fp64): the norm from the fp64 sum, rounded to fp32 as the kernel stores it"""
    norm = np.float32(total_norm(grads))
    coef = clip_coef(norm, max_norm)
    return norm, coef, [g.double() * float(coef) for g in grads]


def adam_update(p, g, st, lr, wd, beta1=0.9, beta2=0.999, eps=1e-8):
    """one torch.optim.Adam step (single-tensor path) on fp64 tensors, in place; st: {'step', 'exp_avg', 'exp_avg_sq'}"""
    if not st:
        st.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
    st["step"] += 1
    if wd != 0:
        g = g + wd * p
    st["exp_avg"] += (g - st["exp_avg"]) * (1 - beta1)
    st["exp_avg_sq"].mul_(beta2).add_((1 - beta2) * g * g)
    bc1, bc2 = 1 - beta1 ** st["step"], 1 - beta2 ** st["step"]
    denom = st["exp_avg_sq"].sqrt() / math.sqrt(bc2) + eps
    p -= (lr / bc1) * st["exp_avg"] / denom


def adamax_update(p, g, st, lr, wd, beta1=0.9, beta2=0.999, eps=1e-8):
    """one torch.optim.Adamax step (single-tensor path) on fp64 tensors, in place; st: {'step', 'exp_avg', 'exp_inf'}"""
    if not st:
        st.update(step=0, exp_avg=torch.zeros_like(p), exp_inf=torch.zeros_like(p))
    st["step"] += 1
    if wd != 0:
        g = g + wd * p
    st["exp_avg"] += (g - st["exp_avg"]) * (1 - beta1)
    st["exp_inf"] = torch.maximum(st["exp_inf"] * beta2, g.abs() + eps)
    p -= (lr / (1 - beta1 ** st["step"])) * st["exp_avg"] / st["exp_inf"]


def run(rule, shapes, steps, wd, max_norm):
    """fp64: `steps` steps of clip (max_norm None: no clipping) then Adam / Adamax on the case -> (params, norms)"""
    update = {"adam": adam_update, "adamax": adamax_update}[rule]
    ps = [p.double() for p in case_params(shapes)]
    sts = [dict() for _ in ps]
    norms = []
    for step in range(steps):
        gs = case_grads(shapes, step)
        if max_norm is None:
            gs = [g.double() for g in gs]
        else:
            norm, _, gs = clip_scale(gs, max_norm)
            norms.append(float(norm))
        for p, g, st in zip(ps, gs, sts):
            update(p, g, st, case_lr(step), wd)
    return ps, norms


# ---- the norm kernel's error bound ---------------------------------------------------------------------------------------
# Counted from grad_sumsq_kernel / grad_norm_finish_kernel (the library is built with -ffp-contract=off: a square and an add are
# two roundings).  Every term is non-negative, so a value that went through k roundings carries a relative error of at most
# (1 + u)^k - 1, and so does any sum of such values:
#   a thread:  1 rounding for a square, then at most 16 adds on the way to the thread's sum (its 16 elements in order)
#   the wave:  6 butterfly adds
#   the block: 3 adds of the four wave sums
# = 26 roundings of u = 2^-24 on the sum of squares.  The finish adds the partials in double (P adds of 2^-53: nothing beside
# u for any P < 2^20), takes the double root -- which halves the relative error -- and rounds once to fp32.
U32 = 2.0 ** -24
SUMSQ_ROUNDINGS = 1 + 16 + 6 + 3


def norm_bound_rel(partials=1):
    """relative bound of the fp32 norm against the fp64 one"""
    sumsq = (1 + U32) ** SUMSQ_ROUNDINGS - 1 + (partials + 2) * 2.0 ** -53
    return (math.sqrt(1 + sumsq) - 1) * (1 + U32) + U32


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))
