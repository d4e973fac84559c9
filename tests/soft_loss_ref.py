"""fp64 reference and error bounds of BCE-with-logits on soft answers (csrc/train.hip: bce_rows_kernel, bce_finish_kernel).

Plain torch in float64 on the CPU.  reference(logits, target, c) takes the fp32 inputs as they are (converted exactly) and the
dense target -- for a SoftAnswers, its .dense(A) -- and returns the row losses, the loss, the gradient, the arg-max and the
score.  The bounds below are conditions derived from the kernel's code, not measurements: they count its roundings.

u = 2^-24 is half an fp32 ulp, the relative error of one correctly rounded fp32 operation; a function documented to "k ulp" is
allowed 2 k u.  The library is compiled with -ffp-contract=off, so every product and sum below rounds on its own.

Per-call allowances of the device math library.  The ROCm installation ships no device-math accuracy document (its share/
tree holds none), so no file can be cited; the allowances used are the OpenCL C single-precision requirements that ROCm's
device library (OCML) is specified to meet: exp 3 ulp, log1p 2 ulp, x / y 2.5 ulp (hipcc's default
fp32 division is correctly rounded, 0.5 ulp; the wider allowance is kept).

Loss.  Per element the kernel forms e = expf(-|x|), l = log1pf(e), m = fmaxf(x, 0) (exact), p = x * t, q = m - p, term = q + l.
  l: its own 2 * LOG1P_ULP u plus the error of e passed on, at most 2 * EXP_ULP u relative (d log1p(e) / log1p(e) <= de / e);
  p, q, term: one rounding each, each relative to at most |m| + |p| + l.
  -> (3 + 2 (EXP_ULP + LOG1P_ULP)) u (|m| + |p| + l) per term.
Sums, each add one rounding relative to at most the sum of the absolute terms: the per-thread run of ceil(A / 256) adds, the
tree of 6 shuffle levels + 3 adds, the finish sum over N the same way (ceil(N / 256) + 9).  The sparse form adds K products, K
adds and one subtraction (2 K + 1), on terms |s_k x| that are the |p| of the dense target for non-negative scores (what the
tests use); where an id repeats, the fp32 dense target the reference reads is itself a sum of up to K scores, K - 1 roundings
away from the exact one.  3 K in all, for the sparse form only: the dense form is counted with K = 0.  The scale: c = (float)scale
and loss = s * c, 2 roundings.  One more for the second-order terms of the 40 to 90 first-order ones.
A value below the smallest normal fp32 (exp(-|x|) for |x| > 87) may be flushed: an absolute 2^-126 per element.

Gradient, per element, (sigma - t) * c with sigma = r or e * r, r = 1 / (1 + e):
  1 + e: 1 u, plus e's error weighted by e / (1 + e) <= 1/2: EXP_ULP u; the divide 2 DIV_ULP u; x < 0: e's 2 EXP_ULP u and the
  product's 1 u  ->  sigma within (3 EXP_ULP + 2 DIV_ULP + 2) u relative;
  sigma - t, * c, c's own rounding: 3 u relative to at most max(sigma, t) c.
  -> (3 EXP_ULP + 2 DIV_ULP + 5 + 1) u * c * max(sigma, |t|), plus c * 2^-126 for a flushed e.
  An id that repeats r times: the kernel adds its scores in slot order, the dense target in the order of its builder; each is
  r - 1 roundings from the exact sum: 2 (r - 1) u c |t| more (grad_bound's `repeats`).
"""
import math

import torch
import torch.nn.functional as F

THREADS = 256                # TR_THREADS of csrc/train.hip
U = 2.0 ** -24
EXP_ULP, LOG1P_ULP, DIV_ULP = 3.0, 2.0, 2.5
TINY = 2.0 ** -126


def loss_roundings(N, A, K=0):
    """K: the slots per row of the sparse form; 0 for a dense target"""
    per_term = 3 + 2 * (EXP_ULP + LOG1P_ULP)
    row = math.ceil(A / THREADS) + 9
    sparse = 3 * K
    finish = math.ceil(N / THREADS) + 9
    return per_term + row + sparse + finish + 2 + 1


GRAD_ROUNDINGS = 3 * EXP_ULP + 2 * DIV_ULP + 5 + 1


def reference(logits, target, c):
    """logits, target (N, A) fp32 CPU tensors, c a Python float -> dict of float64 / int64 CPU tensors:
    row_loss (N,), loss (), grad (N, A), pred (N,), score (N,) = target[n, pred[n]] (fp32, a copy), abs_terms () = the sum of
    |max(x,0)| + |x t| + log1p(exp(-|x|)) over all elements, sigma (N, A)."""
    x, t = logits.double(), target.double()
    sp = torch.log1p(torch.exp(-x.abs()))
    terms = x.clamp(min=0) - x * t + sp
    sigma = torch.sigmoid(x)
    pred = torch.argmax(logits, dim=1)
    return {"row_loss": terms.sum(1), "loss": terms.sum() * c, "grad": (sigma - t) * c, "pred": pred,
            "score": target.gather(1, pred.unsqueeze(1)).squeeze(1), "sigma": sigma,
            "abs_terms": (x.clamp(min=0) + (x * t).abs() + sp).sum()}


def loss_bound(ref, N, A, c, K=0):
    return loss_roundings(N, A, K) * U * float(ref["abs_terms"]) * c + N * A * TINY * c


def grad_bound(ref, target, c, repeats=1):
    """(N, A) float64: the allowance of every gradient element; repeats: the most slots of a row that may share an id"""
    t = target.double().abs()
    return GRAD_ROUNDINGS * U * c * torch.maximum(ref["sigma"], t) + 2 * (repeats - 1) * U * c * t + c * TINY


def score_bound(ref, repeats=1):
    """(N,) float64: score = t[n, pred[n]] is a copy (bound 0, bit equality) unless an id repeats: the kernel adds that id's
    scores in slot order, the dense target in its builder's order, each r - 1 roundings from the exact sum"""
    return 2 * (repeats - 1) * U * ref["score"].double().abs()


def scale_of(reduction, N, A):
    return 1.0 / N if reduction == "batchmean" else 1.0 / (N * A)


def torch_bce(logits, target, reduction):
    """the criterion torch defines, in float64 on the CPU: the self-check's yardstick"""
    x, t = logits.double(), target.double()
    if reduction == "batchmean":
        return F.binary_cross_entropy_with_logits(x, t, reduction="sum") / x.shape[0]
    return F.binary_cross_entropy_with_logits(x, t)


def perm_rows(N, A, amp, seed):
    """tie-free rows: every row a permutation of A distinct values spanning [-amp, amp] (A = 1: the value amp / 2)"""
    g = torch.Generator().manual_seed(seed)
    base = torch.linspace(-amp, amp, A, dtype=torch.float64) if A > 1 else torch.tensor([amp / 2], dtype=torch.float64)
    rows = [base[torch.randperm(A, generator=g)] for _ in range(N)]
    return torch.stack(rows).float().contiguous()


def soft_slots(N, A, K, seed, distinct=True):
    """ids (N, K) int64 in [0, A) (distinct per row when asked: needs K <= A), scores (N, K) fp32 from {0.3, 0.6, 0.9, 1.0}
    rounded to fp32, the min(1, count / 3) scores of the annotators"""
    g = torch.Generator().manual_seed(seed)
    if distinct:
        ids = torch.stack([torch.randperm(A, generator=g)[:K] for _ in range(N)])
    else:
        ids = torch.randint(0, A, (N, K), generator=g)
    vals = torch.tensor([0.3, 0.6, 0.9, 1.0], dtype=torch.float32)
    scores = vals[torch.randint(0, 4, (N, K), generator=g)]
    return ids.to(torch.int64).contiguous(), scores.contiguous()
