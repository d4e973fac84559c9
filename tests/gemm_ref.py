"""fp64 reference of the GEMM entry points (include/vqa_fusion.h: vqf_gemm_f32, vqf_gemm_f32_rowscale, vqf_gemm_f32_batched,
vqf_gemm_f32_sample, vqf_gemm_bf16, vqf_gemm_bf16_rowscale) in plain numpy: it restates what the header promises,

    C[m, n] = relu?( rowscale[(row0 + m) / rps] * sum_k Aop[m, k] Bop[n, k] + bias[n] + C0[m, n] )

and nothing of how csrc/gemm_*.hip get there (no tiles, no slabs, no splits).  tests/test_gemm_ref_cpu.py pins it on torch.matmul.

Operands are fp32 arrays (for the bf16 kernels: fp32 arrays of bf16-representable values, see bf16_round).  product() returns,
beside the fp64 result, the fp64 array `terms` of the same shape: sum_k |a_k b_k| (times |rowscale|) + |bias| + |C0| of each
element.  tests/test_gpu_gemm_small.py bounds the kernel's error by bound(terms, k) = (k + 1) u terms element by element, k an
upper limit on the additions a term passes through and u = 2^-24 (fp32 round to nearest; a bf16 x bf16 product is exact in
fp32), and keeps max(terms) < 2^24 in its integer data set: every partial sum, in any order, is then an fp32 number and the
kernel must return the reference's bits."""
import numpy as np

U = 2.0 ** -24                                # fp32 unit roundoff, round to nearest
EXACT_LIMIT = 2.0 ** 24                       # integers below it are fp32 numbers


def _f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def operand(X, t):
    """the (..., rows, K) view of an operand stored (..., rows, K) (t = 0) or K-major (..., K, rows) (t = 1)"""
    return np.swapaxes(X, -1, -2) if t else X


def product(A, B, ta, tb, bias=None, c0=None, rowscale=None, rps=1, row0=0, relu=False):
    """A (M, K) or (K, M) with ta, B (N, K) or (K, N) with tb, both optionally behind one leading batch axis -> ref, terms
    (fp64, (..., M, N)).  bias (N), c0 (..., M, N): the output's earlier content under VQF_GEMM_ACCUM, rowscale: one scale per
    rps rows, the product's row m being row row0 + m of the scaled matrix; the scale applies to the sum and not to bias or c0,
    the ReLU comes last (gemm_f32.hip's epilogue order, which the header states)."""
    a, b = operand(_f64(A), ta), operand(_f64(B), tb)
    bt = np.swapaxes(b, -1, -2)
    ref, terms = np.matmul(a, bt), np.matmul(np.abs(a), np.abs(bt))
    if rowscale is not None:
        s = _f64(rowscale)[(row0 + np.arange(a.shape[-2])) // rps][:, None]
        ref, terms = ref * s, terms * np.abs(s)
    if bias is not None:
        ref, terms = ref + _f64(bias), terms + np.abs(_f64(bias))
    if c0 is not None:
        ref, terms = ref + _f64(c0), terms + np.abs(_f64(c0))
    if relu:
        ref = np.maximum(ref, 0.0)            # |relu(x) - relu(y)| <= |x - y|: the bound of the sum holds behind it
    return ref, terms


def bound(terms, k, u=U):
    """(k + 1) u terms: k additions and the product's own rounding"""
    return (k + 1) * u * terms


def bf16_round(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def bf16_trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits, as fp32 (what a kernel that loads the wrong half-words would compute)"""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def ints(shape, seed, lim):
    """seeded integers in [-lim, lim], fp32"""
    return _rng(seed).integers(-lim, lim + 1, size=shape).astype(np.float32)


def uniform(shape, seed, scale=1.0):
    """seeded uniform values in [-scale, scale], fp32"""
    return ((_rng(seed).random(size=shape) * 2 - 1) * scale).astype(np.float32)


def operands(kind, ta, tb, M, N, K, seed, batch=None, bias=False, c0=False, rowscale=0, bf16=False, relu_a=False):
    """The data of one case as a dict of fp32 arrays: A, B in their stored layouts, bias (N), c0 ((batch,) M, N), rowscale (one
    per `rowscale` rows, enough for M rows), absent keys = None.
    exact   integers in [-4, 4] for A, [-2, 2] for B, [-8, 8] for bias and c0, powers of two 1/4 .. 2 for rowscale: every value
            depends on its position (seeded draws)
    random  uniform +-1 for A (relu_a: max(0, N(0, 1)), the activations in front of the image projection), +-0.5 for B, +-1 for
            bias and c0, 0.25 <= |s| <= 1.25 for rowscale; bf16: rounded to bf16 values"""
    lead = () if batch is None else (batch,)
    sa = lead + ((K, M) if ta else (M, K))
    sb = lead + ((K, N) if tb else (N, K))
    d = dict(A=None, B=None, bias=None, c0=None, rowscale=None)
    if kind == "exact":
        d["A"], d["B"] = ints(sa, seed, 4), ints(sb, seed + 1, 2)
        if bias:
            d["bias"] = ints((N,), seed + 2, 8)
        if c0:
            d["c0"] = ints(lead + (M, N), seed + 3, 8)
        if rowscale:
            d["rowscale"] = np.exp2(_rng(seed + 4).integers(-2, 2, size=(-(-M // rowscale),))).astype(np.float32)
    else:
        d["A"] = np.maximum(_rng(seed).standard_normal(size=sa), 0).astype(np.float32) if relu_a else uniform(sa, seed)
        d["B"] = uniform(sb, seed + 1, 0.5)
        if bias:
            d["bias"] = uniform((N,), seed + 2)
        if c0:
            d["c0"] = uniform(lead + (M, N), seed + 3)
        if rowscale:
            s = uniform((-(-M // rowscale),), seed + 4)
            d["rowscale"] = np.where(s < 0, s - 0.25, s + 0.25).astype(np.float32)
        if bf16:
            d["A"], d["B"] = bf16_round(d["A"]), bf16_round(d["B"])
    return d


# ---- the check ----------------------------------------------------------------------------------------------------------------------
def check(got, ref, terms, k, u=U):
    """got (fp32 values) against ref: -> (worst err / bound over the elements, flat index of the worst).  An element whose bound is
    zero (all terms zero) must be equal: inf otherwise.  A NaN in got gives inf."""
    got = _f64(got).reshape(ref.shape)
    err = np.abs(got - ref)
    bnd = bound(terms, k, u)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(got) | np.isnan(ratio), np.inf, ratio)
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), i


def same_bits(got, ref):
    """exact data: got (fp32) holds the fp32 image of ref in every element -> (number of elements that differ, first such index).
    +0 and -0 count as the same value: a sum of exact terms that cancel has no sign to reproduce."""
    want = np.asarray(ref, dtype=np.float32)
    assert np.array_equal(want.astype(np.float64), ref), "the reference is not an fp32 number"
    bad = ~(np.asarray(got, dtype=np.float32).reshape(want.shape) == want)          # NaN: differs
    return int(bad.sum()), (int(np.argmax(bad)) if bad.any() else -1)
