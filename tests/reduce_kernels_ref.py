"""fp64 reference of the reduction and logit-head entry points (include/vqa_fusion.h: vqf_colsum_f32, vqf_group_reduce_f32,
vqf_relu_bwd_f32, vqf_relu_bwd_rank1_f32, vqf_scale_rows, vqf_rowdot, vqf_l2_group_norm, vqf_l2_norm_bwd_coef / _lin,
vqf_att_logits_fwd / _fwd_lin, vqf_att_logits_bwd / _rowscale), in plain torch: each function restates what the header promises
and nothing of how csrc/reduce.hip or csrc/attention.hip get there (no tiles, no slots, no partial rows).
tests/test_reduce_kernels_ref_cpu.py pins this file on torch autograd.

Operands are fp64 tensors holding fp32 values.  Every function that sums returns, beside each sum, the fp64 tensor of
sum |terms| of the same shape: tests/test_gpu_reduce_kernels.py bounds the kernel's error by (k + 1) 2^-24 sum |terms| element by
element (k: the longest chain of additions a term passes through), and keeps sum |terms| < 2^24 in its integer data set, where
the kernel must give the reference's bits."""
import numpy as np
import torch

U = 2.0 ** -24                               # fp32 unit roundoff
EPS = float(np.float32(1e-12))               # F.normalize's eps as the kernels hold it


def rnd(shape, seed, scale=1.0):
    """seeded uniform values in [-scale, scale], fp32-representable, as fp64"""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().double()


def ints(shape, seed, lo=-3, hi=3):
    """seeded integers in [lo, hi] as fp64: products and sums of them are exact in fp32 while sum |terms| < 2^24"""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).double()


def pow2(shape, seed, lo=-2, hi=2):
    """seeded powers of two 2^lo .. 2^hi: a product with one is exact"""
    return torch.pow(2.0, ints(shape, seed, lo, hi))


def _rows(M, L):
    return torch.arange(M) // L


# ---- column sums --------------------------------------------------------------------------------------------------------------------
def colsum(x):
    """x (M, N) -> db (N), sum |terms|"""
    return x.sum(0), x.abs().sum(0)


def group_reduce(x, G, J):
    """x (G J, W) -> out (G, W) = sum_j x[g J + j], sum |terms|"""
    v = x.view(G, J, -1)
    return v.sum(1), v.abs().sum(1)


def relu_bwd(dx, y):
    """-> dXpre = dX where Y > 0, else 0 (0.0 and -0.0: 0); dbias, its sum |terms|"""
    dpre = torch.where(y > 0, dx, torch.zeros_like(dx))
    return dpre, dpre.sum(0), dpre.abs().sum(0)


def relu_bwd_rank1(dx, y, wts, dpooled, L, scale):
    """dXpre[m, c] = (dX[m, c] + wts[m] dpooled[m / L, c]) (Y[m, c] > 0 ? scale : 0); wts None: no rank-1 term.
    -> dXpre, |dX| + |rank-1 term| scaled and masked (the terms of an element), dbias, its sum |terms|"""
    rank1 = torch.zeros_like(dx) if wts is None else wts[:, None] * dpooled[_rows(dx.shape[0], L)]
    zero = torch.zeros_like(dx)
    dpre = torch.where(y > 0, (dx + rank1) * scale, zero)
    mag = torch.where(y > 0, (dx.abs() + rank1.abs()) * abs(scale), zero)
    return dpre, mag, dpre.sum(0), mag.sum(0)


# ---- F.normalize over a sample's L rows ---------------------------------------------------------------------------------------------
def scale_rows(R, inv, L):
    """Y[m, :] = R[m, :] inv[m / L]"""
    return R * inv[_rows(R.shape[0], L)][:, None]


def rowdot(Y, dY):
    """-> rowdot[m] = sum_o Y dY, sum |terms|"""
    return (Y * dY).sum(1), (Y * dY).abs().sum(1)


def l2_group_norm(rowssq, N, L):
    """-> norm[n] = sqrt(sum_l rowssq[n L + l]), inv[n] = 1 / max(norm[n], 1e-12), sum |terms| of the sum under the root"""
    v = rowssq.view(N, L)
    norm = v.sum(1).sqrt()
    return norm, 1.0 / norm.clamp_min(EPS), v.abs().sum(1)


def l2_norm_bwd_coef(rdot, norm, inv, N, L):
    """dR = coefA dY - coefB Y: coefA = inv, coefB = inv sum_l rowdot (0 in the clamped branch, norm <= 1e-12) -> coefA, coefB,
    sum |terms| of coefB"""
    v = rdot.view(N, L)
    clamped = norm <= EPS
    zero = torch.zeros_like(norm)
    return inv.clone(), torch.where(clamped, zero, inv * v.sum(1)), torch.where(clamped, zero, inv.abs() * v.abs().sum(1))


def l2_norm_bwd_coef_lin(dl, lin, G, norm, inv, N, L):
    """the un-normalised form, dR = dYs - coefB R: coefB = inv^2 sum_{l, g} dlogits lin (0 in the clamped branch), coefA = unit = 1
    -> coefA, coefB, unit, sum |terms| of coefB"""
    t = (dl * lin).view(N, L * G)
    clamped = norm <= EPS
    zero, one = torch.zeros_like(norm), torch.ones_like(norm)
    return one, torch.where(clamped, zero, inv * inv * t.sum(1)), one.clone(), torch.where(clamped, zero, inv * inv * t.abs().sum(1))


# ---- the G-logit head ---------------------------------------------------------------------------------------------------------------
def att_logits_fwd(hid, w2, b2):
    """hid (M, Hh), w2 (G, Hh), b2 (G) -> logits (M, G), sum |terms| (the bias is a term)"""
    return hid @ w2.t() + b2, hid.abs() @ w2.abs().t() + b2.abs()


def att_logits_fwd_lin(hid, w2, b2, b1):
    """-> lin[m, g] = sum_{j: hid[m, j] > 0} w2[g, j] (hid[m, j] - b1[j]), sum |terms| (an exact zero of hid is excluded)"""
    xl = torch.where(hid > 0, hid - b1, torch.zeros_like(hid))
    return xl @ w2.t(), xl.abs() @ w2.abs().t()


def att_logits_bwd(dl, hid, w2, relu_mask, rowscale=None, rows_per_scale=1):
    """dl (M, G), hid (M, Hh), w2 (G, Hh), G in {1, 2, 3}; relu_mask: through the ReLU that made hid, relu'(0) = 0; rowscale: the
    STORED rows are multiplied by rowscale[m / rows_per_scale], dbias1 sums the unscaled rows.
    -> {dhid_pre (M, Hh), dw2 (G, Hh), db2 (G), dbias1 (Hh)} and, under name + "_abs", the sum |terms| of each"""
    t, tabs = dl @ w2, dl.abs() @ w2.abs()
    if relu_mask:
        zero = torch.zeros_like(t)
        t, tabs = torch.where(hid > 0, t, zero), torch.where(hid > 0, tabs, zero)
    rs = torch.ones(dl.shape[0], 1, dtype=torch.float64) if rowscale is None else rowscale[_rows(dl.shape[0], rows_per_scale)][:, None]
    return dict(dhid_pre=t * rs, dhid_pre_abs=tabs * rs.abs(), dw2=dl.t() @ hid, dw2_abs=dl.abs().t() @ hid.abs(),
                db2=dl.sum(0), db2_abs=dl.abs().sum(0), dbias1=t.sum(0), dbias1_abs=tabs.sum(0))
