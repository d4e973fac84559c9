"""fp64 reference of the MFB fusion entry points (include/vqa_fusion.h: vqf_mfb_fuse_fwd / _bwd and their bf16, _grouped, _len,
_packed, _grouped_packed and _packed_rows forms), in plain torch: the two functions restate what the header promises and nothing of
how csrc/fusion.hip gets there (no threads, no waves, no row splits, no LDS).  tests/test_mfb_fuse_ref_cpu.py pins this file on
tests/mfb_regions_ref.fuse_ref (forward) and on torch autograd of the same chain (backward).

Operands are fp64 tensors holding fp32 (or bf16) values.  One pair of functions covers every form through optional arguments:
  idx       (N) owner image of each question: P is (U L, 5 O), or with roff the packed rows of the U images
  lens      (N) real rows of each QUESTION (the caller's gather lens_u[idx] in the grouped forms), clamped to [1, L]
  roff      (owners + 1) row offsets: P / dP hold the real rows only, owner s has rows roff[s] .. roff[s + 1] - 1
  rows_out  with roff, un-grouped: R / rowssq (forward) and dY / Y (backward) are in the packed row coordinates too
  cascade   (N L, 5 O) third factor;  keep  (N L, 5 O) bool, the explicit mask (philox_ref.keep16 for the in-kernel draw);
  p         the drop probability: a kept element is scaled by the fp32 philox_ref.inv_keep(p) whenever a mask is given
Whatever the padded rows of P, dY and Y hold (NaN in the tests) never reaches an output.

Every output comes with what a per-element bound needs: the forward returns the pooled sums s and A = sum |terms| beside
R = ssqrt(s); the backward returns every gradient with the sum |terms| behind it under name + "_abs", the magnitude of
dS = (coefA dY - coefB Y) 0.5 inv / |Y| being (|coefA dY| + |coefB Y|) 0.5 inv / |Y|."""
import numpy as np
import torch

import philox_ref as PR

U = 2.0 ** -24                               # fp32 unit roundoff
KP = 5                                       # the pooling window


def g(k):
    """(1 + u)^k - 1: the relative error of a value that passed k fp32 roundings"""
    return (1.0 + U) ** k - 1.0


def scale_of(keep, p):
    """the factor of a kept element: fp32 1 / (1 - p) with a mask, 1 without"""
    return 1.0 if keep is None else float(PR.inv_keep(p))


def ssqrt(s):
    """sqrt(relu(s)) - sqrt(relu(-s))"""
    return torch.sign(s) * s.abs().sqrt()


def _spans(N, L, idx, lens, roff):
    """-> owner (N) int64, start (N) first row of P (None: owner * L), cnt (N) real rows, valid (N, L) bool"""
    owner = torch.arange(N) if idx is None else torch.as_tensor(idx, dtype=torch.int64)
    if roff is not None:
        roff = torch.as_tensor(roff, dtype=torch.int64)
        start, cnt = roff[owner], (roff[owner + 1] - roff[owner]).clamp(1, L)
    else:
        start = None
        cnt = torch.full((N,), L, dtype=torch.int64) if lens is None else torch.as_tensor(lens, dtype=torch.int64).clamp(1, L)
    return owner, start, cnt, torch.arange(L)[None, :] < cnt[:, None]


def _prow(owner, start, L):
    """(N, L) the row of P behind (n, l) (meaningful where valid)"""
    first = owner * L if start is None else start
    return first[:, None] + torch.arange(L)[None, :]


def _gather(P, rowmap, valid):
    """P (rows, W) -> (N, L, W): row rowmap[n, l] where valid, exact zeros elsewhere (a padded row is never read)"""
    out = torch.zeros(valid.shape + (P.shape[1],), dtype=P.dtype)
    out[valid] = P[rowmap[valid]]
    return out


def _padded(x, rowmap, valid, rows_out):
    """a per-row operand (N L, W) -- or, rows_out, (Rtot, W) at the packed rows -- as (N, L, W) with exact zeros on padded rows"""
    N, L = valid.shape
    if rows_out:
        return _gather(x, rowmap, valid)
    x = x.view(N, L, -1)
    return torch.where(valid[:, :, None], x, torch.zeros_like(x))


def fuse_fwd(P, pbias, q, N, L, O, keep=None, p=0.0, cascade=None, idx=None, lens=None, roff=None, rows_out=False):
    """-> dict: s, A (N, L, O) pooled sums and their sum |terms|; R = ssqrt(s); rowabs (N, L) = sum_o |s|; rowA (N, L) = sum_o A;
    zdrop (N, L, 5 O) the dropped-out product; valid (N, L).  Padded rows: exact zeros.  rows_out: R, s, A (Rtot, O) and rowabs,
    rowA (Rtot) at the packed rows instead (no padded row exists there)."""
    W5 = KP * O
    owner, start, cnt, valid = _spans(N, L, idx, lens, roff)
    rowmap = _prow(owner, start, L)
    z = _gather(P, rowmap, valid)
    if pbias is not None:
        z = z + pbias
    z = z * q[:, None, :]
    if cascade is not None:
        z = z * cascade.view(N, L, W5)
    if keep is not None:
        z = z * (keep.view(N, L, W5).double() * scale_of(keep, p))
    z = torch.where(valid[:, :, None], z, torch.zeros_like(z))
    s, A = z.view(N, L, O, KP).sum(3), z.abs().view(N, L, O, KP).sum(3)
    out = dict(s=s, A=A, R=ssqrt(s), rowabs=s.abs().sum(2), rowA=A.sum(2), zdrop=z, valid=valid)
    if rows_out:
        Rtot = P.shape[0]
        for k in ("s", "A", "R", "rowabs", "rowA"):
            v = out[k]
            packed = torch.zeros((Rtot,) + tuple(v.shape[2:]), dtype=torch.float64)
            packed[rowmap[valid]] = v[valid]
            out[k] = packed
    return out


def fuse_bwd(dY, Y, inv, coefA, coefB, P, pbias, q, N, L, O, keep=None, p=0.0, cascade=None, dzdrop=None, idx=None, lens=None,
             roff=None, rows_out=False):
    """The header's formulas on the kernel's own operands:
        dS = (coefA dY - coefB Y) 0.5 inv / |Y|, 0 where Y == 0 (-0.0 too);   dz = (dS + dzdrop) keep / (1 - p);
        dP = dz q (cascade);  dq = sum_l dz (P + pbias) (cascade);  dcascade = dz (P + pbias) q;  dbiasP = column sums of dP.
    -> dict: dz, dP, dq, dcascade (None without cascade), dbiasP and under name + "_abs" the sum |terms| of each.
    dP has the shape of P: (N L, 5 O) with exact zero padded rows, (U L, 5 O) summed over each image's questions with idx, the
    packed rows with roff.  dq (N, 5 O); dz / dcascade (N, L, 5 O) in the padded coordinates."""
    W5 = KP * O
    owner, start, cnt, valid = _spans(N, L, idx, lens, roff)
    rowmap = _prow(owner, start, L)
    v3 = valid[:, :, None]
    dY3, Y3 = _padded(dY, rowmap, valid, rows_out), _padded(Y, rowmap, valid, rows_out)
    cA, cB, hi = coefA[:, None, None], coefB[:, None, None], 0.5 * inv[:, None, None]
    live = (Y3 != 0) & v3
    ay = torch.where(live, Y3.abs(), torch.ones_like(Y3))
    zero = torch.zeros_like(Y3)
    dS = torch.where(live, (cA * dY3 - cB * Y3) * hi / ay, zero)
    dS_abs = torch.where(live, ((cA * dY3).abs() + (cB * Y3).abs()) * hi.abs() / ay, zero)
    dz, dz_abs = dS.repeat_interleave(KP, 2), dS_abs.repeat_interleave(KP, 2)
    if dzdrop is not None:
        dzd = dzdrop.view(N, L, W5)
        dz, dz_abs = dz + dzd, dz_abs + dzd.abs()
    if keep is not None:
        kf = keep.view(N, L, W5).double() * scale_of(keep, p)
        dz, dz_abs = dz * kf, dz_abs * kf
    dz, dz_abs = torch.where(v3, dz, torch.zeros_like(dz)), torch.where(v3, dz_abs, torch.zeros_like(dz))
    Pb = _gather(P, rowmap, valid)
    if pbias is not None:
        Pb = Pb + pbias
    qc = q[:, None, :].expand(N, L, W5)
    pc = Pb
    if cascade is not None:
        c3 = cascade.view(N, L, W5)
        qc, pc = qc * c3, Pb * c3
    dPq, dPq_abs = dz * qc, dz_abs * qc.abs()                      # per question row
    dq, dq_abs = (dz * pc).sum(1), (dz_abs * pc.abs()).sum(1)
    out = dict(dz=dz, dz_abs=dz_abs, dq=dq, dq_abs=dq_abs, dbiasP=dPq.sum((0, 1)), dbiasP_abs=dPq_abs.sum((0, 1)),
               dcascade=None, dcascade_abs=None, valid=valid)
    if cascade is not None:
        out["dcascade"], out["dcascade_abs"] = dz * Pb * q[:, None, :], dz_abs * (Pb * q[:, None, :]).abs()
    rows = P.shape[0]
    dP, dP_abs = torch.zeros(rows, W5, dtype=torch.float64), torch.zeros(rows, W5, dtype=torch.float64)
    dP.index_add_(0, rowmap[valid], dPq[valid])
    dP_abs.index_add_(0, rowmap[valid], dPq_abs[valid])
    out["dP"], out["dP_abs"] = dP, dP_abs
    return out


def philox_keep(N, L, O, seed, p):
    """the in-kernel draw of the fusion kernels as an explicit (N L, 5 O) bool tensor"""
    return torch.from_numpy(np.ascontiguousarray(PR.keep16((N * L, KP * O), seed, p)))
