"""fp64 references, with an ELEMENT-WISE error bound per output, of HieCoAtten's streaming passes (vqf_hie_hv_fwd, vqf_hie_head_bwd,
vqf_hie_rank_add, vqf_hie_rank_left, vqf_hie_slab_sum) and of the small kernels only HieCoreFn uses.  Plain torch, written from the
formulas of include/vqa_fusion.h, not from the kernels.  Every function takes fp64 tensors (the fp32 operands of the kernel,
widened exactly) and returns {output name: (value, bound)}: a kernel passes when |got - value| <= bound at EVERY element.

The bounds (u = 2^-23: twice the fp32 unit roundoff, so that fused multiply-adds and any order of summation are covered):
  * a sum of K fp32 products, any order:            (K + 2) u sum|terms|   (the abs-sum is evaluated next to the sum)
  * a sum over rows that are kernel outputs:        + the sum of |coefficient| x the rows' own bound
  * dropout(tanh(arg)), |tanh'| <= 1:               (bound_arg + 2e-7) / (1 - p) + u |value|; 2e-7 = the header's absolute accuracy of
                                                    the fast tanh; exactly 0 where the mask drops
  * dl w sc (1 - t^2), t = hv / sc:                 8 u |dl w sc|   (the cancellation in 1 - t^2 is absolute in a quantity <= 1)
Shapes: a, z, hv, out (N, L, E); C, U (N, T, L); V (N, T, E); keep (N, L, E) of 0 / 1 or None; part (N, T, E) -- or, with Lc (the
rows per chunk of an S-chunk split), `slabs` (S, N, T, E) as well; colpart / wpart (S, N, E): one row per chunk and sample."""
import torch

U = 2.0 ** -23
TANH_ABS = 2e-7


def _scale(keep, p, like):
    """keep / (1 - p) per element (ones without dropout) and 1 / (1 - p)"""
    if keep is None:
        return torch.ones_like(like), 1.0
    inv = 1.0 / (1.0 - p)
    return keep.to(like.dtype) * inv, inv


def _chunks(L, Lc):
    Lc = L if Lc is None else Lc
    return [(l0, min(L, l0 + Lc)) for l0 in range(0, L, Lc)]


def rank_t(Um, V):
    """sum_t Um[n,t,l] V[n,t,:] -> (value, abs-sum), (N, L, E)"""
    return torch.einsum("ntl,nte->nle", Um, V), torch.einsum("ntl,nte->nle", Um.abs(), V.abs())


def row_sums(Um, X, Xb, Lc):
    """The T-row sums sum_l Um[n,t,l] X[n,l,:] per chunk of Lc rows: (S, N, T, E) values and bounds.  Xb: the element-wise bound
    of X when X is itself a kernel output (or None)."""
    L = Um.shape[2]
    vals, bnds = [], []
    for l0, l1 in _chunks(L, Lc):
        u, x = Um[:, :, l0:l1], X[:, l0:l1]
        b = (l1 - l0 + 2) * U * torch.einsum("ntl,nle->nte", u.abs(), x.abs())
        if Xb is not None:
            b = b + torch.einsum("ntl,nle->nte", u.abs(), Xb[:, l0:l1])
        vals.append(torch.einsum("ntl,nle->nte", u, x))
        bnds.append(b)
    return torch.stack(vals), torch.stack(bnds)


def col_sums(X, Xb, Lc):
    """Column sums of the rows of each chunk of a kernel output X with bound Xb: (S, N, E)"""
    L = X.shape[1]
    vals, bnds = [], []
    for l0, l1 in _chunks(L, Lc):
        vals.append(X[:, l0:l1].sum(1))
        bnds.append((l1 - l0 + 2) * U * X[:, l0:l1].abs().sum(1) + Xb[:, l0:l1].sum(1))
    return torch.stack(vals), torch.stack(bnds)


def tanh_drop(arg, arg_bound, keep, p):
    """dropout(tanh(arg)) given the pre-activation and its bound"""
    sc, inv = _scale(keep, p, arg)
    val = torch.tanh(arg) * sc
    return val, ((arg_bound + TANH_ABS) * inv + U * val.abs()) * (sc > 0).to(arg.dtype)


def hv_fwd(a, C, V, keep=None, p=0.0, Lc=None):
    """out = dropout(tanh(a + C^T V)); part[t] = sum_l C[t,l] a[l]"""
    T, L = C.shape[1], C.shape[2]
    r, rabs = rank_t(C, V)
    arg, arg_b = a + r, (T + 3) * U * (a.abs() + rabs)
    out = tanh_drop(arg, arg_b, keep, p)
    slabs, slab_b = row_sums(C, a, None, Lc)
    part = (torch.einsum("ntl,nle->nte", C, a), (L + 2) * U * torch.einsum("ntl,nle->nte", C.abs(), a.abs()))
    return {"out": out, "part": part, "slabs": (slabs, slab_b)}


def head_bwd(hv, dl, w, C, keep=None, p=0.0, part_add=None, Lc=None):
    """out = dl[l] w sc (1 - (hv / sc)^2), sc = keep / (1 - p); part[t] = (part_add[t] +) sum_l C[t,l] out[l];
    wpart = [sum_l dl[l] hv[l,:] | sum_l dl[l]] per chunk.  dl (N, L), w (E)."""
    L = C.shape[2]
    sc, _ = _scale(keep, p, hv)
    t = torch.where(sc > 0, hv / sc.clamp_min(1e-300), torch.zeros_like(hv))
    lin = dl[:, :, None] * w[None, None, :] * sc
    out, out_b = lin * (1.0 - t * t), 8 * U * lin.abs()
    slabs, slab_b = row_sums(C, out, out_b, Lc)
    K = L + (1 if part_add is not None else 0)
    pabs = torch.einsum("ntl,nle->nte", C.abs(), out.abs())
    part = torch.einsum("ntl,nle->nte", C, out)
    if part_add is not None:
        part, pabs = part + part_add, pabs + part_add.abs()
    part_b = (K + 2) * U * pabs + torch.einsum("ntl,nle->nte", C.abs(), out_b)
    wv, wb, sv, sb = [], [], [], []
    for l0, l1 in _chunks(L, Lc):
        d, h = dl[:, l0:l1], hv[:, l0:l1]
        wv.append(torch.einsum("nl,nle->ne", d, h))
        wb.append((l1 - l0 + 2) * U * torch.einsum("nl,nle->ne", d.abs(), h.abs()))
        sv.append(d.sum(1))
        sb.append((l1 - l0 + 2) * U * d.abs().sum(1))
    return {"out": (out, out_b), "part": (part, part_b), "slabs": (slabs, slab_b),
            "wpart": (torch.stack(wv), torch.stack(wb)), "dlsum": (torch.stack(sv), torch.stack(sb))}


def rank_add(a, Um, V, Lc=None):
    """out = a + Um^T V; colpart = the column sums of each chunk's rows of out"""
    T = Um.shape[1]
    r, rabs = rank_t(Um, V)
    out, out_b = a + r, (T + 3) * U * (a.abs() + rabs)
    return {"out": (out, out_b), "colpart": col_sums(out, out_b, Lc)}


def rank_left(Um, V, z, Lc=None):
    """out = Um^T V; part[t] = sum_l Um[t,l] z[l]; colpart as rank_add"""
    T, L = Um.shape[1], Um.shape[2]
    r, rabs = rank_t(Um, V)
    out, out_b = r, (T + 2) * U * rabs
    part = (torch.einsum("ntl,nle->nte", Um, z), (L + 2) * U * torch.einsum("ntl,nle->nte", Um.abs(), z.abs()))
    return {"out": (out, out_b), "part": part, "slabs": row_sums(Um, z, None, Lc), "colpart": col_sums(out, out_b, Lc)}


def slab_sum(part, add=None):
    """out = (add +) sum_s part[s]; part (S, R, W), the slabs as GIVEN (they are this kernel's operands)"""
    S = part.shape[0]
    val, ab = part.sum(0), part.abs().sum(0)
    if add is not None:
        val, ab = val + add, ab + add.abs()
    return val, (S + 1) * U * ab


# ---------------------------------------------------------------------------------------------------------------
# the small kernels only HieCoreFn uses
def relu_bwd_rank1(dx, y, wts, dpooled, L, scale):
    """dXpre[m,c] = (dx[m,c] + wts[m] dpooled[m // L, c]) * (y[m,c] > 0 ? scale : 0); dbias = its column sums (K = M)"""
    M = y.shape[0]
    r1 = torch.zeros_like(dx) if wts is None else wts[:, None] * dpooled.repeat_interleave(L, 0)[:M]
    on = (y > 0).to(dx.dtype)
    val = (dx + r1) * on * scale
    b = 4 * U * (dx.abs() + r1.abs()) * scale * on
    return {"dpre": (val, b), "dbias": (val.sum(0), (M + 2) * U * val.abs().sum(0) + b.sum(0))}


def tanh_dropout_fwd2d(a, b, keep=None, p=0.0):
    arg = a if b is None else a + b
    return tanh_drop(arg, U * (a.abs() + (0 if b is None else b.abs())), keep, p)


def tanh_dropout_bwd2d(dy, y, keep=None, p=0.0):
    """dx = dy sc (1 - (y / sc)^2) with the stored y as the operand"""
    sc, inv = _scale(keep, p, y)
    t = torch.where(sc > 0, y / sc.clamp_min(1e-300), torch.zeros_like(y))
    return dy * sc * (1.0 - t * t), 8 * U * dy.abs() * inv * (sc > 0).to(y.dtype)


def embed_dropout_fwd(W, ids, keep=None, p=0.0):
    """dropout(W[ids]); an id outside [0, V) gives a zero row.  Exact when 1 / (1 - p) is a power of two."""
    V = W.shape[0]
    ok = (ids >= 0) & (ids < V)
    rows = W[ids.clamp(0, V - 1)] * ok[:, None].to(W.dtype)
    sc, inv = _scale(keep, p, rows)
    val = rows * sc
    exact = inv in (1.0, 2.0, 4.0)
    return val, (0.0 if exact else U) * val.abs()


def embed_dropout_bwd(dout, ids, V, keep=None, p=0.0):
    """dW[v] = sum over the tokens with id v of dout sc; rows of ids that never occur are exactly zero"""
    sc, _ = _scale(keep, p, dout)
    g = dout * sc
    ok = (ids >= 0) & (ids < V)
    val = torch.zeros((V, dout.shape[1]), dtype=dout.dtype).index_add_(0, ids[ok], g[ok])
    ab = torch.zeros_like(val).index_add_(0, ids[ok], g[ok].abs())
    cnt = torch.bincount(ids[ok], minlength=V).to(dout.dtype)
    return val, (cnt[:, None] + 2) * U * ab


def multi_add(a, b):
    return a + b, 3 * U * (a.abs() + b.abs())


def att_logits_fwd_lin(hid, w2, b2, b1):
    """logits = hid w2^T + b2: a K = Hh + 1 sum (b2 is its last term), hence Hh + 3; lin[m,g] = sum_{j: hid[m,j] > 0} w2[g,j]
    (hid[m,j] - b1[j]): a K = Hh sum of the terms w2 (hid - b1) -- the one rounding of the subtraction is relative to |hid - b1|
    and sits inside the + 2 at u = 2^-23"""
    Hh = hid.shape[1]
    logits = hid @ w2.t() + b2
    lb = (Hh + 3) * U * (hid.abs() @ w2.abs().t() + b2.abs())
    on = (hid > 0).to(hid.dtype)
    lin = ((hid - b1) * on) @ w2.t()
    nb = (Hh + 2) * U * (((hid - b1).abs() * on) @ w2.abs().t())
    return {"logits": (logits, lb), "lin": (lin, nb)}
