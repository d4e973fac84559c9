"""tests/mfb_fuse_ref.py (the fp64 reference tests/test_gpu_mfb_fuse_kernels.py holds the fusion kernels to) pinned on the CPU, so
that the GPU test cannot share a mistake with its reference: the forward on tests/mfb_regions_ref.fuse_ref (itself pinned on the
oracle), the backward on torch autograd in fp64 of product -> dropout -> 5-wide sum-pool -> signed root -> F.normalize over the
sample.  The data here have one sign per pooling window and at least one kept element in each: autograd has no derivative at a
pooled sum of exactly zero, and this file tests the reference, not a kernel.  The reference is fed the fp64 Y, inv and the
coefA / coefB of reduce_kernels_ref.l2_norm_bwd_coef."""
import pytest
import torch
import torch.nn.functional as F

import mfb_fuse_ref as FR
import mfb_regions_ref as MR
import reduce_kernels_ref as RR

TOL = 1e-12           # fp64 against fp64: two orders of summation
NAN = float("nan")
P_DROP = 0.3

# id, N, U (None: no idx), idx, lens per owner (None: L everywhere), packed, rows_out
FORMS = [
    ("plain", 3, None, None, None, False, False),
    ("len", 3, None, None, [1, 5, 3], False, False),
    ("grouped", 4, 3, [2, 0, 2, 2], None, False, False),
    ("grouped_len", 4, 3, [2, 0, 2, 2], [4, 2, 3], False, False),
    ("packed", 3, None, None, [1, 5, 3], True, False),
    ("grouped_packed", 4, 3, [2, 0, 2, 2], [4, 2, 3], True, False),
    ("packed_rows", 3, None, None, [2, 5, 1], True, True),
]
L, O_ = 5, 8


def _close(a, b, tol=TOL):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _pos(shape, seed):
    return RR.rnd(shape, seed).abs() + 0.1


def _operands(N, U, idx, lens_own, seed=7):
    """padded operands: P (owners L, 5 O) > 0, pb > 0, q of one sign per pooling window, keep with one kept element per window"""
    own = U if U is not None else N
    W5 = 5 * O_
    P, pb = _pos((own * L, W5), seed), _pos((W5,), seed + 1)
    sign = torch.where(RR.ints((N, O_), seed + 2, 0, 1) == 0, -1.0, 1.0).repeat_interleave(5, 1)
    q = _pos((N, W5), seed + 3) * sign
    g = torch.Generator().manual_seed(seed + 4)
    keep = torch.rand(N * L, W5, generator=g) >= P_DROP
    keep[:, ::5] = True
    owner = torch.arange(N) if idx is None else torch.tensor(idx)
    lens_u = torch.full((own,), L) if lens_own is None else torch.tensor(lens_own)
    return P, pb, q, keep, owner, lens_u, lens_u[owner]


def _pack(Ppad, lens_u):
    """the real rows of every owner, one owner after the other, and their offsets"""
    rows = [Ppad.view(-1, L, Ppad.shape[1])[u, :int(c)] for u, c in enumerate(lens_u)]
    roff = torch.zeros(len(lens_u) + 1, dtype=torch.int64)
    roff[1:] = torch.cumsum(lens_u, 0)
    return torch.cat(rows, 0), roff


def _ref_args(form, Ppad, lens_u, lens_q, idx, packed):
    """-> (P as the form takes it with NaN wherever it must not be read, keyword arguments of the reference)"""
    Pn = Ppad.clone().view(-1, L, Ppad.shape[1])
    for u, c in enumerate(lens_u):
        Pn[u, int(c):] = NAN
    Pn = Pn.view(Ppad.shape)
    kw = dict(idx=idx)
    if packed:
        Pn, kw["roff"] = _pack(Ppad, lens_u)
    elif "len" in form:
        kw["lens"] = lens_q
    return Pn, kw


@pytest.mark.parametrize("form,N,U,idx,lens_own,packed,rows", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("drop", [False, True])
def test_forward_is_fuse_ref(form, N, U, idx, lens_own, packed, rows, drop):
    P, pb, q, keep, owner, lens_u, lens_q = _operands(N, U, idx, lens_own)
    keep = keep if drop else None
    p_eff = 1.0 - 1.0 / FR.scale_of(keep, P_DROP)        # fuse_ref divides by 1 - p in fp64; the kernels' scale is the fp32 quotient
    Rr, _, norm, valid = MR.fuse_ref(P, pb, q, lens_q, N, L, O_, keep=keep, p=p_eff, idx=None if idx is None else owner, U=U)
    Pn, kw = _ref_args(form, P, lens_u, lens_q, idx, packed)
    f = FR.fuse_fwd(Pn, pb, q, N, L, O_, keep=keep, p=P_DROP, rows_out=rows, **kw)
    assert torch.equal(f["valid"], valid)
    R = f["R"]
    if rows:                                             # the packed rows are the real rows of the padded result, in order
        assert R.shape == (int(lens_u.sum()), O_)
        assert _close(R, Rr.view(N, L, O_)[valid]) and _close(f["rowabs"], Rr.view(N, L, O_)[valid].pow(2).sum(1))
    else:
        assert _close(R.view(N * L, O_), Rr)
        assert bool((R[~valid] == 0).all()) and bool((f["rowabs"][~valid] == 0).all())
        assert _close(f["rowabs"].sum(1).sqrt(), norm)   # sum_o |s| is the row's sum of squares
    assert not bool(torch.isnan(f["zdrop"]).any()) and bool((f["A"] >= f["s"].abs() - 1e-15).all())


# every form as the image fusion has it, and the plain form with what only it takes (cascade / dzdrop)
BWD_CASES = [f + ("none",) for f in FORMS] + [FORMS[0] + (e,) for e in ("cascade_dzdrop", "dzdrop", "no_pbias_no_drop")]


@pytest.mark.parametrize("form,N,U,idx,lens_own,packed,rows,extras", BWD_CASES, ids=["%s-%s" % (c[0], c[-1]) for c in BWD_CASES])
def test_backward_is_autograd(form, N, U, idx, lens_own, packed, rows, extras):
    W5 = 5 * O_
    P, pb, q, keep, owner, lens_u, lens_q = _operands(N, U, idx, lens_own, seed=21)
    if extras == "no_pbias_no_drop":
        pb, keep = None, None
    casc = _pos((N * L, W5), 31) if extras == "cascade_dzdrop" else None
    dzd = RR.rnd((N * L, W5), 32) if "dzdrop" in extras else None
    G = RR.rnd((N * L, O_), 33)
    valid = MR.valid_mask(lens_q, L)
    scale = FR.scale_of(keep, P_DROP)

    # the chain under autograd, on the padded tensors (finite everywhere; the padded rows are masked out as in mfb_regions_ref)
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (P, pb, q, casc)]
    Pl, pbl, ql, cl = leaves
    Pg = (Pl if pbl is None else Pl + pbl).view(-1, L, W5)[owner]
    z = Pg * ql[:, None, :]
    if cl is not None:
        z = z * cl.view(N, L, W5)
    if keep is not None:
        z = z * (keep.view(N, L, W5).double() * scale)
    z = z * valid[:, :, None].double()
    S = z.view(N, L, O_, 5).sum(3)
    R = FR.ssqrt(torch.where(valid[:, :, None], S, torch.ones_like(S))) * valid[:, :, None].double()
    Y = F.normalize(R.reshape(N, -1)).reshape(N * L, O_)
    loss = (Y * G).sum()
    if dzd is not None:
        loss = loss + (z.view(N * L, W5) * dzd).sum()
    loss.backward()

    # the reference on the kernel's own operands
    Yd = Y.detach()
    norm = R.detach().reshape(N, -1).norm(dim=1)
    inv = 1.0 / norm.clamp_min(RR.EPS)
    rdot, _ = RR.rowdot(Yd, G)
    cA, cB, _ = RR.l2_norm_bwd_coef(rdot, norm, inv, N, L)
    Pn, kw = _ref_args(form, P, lens_u, lens_q, idx, packed)
    dYn, Yn = G.clone(), Yd.clone()
    dYn.view(N, L, O_)[~valid], Yn.view(N, L, O_)[~valid] = NAN, NAN
    if rows:
        dYn, Yn = dYn.view(N, L, O_)[valid], Yn.view(N, L, O_)[valid]
    b = FR.fuse_bwd(dYn, Yn, inv, cA, cB, Pn, pb, q, N, L, O_, keep=keep, p=P_DROP, cascade=casc, dzdrop=dzd, rows_out=rows, **kw)

    dP_auto = Pl.grad
    if packed:
        dP_auto, _ = _pack(dP_auto, lens_u)
    assert b["dP"].shape == dP_auto.shape and _close(b["dP"], dP_auto)
    assert _close(b["dq"], ql.grad)
    if pbl is not None:
        assert _close(b["dbiasP"], pbl.grad)
    else:
        assert _close(b["dbiasP"], Pl.grad.sum(0))
    if cl is not None:
        assert _close(b["dcascade"].view(N * L, W5), cl.grad)
    else:
        assert b["dcascade"] is None
    for k in ("dP", "dq", "dbiasP", "dz") + (("dcascade",) if cl is not None else ()):
        assert not bool(torch.isnan(b[k]).any()), k
        assert bool((b[k + "_abs"] >= b[k].abs() - 1e-12).all()), k
    if not packed and lens_own is not None and idx is None:                # the padded dP rows are exact zeros
        assert bool((b["dP"].view(N, L, W5)[~valid] == 0).all())
    if U is not None and not packed:                                       # image 1 has no question
        assert bool((b["dP"].view(U, L, W5)[1] == 0).all())


def test_backward_at_zero_and_dropped():
    """Y == 0 (0.0 and -0.0) gives dS = 0 whatever dY holds: only dzdrop reaches dz there; a dropped element gives exact zero"""
    N, Lr, O1 = 1, 2, 4
    W5 = 5 * O1
    Y = RR.rnd((N * Lr, O1), 41)
    Y[0, 0], Y[1, 2] = 0.0, -0.0
    dY, P, q = RR.rnd((N * Lr, O1), 42) + 2.0, RR.rnd((N * Lr, W5), 43), RR.rnd((N, W5), 44)
    dzd = RR.rnd((N * Lr, W5), 45)
    keep = torch.ones(N * Lr, W5, dtype=torch.bool)
    keep[0, 7], keep[0, 1] = False, False
    one = torch.ones(N, dtype=torch.float64)
    for extra in (None, dzd):
        b = FR.fuse_bwd(dY, Y, one * 0.5, one * 0.5, one * 0.25, P, None, q, N, Lr, O1, keep=keep, p=0.5, dzdrop=extra)
        dz = b["dz"].view(N * Lr, W5)
        assert float(dz[0, 7]) == 0.0 and float(dz[0, 1]) == 0.0 and float(b["dP"][0, 7]) == 0.0
        want = torch.zeros(5, dtype=torch.float64) if extra is None else extra[1, 10:15] * 2.0
        assert torch.equal(dz[1, 10:15], want)                             # the window of Y[1, 2] = -0.0
        assert bool((b["dz_abs"].view(N * Lr, W5)[1, 10:15] == want.abs()).all())
    # one element by hand: dS = (cA dY - cB Y) 0.5 inv / |Y|, dz = dS * 2, dP = dz q
    b = FR.fuse_bwd(dY, Y, one * 0.5, one * 0.5, one * 0.25, P, None, q, N, Lr, O1, keep=keep, p=0.5)
    dS = (0.5 * dY[0, 3] - 0.25 * Y[0, 3]) * 0.25 / abs(Y[0, 3])
    assert abs(float(b["dP"][0, 15]) - float(dS * 2.0 * q[0, 15])) <= 1e-14 * abs(float(dS * 2.0 * q[0, 15]))


def test_g_and_scale():
    assert FR.g(0) == 0.0 and abs(FR.g(8) / (8 * FR.U) - 1) < 1e-6
    assert FR.scale_of(None, 0.3) == 1.0 and FR.scale_of(torch.ones(1), 0.5) == 2.0
    assert FR.scale_of(torch.ones(1), 0.3) == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.3)))
    k = FR.philox_keep(2, 3, 4, 5, 0.3)
    assert k.shape == (6, 20) and k.dtype == torch.bool and 0.5 < float(k.float().mean()) < 0.9
