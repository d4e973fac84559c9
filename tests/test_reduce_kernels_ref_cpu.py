"""tests/reduce_kernels_ref.py (the fp64 reference tests/test_gpu_reduce_kernels.py holds the kernels to) pinned on torch autograd
in fp64, so that the GPU test cannot share a mistake with its reference: the logit head's backward on autograd of
relu(pre + b1) @ w2.T + b2, the two F.normalize coefficient forms on autograd of F.normalize over a sample's L x W values, the
ReLU / dropout backward with the rank-1 pool term on autograd of a direct consumer plus an attention-weighted pool."""
import pytest
import torch
import torch.nn.functional as F

import reduce_kernels_ref as RR

TOL = 1e-12           # fp64 against fp64: two orders of summation


def _close(a, b, tol=TOL):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _away_from_kink(x, gap=0.05):
    """x with |x| >= gap (the sign kept): no value near the ReLU's kink"""
    return torch.where(x.abs() < gap, torch.where(x < 0, -gap, gap).double(), x)


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("relu_mask", [True, False])
@pytest.mark.parametrize("rps", [None, 1, 3])
def test_att_logits_bwd_is_autograd(G, relu_mask, rps):
    M, Hh = 11, 10
    b1 = RR.rnd((Hh,), 1, 0.5).requires_grad_(True)
    w2, b2 = RR.rnd((G, Hh), 2).requires_grad_(True), RR.rnd((G,), 3).requires_grad_(True)
    dl = RR.rnd((M, G), 4)
    rs = None if rps is None else RR.rnd(((M + rps - 1) // rps,), 5) + 1.5
    rows = torch.ones(M, 1, dtype=torch.float64) if rs is None else rs[torch.arange(M) // rps][:, None]
    # the layer in front: pre = x * rowscale (a row-scaled input) + b1; the gradient into x is the STORED row, b1's the unscaled sum
    if relu_mask:
        x = (_away_from_kink(RR.rnd((M, Hh), 6) + b1.detach()) - b1.detach()) / rows
        x.requires_grad_(True)
        hid = torch.relu(x * rows + b1)
    else:                                                # no ReLU: hid is the layer's output as it is
        x = RR.rnd((M, Hh), 6).requires_grad_(True)
        hid = x * rows + b1
    ((hid @ w2.t() + b2) * dl).sum().backward()
    ref = RR.att_logits_bwd(dl, hid.detach(), w2.detach(), relu_mask, rs, rps or 1)
    assert _close(ref["dhid_pre"], x.grad) and _close(ref["dw2"], w2.grad)
    assert _close(ref["db2"], b2.grad) and _close(ref["dbias1"], b1.grad)
    for k in ("dhid_pre", "dw2", "db2", "dbias1"):      # sum |terms| bounds |sum|, and is the sum of the absolute products
        assert bool((ref[k + "_abs"] >= ref[k].abs() - 1e-15).all()), k
    assert _close(ref["dw2_abs"], dl.abs().t() @ hid.detach().abs())


def test_att_logits_bwd_relu_of_zero_is_zero():
    """hid == 0 exactly (and -0.0): no gradient through the ReLU, whatever dl and w2 hold; without the mask the element counts"""
    dl, w2 = torch.tensor([[2.0], [3.0]]).double(), torch.tensor([[1.0, -1.0, 4.0]]).double()
    hid = torch.tensor([[0.0, 1.0, -0.0], [5.0, 0.0, 2.0]]).double()
    on, off = RR.att_logits_bwd(dl, hid, w2, True), RR.att_logits_bwd(dl, hid, w2, False)
    assert on["dhid_pre"].tolist() == [[0.0, -2.0, 0.0], [3.0, 0.0, 12.0]]
    assert off["dhid_pre"].tolist() == [[2.0, -2.0, 8.0], [3.0, -3.0, 12.0]]
    assert on["dbias1"].tolist() == [3.0, -2.0, 12.0] and on["dbias1_abs"].tolist() == [3.0, 2.0, 12.0]
    assert on["dw2"].tolist() == [[15.0, 2.0, 6.0]] and on["db2"].tolist() == [5.0]
    rs = RR.att_logits_bwd(dl, hid, w2, True, torch.tensor([4.0, 0.5]).double(), 1)
    assert rs["dhid_pre"].tolist() == [[0.0, -8.0, 0.0], [1.5, 0.0, 6.0]] and rs["dbias1"].tolist() == [3.0, -2.0, 12.0]


def test_att_logits_fwd_and_lin():
    M, Hh, G = 5, 9, 2
    hid, b1 = torch.relu(RR.rnd((M, Hh), 7)), RR.rnd((Hh,), 8, 0.5)
    hid[0, :2] = 0.0
    w2, b2 = RR.rnd((G, Hh), 9), RR.rnd((G,), 10)
    logits, la = RR.att_logits_fwd(hid, w2, b2)
    assert _close(logits, F.linear(hid, w2, b2)) and bool((la >= logits.abs()).all())
    lin, _ = RR.att_logits_fwd_lin(hid, w2, b2, b1)
    # lin = the logit minus what does not depend on pre = hid - b1: b2 and the b1 of the live columns
    live = (hid > 0).double()
    assert _close(lin, logits - b2 - (live * b1) @ w2.t())


@pytest.mark.parametrize("L,W", [(1, 6), (4, 3)])
def test_l2_norm_bwd_coef_is_autograd_of_normalize(L, W):
    """dR = coefA dY - coefB Y over a sample's L x W values; sample 1 is all zero: the clamped branch, dR = dY / eps"""
    N = 3
    R = RR.rnd((N, L, W), 11)
    R[1] = 0.0
    R.requires_grad_(True)
    dY = RR.rnd((N, L, W), 12)
    Y = F.normalize(R.view(N, L * W), dim=1).view(N, L, W)
    (Y * dY).sum().backward()
    Yd = Y.detach()
    norm, inv, _ = RR.l2_group_norm((R.detach() ** 2).sum(2).view(-1), N, L)
    assert float(norm[1]) == 0.0 and float(inv[1]) == 1.0 / RR.EPS
    assert _close(RR.scale_rows(R.detach().view(N * L, W), inv, L), Yd.view(N * L, W))
    rdot, _ = RR.rowdot(Yd.view(N * L, W), dY.view(N * L, W))
    cA, cB, _ = RR.l2_norm_bwd_coef(rdot, norm, inv, N, L)
    assert float(cB[1]) == 0.0 and float(cA[1]) == float(inv[1])
    dR = cA[:, None, None] * dY - cB[:, None, None] * Yd
    keep = torch.tensor([0, 2])
    assert _close(dR[keep], R.grad[keep])
    assert _close(dR[1] * RR.EPS, R.grad[1] * 1e-12, 1e-7)         # eps: fp32(1e-12) here, 1e-12 in F.normalize


@pytest.mark.parametrize("G", [1, 2])
def test_l2_norm_bwd_coef_lin_through_a_linear_relu_logits_chain(G):
    """the un-normalised form: the consumer takes R, scales by 1 / norm in its product and hands back dYs = dY / norm;
    sum_g dlogits lin == sum(R dYs) per row, and dR = dYs - coefB R is autograd's gradient through F.normalize"""
    N, L, W, Hh = 3, 4, 5, 7
    R = RR.rnd((N, L, W), 13).requires_grad_(True)
    W1, b1 = RR.rnd((Hh, W), 14), RR.rnd((Hh,), 15, 0.3)
    w2, b2, dl = RR.rnd((G, Hh), 16), RR.rnd((G,), 17), RR.rnd((N * L, G), 18)
    Y = F.normalize(R.view(N, L * W), dim=1).view(N * L, W)
    Y.retain_grad()
    hid = torch.relu(Y @ W1.t() + b1)
    ((hid @ w2.t() + b2) * dl).sum().backward()
    Rd = R.detach().view(N * L, W)
    norm, inv, _ = RR.l2_group_norm((Rd ** 2).sum(1), N, L)
    dYs = RR.scale_rows(Y.grad, inv, L)                                       # dY / norm
    lin, _ = RR.att_logits_fwd_lin(hid.detach(), w2, b2, b1)
    assert _close((dl * lin).sum(1), (Rd * dYs).sum(1))
    cA, cB, unit, _ = RR.l2_norm_bwd_coef_lin(dl, lin, G, norm, inv, N, L)
    assert bool((cA == 1).all()) and bool((unit == 1).all())
    dR = dYs.view(N, L, W) - cB[:, None, None] * R.detach()
    assert _close(dR, R.grad)
    # the clamped branch: no projection term
    zero = torch.zeros(N, dtype=torch.float64)
    cA, cB, unit, ab = RR.l2_norm_bwd_coef_lin(dl, lin, G, zero, torch.full((N,), 1.0 / RR.EPS).double(), N, L)
    assert bool((cB == 0).all()) and bool((ab == 0).all()) and bool((cA == 1).all()) and bool((unit == 1).all())


@pytest.mark.parametrize("with_pool", [True, False])
def test_relu_bwd_rank1_is_autograd(with_pool):
    """Y = dropout_mask * relu(pre) feeds a direct consumer (gradient dX) and a pool sum_l wts[n, l] Y[n L + l] (gradient dpooled)"""
    N, L, C, p = 3, 4, 6, 0.25
    scale = 1.0 / (1.0 - p)
    pre = _away_from_kink(RR.rnd((N * L, C), 19)).requires_grad_(True)
    mask = (RR.rnd((N * L, C), 20) > -0.5).double() * scale
    dX, wts, dpooled = RR.rnd((N * L, C), 21), RR.rnd((N * L,), 22), RR.rnd((N, C), 23)
    Y = mask * torch.relu(pre)
    loss = (Y * dX).sum()
    if with_pool:
        loss = loss + ((wts[:, None] * Y).view(N, L, C).sum(1) * dpooled).sum()
    loss.backward()
    dpre, mag, db, dbabs = RR.relu_bwd_rank1(dX, Y.detach(), wts if with_pool else None, dpooled if with_pool else None, L, scale)
    assert _close(dpre, pre.grad) and _close(db, pre.grad.sum(0))
    assert bool((mag >= dpre.abs() - 1e-15).all()) and _close(dbabs, mag.sum(0))
    # the plain ReLU backward is the same thing without pool and dropout
    d0, b0, a0 = RR.relu_bwd(dX, torch.relu(pre.detach()))
    r0 = RR.relu_bwd_rank1(dX, torch.relu(pre.detach()), None, None, 1, 1.0)
    assert torch.equal(d0, r0[0]) and torch.equal(b0, r0[2]) and torch.equal(a0, r0[3])
    z = torch.tensor([[0.0, -0.0, 1.0, -1.0]]).double()
    assert RR.relu_bwd(torch.full((1, 4), 5.0).double(), z)[0].tolist() == [[0.0, 0.0, 5.0, 0.0]]


def test_sums_and_their_term_magnitudes():
    x = RR.rnd((6, 5), 24)
    s, a = RR.colsum(x)
    assert _close(s, x.sum(0)) and _close(a, x.abs().sum(0))
    s, a = RR.group_reduce(x, 3, 2)
    assert _close(s[1], x[2] + x[3]) and _close(a[2], x[4].abs() + x[5].abs())
    i = RR.ints((1000,), 25)
    assert bool((i == i.round()).all()) and float(i.abs().max()) == 3.0 and float(i.min()) == -3.0
    p = RR.pow2((1000,), 26)
    assert set(p.tolist()) == {0.25, 0.5, 1.0, 2.0, 4.0}
