"""The fp64 references of tests/hie_stream_ref.py ARE the model's operation (no GPU): chained the way functions.HieCoreFn chains the
streaming kernels -- forward hv_fwd (+ slab_sum), backward head_bwd, rank_add, rank_left, slab_sum, the wpart / colpart row sums
-- they reproduce torch.autograd on node_harness.ref_hie_core (hieCoAtten.py:32-49) at 1e-12, for one chunk per sample and for
an emulated three-chunk split; with explicit keep masks the forward reproduces oracle.ref_torch.hiecoatten_forward(drop=...)."""
import pytest
import torch

import hie_stream_ref as R
from node_harness import ref_hie_core
from oracle import ref_torch as O

TOL = 1e-12
N, L, T, D, E, VOC = 3, 20, 7, 24, 16, 30


def _r(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def _params():
    p = dict(w_emb=_r((E, D), 1, 0.3), b_emb=_r((E,), 2, 0.1), w_que=_r((VOC, E), 3), wbv=_r((E, E), 4, 0.3), bbv=_r((E,), 5, 0.1),
             wv=_r((E, E), 6, 0.3), bv=_r((E,), 7, 0.1), wq=_r((E, E), 8, 0.3), bq=_r((E,), 9, 0.1), whv=_r((1, E), 10),
             bhv=_r((1,), 11), whq=_r((1, E), 12), bhq=_r((1,), 13))
    imgf = _r((N, L, D), 14)
    ids = torch.randint(0, VOC, (N, T), generator=torch.Generator().manual_seed(15))
    return imgf, ids, p


def _close(got, ref, what, scale=None):
    err = float((got - ref).abs().max() / ((ref.abs().max() if scale is None else scale) + 1e-300))
    assert err <= TOL, (what, err)


def _graph(imgf, ids, p):
    """ref_hie_core's graph with its intermediates kept (checked against ref_hie_core itself below)"""
    im = torch.relu(imgf @ p["w_emb"].t() + p["b_emb"])
    qu = p["w_que"][ids]
    Cv, Cq = im @ p["wbv"].t() + p["bbv"], qu @ p["wbv"].t() + p["bbv"]
    aff = Cq @ Cv.transpose(1, 2)
    C = torch.tanh(aff)
    im_, qu_ = im @ p["wv"].t() + p["bv"], qu @ p["wq"].t() + p["bq"]
    Hv = torch.tanh(im_ + (qu_.transpose(1, 2) @ C).transpose(1, 2))
    lv = Hv @ p["whv"].t() + p["bhv"]
    av = torch.softmax(lv, dim=1)
    v = (av.transpose(1, 2) @ im).reshape(N, -1)
    ti = (im_.transpose(1, 2) @ C.transpose(1, 2)).transpose(1, 2)
    hq_pre = qu_ + ti
    Hq = torch.tanh(hq_pre)
    aq = torch.softmax(Hq @ p["whq"].t() + p["bhq"], dim=1)
    qv = (aq.transpose(1, 2) @ qu).reshape(N, -1)
    x = torch.cat((v, qv), 0).reshape(N, -1)
    return x, dict(Cv=Cv, Cq=Cq, aff=aff, C=C, im_=im_, qu_=qu_, Hv=Hv, lv=lv, ti=ti, hq_pre=hq_pre)


@pytest.mark.parametrize("S", [1, 3])
def test_chained_references_reproduce_autograd_of_ref_hie_core(S):
    imgf, ids, p = _params()
    p = {k: v.requires_grad_() for k, v in p.items()}
    order = ["w_emb", "b_emb", "w_que", "wbv", "bbv", "wv", "bv", "wq", "bq", "whv", "bhv", "whq", "bhq"]
    dx = _r((N, 2 * E), 16)
    x_ref, _, _ = ref_hie_core(imgf, ids, *[p[k] for k in order])
    pg = dict(zip(order, torch.autograd.grad((x_ref * dx).sum(), [p[k] for k in order])))
    x, t = _graph(imgf, ids, p)
    _close(x.detach(), x_ref.detach(), "instrumented graph vs ref_hie_core")
    names = ["im_", "qu_", "Cv", "Cq", "lv", "hq_pre", "aff"]
    g = dict(zip(names, torch.autograd.grad((x * dx).sum(), [t[k] for k in names])))
    d = {k: v.detach() for k, v in t.items()}
    Lc = None if S == 1 else (L + S - 1) // S

    # forward: Hv and ti as _hie_hv_ti does
    f = R.hv_fwd(d["im_"], d["C"], d["qu_"], Lc=Lc)
    _close(f["out"][0], d["Hv"], "Hv")
    ti = f["part"][0] if S == 1 else R.slab_sum(f["slabs"][0].reshape(S, N * T, E))[0].view(N, T, E)
    assert S == 1 or f["slabs"][0].shape[0] == S
    _close(ti, d["ti"], "ti")

    # backward, in HieCoreFn's order: the head pass (dtq, C dtq (+ dti), dl^T Hv), rank_add, rank_left
    dlv, dti, dC3 = g["lv"].reshape(N, L), g["hq_pre"], g["aff"]
    whv = p["whv"].detach().view(E)
    if S == 1:
        h = R.head_bwd(d["Hv"], dlv, whv, d["C"], part_add=dti)
        dque_ = h["part"][0]
    else:
        h = R.head_bwd(d["Hv"], dlv, whv, d["C"], Lc=Lc)
        dque_ = R.slab_sum(h["slabs"][0].reshape(S, N * T, E), add=dti.reshape(N * T, E))[0].view(N, T, E)
    dtq = h["out"][0]
    a = R.rank_add(dtq, d["C"], dti, Lc=Lc)
    dimg_ = a["out"][0]
    lf = R.rank_left(dC3, d["Cq"], d["Cv"], Lc=Lc)
    dCv = lf["out"][0]
    dCq = lf["part"][0] if S == 1 else R.slab_sum(lf["slabs"][0].reshape(S, N * T, E))[0].view(N, T, E)
    for cp in (a["colpart"][0], lf["colpart"][0], h["wpart"][0]):
        assert cp.shape == (S, N, E)
    _close(dque_, g["qu_"], "dque_")
    _close(dimg_, g["im_"], "dimg_")
    _close(dCv, g["Cv"], "dCv")
    _close(dCq, g["Cq"], "dCq")
    _close(h["wpart"][0].sum((0, 1)), pg["whv"].view(E), "d fc_Whv.weight")
    # (the bias in front of a softmax: mathematically zero, so relative to the terms of the sum)
    _close(h["dlsum"][0].sum().view(1), pg["bhv"], "d fc_Whv.bias", scale=float(dlv.abs().sum()))
    _close(a["colpart"][0].sum((0, 1)), pg["bv"], "d fc_Wv.bias")
    _close(lf["colpart"][0].sum((0, 1)) + dCq.sum((0, 1)), pg["bbv"], "d fc_Wbv.bias")
    # every bound is a bound: positive where the value is not exactly representable, and small
    for res in (f, h, a, lf):
        for k, (val, b) in res.items():
            assert b.shape == val.shape and bool((b >= 0).all()) and float(b.max()) <= 1e-3 * (1 + float(val.abs().max())), k


def test_references_with_keep_masks_reproduce_the_oracle_forward():
    imgf, ids, p = _params()
    sd = {"img_emb.weight": p["w_emb"], "img_emb.bias": p["b_emb"], "que_emb.weight": p["w_que"], "fc_Wbv.weight": p["wbv"],
          "fc_Wbv.bias": p["bbv"], "fc_Wv.weight": p["wv"], "fc_Wv.bias": p["bv"], "fc_Wq.weight": p["wq"], "fc_Wq.bias": p["bq"],
          "fc_Whv.weight": p["whv"], "fc_Whv.bias": p["bhv"], "fc_Whq.weight": p["whq"], "fc_Whq.bias": p["bhq"],
          "fc.weight": _r((5, 2 * E), 20), "fc.bias": _r((5,), 21)}
    km = lambda shape, seed: (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= 0.5).double()
    drop = {"img": km((N, L, E), 31), "que": km((N, T, E), 32), "C": km((N, T, L), 33), "Hv": km((N, L, E), 34), "Hq": km((N, T, E), 35)}
    x_ref, av_ref, aq_ref = O.hiecoatten_forward(sd, imgf, ids, drop=drop)
    im = torch.relu(imgf @ p["w_emb"].t() + p["b_emb"]) * drop["img"] * 2
    qu = R.embed_dropout_fwd(p["w_que"], ids.reshape(-1), drop["que"].view(N * T, E), 0.5)[0].view(N, T, E)
    Cv, Cq = im @ p["wbv"].t() + p["bbv"], qu @ p["wbv"].t() + p["bbv"]
    C = torch.tanh(Cq @ Cv.transpose(1, 2)) * drop["C"] * 2
    im_, qu_ = im @ p["wv"].t() + p["bv"], qu @ p["wq"].t() + p["bq"]
    for Lc in (None, 7):
        f = R.hv_fwd(im_, C, qu_, keep=drop["Hv"], p=0.5, Lc=Lc)
        Hv = f["out"][0]
        assert bool((f["out"][1][drop["Hv"] == 0] == 0).all()) and bool((Hv[drop["Hv"] == 0] == 0).all())
        ti = f["part"][0] if Lc is None else R.slab_sum(f["slabs"][0].reshape(-1, N * T, E))[0].view(N, T, E)
        av = torch.softmax(Hv @ p["whv"].t() + p["bhv"], dim=1)
        Hq = R.tanh_dropout_fwd2d(qu_.reshape(N * T, E), ti.reshape(N * T, E), drop["Hq"].view(N * T, E), 0.5)[0].view(N, T, E)
        aq = torch.softmax(Hq @ p["whq"].t() + p["bhq"], dim=1)
        v, qv = (av.transpose(1, 2) @ im).reshape(N, -1), (aq.transpose(1, 2) @ qu).reshape(N, -1)
        x = torch.cat((v, qv), 0).reshape(N, -1) @ sd["fc.weight"].t() + sd["fc.bias"]
        _close(av.reshape(N, -1), av_ref, "av")
        _close(aq.reshape(N, -1), aq_ref, "aq")
        _close(x, x_ref, "x")


def test_small_kernel_references_against_autograd():
    """relu_bwd_rank1, tanh_dropout_bwd2d, embed_dropout_bwd, att_logits_fwd_lin: the formulas against torch.autograd / a direct sum"""
    M, C, Lr = 14, 8, 4                                     # M not a multiple of Lr: the last sample is short
    pre, wts, dpooled, dx = _r((M, C), 41).requires_grad_(), _r((M,), 42), _r((4, C), 43), _r((M, C), 44)
    keep = (torch.rand((M, C), generator=torch.Generator().manual_seed(45)) >= 0.5).double()
    y = torch.relu(pre) * keep * 2
    pooled = torch.zeros(4, C).double().index_add(0, torch.arange(M) // Lr, y * wts[:, None])
    (gpre,) = torch.autograd.grad((y * dx).sum() + (pooled * dpooled).sum(), pre)
    r = R.relu_bwd_rank1(dx, y.detach(), wts, dpooled, Lr, 2.0)
    _close(r["dpre"][0], gpre, "relu_bwd_rank1")
    _close(r["dbias"][0], gpre.sum(0), "relu_bwd_rank1 dbias")
    a = _r((M, C), 46, 3.0).requires_grad_()
    yt = torch.tanh(a) * keep * 2
    (ga,) = torch.autograd.grad((yt * dx).sum(), a)
    _close(R.tanh_dropout_bwd2d(dx, yt.detach(), keep, 0.5)[0], ga, "tanh_dropout_bwd2d")
    W = _r((6, C), 47).requires_grad_()
    ids = torch.tensor([0, 3, 3, 5, 0, 3, 1, 1, 5, 0, 3, 3, 0, 1])          # id 2 and 4 never occur
    (gW,) = torch.autograd.grad((W[ids] * keep * 2 * dx).sum(), W)
    val, b = R.embed_dropout_bwd(dx, ids, 6, keep, 0.5)
    _close(val, gW, "embed_dropout_bwd")
    assert float(val[2].abs().max()) == 0.0 and float(b[2].max()) == 0.0 and float(val[4].abs().max()) == 0.0
    b1, w2, b2 = _r((C,), 48), _r((2, C), 49), _r((2,), 50)
    hid = torch.relu(pre.detach() + b1)
    res = R.att_logits_fwd_lin(hid, w2, b2, b1)
    _close(res["logits"][0], hid @ w2.t() + b2, "logits")
    _close(res["lin"][0], (pre.detach() * (hid > 0)) @ w2.t(), "lin")       # linear in the layer's input: hid - b1 == pre where hid > 0
