"""The small kernels only functions.HieCoreFn uses -- vqf_relu_bwd_rank1_f32, vqf_tanh_dropout_fwd2d / _bwd2d, vqf_embed_dropout_fwd /
_bwd, vqf_multi_add_f32 / vqf_multi_copy_f32, vqf_att_logits_fwd_lin -- each on its own against the fp64 reference and the
element-wise bound of tests/hie_stream_ref.py."""
import pytest
import torch

import hie_stream_ref as R
from hie_stream_util import Report, _r, _views, _only, _vqa, SENT

pytestmark = pytest.mark.gpu
P = 0.5


def _keep(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) >= P).to(torch.uint8)


@pytest.mark.parametrize("M,C,L", [(50, 64, 7), (3 * 196, 512, 196), (1000, 8, 13), (5, 1024, 5)])
def test_relu_bwd_rank1(M, C, L):
    """M not a multiple of L (the last sample is short), wts=None, in place, with and without the bias sums; y == 0 gets exactly 0"""
    ops = _vqa().ops
    rep = Report(("relu_bwd_rank1", M, C, L), False)
    NS = (M + L - 1) // L
    dx, wts, dpooled = _r((M, C), 1), _r((M,), 2), _r((NS, C), 3)
    y = torch.relu(_r((M, C), 4)) * _keep((M, C), 5).float() * 2
    y[0, :4] = 0.0
    y[M - 1, C - 1] = 0.0
    g = lambda t: t.cuda()
    for w_ in (wts, None):
        res = R.relu_bwd_rank1(dx.double(), y.double(), None if w_ is None else w_.double(), dpooled.double(), L, 2.0)
        dpre, db = ops.relu_bwd_rank1(g(dx), g(y), None if w_ is None else g(w_), g(dpooled), L, 2.0, want_bias=True)
        rep.check("relu_bwd_rank1.dpre", dpre, res["dpre"])
        rep.check("relu_bwd_rank1.dbias", db, res["dbias"])
        assert bool((dpre[g(y) == 0] == 0).all())
        buf = g(dx).clone()
        dpre2, db2 = ops.relu_bwd_rank1(buf, g(y), None if w_ is None else g(w_), g(dpooled), L, 2.0, want_bias=False, out=buf)
        assert db2 is None and torch.equal(dpre2, dpre), "in place / without the bias sums: other bits"
    rep.flush()


@pytest.mark.parametrize("Rr,W", [(98, 64), (7, 512), (301, 4), (42, 1024)])
def test_tanh_dropout_2d(Rr, W):
    """strided rows; explicit keep vs fp64; Philox bits equal the flat kernels' on the contiguous copy; out is b / out is dy"""
    ops = _vqa().ops
    rep = Report(("tanh_dropout_2d", Rr, W), True)
    a, b, dy = _r((Rr, W), 1, 1.5), _r((Rr, W), 2, 1.5), _r((Rr, W), 3)
    keep = _keep((Rr, W), 4)
    _, (aw, bw) = _views(Rr, W, True)
    aw.copy_(a.cuda())
    bw.copy_(b.cuda())
    for tag, drop, kd, p in (("nodrop", (None, 0, 0.0), None, 0.0), ("keep", (keep.cuda(), 0, P), keep.double(), P)):
        fulls, (_, out) = _views(Rr, W, True)
        ops.tanh_dropout_fwd2d(aw, bw, *drop, out=out)
        assert _only(fulls, out)
        rep.check("tanh2d.fwd_" + tag, out, R.tanh_dropout_fwd2d(a.double(), b.double(), kd, p))
        one = ops.tanh_dropout_fwd2d(aw, None, *drop)
        rep.check("tanh2d.fwd1_" + tag, one, R.tanh_dropout_fwd2d(a.double(), None, kd, p))
        dfull, (dyw, dx) = _views(Rr, W, True)
        dyw.copy_(dy.cuda())
        ops.tanh_dropout_bwd2d(dyw, out, *drop, out=dx)
        assert _only(dfull, dyw, dx)
        rep.check("tanh2d.bwd_" + tag, dx, R.tanh_dropout_bwd2d(dy.double(), out.cpu().double(), kd, p))
        ops.tanh_dropout_bwd2d(dyw, out, *drop, out=dyw)       # out is dy
        assert torch.equal(dyw, dx)
        ref_out = out.clone()
        ops.tanh_dropout_fwd2d(aw, bw, *drop, out=bw)          # out is b
        assert torch.equal(bw, ref_out)
        bw.copy_(b.cuda())
    flat = ops.tanh_dropout_fwd(a.cuda(), b.cuda(), seed=99, p_drop=P)
    fulls, (_, out) = _views(Rr, W, True)
    ops.tanh_dropout_fwd2d(aw, bw, None, 99, P, out=out)
    assert torch.equal(out, flat), "fwd2d with strided rows: not the flat kernel's bits"
    dflat = ops.tanh_dropout_bwd(dy.cuda(), flat, seed=99, p_drop=P)
    _, (dyw, dx) = _views(Rr, W, True)
    dyw.copy_(dy.cuda())
    ops.tanh_dropout_bwd2d(dyw, out, None, 99, P, out=dx)
    assert torch.equal(dx, dflat), "bwd2d with strided rows: not the flat kernel's bits"
    rep.flush()


@pytest.mark.parametrize("Tn,V,E", [(42, 30, 64), (300 * 14, 1000, 512), (5, 3, 4), (77, 20, 1024)])
def test_embed_dropout(Tn, V, E):
    """ids repeated; an id that never occurs gets an exact zero row; an id outside [0, V) selects nothing; the mask is
    ops.dropout's on the flat tensor; p = 0 and the explicit mask are bit-equal to the lookup (times 2)"""
    ops = _vqa().ops
    rep = Report(("embed_dropout", Tn, V, E), False)
    W, dout = _r((V, E), 1), _r((Tn, E), 2)
    ids = torch.randint(0, V - 1, (Tn,), generator=torch.Generator().manual_seed(3))       # id V - 1 never occurs
    ids[Tn // 2] = V + 5
    ids[0] = -1
    keep = _keep((Tn, E), 4)
    Wg, idg = W.cuda(), ids.cuda()
    for drop, kd, p in (((None, 0, 0.0), None, 0.0), ((keep.cuda(), 0, P), keep.double(), P)):
        out = ops.embed_dropout_fwd(Wg, idg, *drop)
        ref, bound = R.embed_dropout_fwd(W.double(), ids, kd, p)
        assert float(bound.max()) == 0.0 and torch.equal(out.cpu().double(), ref), "lookup (x 2 where kept) must be bit-exact"
        dW = ops.embed_dropout_bwd(dout.cuda(), idg, V, *drop)
        rep.check("embed.bwd", dW, R.embed_dropout_bwd(dout.double(), ids, V, kd, p))
        assert float(dW[V - 1].abs().max()) == 0.0
    ones = torch.ones((V, E), device="cuda")
    idv = torch.arange(Tn, device="cuda") % V
    z = ops.embed_dropout_fwd(ones, idv, None, 7, P)
    flat = ops.dropout(torch.ones((Tn, E), device="cuda"), seed=7, p_drop=P)
    assert torch.equal(z, flat), "embed_dropout_fwd: not ops.dropout's mask over the flat (T, E) tensor"
    pattern = (flat != 0).to(torch.uint8)
    assert torch.equal(ops.embed_dropout_bwd(dout.cuda(), idg, V, None, 7, P), ops.embed_dropout_bwd(dout.cuda(), idg, V, pattern, 0, P))
    rep.flush()


def test_multi_add_and_multi_copy():
    vqa = _vqa()
    ops = vqa.ops
    rep = Report("multi_add", False)
    sizes = [1, 5, 1023, 4096, 7, 262147, 3, 64, 10]
    src = [_r((n,), 10 + i).cuda() for i, n in enumerate(sizes)]
    oth = [_r((n,), 30 + i).cuda() for i, n in enumerate(sizes)]

    def dst(n):
        full = torch.full((n + 8,), SENT, device="cuda")
        return full, full[4:4 + n]

    for count in range(1, 9):
        ds = [dst(n) for n in sizes[:count]]
        ops.multi_copy([(s, d[1]) for s, d in zip(src, ds)])
        for s, (full, v) in zip(src, ds):
            assert torch.equal(v, s) and bool((full[:4] == SENT).all()) and bool((full[-4:] == SENT).all())
    for count in range(1, 5):
        ds = [dst(n) for n in sizes[2:2 + count]]
        ops.multi_add([(a, b, d[1]) for a, b, d in zip(src[2:], oth[2:], ds)])
        for a, b, (full, v) in zip(src[2:], oth[2:], ds):
            rep.check("multi_add.out", v, R.multi_add(a.cpu().double(), b.cpu().double()))
            assert bool((full[:4] == SENT).all()) and bool((full[-4:] == SENT).all())
    with pytest.raises(vqa.lib.VqfError, match="VQF_E_BADARG"):
        ops.multi_copy([(s, torch.empty_like(s)) for s in src[:9]])
    with pytest.raises(vqa.lib.VqfError, match="VQF_E_BADARG"):
        ops.multi_add([(a, b, torch.empty_like(a)) for a, b in zip(src[:5], oth[:5])])
    rep.flush()


@pytest.mark.parametrize("M,Hh,G", [(42, 64, 1), (588, 512, 2), (7, 1000, 2), (1025, 30, 1)])
def test_att_logits_fwd_lin(M, Hh, G):
    """logits bit-equal to vqf_att_logits_fwd; lin vs fp64; pre-activations exactly 0 do not count in lin"""
    ops = _vqa().ops
    rep = Report(("att_logits_fwd_lin", M, Hh, G), False)
    b1, w2, b2 = _r((Hh,), 1, 0.5), _r((G, Hh), 2), _r((G,), 3)
    hid = torch.relu(_r((M, Hh), 4) + b1)
    hid[0, :3] = 0.0
    logits, lin = ops.att_logits_fwd_lin(hid.cuda(), w2.cuda(), b2.cuda(), b1.cuda())
    assert torch.equal(logits, ops.att_logits_fwd(hid.cuda(), w2.cuda(), b2.cuda()))
    res = R.att_logits_fwd_lin(hid.double(), w2.double(), b2.double(), b1.double())
    rep.check("att_logits_lin.logits", logits, res["logits"])
    rep.check("att_logits_lin.lin", lin, res["lin"])
    rep.flush()
