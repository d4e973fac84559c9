"""AttHeadFn(bf16=True) on the un-grouped region layouts (the node behind MFB / MHBCoAtt regions_bf16_coatt): region counts (`len`),
packed rows (`packed`) and packed rows behind the fusion too (`packed_rows`), with a NormLink (the producer's bf16 copy of x as the
operand, or a cast where it left none) and without.

Cin = 40 and 1000 (K padded to 64 and 1024), hidden 64, C = 8, N = 3, L = 5 and 37; the weight gradient's K is N L = 15 / 111 or the
packed row count, padded to a multiple of 32 with exact zero rows in BOTH bf16 operands.

  bit anchor    every count equal to L: pooled and every gradient carry the bits of the same call with layout=None on the same
                tensors (packed-rows: the same rows).
  mixed counts  counts 1, L and one between.  pooled and every gradient against an fp64 evaluation of the node on the same
                bf16-rounded operands (tests/node_harness.py's emulation: the operands of the first layer's products rounded, the
                gradient that enters them rounded behind the 1/norm factor, the kernel's ReLU decisions taken as given) within
                node_harness.BENIGN_TOL_BF16 = 2e-3; the attention weights exact zeros behind each count; both operands of dW1
                bf16 with ops.pad_rows(rows) rows and zero tails; the d1 / dx rows of padded positions exact zeros; other finite
                values in the padded rows of feat change no bit; a second call gives the same bits.
  shared images the node still refuses bf16.
"""
import importlib

import pytest
import torch

import node_harness as NH

pytestmark = pytest.mark.gpu

N, HID, C = 3, 64, 8
TOL = NH.BENIGN_TOL_BF16
FORMS = ("len", "packed", "packed_rows")
LINKS = ("link_xb", "link_cast", "nolink")


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def fn(vqa):
    return importlib.import_module(vqa.__name__ + ".host.functions")


@pytest.fixture(scope="module")
def grouping(vqa):
    return importlib.import_module(vqa.__name__ + ".host.grouping")


def _rnd(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).float()


def _counts(L, full):
    return [L] * N if full else [1, L, (L + 1) // 2]


def _data(Cin, L, full):
    """CPU fp32 operands in the padded coordinates: x (N L, Cin) with zero rows behind each count (what the fusion hands on), feat
    (N, L, C) zero-padded, the head's parameters, the cotangent"""
    counts = torch.tensor(_counts(L, full))
    valid = torch.arange(L)[None, :] < counts[:, None]
    s = 100 * Cin + L
    x = _rnd((N, L, Cin), s + 1) * valid[:, :, None]
    feat = _rnd((N, L, C), s + 2) * valid[:, :, None]
    w1, b1 = _rnd((HID, Cin), s + 3, Cin ** -0.5), _rnd((HID,), s + 4, 0.1)
    w2, b2 = _rnd((2, HID), s + 5, HID ** -0.5), _rnd((2,), s + 6, 0.1)
    dout = _rnd((N, 2 * C), s + 7)
    inv = 1.0 / x.reshape(N, -1).double().norm(dim=1).float()
    return dict(counts=counts, valid=valid, x=x.reshape(N * L, Cin), feat=feat, w1=w1, b1=b1, w2=w2, b2=b2, dout=dout, inv=inv, L=L,
                Cin=Cin)


def _layout(grouping, form, d):
    L, counts = d["L"], d["counts"]
    if form == "len":
        return grouping.RegionLayout(N, N, L, None, counts.cuda())
    off = torch.zeros(N + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(counts, 0)
    lay = grouping.RegionLayout(N, N, L, None, None, off.cuda(), int(counts.sum()))
    return lay.packed_rows() if form == "packed_rows" else lay


def _run(vqa, fn, d, form, link_kind, layout, feat_pad=None, spy=None):
    """one forward + backward of the node -> dict of CPU tensors (pooled, the gradients, the saved hid1 / wts / x operand)"""
    ops = vqa.ops
    v = d["valid"].reshape(-1)
    rows_packed = form == "packed_rows"
    x = (d["x"][v] if rows_packed else d["x"]).cuda().requires_grad_(True)
    featp = d["feat"] if feat_pad is None else feat_pad
    feat = (featp.reshape(-1, C)[v] if form in ("packed", "packed_rows") else featp).cuda().contiguous()
    par = [d[k].cuda().requires_grad_(True) for k in ("w1", "b1", "w2", "b2")]
    w1 = par[0].view(HID, d["Cin"], 1, 1)                                         # the conv's weight shape
    link = None
    if link_kind != "nolink":
        link = fn.NormLink(want_xb=True)
        owner = torch.arange(N)[:, None].expand(N, d["L"]).reshape(-1)[v]
        scale, per = (d["inv"][owner].cuda(), 1) if rows_packed else (d["inv"].cuda(), d["L"])
        xb = None
        if link_kind == "link_xb":                                                # what the fusion's _rb kernels leave: rows and K padded
            xb = [ops.cast_bf16(x.detach(), 32, ops.K_PAD_ROWS if layout is not None else None)]
        fn._arm_link(link, scale, per, xb)
    pooled = fn.AttHeadFn.apply(x, feat, w1, par[1], None, None, par[2].view(2, HID, 1, 1), par[3], False, True, link, False, layout)
    saved = pooled.grad_fn.saved_tensors
    if link_kind == "link_xb":
        assert saved[0].data_ptr() == xb[0].data_ptr(), "the producer's bf16 copy must be the operand"
    res = dict(pooled=pooled.detach().cpu(), hid1=saved[5].detach().cpu(), wts=saved[7].detach().cpu(), xop=saved[0].detach().cpu())
    seen = {}
    if spy is not None:
        gemm = ops.gemm_bf16

        def spy_gemm(a, b, ta=False, tb=False, **kw):
            if ta:
                seen["d1"], seen["xop"] = a.detach().clone().cpu(), b.detach().clone().cpu()
            elif tb:
                seen["dx_M"] = kw.get("M")
            return gemm(a, b, ta=ta, tb=tb, **kw)

        spy.setattr(ops, "gemm_bf16", spy_gemm)
    pooled.backward(d["dout"].cuda())
    torch.cuda.synchronize()
    if spy is not None:
        spy.undo()
    res.update(dx=x.grad.cpu(), dw1=par[0].grad.cpu(), db1=par[1].grad.cpu(), dw2=par[2].grad.cpu(), db2=par[3].grad.cpu())
    if link is not None:
        dl, lin = link.lin
        res.update(link_dlogits=dl.detach().cpu(), link_lin=lin.detach().cpu())
    res.update(seen)
    return res


GRADS = ("pooled", "dx", "dw1", "db1", "dw2", "db2")


def _same_bits(a, b, what, keys=GRADS):
    for k in keys:
        assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), "%s: %s differs" % (what, k)


# ---- the bit anchor --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link_kind", LINKS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Cin,L", [(40, 5), (1000, 37), (40, 37)])
def test_full_counts_carry_the_bits_of_the_plain_node(vqa, fn, grouping, Cin, L, form, link_kind):
    d = _data(Cin, L, full=True)
    plain = _run(vqa, fn, d, "plain", link_kind, None)
    got = _run(vqa, fn, d, form, link_kind, _layout(grouping, form, d))
    _same_bits(got, plain, "%s layout against layout=None" % form)
    assert float(plain["dw1"].abs().max()) > 0 and float(plain["dx"].abs().max()) > 0
    if link_kind != "nolink":
        _same_bits(got, plain, "what the link hands back", keys=("link_dlogits", "link_lin"))


# ---- mixed counts ----------------------------------------------------------------------------------------------------------------------
def _ref64(d, got, form, linked):
    """the node in fp64 on the padded coordinates, on the bf16-rounded operands, masked softmax over each sample's real regions
    -> {pooled, dx (the node's rows), dw1, db1, dw2, db2}"""
    L, Cin = d["L"], d["Cin"]
    valid, v = d["valid"], d["valid"].reshape(-1)
    leaves = {k: d[k].double().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2")}
    hid1 = got["hid1"]
    mask = torch.zeros(N * L, HID, dtype=torch.bool)
    if form == "packed_rows":
        mask[v] = hid1 > 0
    else:
        mask = hid1 > 0
    sc = d["inv"].double().repeat_interleave(L)[:, None] if linked else 1.0
    hid = NH._GradRound.apply(NH._RoundSTE.apply(leaves["x"]) @ NH._RoundSTE.apply(leaves["w1"]).t()) * sc + leaves["b1"]
    hid = hid * mask.double()
    logits = (hid @ leaves["w2"].t() + leaves["b2"]).view(N, L, 2)
    wts = torch.softmax(logits.masked_fill(~valid[:, :, None], float("-inf")), dim=1)
    pooled = torch.einsum("nsg,nsc->ngc", wts, d["feat"].double()).reshape(N, -1)
    g = torch.autograd.grad(pooled, [leaves[k] for k in ("x", "w1", "b1", "w2", "b2")], d["dout"].double())
    dx = g[0][v] if form == "packed_rows" else g[0]
    return dict(pooled=pooled.detach(), dx=dx, dw1=g[1], db1=g[2], dw2=g[3], db2=g[4]), wts.detach()


@pytest.mark.parametrize("link_kind", LINKS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Cin,L", [(40, 5), (1000, 37), (1000, 5), (40, 37)])
def test_mixed_counts(vqa, fn, grouping, Cin, L, form, link_kind, monkeypatch):
    ops = vqa.ops
    d = _data(Cin, L, full=False)
    counts, valid, v = d["counts"], d["valid"], d["valid"].reshape(-1)
    assert counts.tolist() == [1, L, (L + 1) // 2]
    layout = _layout(grouping, form, d)
    got = _run(vqa, fn, d, form, link_kind, layout, spy=monkeypatch)
    rows = int(counts.sum()) if form == "packed_rows" else N * L
    assert rows % 32 != 0
    ref, wts64 = _ref64(d, got, form, link_kind != "nolink")
    for k in GRADS:
        if k == "db2":                     # mathematically zero (a constant added in front of a softmax): against the scale of dw2
            err = float((got[k].double() - ref[k]).norm()) / float(ref["dw2"].norm())
        else:
            err = NH._nrel(got[k].reshape(ref[k].shape), ref[k])
        print("AttHeadFn[bf16] %s %s Cin=%d L=%d: %s err %.3e (bound %.0e)" % (form, link_kind, Cin, L, k, err, TOL))
        assert err <= TOL, (k, err)
        assert k == "db2" or float(ref[k].abs().max()) > 0
    # the attention weights: (N, 2, L), exact zeros behind each count, the fp64 weights in front
    wts = got["wts"]
    behind = ~valid[:, None, :].expand(N, 2, L)
    assert wts.shape == (N, 2, L) and float(wts[behind].abs().max()) == 0.0 and float(wts[~behind].min()) > 0.0
    assert float((wts.double() - wts64.permute(0, 2, 1)).abs().max()) <= TOL
    # both operands of dW1: bf16, pad_rows(rows) rows, exact zeros behind the real ones; the products in front keep M = rows
    d1, xop = got["d1"], got["xop"]
    Rp = ops.pad_rows(rows)
    assert d1.dtype == xop.dtype == torch.bfloat16 and d1.shape == (Rp, HID) and xop.shape == (Rp, (Cin + 31) // 32 * 32) and Rp > rows
    assert bool((d1[rows:].view(torch.int16) == 0).all()) and bool((xop[rows:].view(torch.int16) == 0).all())
    assert bool((xop[:, Cin:].view(torch.int16) == 0).all())
    assert got["dx_M"] == rows and got["dx"].shape == (rows, Cin) and got["hid1"].shape == (rows, HID)
    if form != "packed_rows":                                                     # the padded positions: zero d1 and dx rows
        assert float(d1[:rows][~v].float().abs().max()) == 0.0 and float(got["dx"][~v].abs().max()) == 0.0
        assert float(got["dx"][v].abs().max()) > 0.0
    # the weight gradient against fp64 on the very operands the GEMM took
    want = d1.double().t() @ xop.double()[:, :Cin]
    assert NH._nrel(got["dw1"].reshape(want.shape), want) <= 2e-5
    # a second call: the same bits
    _same_bits(_run(vqa, fn, d, form, link_kind, layout), got, "a second call")
    if form == "len":                                                             # other finite values in feat's padded rows: no bit changes
        junk = torch.where(valid[:, :, None], d["feat"], _rnd((N, L, C), 77, 3.0))
        assert not torch.equal(junk, d["feat"])
        _same_bits(_run(vqa, fn, d, form, link_kind, layout, feat_pad=junk), got, "junk in the padded rows of feat")


def test_shared_images_stay_refused(vqa, fn, grouping):
    d = _data(40, 5, full=True)
    layout = grouping.RegionLayout(N, N, 5, torch.arange(N, device="cuda"))
    assert layout.grouped
    args = [d["x"].cuda(), d["feat"].cuda(), d["w1"].cuda().view(HID, 40, 1, 1), d["b1"].cuda(), None, None,
            d["w2"].cuda().view(2, HID, 1, 1), d["b2"].cuda(), False]
    with pytest.raises(vqa.VqfError, match="fp32 only where images are shared"):
        fn.AttHeadFn.apply(*args, True, None, False, layout)
    fn.AttHeadFn.apply(*args, False, None, False, layout)                         # fp32: taken as before
