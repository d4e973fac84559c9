"""MFB / MHBCoAtt regions_bf16_coatt (the bf16 co-attention head on packed and counted regions) on the GPU, model level, with the
models, the steps and the launch census of tests/test_gpu_mfb_regions_bf16.py (imported, not restated; MFB runs with unit_softmax =
False, as there).  The comparison is always the same model with regions_bf16 = True and regions_bf16_coatt = False.

  small    N = 4, L = 9, counts 1, 9, 4, 7 (R = 21, N L = 36), D = 2048, O = 1000, the models' hidden widths; MFB, multilayer MFB, MHBCoAtt; a
           PackedRegions (packed_coatt both ways) and the pair; train steps with explicit keep masks, and eval.  Outputs within 3e-2
           (max-norm relative, tests/test_gpu_bf16.py::_rel: the README's bf16 criterion) and not bit-equal; the launch census shows
           co_att_conv1's three products as bf16 GEMMs of their shapes -- the weight gradient's K the row count rounded up to 32 --
           and no fp32 product of those shapes, while without the attribute they are fp32; two consecutive steps give the same bits;
           every overlap_streams / side_bf16 / fuse_bf16_dp / fold_norm setting.  At 21 and 36 rows the projection stays fp32 (the
           large-tile GEMM does not apply), so x is cast: the next case has the fusion's own copy.
  ragged   N = 12, L = 100, R = 1037: the projection is stored in bf16, the fusion kernel leaves the bf16 copy of R with
           pad_rows(rows) rows and co_att_conv1's forward takes that very tensor (no cast pass over R); 3e-2, not equal, same bits twice.
  off      regions_bf16_coatt = False is the model as constructed, bit for bit and launch for launch; a plain tensor is not touched by
           the attribute under any gemm_dtype.
"""
import importlib

import pytest
import torch

import mfb_regions_ref as RR
import test_gpu_mfb_regions_bf16 as TB
from test_gpu_bf16 import _rel

pytestmark = pytest.mark.gpu

BF16_TOL = TB.BF16_TOL                                   # 3e-2: the project's stated bf16 criterion
SMALL = dict(N=4, L=9, D=2048, counts=[1, 9, 4, 7])
FORMS = ("packed", "packed-rows", "pair")
CIN = 1000                                               # co_att_conv1: (hidden, 1000); hidden is 1024 in MFB, 512 in MHBCoAtt


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def functions(vqa):
    return importlib.import_module(vqa.__name__ + ".host.functions")


@pytest.fixture(autouse=True)
def _attribute_off_afterwards():
    """the models are shared with tests/test_gpu_mfb_regions_bf16.py, whose _build does not know the new attribute"""
    yield
    for built in TB._BUILT.values():
        built[0].regions_bf16_coatt = False
        built[0].fold_norm = True
        built[0].set_keep_masks()


def _build(vqa, kind, shape):
    built = TB._build(vqa, kind, shape)
    TB._set(built[0], regions_bf16_coatt=False, fold_norm=True)
    return built


def _feats(form, img, counts, packed):
    return packed if form.startswith("packed") else (img, counts)


def _keep(model, N, L, seed=5):
    g = torch.Generator().manual_seed(seed)
    W5 = model.img_conv1d.out_channels
    masks = dict(m1=(torch.rand(N * L, W5, generator=g) >= 0.1), m2=(torch.rand(N, W5, generator=g) >= 0.1),
                 m3=(torch.rand(N, W5, generator=g) >= 0.1))
    return {k: v.to(torch.uint8).cuda() for k, v in masks.items()}


def _products(ops, model, rows):
    """(bf16 launches, fp32 launches) of co_att_conv1's forward, dx and dW1 at `rows` rows since the last prof_reset"""
    HID = model.co_att_conv1.weight.shape[0]
    Kp, Rp = (CIN + 31) // 32 * 32, ops.pad_rows(rows)
    bf = (ops.prof_shape("gemm_bf16", rows, HID, Kp)[0], ops.prof_shape("gemm_bf16", rows, CIN, HID)[0],
          ops.prof_shape("gemm_bf16", HID, Kp, Rp)[0])
    f32 = (ops.prof_gemm(0, 0, rows, HID, CIN)[0], ops.prof_gemm(0, 1, rows, CIN, HID)[0], ops.prof_gemm(1, 1, HID, CIN, rows)[0])
    return bf, f32


def _census_step(ops, model, kind, feats, q, tgt):
    res, census = TB._census(ops, lambda: TB._step(model, kind, feats, q, tgt))
    return res, census


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", TB.KINDS)
def test_small(vqa, kind, form, monkeypatch):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, SMALL)
    N, L = img.shape[0], img.shape[1]
    rows = int(counts.sum()) if form == "packed-rows" else N * L
    assert (int(counts.sum()), N * L) == (21, 36) and model.co_att_conv1.weight.shape[1] == CIN
    feats = _feats(form, img, counts, packed)
    TB._set(model, regions_bf16=True, packed_coatt=form == "packed-rows")
    model.set_keep_masks(**_keep(model, N, L))
    base, _ = _census_step(ops, model, kind, feats, q, tgt)
    bf, f32 = _products(ops, model, rows)
    assert bf == (0, 0, 0) and min(f32) >= 1, ("without the attribute the three products are fp32", bf, f32)
    model.regions_bf16_coatt = True
    seen, gemm, hid = {}, ops.gemm_bf16, model.co_att_conv1.weight.shape[0]

    def spy_gemm(a, b, ta=False, tb=False, **kw):
        if ta and a.shape[1] == hid and b.shape[1] == (CIN + 31) // 32 * 32:      # dW1 = d1^T x
            seen["d1"], seen["x"] = a.detach().clone(), b.detach().clone()
        return gemm(a, b, ta=ta, tb=tb, **kw)

    monkeypatch.setattr(ops, "gemm_bf16", spy_gemm)
    got, _ = _census_step(ops, model, kind, feats, q, tgt)
    monkeypatch.undo()
    bf, f32 = _products(ops, model, rows)
    assert bf == (1, 1, 1) and f32 == (0, 0, 0), ("co_att_conv1's three products must be bf16 GEMMs", bf, f32)
    err = _rel(got[0], base[0])
    print("regions_bf16_coatt %s %s: output rel err against regions_bf16 alone %.3e" % (kind, form, err))
    assert err <= BF16_TOL
    assert not torch.equal(got[0], base[0])                                       # the bf16 head really ran
    assert set(got[1]) == set(base[1]) and all(bool(torch.isfinite(g).all()) for g in got[1].values())
    assert float(got[1]["co_att_conv1.weight"].abs().max()) > 0.0
    # the weight gradient: both operands bf16 with the row count rounded up to 32 and exact zeros behind the real rows; the product
    # within the fp32-accumulation bound of the fp64 product of those very operands.  (Against the fp32 head the gradient is only
    # printed: its rows nearly cancel over a sample's regions -- a softmax's dlogits sum to zero -- so bf16 operands move it by far
    # more than their own 2^-9, here as on a plain tensor with "bf16-att".)
    d1, x = seen["d1"], seen["x"]
    Rp = ops.pad_rows(rows)
    assert d1.dtype == x.dtype == torch.bfloat16 and d1.shape[0] == x.shape[0] == Rp > rows
    assert bool((d1[rows:].view(torch.int16) == 0).all()) and bool((x[rows:].view(torch.int16) == 0).all())
    ref = (d1.double().t() @ x.double())[:, :CIN]
    gerr = _rel(got[1]["co_att_conv1.weight"].view(ref.shape), ref)
    print("regions_bf16_coatt %s %s: co_att_conv1.weight.grad rel err against fp64 of the same bf16 operands %.3e; against the fp32 "
          "head %.3e" % (kind, form, gerr, _rel(got[1]["co_att_conv1.weight"], base[1]["co_att_conv1.weight"])))
    assert gerr <= TB.GEMM_TOL and float(ref.abs().max()) > 0.0
    TB._same_bits(TB._step(model, kind, feats, q, tgt), got, "a second step")     # no atomics
    # eval: the same criterion
    model.eval()
    with torch.no_grad():
        a = model.forward(feats, q)
        a2 = model.forward(feats, q)
        model.regions_bf16_coatt = False
        b = model.forward(feats, q)
    model.train()
    assert torch.equal(a, a2) and _rel(a, b) <= BF16_TOL and not torch.equal(a, b)


@pytest.mark.parametrize("fold", [True, False], ids=["fold_norm", "no_fold_norm"])
@pytest.mark.parametrize("ov,side,fuse_dp", TB.SETTINGS, ids=["ov_%s_side_%s_fusedp_%s" % s for s in TB.SETTINGS])
@pytest.mark.parametrize("kind", ["mfb", "mhbcoatt"])
def test_small_every_setting(vqa, kind, ov, side, fuse_dp, fold):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, SMALL)
    rows = int(counts.sum())
    TB._set(model, regions_bf16=True, packed_coatt=True, overlap_streams=ov, side_bf16=side, fuse_bf16_dp=fuse_dp, fold_norm=fold)
    base = TB._step(model, kind, packed, q, tgt)
    model.regions_bf16_coatt = True
    got, _ = _census_step(ops, model, kind, packed, q, tgt)
    bf, f32 = _products(ops, model, rows)
    assert bf == (1, 1, 1) and f32 == (0, 0, 0), (bf, f32)
    err = _rel(got[0], base[0])
    print("regions_bf16_coatt %s overlap_streams=%s side_bf16=%s fuse_bf16_dp=%s fold_norm=%s: rel err %.3e"
          % (kind, ov, side, fuse_dp, fold, err))
    assert err <= BF16_TOL and not torch.equal(got[0], base[0])
    assert all(bool(torch.isfinite(g).all()) for g in got[1].values())


@pytest.mark.parametrize("form", ["packed", "packed-rows", "pair"])
@pytest.mark.parametrize("kind", ["mfb", "mhbcoatt"])
def test_ragged_takes_the_fusion_kernels_own_copy(vqa, functions, kind, form, monkeypatch):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, TB.RAGGED)
    N, L = img.shape[0], img.shape[1]
    rows = int(counts.sum()) if form == "packed-rows" else N * L
    feats = _feats(form, img, counts, packed)
    TB._set(model, regions_bf16=True, packed_coatt=form == "packed-rows")
    base = TB._step(model, kind, feats, q, tgt)
    model.regions_bf16_coatt = True
    seen = {}
    arm, rowscale, pool = functions._arm_link, ops.gemm_bf16_rowscale, functions._pool_fwd

    def spy_arm(link, inv, Lr, xb=None):
        seen["xb"] = xb[0] if xb else None
        return arm(link, inv, Lr, xb)

    def spy_rowscale(a, b, *args, **kw):
        seen["a"], seen["M"] = a, kw.get("M")
        return rowscale(a, b, *args, **kw)

    def spy_pool(feat, logits, unit, layout):
        res = pool(feat, logits, unit, layout)
        if layout is not None and res[0].shape[-1] == L:
            seen["wts"] = res[0].detach().clone()
        return res

    monkeypatch.setattr(functions, "_arm_link", spy_arm)
    monkeypatch.setattr(ops, "gemm_bf16_rowscale", spy_rowscale)
    monkeypatch.setattr(functions, "_pool_fwd", spy_pool)
    got, census = _census_step(ops, model, kind, feats, q, tgt)
    monkeypatch.undo()
    bf, f32 = _products(ops, model, rows)
    assert bf == (1, 1, 1) and f32 == (0, 0, 0), (bf, f32)
    xb = seen["xb"]
    assert xb is not None and xb.dtype == torch.bfloat16 and xb.shape == (ops.pad_rows(rows), 1024)
    assert seen["a"].data_ptr() == xb.data_ptr() and seen["M"] == rows             # the copy IS the operand, M the real rows
    assert bool((xb[rows:].view(torch.int16) == 0).all()) and bool((xb[:, CIN:].view(torch.int16) == 0).all())
    valid = RR.valid_mask(counts.cpu(), L).cuda()
    if form != "packed-rows":                                                     # zero rows behind each count
        assert bool((xb[:rows][~valid.view(-1)].view(torch.int16) == 0).all())
    wts = seen["wts"]
    behind = ~valid[:, None, :].expand_as(wts)
    assert float(wts[behind].abs().max()) == 0.0 and float(wts[~behind].abs().min()) > 0.0
    err = _rel(got[0], base[0])
    print("regions_bf16_coatt %s ragged %s: output rel err against regions_bf16 alone %.3e" % (kind, form, err))
    assert err <= BF16_TOL and not torch.equal(got[0], base[0])
    assert all(bool(torch.isfinite(g).all()) for g in got[1].values())
    TB._same_bits(TB._step(model, kind, feats, q, tgt), got, "a second step")
    assert census.get("cast_f32_bf16", 0) >= 1                                     # (the rows and the weights are still cast per step)


@pytest.mark.parametrize("kind", ["mfb", "mhbcoatt"])
def test_off_is_the_model_as_constructed_and_a_plain_tensor_is_not_touched(vqa, kind):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, SMALL)
    fresh = type(model)(model.cfg)                                                # a model nobody set the attribute on
    assert fresh.regions_bf16_coatt is False
    fresh.load_state_dict(model.state_dict())
    fresh = fresh.cuda().train()
    if kind != "mhbcoatt":
        fresh.unit_softmax = False
    for rb in (False, True):
        for feats in (packed, (img, counts), img):
            TB._set(fresh, regions_bf16=rb)
            TB._set(model, regions_bf16=rb, regions_bf16_coatt=False)
            a, ca = TB._census(ops, lambda: TB._step(fresh, kind, feats, q, tgt))
            b, cb = TB._census(ops, lambda: TB._step(model, kind, feats, q, tgt))
            TB._same_bits(a, b, "regions_bf16_coatt = False against a model as constructed")
            assert ca == cb                                                        # launch for launch
    # a plain tensor: the attribute changes no bit and no launch, under every gemm_dtype
    for dt in ("fp32", "bf16", "bf16-img", "bf16-att", "bf16-all"):
        for rb in (False, True):
            TB._set(model, gemm_dtype=dt, regions_bf16=rb, regions_bf16_coatt=False)
            a, ca = TB._census(ops, lambda: TB._step(model, kind, img, q, tgt))
            model.regions_bf16_coatt = True
            b, cb = TB._census(ops, lambda: TB._step(model, kind, img, q, tgt))
            TB._same_bits(a, b, "a plain tensor with gemm_dtype %s" % dt)
            assert ca == cb
    # a region form where regions_bf16 does not apply is refused by name, on the GPU as on the CPU
    TB._set(model, gemm_dtype="fp32", regions_bf16=False, regions_bf16_coatt=True)
    for feats in (packed, (img, counts)):
        with pytest.raises(vqa.VqfError, match="regions_bf16_coatt.*regions_bf16 = True"):
            model.forward(feats, q)
    TB._set(model, regions_bf16=True)                                             # with img_index regions_bf16's own refusal speaks
    with pytest.raises(vqa.VqfError, match="regions_bf16.*img_index"):
        model.forward(packed, q, img_index=torch.arange(img.shape[0], device="cuda"))
