"""MFB / MHBCoAtt regions_bf16 (the bf16 image projection on packed and counted regions) on the GPU, model level.

Train steps draw their dropout masks in the kernels (Philox) from seeds of torch's CPU generator, re-seeded before every step: two
steps of one model see the same masks, whatever regions_bf16 is (the element indices stay those of the padded tensor).
MFB runs with unit_softmax = False throughout: under the reference's unit softmax the fusion over the regions cannot reach MFB's
logits and img_conv1d's gradient is exactly zero, so nothing this attribute touches would show.

  full counts   D = 2048, O = 1000, N = 8, L = 100 (N L = 800, a multiple of 32): on a PackedRegions and on the pair, every count L,
                outputs and every gradient carry the BITS of the plain tensor with gemm_dtype = "bf16-img".
  ragged        N = 12, L = 100, counts 100 x 10, 36, 1: R = 1037 (5 x 20 tiles of the forward product, not a multiple of 32).
                Outputs within 3e-2 (max-norm relative, tests/test_gpu_bf16.py::_rel -- the project's bf16 criterion) of
                regions_bf16 = False and not equal to it; the large-tile bf16 GEMM takes exactly the two products of a step and the
                128x128 one none; img_conv1d's weight gradient within 2e-5 of the fp64 product of the bf16 operands the node handed
                to the GEMM (whose tails are exact zeros); attention weights exact zeros behind each count; other finite values in
                the padded rows of the pair change no bit.
  small dims    D = 96, L = 20 (fp32 P, bf16 dP: the large-tile kernel does not apply): 3e-2 and not equal; packed and packed-rows
                agree within 1e-4; every overlap_streams / side_bf16 / fuse_bf16_dp setting.
  default off   regions_bf16 = False is the model as constructed, bit for bit; a plain tensor is not touched by the attribute.
"""
import importlib

import pytest
import torch

import recipe
import mfb_regions_ref as RR
import test_gpu_mfb_regions as TR
import test_gpu_mfb_packed as TP
from cases import make_cfg
from test_gpu_bf16 import _rel

pytestmark = pytest.mark.gpu

BF16_TOL = 3e-2                                          # the project's stated bf16 criterion (README, tests/test_gpu_bf16.py)
GEMM_TOL = 2e-5                                          # tests/test_gpu_bf16.py: fp32 accumulation against fp64 on the same bf16 values
FULL = dict(N=8, L=100, D=2048, counts=[100] * 8)
RAGGED = dict(N=12, L=100, D=2048, counts=[100] * 10 + [36, 1])
SMALL = dict(N=3, L=20, D=96, counts=[7, 20, 1])
KINDS = ["mfb", "mfb_multilayer", "mhbcoatt"]
# overlap_streams x side_bf16 x fuse_bf16_dp, as the plain bf16 path treats them: one node (ImgFuseFn) unless fuse_bf16_dp is off or
# a real second stream has side_bf16; then img_project + ImgProjLateFn + MfbFuseFn (a bf16 P0 where the large-tile GEMM stores one),
# or, "same-stream", ImgProjFn with an fp32 P0, whose fp32 dP is cast -- with the row padding -- for the weight gradient
SETTINGS = [(ov, side, dp) for ov in (True, False, "same-stream") for side in (False, True) for dp in (True, False)]
_MODELS, _BUILT, _BASE = {}, {}, {}


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def functions(vqa):
    return importlib.import_module(vqa.__name__ + ".host.functions")


def _build(vqa, kind, shape):
    """(model, img zero-padded (N, L, D), counts, PackedRegions, q, tgt) of one kind at one shape; built once, attributes reset"""
    key = (kind, shape["N"], shape["L"], shape["D"])
    if key not in _BUILT:
        mhb = kind == "mhbcoatt"
        base = TR.MHB3 if mhb else (TR.MFBM if kind == "mfb_multilayer" else TR.MFB3)
        case = dict(base, N=shape["N"], L=shape["L"], D=shape["D"], name="regions_bf16_%s_n%d_l%d_d%d" % key)
        cfg = make_cfg(case)
        N, L, D = shape["N"], shape["L"], shape["D"]
        if (kind, L, D) not in _MODELS:                                           # (the parameters do not depend on N)
            model = (vqa.MHBCoAtt if mhb else vqa.MFB)(cfg)
            model.load_state_dict({k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"]))
                                   for k, v in model.state_dict().items()})
            _MODELS[(kind, L, D)] = model.cuda().train()
        model = _MODELS[(kind, L, D)]
        counts = torch.tensor(shape["counts"], dtype=torch.int64, device="cuda")
        img = torch.from_numpy(recipe.img_features(N, L, D, case["salt"])).cuda()
        img = torch.where(RR.valid_mask(counts.cpu(), L).cuda()[:, :, None], img, torch.zeros_like(img))
        q = torch.from_numpy(recipe.question_tokens(N, case["T"], cfg.q_vocab_size, case["salt"])).cuda()
        tgt = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, case["salt"]) if mhb
                               else recipe.hard_answers(N, cfg.a_vocab_size, case["salt"])).cuda()
        _BUILT[key] = (model, img, counts, TP._packed(vqa, img, counts), q, tgt)
    model = _BUILT[key][0]
    _set(model, gemm_dtype="fp32", regions_bf16=False, packed_coatt=False, overlap_streams=True, side_bf16=False, fuse_bf16_dp=True)
    if kind != "mhbcoatt":
        model.unit_softmax = False
    return _BUILT[key]


def _set(model, **attrs):
    for k, v in attrs.items():
        setattr(model, k, v)


def _step(model, kind, feats, q, tgt):
    """one train step under a fixed seed -> (out, {name: grad}), clones"""
    torch.manual_seed(20240)
    out, grads = TR._step(model, kind == "mhbcoatt", feats, q, tgt)
    return out.clone(), {k: v.clone() for k, v in grads.items()}


def _forms(img, counts, packed):
    return {"packed": packed, "pair": (img, counts)}


def _fp32(vqa, kind, shape, form):
    """the step with regions_bf16 = False (default settings) on one call form: computed once, never modified"""
    key = (kind, shape["N"], shape["L"], shape["D"], form)
    if key not in _BASE:
        model, img, counts, packed, q, tgt = _build(vqa, kind, shape)
        _set(model, packed_coatt=form == "packed-rows")
        feats = packed if form.startswith("packed") else (img, counts)
        _BASE[key] = _step(model, kind, feats, q, tgt)
    return _BASE[key]


def _same_bits(a, b, what):
    out_a, ga = a
    out_b, gb = b
    assert torch.equal(out_a, out_b), what + ": outputs differ"
    assert set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), "%s: gradient of %s differs" % (what, k)


# ---- full counts: the bits of the plain "bf16-img" model -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mfb", "mhbcoatt"])
def test_full_counts_carry_the_bits_of_the_plain_bf16_img_model(vqa, kind):
    model, img, counts, packed, q, tgt = _build(vqa, kind, FULL)
    assert img.shape[0] * img.shape[1] == 800 and 800 % 32 == 0 and bool((counts == img.shape[1]).all())
    before = vqa.ops.stat("gemm_bf16_big")
    _set(model, gemm_dtype="bf16-img")
    plain = _step(model, kind, img, q, tgt)
    assert vqa.ops.stat("gemm_bf16_big") - before == 2                            # the plain model's projection and weight gradient
    _set(model, gemm_dtype="fp32", regions_bf16=True)
    for name, feats in _forms(img, counts, packed).items():
        before = vqa.ops.stat("gemm_bf16_big")
        got = _step(model, kind, feats, q, tgt)
        assert vqa.ops.stat("gemm_bf16_big") - before == 2, name
        _same_bits(got, plain, "regions_bf16 on the %s form against the plain tensor with bf16-img" % name)
    assert float(plain[1]["img_conv1d.weight"].abs().max()) > 0.0
    _set(model, regions_bf16=False)                                               # and the fp32 form is another result
    assert not torch.equal(_step(model, kind, packed, q, tgt)[0], plain[0])


# ---- ragged counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "packed-rows", "pair"])
@pytest.mark.parametrize("kind", ["mfb", "mhbcoatt"])
def test_ragged_counts(vqa, functions, kind, form, monkeypatch):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, RAGGED)
    N, L = img.shape[0], img.shape[1]
    R = int(counts.sum())
    assert R == 1037 and R >= 1025 and R % 32 != 0 and packed.rows.shape[0] == R
    out0, grads0 = _fp32(vqa, kind, RAGGED, form)
    _set(model, regions_bf16=True, packed_coatt=form == "packed-rows")
    feats = packed if form.startswith("packed") else (img, counts)
    seen = {}
    wgrad, pool = functions._img_wgrad, functions._pool_fwd

    def spy_wgrad(dP, img2, wi):
        seen["dP"], seen["img2"] = dP.detach().clone(), img2.detach().clone()
        return wgrad(dP, img2, wi)

    def spy_pool(feat, logits, unit, layout):
        res = pool(feat, logits, unit, layout)
        if layout is not None and res[0].shape[-1] == L:
            seen["wts"] = res[0].detach().clone()
        return res

    monkeypatch.setattr(functions, "_img_wgrad", spy_wgrad)
    monkeypatch.setattr(functions, "_pool_fwd", spy_pool)
    big, small = ops.stat("gemm_bf16_big"), ops.stat("gemm_bf16_tile128")
    out, grads = _step(model, kind, feats, q, tgt)
    assert ops.stat("gemm_bf16_big") - big == 2                                    # the projection and its weight gradient
    assert ops.stat("gemm_bf16_tile128") - small == 0
    monkeypatch.undo()
    err = _rel(out, out0)
    print("regions_bf16 %s %s: output rel err against fp32 %.3e" % (kind, form, err))
    assert err <= BF16_TOL
    assert not torch.equal(out, out0)                                             # the bf16 kernels really ran
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and set(grads) == set(grads0)
    # the weight gradient: both operands bf16, K a multiple of 32, exact zeros behind the real rows, fp32 accumulation
    rows = R if form.startswith("packed") else N * L
    dP, img2 = seen["dP"], seen["img2"]
    assert dP.dtype == img2.dtype == torch.bfloat16 and dP.shape[0] == img2.shape[0] == (rows + 31) // 32 * 32 and dP.shape[0] > rows
    assert bool((dP[rows:].view(torch.int16) == 0).all()) and bool((img2[rows:].view(torch.int16) == 0).all())
    ref = dP.double().t() @ img2.double()
    gerr = _rel(grads["img_conv1d.weight"].view(ref.shape), ref)
    print("regions_bf16 %s %s: img_conv1d.weight.grad rel err against fp64 of the same bf16 operands %.3e" % (kind, form, gerr))
    assert gerr <= GEMM_TOL and float(ref.abs().max()) > 0.0
    if form == "pair":                                                            # the padded dP rows are exact zeros too
        pad = ~RR.valid_mask(counts.cpu(), L).cuda().view(-1)
        assert bool((dP[:rows][pad].view(torch.int16) == 0).all())
    # the attention weights: (N, G, L), exact zeros behind each count
    wts = seen["wts"]
    behind = ~RR.valid_mask(counts.cpu(), L).cuda()[:, None, :].expand_as(wts)
    assert float(wts[behind].abs().max()) == 0.0 and float(wts[~behind].abs().min()) > 0.0
    # a second step: the same bits
    _same_bits(_step(model, kind, feats, q, tgt), (out, grads), "a second step")
    if form == "pair":                                                            # other finite values in the padded rows: no bit changes
        junk = torch.from_numpy(recipe.sym_tensor(tuple(img.shape), 2.0, 91)).cuda()
        img_j = torch.where(RR.valid_mask(counts.cpu(), L).cuda()[:, :, None], img, junk)
        assert not torch.equal(img_j, img)
        _same_bits(_step(model, kind, (img_j, counts), q, tgt), (out, grads), "junk in the padded rows")
    # eval mode: the same criterion
    model.eval()
    with torch.no_grad():
        a = model.forward(feats, q)
        model.regions_bf16 = False
        b = model.forward(feats, q)
    model.train()
    assert _rel(a, b) <= BF16_TOL and not torch.equal(a, b)


@pytest.mark.parametrize("ov,side,fuse_dp", SETTINGS, ids=["ov_%s_side_%s_fusedp_%s" % s for s in SETTINGS])
@pytest.mark.parametrize("kind", ["mfb", "mhbcoatt"])
def test_ragged_counts_every_setting(vqa, kind, ov, side, fuse_dp):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, RAGGED)
    out0, _ = _fp32(vqa, kind, RAGGED, "packed")
    _set(model, regions_bf16=True, overlap_streams=ov, side_bf16=side, fuse_bf16_dp=fuse_dp)
    big, small = ops.stat("gemm_bf16_big"), ops.stat("gemm_bf16_tile128")
    out, grads = _step(model, kind, packed, q, tgt)
    assert ops.stat("gemm_bf16_big") - big == 2 and ops.stat("gemm_bf16_tile128") - small == 0
    err = _rel(out, out0)
    print("regions_bf16 %s overlap_streams=%s side_bf16=%s fuse_bf16_dp=%s: rel err %.3e" % (kind, ov, side, fuse_dp, err))
    assert err <= BF16_TOL and not torch.equal(out, out0)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and float(grads["img_conv1d.weight"].abs().max()) > 0.0


# ---- small dims: fp32 P, bf16 dP -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_small_dims(vqa, kind):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, SMALL)
    D, W5 = img.shape[2], model.img_conv1d.out_channels
    assert D % 8 == 0 and W5 % 8 == 0 and int(counts.sum()) == 28
    outs = {}
    for form in ("packed", "packed-rows", "pair"):
        out0, grads0 = _fp32(vqa, kind, SMALL, form)
        feats = packed if form.startswith("packed") else (img, counts)
        for ov, side, fuse_dp in SETTINGS:
            _set(model, regions_bf16=True, packed_coatt=form == "packed-rows", overlap_streams=ov, side_bf16=side, fuse_bf16_dp=fuse_dp)
            big = ops.stat("gemm_bf16_big")
            out, grads = _step(model, kind, feats, q, tgt)
            assert ops.stat("gemm_bf16_big") == big                                # 28 rows: the large-tile kernel does not apply
            err = _rel(out, out0)
            print("regions_bf16 %s small %s overlap_streams=%s side_bf16=%s fuse_bf16_dp=%s: rel err %.3e"
                  % (kind, form, ov, side, fuse_dp, err))
            assert err <= BF16_TOL and not torch.equal(out, out0)
            assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and set(grads) == set(grads0)
            assert float(grads["img_conv1d.weight"].abs().max()) > 0.0
            if (ov, side, fuse_dp) == SETTINGS[0]:
                outs[form] = out
    e = _rel(outs["packed-rows"], outs["packed"])
    print("regions_bf16 %s small: packed-rows against packed %.3e" % (kind, e))
    assert e <= 1e-4                                                              # the README's bound for packed_coatt


# ---- default off -----------------------------------------------------------------------------------------------------------------------
def _census(ops, fn):
    fn()
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    return res, {k: v[0] for k, v in ops.prof_report().items()}


@pytest.mark.parametrize("kind", ["mfb", "mhbcoatt"])
def test_default_off_and_a_plain_tensor_is_not_touched(vqa, kind):
    ops = vqa.ops
    model, img, counts, packed, q, tgt = _build(vqa, kind, SMALL)
    cls = type(model)
    fresh = cls(model.cfg)                                                        # a model nobody set the attribute on
    assert fresh.regions_bf16 is False
    fresh.load_state_dict(model.state_dict())
    fresh = fresh.cuda().train()
    if kind != "mhbcoatt":
        fresh.unit_softmax = False
    for feats in (packed, (img, counts), img):
        a, ca = _census(ops, lambda: _step(fresh, kind, feats, q, tgt))
        model.regions_bf16 = False
        b, cb = _census(ops, lambda: _step(model, kind, feats, q, tgt))
        _same_bits(a, b, "regions_bf16 = False against a model as constructed")
        assert ca == cb                                                            # launch for launch
    # a plain tensor: the attribute changes no bit and no launch, in fp32 and beside a gemm_dtype of its own
    for dt in ("fp32", "bf16-img"):
        _set(model, gemm_dtype=dt, regions_bf16=False)
        a, ca = _census(ops, lambda: _step(model, kind, img, q, tgt))
        model.regions_bf16 = True
        b, cb = _census(ops, lambda: _step(model, kind, img, q, tgt))
        _same_bits(a, b, "a plain tensor with gemm_dtype %s" % dt)
        assert ca == cb
    _set(model, gemm_dtype="fp32", regions_bf16=True)                             # with img_index the region forms are refused by name
    with pytest.raises(vqa.VqfError, match="regions_bf16.*img_index"):
        model.forward(packed, q, img_index=torch.arange(img.shape[0], device="cuda"))
