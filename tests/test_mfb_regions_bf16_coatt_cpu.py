"""MFB / MHBCoAtt regions_bf16_coatt (the bf16 co-attention head on packed and counted regions), the part that needs no GPU: the three
new entry points in the header, the binding table and the built library; the error codes they return before any launch; the attribute,
its refusal on a region form where regions_bf16 does not apply (in front of every check that looks at a device, naming both
attributes), what it leaves alone (a plain tensor; regions_bf16's own refusal together with img_index) and its documentation.
"""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from cases import MFB_CASES, MHBCOATT_CASES, make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("len", "packed", "packed_rows")
NEW = ["vqf_mfb_fuse_fwd_%s_pbf16_rb" % f for f in FORMS]


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def _declared():
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _params(txt, name):
    return [a.strip() for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]


def test_header_binding_table_and_library_agree_on_the_new_names_within_abi_7(vqa):
    txt = _declared()
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7
    for name in NEW:
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
        mine, sib = vqa.lib.SIGNATURES[name][1], vqa.lib.SIGNATURES[name[:-len("_rb")]][1]
        assert len(mine) == len(_params(txt, name)), name
        # the arguments of the form without _rb, and behind R: the copy, its pitch, its allocated rows
        decl = _params(txt, name)
        names = [p.split()[-1].lstrip("*") for p in decl]
        at = names.index("R_bf16")
        assert decl[at:at + 3] == ["void* R_bf16", "int ldrb", "int rb_rows"] and names[at + 3] == "rowssq", name
        assert mine[:at] + mine[at + 3:] == sib and mine[at:at + 3] == [vqa.lib.c_p, vqa.lib.c_i, vqa.lib.c_i], name
    src = open(os.path.join(ROOT, "vqa-attention-networks_amd", "csrc", "fusion_regions_bf16.hip")).read()
    assert all(n in src for n in NEW)                                             # beside their siblings


def test_argument_checks_need_no_gpu(vqa):
    lib = vqa.lib.load()
    fake = 4096                                   # never dereferenced: every call below is refused first
    BADARG, ALIGN, UNSUPPORTED = -1, -2, -3
    N, R, L, O = 2, 5, 3, 8
    for form in FORMS:
        dims = (N, L) if form == "len" else (N, R, L)
        rows = R if form == "packed_rows" else N * L

        def fwd(arr=fake, O=O, dims=dims, P=fake, q=fake, Rout=fake, Rb=fake, ldrb=32, rb_rows=32, ssq=fake):
            fn = getattr(lib, "vqf_mfb_fuse_fwd_%s_pbf16_rb" % form)
            return fn(P, None, q, arr, None, 0, 0.0, *dims, O, Rout, Rb, ldrb, rb_rows, ssq, None)

        assert fwd(arr=None) == BADARG                                             # null lens / roff
        assert fwd(arr=fake + 2) == BADARG                                         # ... misaligned
        for null in ("P", "q", "Rout", "Rb", "ssq"):                               # every other pointer
            assert fwd(**{null: None}) == BADARG, (form, null)
        for i in range(len(dims)):                                                 # a zero and a negative extent
            assert fwd(dims=dims[:i] + (0,) + dims[i + 1:]) == BADARG, (form, i)
            assert fwd(dims=dims[:i] + (-1,) + dims[i + 1:]) == BADARG, (form, i)
        assert fwd(O=0) == BADARG
        assert fwd(O=10) == UNSUPPORTED                                            # O % 4
        assert fwd(ldrb=28) == BADARG and fwd(ldrb=O) == BADARG and fwd(ldrb=0) == BADARG    # a pitch below O rounded up to 32
        assert fwd(O=40, ldrb=32) == BADARG and fwd(O=40, ldrb=40) == BADARG
        assert fwd(ldrb=34) == BADARG and fwd(ldrb=1028) == BADARG                 # the pitch's own bounds: % 4, <= 1024
        assert fwd(rb_rows=rows - 1) == BADARG and fwd(rb_rows=0) == BADARG        # fewer rows than the kernel writes
        assert fwd(Rb=fake + 8) == ALIGN                                           # the copy: 16-byte aligned
        assert fwd(Rout=fake + 4) == ALIGN and fwd(P=fake + 8) == ALIGN            # as the forms without _rb
    for form in ("packed", "packed_rows"):                                         # L > 1024: the packed forms' limit
        fn = getattr(lib, "vqf_mfb_fuse_fwd_%s_pbf16_rb" % form)
        assert fn(fake, None, fake, fake, None, 0, 0.0, N, R, 2000, O, fake, fake, 32, 1 << 20, fake, None) == UNSUPPORTED


# ---- the models -----------------------------------------------------------------------------------------------------------------------
def _features(counts, D, seed=3):
    rng = np.random.RandomState(seed)
    return [rng.randn(k, D) for k in counts]


@pytest.mark.parametrize("mhb", [False, True], ids=["mfb", "mhbcoatt"])
def test_regions_bf16_coatt_is_an_attribute_with_one_refusal(vqa, mhb):
    case = MHBCOATT_CASES[1] if mhb else MFB_CASES[2]
    cfg = make_cfg(case)
    cls, who = (vqa.MHBCoAtt, "MHBCoAtt") if mhb else (vqa.MFB, "MFB")
    model = cls(cfg)
    assert model.regions_bf16_coatt is False and model.regions_bf16 is False
    keys = list(model.state_dict().keys())
    model.regions_bf16_coatt = True
    assert list(model.state_dict().keys()) == keys                                # same parameters, same state_dict
    D = cfg.img_feature_channel
    packed = vqa.pack_region_features(_features((3, 10, 1, 7), D))
    img, lens = vqa.pad_region_features(_features((3, 10, 1, 7), D))
    q7 = torch.ones(7, case["T"], dtype=torch.long)
    q4 = torch.ones(4, case["T"], dtype=torch.long)
    idx = torch.tensor([2, 0, 0, 3, 0, 2, 1])

    def refused(form, *args, **kw):
        with pytest.raises(vqa.VqfError, match="regions_bf16_coatt.*regions_bf16 = True") as e:
            model(form, *args, **kw)
        assert who in str(e.value) and "regions_bf16_coatt" in str(e.value) and "gemm_dtype" in str(e.value)

    # regions_bf16 = False: refused on both region forms, on CPU tensors -- before anything looks at a device
    for form in (packed, (img, lens)):
        refused(form, q4)
        refused(form, q7, img_index=idx)                                          # (regions_bf16 does not apply here either)
    # a gemm_dtype other than "fp32": refused by this attribute, whatever regions_bf16 is, in front of that dtype's own refusals
    for rb in (False, True):
        model.regions_bf16 = rb
        for dt in ("bf16-att", "bf16", "bf16-all"):
            model.gemm_dtype = dt
            for form in (packed, (img, lens)):
                refused(form, q4)
    model.gemm_dtype = "fp32"
    # where regions_bf16 applies nothing is refused: the next check speaks
    model.regions_bf16 = True
    for form in (packed, (img, lens)):
        with pytest.raises(vqa.VqfError, match="GPU tensors"):
            model(form, q4)
    # together with img_index regions_bf16's own refusal fires, with its text
    for form in (packed, (img, lens)):
        with pytest.raises(vqa.VqfError, match="regions_bf16 = True does not take img_index"):
            model(form, q7, img_index=idx)
    # a plain tensor is not refused, with img_index or without, whatever the two attributes and gemm_dtype are
    for rb in (False, True):
        model.regions_bf16 = rb
        for dt in ("fp32", "bf16-att"):
            model.gemm_dtype = dt
            for args, kw in (((img, q7), dict(img_index=idx)), ((img, q4), {}), (((img, None), q4), {})):
                with pytest.raises(vqa.VqfError, match="GPU tensors"):
                    model(*args, **kw)
    # and without the attribute nothing of this is looked at
    _ = [setattr(model, k, v) for k, v in dict(gemm_dtype="fp32", regions_bf16=False, regions_bf16_coatt=False).items()]
    for form in (packed, (img, lens)):
        with pytest.raises(vqa.VqfError, match="GPU tensors"):
            model(form, q4)


def test_the_pruned_mode_is_not_touched(vqa):
    """MFB under the reference's unit softmax with pruned = True has no co-attention head: the attribute refuses nothing there"""
    case = MFB_CASES[2]
    model = vqa.MFB(make_cfg(case))
    model.pruned, model.unit_softmax, model.regions_bf16_coatt = True, True, True
    packed = vqa.pack_region_features(_features((3, 10, 1, 7), model.cfg.img_feature_channel))
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        model(packed, torch.ones(4, case["T"], dtype=torch.long))


def test_the_check_itself(vqa):
    mfb = importlib.import_module(vqa.__name__ + ".host.mfb")
    packed = vqa.pack_region_features(_features((3, 10, 1, 7), 16))
    img, lens = vqa.pad_region_features(_features((3, 10, 1, 7), 16))
    chk = mfb.regions_bf16_coatt_check
    for form in (packed, (img, lens), [img, lens]):
        assert chk("X", form, None, "fp32", True, True) is None                    # regions_bf16 applies
        assert chk("X", form, None, "fp32", False, False) is None                  # the attribute is off
        assert chk("X", form, None, "bf16", False, False) is None
        for dt, rb in (("fp32", False), ("bf16-att", True), ("bf16-att", 5000)):
            with pytest.raises(vqa.VqfError, match="^X: regions_bf16_coatt = True needs regions_bf16 = True and gemm_dtype"):
                chk("X", form, None, dt, rb, True)
    for plain in (img, (img, None)):
        assert chk("X", plain, None, "fp32", False, True) is None and chk("X", plain, None, "bf16-att", False, True) is None
    # the nodes' side of the request: a NormLink asks for the bf16 copy only when told to
    fn = importlib.import_module(vqa.__name__ + ".host.functions")
    assert fn.NormLink().want_xb is False and fn.NormLink(want_xb=True).want_xb is True


def test_the_attribute_is_documented(vqa):
    for cls in (vqa.MFB, vqa.MHBCoAtt):
        doc = cls.forward.__doc__
        assert "regions_bf16_coatt" in doc
        tail = doc.split("regions_bf16_coatt", 1)[1]
        assert "co_att_conv1" in tail and "bf16" in tail and "VqfError" in tail and "plain tensor" in tail
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "regions_bf16_coatt" in readme
