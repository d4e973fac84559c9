"""MFB / MHBCoAtt regions_bf16 (the bf16 image projection on packed and counted regions), the part that needs no GPU: the new entry
points in the header, the binding table and the built library; the error codes they return before any launch; the attribute, its two
refusals (together with img_index: in front of every check that looks at a device; a channel count or a projection width that is no
multiple of 8) and what it leaves alone (every gemm_dtype other than "fp32" keeps its own refusals, a plain tensor is not touched).
"""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from cases import MFB_CASES, MHBCOATT_CASES, make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
FWD = ["vqf_mfb_fuse_fwd_%s_pbf16" % f for f in ("len", "packed", "packed_rows")]
BWD = ["vqf_mfb_fuse_bwd_%s_%s" % (f, k) for f in ("len", "packed", "packed_rows") for k in ("pbf16", "bf16dp")]
NEW = FWD + BWD + ["vqf_cast_f32_bf16_rows"]


def _declared():
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _params(txt, name):
    return [a.strip() for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1).split(",")]


def test_header_binding_table_and_library_agree_on_the_new_names_within_abi_7(vqa):
    txt = _declared()
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    for name in NEW:
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
        assert len(vqa.lib.SIGNATURES[name][1]) == len(_params(txt, name)), name
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7
    # a forward takes the arguments of its fp32 sibling; a backward those of its sibling and dP_rows, an int right behind dP
    for name in FWD:
        assert vqa.lib.SIGNATURES[name] == vqa.lib.SIGNATURES[name[:-len("_pbf16")]], name
    for name in BWD:
        sib = vqa.lib.SIGNATURES[name.rsplit("_", 1)[0]][1]
        mine = vqa.lib.SIGNATURES[name][1]
        names = [p.split()[-1].lstrip("*") for p in _params(txt, name)]
        at = names.index("dP_rows")
        assert names[at - 1] == "dP_bf16" and _params(txt, name)[at] == "int dP_rows", name
        assert len(mine) == len(sib) + 1 and mine[:at] + mine[at + 1:] == sib and mine[at] is vqa.lib.c_i, name
    assert vqa.lib.SIGNATURES["vqf_cast_f32_bf16_rows"][1][:6] == vqa.lib.SIGNATURES["vqf_cast_f32_bf16"][1][:6]
    # the frozen table of the region entry points is about four sources: none of them spells a new public name
    for f in ("fusion", "attention", "hie_ladder_alt", "hie"):
        src = open(os.path.join(ROOT, "vqa-attention-networks_amd", "csrc", f + ".hip")).read()
        assert not [n for n in NEW if n in src], f


def test_argument_checks_need_no_gpu(vqa):
    lib = vqa.lib.load()
    fake = 4096                                   # never dereferenced: every call below is refused first
    BADARG, UNSUPPORTED = -1, -3
    N, R, L, O = 2, 5, 3, 8
    ws = lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O)
    for form in ("len", "packed", "packed_rows"):
        dims = (N, L) if form == "len" else (N, R, L)
        rows = N * L if form == "len" else R

        def fwd(arr, O=O, dims=dims):
            fn = getattr(lib, "vqf_mfb_fuse_fwd_%s_pbf16" % form)
            return fn(fake, None, fake, arr, None, 0, 0.0, *dims, O, fake, fake, None)

        assert fwd(None) == BADARG                                                  # null lens / roff
        assert fwd(fake + 2) == BADARG                                              # misaligned
        assert fwd(fake, O=10) == UNSUPPORTED                                       # O % 4
        assert fwd(fake, dims=(0,) + dims[1:]) == BADARG
        for kind in ("pbf16", "bf16dp"):
            def bwd(arr, dP_rows, O=O, dP=fake):
                fn = getattr(lib, "vqf_mfb_fuse_bwd_%s_%s" % (form, kind))
                return fn(fake, fake, fake, fake, fake, fake, None, fake, arr, None, 0, 0.0, *dims, O, dP, dP_rows, fake, None, fake, ws,
                          None)

            assert bwd(None, 32) == BADARG
            assert bwd(fake + 2, 32) == BADARG
            assert bwd(fake, rows - 1) == BADARG                                    # dP_rows below the rows the kernels own
            assert bwd(fake, 0) == BADARG
            assert bwd(fake, 32, O=10) == UNSUPPORTED
            assert bwd(None, rows - 1, O=10) == BADARG                              # the array speaks first, then dP_rows, then O
            assert bwd(fake, rows - 1, O=10) == BADARG
            assert bwd(fake, 32, dP=None) == BADARG
    fn = lib.vqf_mfb_fuse_fwd_packed_pbf16                                          # L > 1024: the packed forms' limit
    assert fn(fake, None, fake, fake, None, 0, 0.0, N, R, 2000, O, fake, fake, None) == UNSUPPORTED
    cast = lib.vqf_cast_f32_bf16_rows
    assert cast(fake, 5, 8, 8, fake, 8, 4, None) == BADARG                          # y_rows < R
    assert cast(None, 5, 8, 8, fake, 8, 32, None) == BADARG
    assert cast(fake, 5, 8, 8, fake, 12, 32, None) == -2                            # VQF_E_ALIGN: ldy % 8, as vqf_cast_f32_bf16


# ---- the models -----------------------------------------------------------------------------------------------------------------------
def _features(counts, D, seed=3):
    rng = np.random.RandomState(seed)
    return [rng.randn(k, D) for k in counts]


@pytest.mark.parametrize("mhb", [False, True], ids=["mfb", "mhbcoatt"])
def test_regions_bf16_is_an_attribute_with_two_refusals(vqa, mhb):
    case = MHBCOATT_CASES[1] if mhb else MFB_CASES[2]
    cfg = make_cfg(case)
    cls, who = (vqa.MHBCoAtt, "MHBCoAtt") if mhb else (vqa.MFB, "MFB")
    model = cls(cfg)
    assert model.regions_bf16 is False
    keys = list(model.state_dict().keys())
    model.regions_bf16 = True
    assert list(model.state_dict().keys()) == keys                                # same parameters, same state_dict
    D = cfg.img_feature_channel
    assert D % 8 == 0
    packed = vqa.pack_region_features(_features((3, 10, 1, 7), D))
    img, lens = vqa.pad_region_features(_features((3, 10, 1, 7), D))
    q7 = torch.ones(7, case["T"], dtype=torch.long)
    q4 = torch.ones(4, case["T"], dtype=torch.long)
    idx = torch.tensor([2, 0, 0, 3, 0, 2, 1])
    # together with img_index: refused on both region forms, on CPU tensors -- in front of every check that looks at a device
    for form in (packed, (img, lens)):
        with pytest.raises(vqa.VqfError, match="regions_bf16.*img_index") as e:
            model(form, q7, img_index=idx)
        assert who in str(e.value)
    # a plain tensor is not touched by the attribute, with img_index or without: the next check speaks
    for args, kw in (((img, q7), dict(img_index=idx)), ((img, q4), {}), (((img, None), q4), {})):
        with pytest.raises(vqa.VqfError, match="GPU tensors"):
            model(*args, **kw)
    # without img_index and with a channel count that is a multiple of 8 the attribute refuses nothing
    for form in (packed, (img, lens)):
        with pytest.raises(vqa.VqfError, match="GPU tensors"):
            model(form, q4)
    # every gemm_dtype other than "fp32" keeps its own refusals, with their messages
    for dt in ("bf16", "bf16-img", "bf16-all"):
        model.gemm_dtype = dt
        with pytest.raises(vqa.VqfError, match="PackedRegions is fp32 only.*bf16"):
            model(packed, q4)
        with pytest.raises(vqa.VqfError, match="PackedRegions is fp32 only.*bf16"):
            model(packed, q7, img_index=idx)
    model.gemm_dtype = "fp32"
    # D not a multiple of 8: refused by name, on CPU tensors
    for form in (vqa.pack_region_features(_features((3, 10, 1, 7), D + 4)), vqa.pad_region_features(_features((3, 10, 1, 7), D + 4))):
        with pytest.raises(vqa.VqfError, match="regions_bf16.*multiples of 8") as e:
            model(form, q4)
        assert who in str(e.value) and "D=%d" % (D + 4) in str(e.value)
    model.regions_bf16 = False                                                     # ... and only with the attribute
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        model(vqa.pack_region_features(_features((3, 10, 1, 7), D + 4)), q4)
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        model(packed, q7, img_index=idx)


def test_the_projection_width_is_checked_too(vqa):
    """fusion_region_layout's keyword is False or the projection's width 5*O (True: the models' 5000)"""
    mfb = importlib.import_module(vqa.__name__ + ".host.mfb")
    packed = vqa.pack_region_features(_features((3, 10, 1, 7), 16))
    q4 = torch.ones(4, 5, dtype=torch.long)
    with pytest.raises(vqa.VqfError, match="regions_bf16.*multiples of 8.*5\\*O=60"):
        mfb.fusion_region_layout("MFB", packed, q4, None, "fp32", False, 60)
    for width in (True, 5000, 40, False):                                          # accepted: the next check speaks
        with pytest.raises(vqa.VqfError, match="GPU tensors|questions' device"):
            mfb.fusion_region_layout("MFB", packed, q4, None, "fp32", False, width)
    with pytest.raises(vqa.VqfError, match="PackedRegions is fp32 only"):          # another gemm_dtype: not this attribute's business
        mfb.fusion_region_layout("MFB", packed, q4, None, "bf16", False, 60)
    import inspect
    assert list(inspect.signature(mfb.fusion_region_layout).parameters)[-1] == "regions_bf16"
    assert inspect.signature(mfb.fusion_region_layout).parameters["regions_bf16"].default is False


def test_the_attribute_is_documented(vqa):
    for cls in (vqa.MFB, vqa.MHBCoAtt):
        doc = cls.forward.__doc__
        assert "regions_bf16" in doc
        tail = doc.split("regions_bf16", 1)[1]
        assert "img_index" in tail and "bf16" in tail and "fp32" in tail
