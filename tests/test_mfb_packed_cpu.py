"""Packed region features of MFB / MHBCoAtt (forward(PackedRegions(rows, offsets, max_regions), ...)), the part that needs no GPU:
data_loader.pack_region_features against pad_region_features and the layout helpers of tests/mfb_packed_ref.py, the refusals of
the models (VqfError, raised before anything touches a device), and the new entry points in the header, the binding table and the
built library.
"""
import os
import re

import numpy as np
import pytest
import torch

import mfb_packed_ref as PR
from cases import MFB_CASES, MHBCOATT_CASES, make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _features(counts=(3, 10, 1, 7), D=6, seed=3):
    rng = np.random.RandomState(seed)
    return [rng.randn(k, D) for k in counts]


# ---- data_loader.pack_region_features ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multiple", [1, 8, 3])
def test_pack_unpack_is_pad_region_features_bit_for_bit(vqa, multiple):
    feats = _features()
    packed = vqa.pack_region_features(feats, multiple=multiple)
    assert isinstance(packed, vqa.PackedRegions) and not packed.rows.is_cuda and not packed.offsets.is_cuda
    img, lens = vqa.pad_region_features(feats, multiple=multiple)
    uimg, ulens = packed.unpack()
    assert uimg.dtype == torch.float32 and ulens.dtype == torch.int64
    assert torch.equal(uimg, img) and torch.equal(ulens, lens)
    assert packed.max_regions == img.shape[1] and isinstance(packed.max_regions, int)
    # the same layout as the independent helpers
    assert torch.equal(packed.rows, PR.pack_rows(img, lens)) and torch.equal(packed.offsets, PR.offsets_of(lens))
    pimg, plens = PR.unpack_rows(packed.rows, packed.offsets, packed.max_regions)
    assert torch.equal(pimg, img) and torch.equal(plens, lens)
    # an iterator, float64 input and a single image, as pad_region_features takes them
    one = vqa.pack_region_features(iter([np.ones((2, 4), dtype=np.float64)]), multiple=2)
    assert tuple(one.rows.shape) == (2, 4) and one.offsets.tolist() == [0, 2] and one.max_regions == 2
    assert vqa.data_loader.pack_region_features is vqa.pack_region_features


def test_offsets_invariants(vqa):
    counts = (5, 1, 12, 12, 2)
    packed = vqa.pack_region_features(_features(counts, D=4, seed=5))
    off = packed.offsets
    assert off.dtype == torch.int64 and tuple(off.shape) == (len(counts) + 1,)
    assert int(off[0]) == 0 and int(off[-1]) == packed.rows.shape[0] == sum(counts)
    d = off[1:] - off[:-1]
    assert d.tolist() == list(counts) and int(d.min()) >= 1 and int(d.max()) <= packed.max_regions == 12
    assert packed.rows.dtype == torch.float32 and packed.rows.is_contiguous()
    moved = packed.to("cpu")
    assert isinstance(moved, vqa.PackedRegions) and moved.max_regions == 12 and torch.equal(moved.rows, packed.rows)
    assert torch.equal(moved.offsets, packed.offsets)


def test_pack_region_features_refuses_what_pad_region_features_refuses(vqa):
    for bad in ([], [np.ones((3, 4)), np.ones((3, 5))], [np.ones(4)], [np.ones((0, 4))]):
        with pytest.raises(ValueError):
            vqa.pad_region_features(bad)
        with pytest.raises(ValueError, match="pack_region_features"):
            vqa.pack_region_features(bad)
    with pytest.raises(ValueError, match="pack_region_features"):
        vqa.pack_region_features([np.ones((3, 4))], multiple=0)


# ---- the models' refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mhb", [False, True], ids=["mfb", "mhbcoatt"])
def test_model_refusals_are_vqf_errors(vqa, mhb):
    """Every refusal is raised from the checks in front of the first launch, so none of them needs a GPU; each names what was passed."""
    case = MHBCOATT_CASES[1] if mhb else MFB_CASES[2]
    cfg = make_cfg(case)
    model = (vqa.MHBCoAtt if mhb else vqa.MFB)(cfg)
    D = cfg.img_feature_channel
    good = vqa.pack_region_features(_features((3, 10, 1, 7), D=D))
    q = torch.ones(4, case["T"], dtype=torch.long)
    P = vqa.PackedRegions
    rows, off, L = good.rows, good.offsets, good.max_regions
    with pytest.raises(vqa.VqfError, match="GPU tensors"):                       # CPU tensors: no CPU fallback
        model(good, q)
    for bad, what in ((P(rows.double(), off, L), "rows"), (P(rows.view(1, -1, D), off, L), "rows"), (P(rows.to(torch.bfloat16), off, L), "rows"),
                      (P([1.0], off, L), "rows"),
                      (P(rows, off.float(), L), "offsets"), (P(rows, off.to(torch.int16), L), "offsets"), (P(rows, off.tolist(), L), "offsets"),
                      (P(rows, off[:-1], L), "offsets"), (P(rows, off.view(-1, 1), L), "offsets"), (P(rows, off.to("meta"), L), "offsets.*device"),
                      (P(rows, off, 0), "max_regions"), (P(rows, off, 1025), "max_regions"), (P(rows, off, 10.0), "max_regions"),
                      (P(rows, off, True), "max_regions")):
        with pytest.raises(vqa.VqfError, match=what):
            model(bad, q)
    # with img_index the offsets are per image: N questions over U = 4 images
    q7 = torch.ones(7, case["T"], dtype=torch.long)
    idx = torch.tensor([2, 0, 0, 3, 0, 2, 1])
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        model(good, q7, img_index=idx)
    with pytest.raises(vqa.VqfError, match="offsets"):
        model(good, q7)                                                          # without img_index: one owner per question
    # a PackedRegions inside a pair
    for pair in ((good, torch.tensor([3, 10, 1, 7])), (good, None), [good, good]):
        with pytest.raises(vqa.VqfError, match="PackedRegions"):
            model(pair, q)
    # bf16
    for dt in ("bf16", "bf16-img", "bf16-all", "bf16-att"):
        model.gemm_dtype = dt
        with pytest.raises(vqa.VqfError, match="PackedRegions is fp32 only.*%s" % dt):
            model(good, q)


def test_the_call_forms_are_documented(vqa):
    assert "PackedRegions" in vqa.MFB.forward.__doc__ and "PackedRegions" in vqa.MHBCoAtt.forward.__doc__
    assert "PackedRegions" in vqa.evaluate.predict.__doc__
    assert "unpack" in vqa.PackedRegions.__doc__


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW = ["vqf_mfb_fuse_packed_supported", "vqf_mfb_fuse_fwd_packed", "vqf_mfb_fuse_bwd_packed", "vqf_mfb_fuse_fwd_grouped_packed",
       "vqf_mfb_fuse_bwd_grouped_packed", "vqf_glimpse_pool_fwd_packed", "vqf_glimpse_pool_bwd_packed"]


def test_header_binding_table_and_library_agree_on_the_packed_forms_within_abi_7(vqa):
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    for name in NEW:
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
        # as many arguments in the binding as in the declaration
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(vqa.lib.SIGNATURES[name][1]) == len(decl.split(",")), name
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7


def test_packed_supported_and_argument_checks_need_no_gpu(vqa):
    lib = vqa.lib.load()
    assert lib.vqf_mfb_fuse_packed_supported(512, 512, 27000, 100, 1000) == 1
    assert lib.vqf_mfb_fuse_packed_supported(7, 3, 28, 20, 1000) == 1 and lib.vqf_mfb_fuse_packed_supported(2, 2, 2, 1, 8) == 1
    for bad in ((0, 3, 28, 20, 1000), (7, 0, 28, 20, 1000), (7, 3, 0, 20, 1000), (7, 3, 28, 0, 1000), (7, 3, 28, 1025, 1000),
                (7, 3, 28, 20, 1002), (7, 3, 28, 20, 1028), (70000, 3, 28, 20, 1000), (7, 70000, 28, 20, 1000), (7, 3, 1 << 29, 20, 1000)):
        assert lib.vqf_mfb_fuse_packed_supported(*bad) == 0, bad
    fake = 4096                                   # never dereferenced: every call below is refused first
    BADARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    # a null or misaligned roff, R <= 0
    assert lib.vqf_mfb_fuse_fwd_packed(fake, None, fake, None, None, 0, 0.0, 2, 5, 3, 8, fake, fake, None) == BADARG
    assert lib.vqf_mfb_fuse_fwd_packed(fake, None, fake, fake + 2, None, 0, 0.0, 2, 5, 3, 8, fake, fake, None) == BADARG
    assert lib.vqf_mfb_fuse_fwd_packed(fake, None, fake, fake, None, 0, 0.0, 2, 0, 3, 8, fake, fake, None) == BADARG
    assert lib.vqf_mfb_fuse_fwd_packed(fake, None, fake, fake, None, 0, 0.0, 2, 5, 3, 10, fake, fake, None) == UNSUPPORTED
    assert lib.vqf_mfb_fuse_fwd_packed(fake, None, fake, fake, None, 0, 0.0, 2, 5, 2000, 8, fake, fake, None) == UNSUPPORTED
    bwd = (fake, fake, fake, fake, fake, fake, None, fake)
    assert lib.vqf_mfb_fuse_bwd_packed(*bwd, None, None, 0, 0.0, 2, 5, 3, 8, fake, fake, None, fake, 1 << 30, None) == BADARG
    assert lib.vqf_mfb_fuse_bwd_packed(*bwd, fake, None, 0, 0.0, 2, -1, 3, 8, fake, fake, None, fake, 1 << 30, None) == BADARG
    assert lib.vqf_mfb_fuse_fwd_grouped_packed(fake, None, fake, fake, None, None, 0, 0.0, 2, 2, 5, 3, 8, fake, fake, None) == BADARG
    assert lib.vqf_mfb_fuse_fwd_grouped_packed(fake, None, fake, None, fake, None, 0, 0.0, 2, 2, 5, 3, 8, fake, fake, None) == BADARG
    assert lib.vqf_mfb_fuse_fwd_grouped_packed(fake, None, fake, fake, fake + 1, None, 0, 0.0, 2, 2, 5, 3, 8, fake, fake, None) == BADARG
    gb = bwd + (fake, fake, fake)
    assert lib.vqf_mfb_fuse_bwd_grouped_packed(*gb, None, None, 0, 0.0, 2, 2, 5, 3, 8, fake, fake, None, fake, 1 << 30, None) == BADARG
    assert lib.vqf_mfb_fuse_bwd_grouped_packed(*gb, fake, None, 0, 0.0, 2, 2, 0, 3, 8, fake, fake, None, fake, 1 << 30, None) == BADARG
    need = lib.vqf_mfb_fuse_bwd_grouped_ws_bytes(2, 2, 3, 8)
    assert need > 0
    assert lib.vqf_mfb_fuse_bwd_grouped_packed(*gb, fake, None, 0, 0.0, 2, 2, 5, 3, 8, fake, fake, None, fake, need - 4, None) == WORKSPACE
    assert lib.vqf_mfb_fuse_bwd_grouped_packed(*gb, fake, None, 0, 0.0, 2, 2, 5, 3, 8, fake, fake, None, None, need, None) == WORKSPACE
    assert lib.vqf_glimpse_pool_fwd_packed(fake, fake, None, None, 2, 2, 5, 3, 8, 2, 0, fake, fake, None) == BADARG
    assert lib.vqf_glimpse_pool_fwd_packed(fake, fake, None, fake + 2, 2, 2, 5, 3, 8, 2, 0, fake, fake, None) == BADARG
    assert lib.vqf_glimpse_pool_fwd_packed(fake, fake, None, fake, 2, 2, 0, 3, 8, 2, 0, fake, fake, None) == BADARG
    assert lib.vqf_glimpse_pool_fwd_packed(fake, fake, None, fake, 2, 3, 5, 3, 8, 2, 0, fake, fake, None) == BADARG       # idx NULL: U = N
    assert lib.vqf_glimpse_pool_fwd_packed(fake, fake, fake, fake, 2, 3, 5, 3, 6, 2, 0, fake, fake, None) == UNSUPPORTED  # C % 4
    assert lib.vqf_glimpse_pool_fwd_packed(fake, fake, fake, fake, 2, 3, 5, 2000, 8, 2, 0, fake, fake, None) == UNSUPPORTED
    assert lib.vqf_glimpse_pool_bwd_packed(fake, None, fake, fake, None, None, 2, 2, 5, 3, 8, 2, 0, fake, None) == BADARG
    assert lib.vqf_glimpse_pool_bwd_packed(fake, None, fake, fake, fake + 2, fake, 2, 2, 5, 3, 8, 2, 0, fake, None) == BADARG
    assert lib.vqf_glimpse_pool_bwd_packed(fake, None, fake, fake, fake, fake, 2, 2, 5, 3, 8, 4, 0, fake, None) == UNSUPPORTED
