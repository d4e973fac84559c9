"""Packed region features of HieCoAttenLadder (forward(PackedRegions(rows, offsets, max_regions), ids, q_length, img_index)), the
part that needs no GPU: the refusals (VqfError, raised before anything touches a device), the new entry points in the header, the
binding table and the built library, their argument checks on pointers that are never dereferenced, and the counts the model
derives from the offsets.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

import mfb_packed_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, E, T = 12, 32, 5
NEW = {"vqf_tanh_dropout_unpack_supported": 4, "vqf_tanh_dropout_unpack_fwd": 11, "vqf_tanh_dropout_pack_bwd": 12}


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _grouping(vqa):
    return sys.modules[vqa.PackedRegions.__module__]                              # host/grouping.py


def _features(counts=(3, 10, 1, 7), seed=3):
    rng = np.random.RandomState(seed)
    return [rng.randn(k, D) for k in counts]


def _model(vqa, coatt):
    return vqa.HieCoAttenLadder(img_size=D, vocab_size=20, embed_size=E, hidden_size=10, output_size=6, coatt=coatt)


# ---- the model's refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coatt", ["parallel", "alternating"])
def test_model_refusals_are_vqf_errors(vqa, coatt):
    """Every refusal is raised from the checks in front of the first launch, so none of them needs a GPU; each names what was passed."""
    model = _model(vqa, coatt)
    good = vqa.pack_region_features(_features())
    q = torch.ones(4, T, dtype=torch.long)
    P = vqa.PackedRegions
    rows, off, L = good.rows, good.offsets, good.max_regions
    with pytest.raises(vqa.VqfError, match="GPU tensors"):                       # CPU tensors: no CPU fallback
        model(good, q)
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        model(good, q, torch.tensor([5, 1, 2, 3]))
    for bad, what in ((P(rows.double(), off, L), "rows"), (P(rows.view(1, -1, D), off, L), "rows"), (P(rows.to(torch.bfloat16), off, L), "rows"),
                      (P([1.0], off, L), "rows"), (P(rows[:0], off, L), "rows"),
                      (P(rows, off.float(), L), "offsets"), (P(rows, off.to(torch.int16), L), "offsets"), (P(rows, off.tolist(), L), "offsets"),
                      (P(rows, off[:-1], L), "offsets"), (P(rows, off.view(-1, 1), L), "offsets"), (P(rows, off.to("meta"), L), "offsets.*device"),
                      (P(rows, off, 0), "max_regions"), (P(rows, off, 1025), "max_regions"), (P(rows, off, 10.0), "max_regions"),
                      (P(rows, off, True), "max_regions"),
                      (P(rows.to("meta"), off, L), "rows.*device.*meta"),            # rows not on the questions' device
                      (P(rows[:, :8].contiguous(), off, L), "img_size = %d.*8" % D)):
        with pytest.raises(vqa.VqfError, match=what):
            model(bad, q)
    # with img_index the offsets are per image: N = 7 questions over U = 4 images
    q7 = torch.ones(7, T, dtype=torch.long)
    idx = torch.tensor([2, 0, 0, 3, 0, 2, 1])
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        model(good, q7, None, idx)
    with pytest.raises(vqa.VqfError, match="offsets"):
        model(good, q7)                                                          # without img_index: one owner per question
    # a PackedRegions inside a pair
    for pair in ((good, torch.tensor([3, 10, 1, 7])), (good, None), [good, good]):
        with pytest.raises(vqa.VqfError, match="PackedRegions"):
            model(pair, q)


def test_shape_limits_of_the_new_kernels_are_refused(vqa):
    """more owners than the grid's 16-bit extent; an embed_size the 16-byte accesses cannot take"""
    U = 65536
    q = torch.ones(U, 1, dtype=torch.long)
    packed = vqa.PackedRegions(torch.zeros(U, D), torch.arange(U + 1), 1)
    with pytest.raises(vqa.VqfError, match="images=65536"):
        _model(vqa, "parallel")(packed, q)
    m6 = vqa.HieCoAttenLadder(img_size=D, vocab_size=20, embed_size=6, hidden_size=10, output_size=6)
    with pytest.raises(vqa.VqfError, match="E=6"):
        m6(vqa.pack_region_features(_features()), torch.ones(4, T, dtype=torch.long))


def test_forward_keeps_its_parameter_list_and_the_call_forms_are_documented(vqa):
    import inspect
    assert list(inspect.signature(vqa.HieCoAttenLadder.forward).parameters) == ["self", "img_features", "que_features", "q_length",
                                                                                "img_index"]
    assert "PackedRegions" in vqa.HieCoAttenLadder.__doc__ and "PackedRegions" in sys.modules[vqa.HieCoAttenLadder.__module__].__doc__
    assert "HieCoAttenLadder" in vqa.PackedRegions.__doc__ and "HieCoAttenLadder" in _grouping(vqa).__doc__.split("packed region features")[1]
    doc = vqa.evaluate.predict.__doc__
    assert "PackedRegions" in doc and "HieCoAttenLadder" in doc[doc.index("PackedRegions"):]


# ---- the counts the model derives from the offsets --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_counts_from_offsets_are_those_of_unpack(vqa, dtype):
    counts = (5, 1, 12, 12, 2)
    packed = vqa.pack_region_features(_features(counts, seed=5))
    packed = vqa.PackedRegions(packed.rows, packed.offsets.to(dtype), packed.max_regions)
    off, L = packed.offsets, packed.max_regions
    lens = _grouping(vqa)._region_lens(off[1:] - off[:-1], L)                       # what forward() hands the region-count kernels
    img, ulens = packed.unpack()
    assert lens.dtype == torch.int32 and lens.tolist() == ulens.tolist() == list(counts)
    assert torch.equal(img, PR.unpack_rows(packed.rows, off, L)[0])
    idx = _grouping(vqa)._group_index(torch.tensor([4, 0, 0, 2, 4, 1, 0]), len(counts))[0]
    lens_q, lens_u = _grouping(vqa)._region_lens(off[1:] - off[:-1], L, idx)
    assert lens_u.tolist() == list(counts) and lens_q.tolist() == [counts[i] for i in (4, 0, 0, 2, 4, 1, 0)]
    # malformed offsets are clamped like any img_length: to [1, L]
    assert _grouping(vqa)._region_lens(torch.tensor([0, 30, -4, 5]).to(dtype), L).tolist() == [1, L, 1, 5]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree_on_the_new_names_within_abi_7(vqa):
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    for name, nargs in NEW.items():
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(vqa.lib.SIGNATURES[name][1]) == len(decl.split(",")) == nargs, name
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7
    names = [lib.vqf_prof_kernel_name(i).decode() for i in range(lib.vqf_prof_num_kernels())]
    assert "tanh_dropout_unpack_fwd" in names and "tanh_dropout_pack_bwd" in names
    assert names.index("tanh_dropout_fwd") < names.index("zero_cols_len") < names.index("tanh_dropout_unpack_fwd")   # appended, none renamed
    for fn in ("tanh_dropout_unpack_supported", "tanh_dropout_unpack_fwd", "tanh_dropout_pack_bwd"):
        assert callable(getattr(vqa.ops, fn))
    assert issubclass(vqa.functions.TanhDropUnpackFn, torch.autograd.Function)


def test_supported_and_argument_checks_need_no_gpu(vqa):
    lib = vqa.lib.load()
    sup = lib.vqf_tanh_dropout_unpack_supported
    for ok in ((256, 14000, 100, 512), (1, 1, 1, 4), (65535, (1 << 29) - 1, 1024, 65536), (3, 1538, 1024, 1024)):
        assert sup(*ok) == 1 and vqa.ops.tanh_dropout_unpack_supported(*ok), ok
    for bad in ((0, 5, 3, 8), (65536, 5, 3, 8), (2, 0, 3, 8), (2, -1, 3, 8), (2, 1 << 29, 3, 8), (2, 5, 0, 8), (2, 5, 1025, 8), (2, 5, 3, 0),
                (2, 5, 3, 6), (2, 5, 3, 10), (2, 5, 3, 65540)):
        assert sup(*bad) == 0 and not vqa.ops.tanh_dropout_unpack_supported(*bad), bad
    fake = 4096                                   # never dereferenced: every call below is refused first
    BADARG, ALIGN, UNSUPPORTED = -1, -2, -3
    fwd = lambda z=fake, roff=fake, keep=None, p=0.0, U=2, R=5, L=3, E=8, y=fake: \
        lib.vqf_tanh_dropout_unpack_fwd(z, roff, keep, 0, p, U, R, L, E, y, None)
    bwd = lambda dy=fake, y=fake, roff=fake, keep=None, p=0.0, U=2, R=5, L=3, E=8, dz=fake: \
        lib.vqf_tanh_dropout_pack_bwd(dy, y, roff, keep, 0, p, U, R, L, E, dz, None)
    for f in (fwd, bwd):
        assert f(roff=None) == BADARG and f(roff=fake + 2) == BADARG           # a null or misaligned roff
        assert f(R=0) == BADARG and f(R=-3) == BADARG and f(U=0) == BADARG and f(L=0) == BADARG and f(E=0) == BADARG
        assert f(p=1.0) == BADARG and f(p=-0.5) == BADARG
        assert f(E=6) == UNSUPPORTED and f(E=10) == UNSUPPORTED and f(L=1025) == UNSUPPORTED and f(L=2000) == UNSUPPORTED
        assert f(U=65536) == UNSUPPORTED and f(R=1 << 29) == UNSUPPORTED
        assert f(keep=fake + 2) == ALIGN
        # the query agrees with the calls
        for dims in ((2, 5, 3, 6), (2, 5, 1025, 8), (65536, 5, 3, 8)):
            assert sup(*dims) == 0 and f(U=dims[0], R=dims[1], L=dims[2], E=dims[3]) == UNSUPPORTED
    assert fwd(z=None) == BADARG and fwd(y=None) == BADARG and fwd(z=fake + 4) == ALIGN and fwd(y=fake + 8) == ALIGN
    assert bwd(dy=None) == BADARG and bwd(y=None) == BADARG and bwd(dz=None) == BADARG
    assert bwd(dy=fake + 4) == ALIGN and bwd(y=fake + 4) == ALIGN and bwd(dz=fake + 8) == ALIGN
    # the wrappers refuse what they are handed before any pointer is taken
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        vqa.ops.tanh_dropout_unpack_fwd(torch.zeros(5, 8), torch.zeros(3, dtype=torch.int32), 2, 3)
