"""Region counts of MFB / MHBCoAtt (forward((img, img_length), ...)), the part that needs no GPU.

tests/mfb_regions_ref.py, the masked restatement the GPU tests compare against, is pinned on the oracle two ways: (a) with
lens = L everywhere it is the oracle, to fp64 rounding; (b) for MFB, whose samples are independent, row n is the oracle on the
single sample img[n, :lens[n]] with the matching rows of the keep masks -- logits, and the gradients summed over the samples.
Also here: data_loader.pad_region_features, the new entry points in the header and the binding table, the forward signatures.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import recipe
import mfb_regions_ref as RR
from cases import MFB_CASES, MHBCOATT_CASES, make_cfg
from golden_util import recipe_sd
from oracle import ref_torch as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _inputs(case, mhb, dt):
    cfg = make_cfg(case)
    N, T, L, D, H, s = case["N"], case["T"], cfg.img_feature_dim, cfg.img_feature_channel, cfg.hidden_dim, case["salt"]
    img = torch.from_numpy(recipe.img_features(N, L, D, s)).to(dt)
    q = torch.from_numpy(recipe.question_tokens(N, T, cfg.q_vocab_size, s))
    ml = torch.from_numpy(recipe.keep_mask((N, T, H), 0.3, "l"))
    drop = dict(m1=torch.from_numpy(recipe.keep_mask((N * L, 5000), 0.1, "m1")).view(N, L, 5000),
                m2=torch.from_numpy(recipe.keep_mask((N, 5000), 0.1, "m2")),
                m3=torch.from_numpy(recipe.keep_mask((N, 5000), 0.1, "m3")), l=ml.permute(1, 0, 2) if mhb else ml)
    sd = {k: v.to(dt).requires_grad_(True) for k, v in recipe_sd(O.mfb_shapes(cfg, mhb=mhb), s).items()}
    return cfg, img, q, drop, sd


@pytest.mark.parametrize("case,mhb,live", [(MFB_CASES[2], False, False), (MFB_CASES[2], False, True), (MFB_CASES[4], False, True),
                                           (MHBCOATT_CASES[1], True, False), (MHBCOATT_CASES[3], True, False)],
                         ids=["mfb", "mfb_live", "mfb_multilayer_live", "mhbcoatt", "mhbcoatt_glove"])
def test_full_lengths_are_the_oracle_fp64(case, mhb, live):
    cfg, img, q, drop, sd = _inputs(case, mhb, torch.float64)
    N, L = img.shape[:2]
    glove = None
    if case["glove"]:
        glove = torch.from_numpy(recipe.sym_tensor((N, case["T"], cfg.emb_dim), 0.5, recipe.name_seed("glove", case["salt"]))).double()
    lens = torch.full((N,), L)
    if mhb:
        a = RR.mhbcoatt_forward(sd, cfg, img, q, lens, glove=glove, drop=drop)
        b = O.mhbcoatt_forward(sd, cfg, img, q, glove=glove, drop=drop)
    else:
        a = RR.mfb_forward(sd, cfg, img, q, lens, drop=drop, live_softmax=live)
        b = O.mfb_forward(sd, cfg, img, q, drop=drop, live_softmax=live)
    assert float((a - b).detach().abs().max()) <= 1e-12 * float(b.detach().abs().max())
    w = torch.from_numpy(recipe.sym_tensor(tuple(a.shape), 1.0, 77)).double()
    ga = torch.autograd.grad((a * w).sum(), list(sd.values()), allow_unused=True)
    gb = torch.autograd.grad((b * w).sum(), list(sd.values()), allow_unused=True)
    gmax = max(float(g.abs().max()) for g in gb if g is not None)
    for k, x, y in zip(sd, ga, gb):
        assert (x is None) == (y is None), k
        if y is not None:
            assert float((x - y).abs().max()) <= 1e-11 * gmax, k
    # counts beyond L and below 1 are clamped
    c = (RR.mhbcoatt_forward(sd, cfg, img, q, lens + 9, glove=glove, drop=drop) if mhb else
         RR.mfb_forward(sd, cfg, img, q, lens + 9, drop=drop, live_softmax=live))
    assert torch.equal(a, c)


@pytest.mark.parametrize("case,live", [(MFB_CASES[3], False), (MFB_CASES[3], True), (MFB_CASES[4], True)],
                         ids=["mfb_n5", "mfb_n5_live", "mfb_multilayer_live"])
def test_mfb_row_n_is_the_oracle_on_its_own_regions_fp64(case, live):
    """MFB's samples are independent: row n of the masked model == the oracle on the single sample cut to its real regions."""
    cfg, img, q, drop, sd = _inputs(case, False, torch.float64)
    N, L = img.shape[:2]
    lens = torch.tensor([1, L, L - 1, 7, 4][:N])
    # what the padded rows hold must not matter: any finite values
    pad = ~RR.valid_mask(lens, L)
    img = torch.where(pad[:, :, None], torch.from_numpy(recipe.sym_tensor(tuple(img.shape), 3.0, 5)).double(), img)
    tgt = torch.from_numpy(recipe.hard_answers(N, cfg.a_vocab_size, case["salt"]))
    a = RR.mfb_forward(sd, cfg, img, q, lens, drop=drop, live_softmax=live)
    ga = torch.autograd.grad(torch.nn.functional.cross_entropy(a, tgt, reduction="sum"), list(sd.values()), allow_unused=True)
    rows, gsum = [], None
    for n in range(N):
        k = int(lens[n])
        d1 = dict(m1=drop["m1"][n:n + 1, :k], m2=drop["m2"][n:n + 1], l=drop["l"][n:n + 1])
        b = O.mfb_forward(sd, cfg, img[n:n + 1, :k], q[n:n + 1], drop=d1, live_softmax=live)
        rows.append(b.detach())
        g = torch.autograd.grad(torch.nn.functional.cross_entropy(b, tgt[n:n + 1], reduction="sum"), list(sd.values()),
                                allow_unused=True)
        gsum = list(g) if gsum is None else [x if y is None else (y if x is None else x + y) for x, y in zip(gsum, g)]
    b = torch.cat(rows)
    assert float((a - b).detach().abs().max()) <= 1e-12 * float(b.detach().abs().max())
    # gradients: the batched and the per-sample products round differently (1e-16), and the signed square root's second
    # derivative (|s|^-3/2 / 4 at pooled sums down to ~1e-4) carries that into the gradients at ~1e-10: golden_util.check_grads64's
    # fp64 criterion, 1e-8
    gmax = max(float(g.abs().max()) for g in gsum if g is not None)
    live_img = 0.0
    for k, x, y in zip(sd, ga, gsum):
        assert (x is None) == (y is None), k
        if y is not None:
            assert float((x - y).abs().max()) <= 1e-8 * gmax, k
            if k == "img_conv1d.weight":
                live_img = float(y.abs().max())
    assert (live_img > 0.0) == live              # under the singleton-axis softmax the projection is dead, as in the reference


def test_padding_width_does_not_matter_fp64():
    """MHBCoAtt (the samples interact through the batch-axis LSTM, not through the regions): widening the pad changes nothing."""
    case = MHBCOATT_CASES[1]
    cfg, img, q, drop, sd = _inputs(case, True, torch.float64)
    N, L, D = img.shape
    lens = torch.tensor([3, L, 9])
    a = RR.mhbcoatt_forward(sd, cfg, img, q, lens)
    wide = torch.cat((img, torch.from_numpy(recipe.sym_tensor((N, 5, D), 2.0, 8)).double()), 1)
    b = RR.mhbcoatt_forward(sd, cfg, wide, q, lens)
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    full = O.mhbcoatt_forward(sd, cfg, img, q)
    assert float((a - full).abs().max()) > 1e-6 * float(a.abs().max())      # and the counts do matter


# ---- data_loader.pad_region_features ---------------------------------------------------------------------------------------------
def test_pad_region_features(vqa):
    rng = np.random.RandomState(3)
    feats = [rng.randn(k, 6) for k in (3, 10, 1, 7)]
    img, lens = vqa.pad_region_features(feats)
    assert img.dtype == torch.float32 and lens.dtype == torch.int64 and not img.is_cuda and not lens.is_cuda
    assert tuple(img.shape) == (4, 10, 6) and lens.tolist() == [3, 10, 1, 7]
    for n, f in enumerate(feats):
        assert np.array_equal(img[n, :f.shape[0]].numpy(), f.astype(np.float32))
        assert float(img[n, f.shape[0]:].abs().max()) == 0.0 if f.shape[0] < 10 else True
    img8, lens8 = vqa.pad_region_features(iter(feats), multiple=8)
    assert tuple(img8.shape) == (4, 16, 6) and torch.equal(lens8, lens) and torch.equal(img8[:, :10], img)
    assert float(img8[:, 10:].abs().max()) == 0.0
    one, l1 = vqa.pad_region_features([np.ones((2, 4), dtype=np.float64)], multiple=2)
    assert tuple(one.shape) == (1, 2, 4) and l1.tolist() == [2]
    assert vqa.data_loader.pad_region_features is vqa.pad_region_features


def test_pad_region_features_refusals(vqa):
    for bad in ([], [np.ones((3, 4)), np.ones((3, 5))], [np.ones(4)], [np.ones((0, 4))]):
        with pytest.raises(ValueError):
            vqa.pad_region_features(bad)
    with pytest.raises(ValueError):
        vqa.pad_region_features([np.ones((3, 4))], multiple=0)


# ---- the C ABI and the public interface --------------------------------------------------------------------------------------------
NEW = ["vqf_mfb_fuse_fwd_len", "vqf_mfb_fuse_bwd_len", "vqf_mfb_fuse_fwd_grouped_len", "vqf_mfb_fuse_bwd_grouped_len",
       "vqf_glimpse_pool_fwd_grouped_len", "vqf_glimpse_pool_bwd_grouped_len"]


def test_header_and_binding_table_declare_the_region_count_forms_within_abi_7(vqa):
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    for name in NEW:
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7


def test_null_lens_is_a_bad_argument_without_a_gpu(vqa):
    """The argument checks come before any launch: a null or misaligned lens returns VQF_E_BADARG (-1)."""
    lib = vqa.lib.load()
    fake = 4096                                   # never dereferenced: every call below is refused first
    assert lib.vqf_mfb_fuse_fwd_len(fake, None, fake, None, None, 0, 0.0, 2, 3, 8, fake, fake, None) == -1
    assert lib.vqf_mfb_fuse_fwd_len(fake, None, fake, fake + 2, None, 0, 0.0, 2, 3, 8, fake, fake, None) == -1
    assert lib.vqf_mfb_fuse_bwd_len(fake, fake, fake, fake, fake, fake, None, fake, None, None, 0, 0.0, 2, 3, 8, fake, fake, None,
                                    fake, 1 << 30, None) == -1
    assert lib.vqf_mfb_fuse_fwd_grouped_len(fake, None, fake, fake, None, fake, None, 0, 0.0, 2, 2, 3, 8, fake, fake, None) == -1
    assert lib.vqf_mfb_fuse_fwd_grouped_len(fake, None, fake, fake, fake, fake + 1, None, 0, 0.0, 2, 2, 3, 8, fake, fake, None) == -1
    assert lib.vqf_mfb_fuse_bwd_grouped_len(fake, fake, fake, fake, fake, fake, None, fake, fake, fake, fake, fake, None, None, 0, 0.0,
                                            2, 2, 3, 8, fake, fake, None, fake, 1 << 30, None) == -1
    assert lib.vqf_glimpse_pool_fwd_grouped_len(fake, fake, fake, None, 2, 2, 3, 8, 2, fake, fake, None) == -1
    assert lib.vqf_glimpse_pool_bwd_grouped_len(fake, None, fake, fake, fake, fake, fake, fake + 2, 2, 2, 3, 8, 2, fake, None, None) == -1


def test_counts_travel_with_the_features_and_forward_keeps_its_parameters(vqa):
    """forward()'s parameter lists are pinned (tests/test_mfb_shared_cpu.py): the counts come as the pair (img, img_length)."""
    import importlib
    p = list(inspect.signature(vqa.MFB.forward).parameters)
    assert p == ["self", "img_features", "questions", "is_training", "img_index"]
    p = list(inspect.signature(vqa.MHBCoAtt.forward).parameters)
    assert p == ["self", "img_features", "questions", "glove_matrix", "is_training", "img_index"]
    assert "img_length" in vqa.MFB.forward.__doc__ and "img_length" in vqa.MHBCoAtt.forward.__doc__
    assert "img_length" in vqa.evaluate.predict.__doc__
    split = importlib.import_module(vqa.__name__ + ".host.mfb").split_region_features
    img, lens = torch.zeros(2, 3, 4), torch.ones(2, dtype=torch.int64)
    assert split("MFB", img) == (img, None) and split("MFB", (img, None)) == (img, None)
    a, b = split("MFB", [img, lens])
    assert a is img and b is lens
    for bad in ((img,), (img, lens, lens), ([1, 2], lens)):
        with pytest.raises(vqa.VqfError, match="img_length"):
            split("MFB", bad)


def test_img_length_refusals_that_need_no_gpu(vqa):
    import importlib
    gr = importlib.import_module(vqa.__name__ + ".host.grouping")
    dev = torch.device("cpu")
    gr.check_img_length("MFB", torch.ones(5, dtype=torch.int32), 5, dev)
    for bad in (torch.ones(5), [3, 4, 5, 6, 7], torch.ones(4, dtype=torch.int64), torch.ones((5, 1), dtype=torch.int64)):
        with pytest.raises(vqa.VqfError, match="img_length"):
            gr.check_img_length("MFB", bad, 5, dev)
    with pytest.raises(vqa.VqfError, match="img_length.*device"):
        gr.check_img_length("MFB", torch.ones(5, dtype=torch.int64), 5, torch.device("cuda", 0))
    # the counts are clamped to [1, L] without a host read; with an index the per-question counts are one gather
    lens = gr._region_lens(torch.tensor([0, 3, 99, -4]), 20)
    assert lens.dtype == torch.int32 and lens.tolist() == [1, 3, 20, 1]
    lq, lu = gr._region_lens(torch.tensor([5, 99, 2]), 20, torch.tensor([2, 0, 0, 2], dtype=torch.int32))
    assert lu.tolist() == [5, 20, 2] and lq.tolist() == [2, 5, 5, 2] and lq.dtype == lu.dtype == torch.int32
