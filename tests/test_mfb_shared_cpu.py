"""Shared images of MFB / MHBCoAtt (forward(..., img_index)), the part that needs no GPU: the loader's group_batch, the header's
new entry points and their size queries, the forward signatures, and the fp64 identity the grouped backward rests on.  The
specification needs no new reference: it is oracle.ref_torch.mfb_forward / mhbcoatt_forward on img[idx]."""
import inspect
import os
import re

import pytest
import torch

import recipe
from cases import MHBCOATT_CASES, make_cfg
from golden_util import recipe_sd
from oracle import ref_torch as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _group_batch_loop(ids):
    rows, index = [], []
    for n, k in enumerate(ids):
        first = [m for m in range(n + 1) if ids[m] == k][0]
        if first == n:
            rows.append(n)
        index.append(rows.index(first))
    return rows, index


@pytest.mark.parametrize("ids", [
    [40, 7, 40, 40, 9, 7, 40],                       # first-occurrence order, not sorted order
    ["COCO_3", "COCO_1", "COCO_2"],                  # singletons: rows = arange, index = arange
    [5, 5, 5, 5],                                    # all ids equal: one image
    [11],
    [(1, "a"), (0, "b"), (1, "a")],                  # any hashable id
])
def test_group_batch_against_a_plain_loop(vqa, ids):
    rows, index = vqa.group_batch(ids)
    r_ref, i_ref = _group_batch_loop(ids)
    assert rows.dtype == torch.int64 and index.dtype == torch.int64 and not rows.is_cuda and not index.is_cuda
    assert rows.tolist() == r_ref and index.tolist() == i_ref
    assert [ids[r] for r in rows.tolist()] == list(dict.fromkeys(ids))          # the distinct ids in order of appearance
    assert all(ids[rows[u]] == ids[n] for n, u in enumerate(index.tolist()))     # question n finds its own image
    assert vqa.group_batch(iter(ids))[1].tolist() == i_ref                       # any iterable
    assert vqa.data_loader.group_batch is vqa.group_batch


def test_group_batch_refuses_an_empty_batch(vqa):
    with pytest.raises(ValueError):
        vqa.group_batch([])


NEW = ["vqf_mfb_fuse_grouped_supported", "vqf_mfb_fuse_fwd_grouped", "vqf_mfb_fuse_bwd_grouped_ws_bytes", "vqf_mfb_fuse_bwd_grouped"]


def test_header_declares_the_grouped_fusion_within_abi_7(vqa):
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    for name in NEW:
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7
    names = [lib.vqf_prof_kernel_name(i) for i in range(lib.vqf_prof_num_kernels())]
    assert b"mfb_fuse_bwd_image" in names


def test_grouped_fusion_envelope_and_workspace(vqa):
    lib = vqa.lib.load()
    ok = lib.vqf_mfb_fuse_grouped_supported
    assert ok(512, 128, 196, 1000) == 1 and ok(7, 3, 5, 1000) == 1 and ok(6, 1, 3, 8) == 1 and ok(1, 65535, 1, 4) == 1
    assert ok(65535, 65535, 196, 1000) == 1
    assert ok(65536, 3, 5, 1000) == 0 and ok(7, 65536, 5, 1000) == 0 and ok(7, 0, 5, 1000) == 0 and ok(0, 3, 5, 1000) == 0
    assert ok(7, 3, 5, 1002) == 0 and ok(7, 3, 5, 1028) == 0 and ok(7, 3, 0, 1000) == 0
    ws = lib.vqf_mfb_fuse_bwd_grouped_ws_bytes
    # dq partials as the plain backward has them, one bias-partial row per (image, row split), the reducer's 32 rows
    plain = lib.vqf_mfb_fuse_bwd_ws_bytes
    for N, U, L, Os in ((512, 128, 196, 1000), (7, 3, 5, 1000), (6, 1, 3, 8), (11, 2, 196, 1000), (512, 512, 196, 1000)):
        row = 5 * Os * 4
        dq_rows = (plain(N, L, Os) // row - 32) // 2
        got = ws(N, U, L, Os)
        assert got % row == 0 and got // row > dq_rows + 32
        img_rows = got // row - dq_rows - 32
        assert img_rows % U == 0 and 1 <= img_rows // U <= 32 and (img_rows // U) * 2 <= max(L, 2)      # every split owns a row pair
    assert ws(0, 3, 5, 1000) == 0 and ws(7, -1, 5, 1000) == 0
    # no workspace row scales with N * L: the size is far below one (N*L, 5*O) tensor
    assert ws(512, 128, 196, 1000) < 512 * 196 * 5000 * 4 // 8


def test_forward_signatures_keep_the_positional_call_forms(vqa):
    p = list(inspect.signature(vqa.MFB.forward).parameters)
    assert p == ["self", "img_features", "questions", "is_training", "img_index"]
    p = list(inspect.signature(vqa.MHBCoAtt.forward).parameters)
    assert p == ["self", "img_features", "questions", "glove_matrix", "is_training", "img_index"]
    assert inspect.signature(vqa.MFB.forward).parameters["img_index"].default is None
    import importlib
    hl = importlib.import_module(vqa.__name__ + ".host.hie_ladder")
    gr = importlib.import_module(vqa.__name__ + ".host.grouping")
    assert hl._group_index is gr._group_index


def test_refusals_that_need_no_gpu(vqa):
    import importlib
    gr = importlib.import_module(vqa.__name__ + ".host.grouping")
    dev = torch.device("cpu")
    gr.check_img_index("MFB", torch.zeros(5, dtype=torch.int32), 5, 3, dev)
    for bad, N, U in ((torch.zeros(5), 5, 3), ([0, 1], 2, 3), (torch.zeros(4, dtype=torch.int64), 5, 3),
                      (torch.zeros((5, 1), dtype=torch.int64), 5, 3), (torch.zeros(5, dtype=torch.int64), 5, 65536),
                      (torch.zeros(65536, dtype=torch.int64), 65536, 3)):
        with pytest.raises(vqa.VqfError, match="MFB"):
            gr.check_img_index("MFB", bad, N, U, dev)
    with pytest.raises(vqa.VqfError, match="device"):
        gr.check_img_index("MFB", torch.zeros(5, dtype=torch.int64), 5, 3, torch.device("cuda", 0))


def test_shared_projection_gradient_is_the_grouped_sum_fp64():
    """The identity the grouped backward rests on, in fp64 on the oracle: the img_conv1d.weight gradient of the model called on
    img[idx] equals (index_add of the per-question dP into image rows)^T times img -- dP summed per image, then ONE product
    over U*L rows -- and the bias gradient is that sum's column sum."""
    case = MHBCOATT_CASES[1]
    cfg = make_cfg(case)
    U, T, L, D = case["N"], case["T"], cfg.img_feature_dim, cfg.img_feature_channel
    N = 2 * U + 1
    idx = torch.tensor([2, 0, 0, 2, 0, 2, 0])                           # image 1 without a question, unsorted
    img = torch.from_numpy(recipe.img_features(U, L, D, case["salt"])).double()
    q = torch.from_numpy(recipe.question_tokens(N, T, cfg.q_vocab_size, case["salt"]))
    soft = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, case["salt"])).double()
    sd = {k: v.double().requires_grad_(True) for k, v in recipe_sd(O.mfb_shapes(cfg, mhb=True), case["salt"]).items()}
    t = O.mhbcoatt_forward(sd, cfg, img[idx], q, return_all=True)
    t["P"].retain_grad()
    O.kldiv_loss(t["out"], soft).backward()
    dP = t["P"].grad                                                    # (N, L, 5000), per question
    dPu = torch.zeros((U, L, dP.shape[2]), dtype=torch.float64).index_add_(0, idx, dP)
    assert float(dPu[1].abs().max()) == 0.0
    dW = dPu.reshape(U * L, -1).t() @ img.reshape(U * L, D)
    g = sd["img_conv1d.weight"].grad.flatten(1)
    assert float(g.abs().max()) > 0.0
    assert float((dW - g).abs().max()) <= 1e-12 * float(g.abs().max())
    gb = sd["img_conv1d.bias"].grad
    assert float((dPu.sum((0, 1)) - gb).abs().max()) <= 1e-12 * float(gb.abs().max())
