"""Shared images of HieCoAttenLadder (forward(..., img_index)), the part that needs no GPU: the grouping helper on CPU tensors,
the fp64 specification (tests/hie_ladder_shared_ref.py) against the references it is built from, the size queries of the
grouped entry points, and the forward's signature.  Out-of-range indices are exercised here only."""
import inspect

import pytest
import torch

import hie_ladder_ref as R
import hie_ladder_len_ref as RL
import hie_ladder_alt_ref as RA
import hie_ladder_shared_ref as RS

L, D, E, H, O, V, T = 7, 12, 16, 10, 6, 23, 6


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


@pytest.fixture(scope="module")
def group_index(vqa):
    import importlib
    return importlib.import_module(vqa.__name__ + ".host.hie_ladder")._group_index


# ---- _group_index ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_group_index_unsorted_with_empty_and_large_groups(group_index, dtype):
    #                    n: 0  1  2  3  4  5  6  7  8
    idx = torch.tensor([3, 0, 3, 3, 0, 3, 4, 3, 3], dtype=dtype)            # image 1 and 2 empty, image 3 with six questions
    i32, order, off = group_index(idx, 5)
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.device == idx.device for t in (i32, order, off))
    assert i32.tolist() == [3, 0, 3, 3, 0, 3, 4, 3, 3]
    assert order.tolist() == [1, 4, 0, 2, 3, 5, 7, 8, 6]                     # stable: ascending n inside an image
    assert off.tolist() == [0, 2, 2, 2, 8, 9]


def test_group_index_clamps_and_ignores_the_integer_type(group_index):
    raw = [7, -1, 2, 0, 3, -500, 2, 1 << 20]
    U = 3
    a = group_index(torch.tensor(raw, dtype=torch.int64), U)
    b = group_index(torch.tensor(raw, dtype=torch.int32), U)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a[0].tolist() == [2, 0, 2, 0, 2, 0, 2, 2]                          # below 0 -> 0, at or above U -> U - 1
    assert a[1].tolist() == [1, 3, 5, 0, 2, 4, 6, 7] and a[2].tolist() == [0, 3, 3, 8]
    # every shape the model accepts: N < U, N > U, U = 1, one question
    for n, u in ((2, 6), (9, 2), (5, 1), (1, 1)):
        g = torch.Generator().manual_seed(n * 10 + u)
        idx = torch.randint(0, u, (n,), generator=g)
        i32, order, off = group_index(idx, u)
        assert off.shape == (u + 1,) and int(off[0]) == 0 and int(off[-1]) == n and bool((off[1:] >= off[:-1]).all())
        assert sorted(order.tolist()) == list(range(n))
        for k in range(u):
            members = order[int(off[k]):int(off[k + 1])].tolist()
            assert members == [j for j in range(n) if int(idx[j]) == k]


# ---- the specification ----------------------------------------------------------------------------------------------------------
def _sd(vqa, coatt, seed=0):
    m = vqa.HieCoAttenLadder(block_num=L, word_num=T, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O, coatt=coatt)
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * 0.6 for k, v in m.state_dict().items()}


def _case(U, N, seed=1):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(U, L, D, generator=g, dtype=torch.float64)
    ids = torch.randint(1, V, (N, T), generator=g)
    lens = torch.randint(1, T + 1, (N,), generator=g)
    ids = torch.where(RL.valid_mask(lens, T), ids, torch.zeros_like(ids))
    masks = {"img": (torch.rand(U * L, E, generator=g) >= 0.5).to(torch.uint8),
             "word": (torch.rand(N * T, E, generator=g) >= 0.5).to(torch.uint8),
             "ans_w": (torch.rand(N, E, generator=g) >= 0.5).to(torch.uint8)}
    return img, ids, lens, masks, g


def _under(coatt, sd, img, ids, lens, masks):
    if coatt == "alternating":
        return RA.forward(sd, img, ids, lens, masks=masks)
    return R.forward(sd, img, ids, masks=masks) if lens is None else RL.forward(sd, img, ids, lens, masks=masks)


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("coatt", ["parallel", "alternating"])
def test_identity_index_is_the_underlying_reference(vqa, coatt, with_lens):
    N = 4
    sd = _sd(vqa, coatt)
    img, ids, lens, masks, _ = _case(N, N)
    lens = lens if with_lens else None
    a = RS.forward(sd, img, ids, torch.arange(N), lens, masks=masks, coatt=coatt)
    b = _under(coatt, sd, img, ids, lens, masks)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("coatt", ["parallel", "alternating"])
def test_permuting_questions_and_index_permutes_the_outputs(vqa, coatt):
    U, N = 3, 7
    sd = _sd(vqa, coatt)
    img, ids, lens, masks, g = _case(U, N)
    idx = torch.tensor([2, 0, 2, 0, 0, 2, 0])                                # image 1 without a question
    perm = torch.randperm(N, generator=g)
    a = RS.forward(sd, img, ids, idx, lens, coatt=coatt)
    b = RS.forward(sd, img, ids[perm], idx[perm], lens[perm], coatt=coatt)
    for x, y in zip(a, b):
        assert float((x[perm] - y).abs().max()) <= 1e-12 * max(1.0, float(x.abs().max()))
    # out-of-range values are the clamped ones, int32 is int64
    wild = torch.tensor([9, -4, 2, 0, -1, 1 << 20, 0], dtype=torch.int32)
    c = RS.forward(sd, img, ids, wild, lens, coatt=coatt)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


@pytest.mark.parametrize("coatt", ["parallel", "alternating"])
def test_img_emb_gradient_is_the_expanded_models(vqa, coatt):
    """the shared call's gradients (index_select's backward sums each image's questions) are those of the expanded batch run
    through the underlying reference; an image without a question adds nothing"""
    U, N = 3, 6
    img, ids, lens, masks, g = _case(U, N, seed=4)
    idx = torch.tensor([2, 2, 0, 2, 0, 2])
    grads = []
    for shared in (True, False):
        sd = {k: v.clone().requires_grad_(True) for k, v in _sd(vqa, coatt).items()}
        if shared:
            out = RS.forward(sd, img, ids, idx, lens, masks=masks, coatt=coatt)
        else:
            out = _under(coatt, sd, img[idx], ids, lens, RS.expand_masks(masks, idx, U))
        gg = torch.Generator().manual_seed(11)
        sum((o * torch.randn(o.shape, generator=gg, dtype=torch.float64)).sum() for o in out).backward()
        grads.append({k: v.grad for k, v in sd.items()})
    assert float(grads[0]["img_emb.weight"].abs().max()) > 0
    for k in grads[0]:
        assert float((grads[0][k] - grads[1][k]).abs().max()) <= 1e-12 * max(1.0, float(grads[1][k].abs().max())), k


# ---- the library's queries and the signature --------------------------------------------------------------------------------------
def test_grouped_size_queries_need_no_gpu(vqa):
    lib = vqa.lib.load()
    for N, U, S, E_ in ((7, 3, 5, 32), (6, 1, 37, 96), (256, 64, 196, 512), (2, 65535, 14, 1024), (65535, 1, 1, 32)):
        for G in (1, 2, 3):
            assert lib.vqf_guided_logits_grouped_supported(N, U, S, E_, G) == 1
            assert lib.vqf_glimpse_pool_grouped_supported(N, U, S, E_, G) == 1
            assert lib.vqf_guided_logits_bwd_grouped_ws_bytes(N, U, S, E_, G) >= (N + U + 32) * G * E_ * 4
    for N, U, S, E_, G in ((7, 0, 5, 32, 3), (7, 65536, 5, 32, 3), (65536, 3, 5, 32, 3), (7, 3, 1025, 32, 3), (7, 3, 5, 48, 3),
                           (7, 3, 5, 32, 4)):
        assert lib.vqf_guided_logits_grouped_supported(N, U, S, E_, G) == 0
    assert lib.vqf_glimpse_pool_grouped_supported(7, 65536, 5, 32, 3) == 0 and lib.vqf_glimpse_pool_grouped_supported(7, 3, 5, 30, 3) == 0
    assert lib.vqf_guided_logits_bwd_grouped_ws_bytes(7, 0, 5, 32, 3) == 0
    # one partial row of dgp per question and chunk, one of dw per image and chunk: 196 rows are four chunks of 49
    assert lib.vqf_guided_logits_bwd_grouped_ws_bytes(256, 64, 196, 512, 3) == ((256 + 64) * 4 + 32) * 3 * 512 * 4
    assert lib.vqf_row_block_supported(7, 3, 5 * 32) == 1 and lib.vqf_row_block_supported(7, 3, 6) == 0
    assert lib.vqf_row_block_supported(7, 65536, 32) == 0 and lib.vqf_row_block_supported(0, 3, 32) == 0


def test_forward_takes_img_index_and_refuses_cpu_tensors(vqa):
    m = vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=32, hidden_size=10, output_size=6)
    names = list(inspect.signature(m.forward).parameters)
    assert names == ["img_features", "que_features", "q_length", "img_index"]
    assert inspect.signature(m.forward).parameters["img_index"].default is None
    with pytest.raises(vqa.VqfError):
        m(torch.randn(2, 9, 12), torch.randint(0, 20, (3, 5)), None, torch.tensor([0, 1, 1]))
    with pytest.raises(vqa.VqfError):
        vqa.ops.row_block_gather(torch.zeros(2, 8), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(vqa.VqfError):
        vqa.ops.guided_logits_fwd_grouped(torch.zeros(6, 32), torch.zeros(3, 32), torch.zeros(1, 32), torch.zeros(3, dtype=torch.int32),
                                          3, 2, 3)
    assert "img_index" in vqa.predict.__doc__
