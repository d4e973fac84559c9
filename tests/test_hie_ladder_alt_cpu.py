"""HieCoAttenLadder(coatt="alternating") on the host: the mode switch and its parameter layout, properties of the fp64
restatement (tests/hie_ladder_alt_ref.py, with and without question lengths), the guided-logits size queries, and the refusal
of CPU tensors (no CPU fallback)."""
import pytest
import torch

import hie_ladder_alt_ref as RA
import hie_ladder_len_ref as RL

PAD = 0


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _sd(model, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(v.shape, generator=g, dtype=dtype) - 0.5) * (0.4 if v.dim() > 1 else 0.2)
            for k, v in model.state_dict().items()}


def _small(vqa, **kw):
    return vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=8, hidden_size=10, output_size=6, coatt="alternating", **kw)


def test_alternating_constructs_with_its_state_dict(vqa):
    E, D, V, H, O = 16, 24, 50, 40, 30
    kw = dict(block_num=7, word_num=5, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O)
    m = vqa.HieCoAttenLadder(coatt="alternating", **kw)
    assert m.coatt_mode == "alternating"
    want = {}
    for i in range(3):
        for step in ("sum", "img", "que"):
            want["coatt.%d.%s_x.weight" % (i, step)] = (E, E)
            want["coatt.%d.%s_x.bias" % (i, step)] = (E,)
            want["coatt.%d.%s_h.weight" % (i, step)] = (1, E)
        for step in ("img", "que"):
            want["coatt.%d.%s_g.weight" % (i, step)] = (E, E)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert {k: v for k, v in got.items() if k.startswith("coatt.")} == want
    # everything outside the levels is the parallel model's, key for key
    par = vqa.HieCoAttenLadder(**kw)
    assert par.coatt_mode == "parallel" and vqa.HieCoAttenLadder(coatt="parallel", **kw).coatt_mode == "parallel"
    rest = {k: tuple(v.shape) for k, v in par.state_dict().items() if not k.startswith("coatt.")}
    assert {k: v for k, v in got.items() if not k.startswith("coatt.")} == rest and len(rest) == 21
    assert isinstance(m.coatt, torch.nn.ModuleList) and len(m.coatt) == 3


def test_default_mode_draws_the_same_initial_weights(vqa):
    kw = dict(img_size=12, vocab_size=20, embed_size=8, hidden_size=10, output_size=6)
    torch.manual_seed(3)
    a = vqa.HieCoAttenLadder(**kw).state_dict()
    torch.manual_seed(3)
    b = vqa.HieCoAttenLadder(coatt="parallel", **kw).state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("bad", ["", "Alternating", "both", None, 1])
def test_unknown_mode_raises(vqa, bad):
    with pytest.raises(ValueError):
        vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=8, hidden_size=10, output_size=6, coatt=bad)


def test_guided_logits_size_queries_need_no_gpu(vqa):
    lib = vqa.lib.load()
    for N, S, E in ((2, 1, 64), (300, 37, 96), (3, 14, 512), (2, 196, 1024), (256, 196, 512), (1, 1024, 32), (5, 1023, 1024)):
        for G in (1, 2, 3):
            assert lib.vqf_guided_logits_supported(N, S, E, G) == 1
            assert lib.vqf_guided_logits_bwd_ws_bytes(N, S, E, G) >= (2 * N + 32) * G * E * 4
    for N, S, E, G in ((2, 0, 64, 1), (2, 1025, 64, 1), (2, 5, 48, 1), (2, 5, 1056, 1), (2, 5, 64, 0), (2, 5, 64, 4), (0, 5, 64, 1)):
        assert lib.vqf_guided_logits_supported(N, S, E, G) == 0
    assert lib.vqf_guided_logits_bwd_ws_bytes(0, 5, 64, 1) == 0
    # one partial row of dgp and of dw per workgroup: 196 rows are four chunks of 49
    assert lib.vqf_guided_logits_bwd_ws_bytes(256, 196, 512, 3) == (2 * 256 * 4 + 32) * 3 * 512 * 4


def _case(vqa, N=4, L=9, T=6, seed=1):
    m = _small(vqa)
    sd = _sd(m)
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(N, L, 12, generator=g, dtype=torch.float64)
    ids = torch.randint(1, 20, (N, T), generator=g)
    return m, sd, img, ids, g


def test_permuting_regions_leaves_logits_unchanged(vqa):
    _, sd, img, ids, g = _case(vqa)
    perm = torch.randperm(9, generator=g)
    for lengths in (None, torch.tensor([2, 1, 6, 4])):
        a, av, aq = RA.forward(sd, img, ids, lengths)
        b, bv, bq = RA.forward(sd, img[:, perm], ids, lengths)
        assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
        assert float((av[:, :, perm] - bv).abs().max()) <= 1e-12
        assert float((aq - bq).abs().max()) <= 1e-12
        assert float((av.sum(2) - 1).abs().max()) <= 1e-12 and float((aq.sum(2) - 1).abs().max()) <= 1e-12


def test_the_levels_are_the_three_steps(vqa):
    """the restatement against the equations written out with plain loops for one sample and one level"""
    _, sd, img, ids, _ = _case(vqa, N=2)
    import hie_ladder_ref as R
    V = torch.tanh(img @ sd["img_emb.weight"].t() + sd["img_emb.bias"])
    Q = R.phrase_level(torch.tanh(sd["word_emb.weight"][ids]), sd)
    v, q, av, aq = RA.coattention(V, Q, sd, 1)
    W = lambda n: sd["coatt.1." + n]
    for n in range(2):
        ls = torch.stack([torch.tanh(W("sum_x.weight") @ Q[n, t] + W("sum_x.bias")) @ W("sum_h.weight")[0] for t in range(6)])
        s = (torch.softmax(ls, 0).unsqueeze(1) * Q[n]).sum(0)
        lv = torch.stack([torch.tanh(W("img_x.weight") @ V[n, l] + W("img_x.bias") + W("img_g.weight") @ s) @ W("img_h.weight")[0]
                          for l in range(9)])
        vv = (torch.softmax(lv, 0).unsqueeze(1) * V[n]).sum(0)
        lq = torch.stack([torch.tanh(W("que_x.weight") @ Q[n, t] + W("que_x.bias") + W("que_g.weight") @ vv) @ W("que_h.weight")[0]
                          for t in range(6)])
        qq = (torch.softmax(lq, 0).unsqueeze(1) * Q[n]).sum(0)
        assert float((av[n] - torch.softmax(lv, 0)).abs().max()) <= 1e-12 and float((aq[n] - torch.softmax(lq, 0)).abs().max()) <= 1e-12
        assert float((v[n] - vv).abs().max()) <= 1e-12 and float((q[n] - qq).abs().max()) <= 1e-12


def test_padded_batch_is_the_truncated_samples(vqa):
    N, T = 5, 7
    _, sd, img, ids, _ = _case(vqa, N=N, T=T, seed=2)
    lengths = torch.tensor([2, 1, T, 4, 6])
    valid = RL.valid_mask(lengths, T)
    ids = torch.where(valid, ids, torch.full_like(ids, PAD))
    logits, av, aq = RA.forward(sd, img, ids, lengths)
    for n in range(N):
        k = int(lengths[n])
        l1, av1, aq1 = RA.forward(sd, img[n:n + 1], ids[n:n + 1, :k])
        assert float((logits[n] - l1[0]).abs().max()) <= 1e-12 * float(l1.abs().max())
        assert float((av[n] - av1[0]).abs().max()) <= 1e-12
        assert float((aq[n, :, :k] - aq1[0]).abs().max()) <= 1e-12
    expand = valid.unsqueeze(1).expand(N, 3, T)
    assert torch.equal(aq[~expand], torch.zeros_like(aq[~expand]))            # exactly 0 on padding
    # other padding ids: the same values
    ids2 = torch.where(valid, ids, torch.full_like(ids, 17))
    l2, av2, aq2 = RA.forward(sd, img, ids2, lengths)
    assert torch.equal(logits, l2) and torch.equal(av, av2) and torch.equal(aq, aq2)


def test_padding_id_gets_no_gradient(vqa):
    N, T = 5, 7
    _, sd, img, ids, g = _case(vqa, N=N, T=T, seed=3)
    lengths = torch.tensor([2, 1, T, 4, 6])
    ids = torch.where(RL.valid_mask(lengths, T), ids, torch.full_like(ids, PAD))       # real words are 1 .. 19
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logits, av, aq = RA.forward(leaves, img, ids, lengths)
    wl, wv, wq = (torch.randn(t.shape, generator=g, dtype=torch.float64) for t in (logits, av, aq))
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    gw = leaves["word_emb.weight"].grad
    assert torch.equal(gw[PAD], torch.zeros_like(gw[PAD]))
    assert float(gw[int(ids[0, 0])].abs().max()) > 0
    assert all(v.grad is not None and float(v.grad.abs().max()) > 0 for v in leaves.values())     # every weight takes part


def test_full_lengths_are_the_unmasked_spec(vqa):
    N, T = 4, 6
    _, sd, img, ids, _ = _case(vqa, N=N, T=T)
    a = RA.forward(sd, img, ids)
    for full in (torch.full((N,), T), torch.full((N,), T + 3)):
        b = RA.forward(sd, img, ids, full)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = RA.forward(sd, img, ids, torch.tensor([T, T, 2, T]))
    assert not torch.equal(a[0], c[0])


def test_cpu_tensors_raise(vqa):
    m = vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=32, hidden_size=10, output_size=6, coatt="alternating")
    with pytest.raises(vqa.VqfError):
        m(torch.randn(2, 9, 12), torch.randint(0, 20, (2, 5)))
    with pytest.raises(vqa.VqfError):
        m(torch.randn(2, 9, 12), torch.randint(0, 20, (2, 5)), torch.tensor([5, 2]))
    with pytest.raises(vqa.VqfError):
        vqa.ops.guided_logits_fwd(torch.zeros(6, 32), None, torch.zeros(1, 32), 2, 3)
    with pytest.raises(vqa.VqfError):
        vqa.ops.guided_logits_bwd(torch.zeros(6, 1), torch.zeros(6, 32), None, torch.zeros(1, 32), 2, 3)
