"""Question lengths of HieCoAttenLadder, the part that needs no GPU: (1) the masked restatement (tests/hie_ladder_len_ref.py)
is pinned to the unmasked one (tests/hie_ladder_ref.py) run sample by sample on the questions cut to their own lengths;
(2) the model's forward takes the reference training loop's third argument (solver.py:84-89, model.forward(i, q, q_l))."""
import inspect

import pytest
import torch

import hie_ladder_ref as R
import hie_ladder_len_ref as RL

N, T, L, D, E, H, O, V = 5, 9, 7, 12, 16, 10, 6, 23
LENGTHS = [9, 1, 2, 5, 3]
PAD = 0


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _sd(vqa, seed=0):
    m = vqa.HieCoAttenLadder(block_num=L, word_num=T, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O)
    g = torch.Generator().manual_seed(seed)
    return {k: ((torch.rand(v.shape, generator=g, dtype=torch.float64) * 2 - 1) * 0.6).requires_grad_(True)
            for k, v in m.state_dict().items()}


def _inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(N, L, D, generator=g, dtype=torch.float64)
    ids = torch.randint(1, V, (N, T), generator=g)
    lens = torch.tensor(LENGTHS)
    ids = torch.where(torch.arange(T).unsqueeze(0) < lens.unsqueeze(1), ids, torch.full_like(ids, PAD))   # right-padded with id 0
    return img, ids, lens


def _masks(seed=2, p=0.5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=g) >= p).to(torch.uint8)
    return {"img": mk(N * L, E), "word": mk(N * T, E), "ans_w": mk(N, E), "ans_p": mk(N, 2 * E), "ans_s": mk(N, 2 * E),
            "ans_h": mk(N, H)}


def _sample_masks(masks, n, ln):
    """the keep-masks of sample n alone, its question cut to ln words"""
    return {"img": masks["img"].view(N, L, E)[n].reshape(L, E), "word": masks["word"].view(N, T, E)[n, :ln].reshape(ln, E),
            "ans_w": masks["ans_w"][n:n + 1], "ans_p": masks["ans_p"][n:n + 1], "ans_s": masks["ans_s"][n:n + 1],
            "ans_h": masks["ans_h"][n:n + 1]}


def _weights(seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, O, generator=g, dtype=torch.float64), torch.randn(N, 3, L, generator=g, dtype=torch.float64),
            torch.randn(N, 3, T, generator=g, dtype=torch.float64))


def _grads(sd):
    out = {k: (torch.zeros_like(v) if v.grad is None else v.grad.clone()) for k, v in sd.items()}
    for v in sd.values():
        v.grad = None
    return out


@pytest.mark.parametrize("with_masks", [False, True])
def test_masked_restatement_is_the_truncated_unmasked_model(vqa, with_masks):
    """The defining property, fp64: the masked model on the padded batch equals, sample by sample, the unmasked model on that
    sample alone cut to its own length -- outputs and summed parameter gradients within 1e-12 (fp64 rounding of sums of a few
    hundred terms of size <= 1: ~1e-15 measured)."""
    sd = _sd(vqa)
    img, ids, lens = _inputs()
    masks = _masks() if with_masks else None
    wl, wv, wq = _weights()
    logits, av, aq = RL.forward(sd, img, ids, lens, masks=masks)
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    g_masked = _grads(sd)
    worst = 0.0
    for n, ln in enumerate(LENGTHS):
        sm = _sample_masks(masks, n, ln) if with_masks else None
        l1, av1, aq1 = R.forward(sd, img[n:n + 1], ids[n:n + 1, :ln], masks=sm)
        ((l1 * wl[n:n + 1]).sum() + (av1 * wv[n:n + 1]).sum() + (aq1 * wq[n:n + 1, :, :ln]).sum()).backward()   # grads accumulate
        for a, b in ((logits[n:n + 1], l1), (av[n:n + 1], av1), (aq[n:n + 1, :, :ln], aq1)):
            worst = max(worst, float((a - b).detach().abs().max()))
        assert torch.equal(aq[n, :, ln:].detach(), torch.zeros(3, T - ln, dtype=torch.float64))
        assert float((aq[n, :, :ln].detach().sum(1) - 1).abs().max()) <= 1e-12
    g_sum = _grads(sd)
    gworst = max(float((g_masked[k] - g_sum[k]).abs().max()) for k in sd)
    print("masked vs truncated: outputs %.2e, summed gradients %.2e" % (worst, gworst))
    assert worst <= 1e-12 and gworst <= 1e-12
    assert torch.equal(g_masked["word_emb.weight"][PAD], torch.zeros(E, dtype=torch.float64))   # id 0 occurs only as padding
    # and the unmasked model on the padded batch is a different function: the tests can tell the two apart
    with torch.no_grad():
        lu, _, _ = R.forward(sd, img, ids, masks=masks)
    assert float((lu - logits.detach()).abs().max()) > 1e-3


def test_padding_ids_do_not_matter_and_full_lengths_are_the_unmasked_model(vqa):
    sd = _sd(vqa)
    img, ids, lens = _inputs()
    masks = _masks()
    wl, wv, wq = _weights()

    def run(fn):
        logits, av, aq = fn()
        ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
        return logits.detach(), av.detach(), aq.detach(), _grads(sd)

    a = run(lambda: RL.forward(sd, img, ids, lens, masks=masks))
    ids2 = torch.where(torch.arange(T).unsqueeze(0) < lens.unsqueeze(1), ids, torch.full_like(ids, 7))   # other padding ids
    b = run(lambda: RL.forward(sd, img, ids2, lens, masks=masks))
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and all(torch.equal(a[3][k], b[3][k]) for k in sd)
    full = torch.full((N,), T)
    c = run(lambda: RL.forward(sd, img, ids, full, masks=masks))
    d = run(lambda: R.forward(sd, img, ids, masks=masks))
    assert all(torch.equal(x, y) for x, y in zip(c[:3], d[:3])) and all(torch.equal(c[3][k], d[3][k]) for k in sd)
    # lengths outside [1, T] are clamped
    e = run(lambda: RL.forward(sd, img, ids, torch.tensor([T + 5, 0, 2, 5, 3]), masks=masks))
    assert all(torch.equal(x, y) for x, y in zip(a[:3], e[:3])) and all(torch.equal(a[3][k], e[3][k]) for k in sd)


def test_forward_takes_the_training_loops_third_argument(vqa):
    """solver.py:84-89 calls model.forward(i, q, q_l) for every model that is not mhb*: the ladder accepts that form, and
    refuses CPU tensors with VqfError as the two-argument call does (no CPU fallback), not with TypeError."""
    sig = inspect.signature(vqa.HieCoAttenLadder.forward)
    names = list(sig.parameters)
    assert names[:4] == ["self", "img_features", "que_features", "q_length"]
    assert sig.parameters["q_length"].default is None
    m = vqa.HieCoAttenLadder(block_num=L, word_num=T, img_size=D, vocab_size=V, embed_size=32, hidden_size=H, output_size=O)
    img, ids, lens = _inputs()
    with pytest.raises(vqa.VqfError):
        m(img.float(), ids, lens)
    with pytest.raises(vqa.VqfError):
        m.forward(img.float(), ids, lens)
