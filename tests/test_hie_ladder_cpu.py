"""HieCoAttenLadder on the host: the parameter layout of the specification, properties of the fp64 restatement
(tests/hie_ladder_ref.py), and the refusal of CPU tensors (no CPU fallback)."""
import pytest
import torch

import hie_ladder_ref as R


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


def _sd(model, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.rand(v.shape, generator=g, dtype=dtype) - 0.5) * (0.4 if v.dim() > 1 else 0.2)
            for k, v in model.state_dict().items()}


def test_state_dict_keys_and_shapes(vqa):
    E, D, V, H, O = 16, 24, 50, 40, 30
    m = vqa.HieCoAttenLadder(block_num=7, word_num=5, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O)
    want = {
        "img_emb.weight": (E, D), "img_emb.bias": (E,),
        "word_emb.weight": (V, E),
        "phrase_uni.weight": (E, E, 1), "phrase_uni.bias": (E,),
        "phrase_bi.weight": (E, E, 2), "phrase_bi.bias": (E,),
        "phrase_tri.weight": (E, E, 3), "phrase_tri.bias": (E,),
        "sent_lstm.weight_ih_l0": (4 * E, E), "sent_lstm.weight_hh_l0": (4 * E, E),
        "sent_lstm.bias_ih_l0": (4 * E,), "sent_lstm.bias_hh_l0": (4 * E,),
        "ans_w.weight": (E, E), "ans_w.bias": (E,),
        "ans_p.weight": (E, 2 * E), "ans_p.bias": (E,),
        "ans_s.weight": (H, 2 * E), "ans_s.bias": (H,),
        "ans_h.weight": (O, H), "ans_h.bias": (O,),
    }
    for i in range(3):
        for n in ("Wb", "Wv", "Wq"):
            want["coatt.%d.%s.weight" % (i, n)] = (E, E)
        want["coatt.%d.whv.weight" % i] = (1, E)
        want["coatt.%d.whq.weight" % i] = (1, E)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert m.word_emb.padding_idx is None


def test_dropin_exports_the_ladder(vqa):
    import os
    path = os.path.join(os.path.dirname(vqa.__file__), "dropin", "hieCoAtten.py")
    src = open(path).read()
    assert "HieCoAttenLadder" in src
    assert vqa.HieCoAttenLadder.__name__ == "HieCoAttenLadder"


def test_permuting_regions_leaves_logits_unchanged(vqa):
    m = vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=8, hidden_size=10, output_size=6)
    sd = _sd(m)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(3, 9, 12, generator=g, dtype=torch.float64)
    ids = torch.randint(0, 20, (3, 5), generator=g)
    perm = torch.randperm(9, generator=g)
    a, av, aq = R.forward(sd, img, ids)
    b, bv, bq = R.forward(sd, img[:, perm], ids)
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    assert float((av[:, :, perm] - bv).abs().max()) <= 1e-12
    assert float((aq - bq).abs().max()) <= 1e-12


def test_phrase_level_at_one_word(vqa):
    m = vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=8, hidden_size=10, output_size=6)
    sd = _sd(m)
    x = torch.randn(4, 1, 8, dtype=torch.float64)
    got = R.phrase_level(x, sd)
    cands = [torch.tanh(x[:, 0] @ sd[n + ".weight"][:, :, 0].t() + sd[n + ".bias"]) for n in ("phrase_uni", "phrase_bi", "phrase_tri")]
    want = torch.stack(cands, 0).max(0).values
    assert float((got[:, 0] - want).abs().max()) <= 1e-15


def test_cpu_tensors_raise(vqa):
    m = vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=32, hidden_size=10, output_size=6)
    with pytest.raises(vqa.VqfError):
        m(torch.randn(2, 9, 12), torch.randint(0, 20, (2, 5)))
