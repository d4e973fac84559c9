"""HieCoAttenLadder with question lengths on the MI355X: forward(img, ids, q_length) against the fp64 masked restatement
(tests/hie_ladder_len_ref.py, pinned on the CPU by tests/test_hie_ladder_lengths_cpu.py), the exact properties of the masking,
the structure of the masked step (no extra launch, no torch math, no host read of the lengths) and its determinism.
Criteria as in tests/test_gpu_hie_ladder.py: rel_err <= 1e-4 on logits / av / aq, grad_parity with explicit keep-masks."""
import warnings

import pytest
import torch

import hie_ladder_len_ref as RL
from golden_util import rel_err, grad_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 0


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


def _model(vqa, L, E, D, V=40, H=48, O=30, seed=0, drop_p=0.5):
    torch.manual_seed(seed)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O, drop_p=drop_p)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in m.parameters():                     # weights of a size that keeps every level's softmax away from one-hot
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    return m.to(DEV)


def _lengths(N, T, seed=0):
    """always 2, 1 and T (clipped to T) where N allows, then seeded values in [1, T]"""
    g = torch.Generator().manual_seed(seed + 7)
    base = [min(2, T), 1, T]
    extra = torch.randint(1, T + 1, (max(N - 3, 0),), generator=g).tolist()
    return torch.tensor((base + extra)[:N], dtype=torch.int64)


def _inputs(N, L, D, T, V=40, seed=0, lens=None):
    """img, right-padded ids (padding id 0, real words 1 .. V - 1), lengths -- on the GPU"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(N, L, D, generator=g)
    ids = torch.randint(1, V, (N, T), generator=g)
    lens = _lengths(N, T, seed) if lens is None else lens
    ids = torch.where(torch.arange(T).unsqueeze(0) < lens.clamp(1, T).unsqueeze(1), ids, torch.full_like(ids, PAD))
    return img.to(DEV), ids.to(DEV), lens.to(DEV)


def _masks(N, L, T, E, H, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=g) >= p).to(torch.uint8).to(DEV)
    return {"img": mk(N * L, E), "word": mk(N * T, E), "ans_w": mk(N, E), "ans_p": mk(N, 2 * E), "ans_s": mk(N, 2 * E),
            "ans_h": mk(N, H)}


def _sd_leaves(m, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}


def _loss_weights(logits, av, aq, seed=9):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(logits.shape, generator=g).to(DEV), torch.randn(av.shape, generator=g).to(DEV),
            torch.randn(aq.shape, generator=g).to(DEV))


def _step(m, img, ids, lens):
    """one forward + backward of a weighted sum of all three outputs -> (logits, av, aq, {name: grad})"""
    m.zero_grad()
    logits, av, aq = m(img, ids, lens) if lens is not None else m(img, ids)
    wl, wv, wq = _loss_weights(logits, av, aq)
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    return logits.detach().clone(), av.detach().clone(), aq.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and set(a[3]) == set(b[3]) and \
        all(torch.equal(a[3][k], b[3][k]) for k in a[3])


# ---- 3. eval forward, both routes (T <= 16 streaming, T > 16 batched GEMM) ------------------------------------------------------
@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [1, 5, 14, 22])
@pytest.mark.parametrize("N", [1, 3, 5])
def test_model_eval_vs_fp64(vqa, N, T, L, E, D):
    m = _model(vqa, L, E, D).eval()
    img, ids, lens = _inputs(N, L, D, T)
    with torch.no_grad():
        logits, av, aq = m(img, ids, lens)
        sd = {k: v.double() for k, v in m.state_dict().items()}
        rl, rav, raq = RL.forward(sd, img.double(), ids, lens)
    assert logits.shape == (N, 30) and av.shape == (N, 3, L) and aq.shape == (N, 3, T)
    errs = [rel_err(a.cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
    print("eval N=%d T=%d L=%d E=%d lens=%s: rel_err logits %.2e av %.2e aq %.2e" % (N, T, L, E, lens.tolist(), *errs))
    assert max(errs) <= 1e-4
    valid = RL.valid_mask(lens, T).unsqueeze(1).expand(N, 3, T)
    assert torch.equal(aq[~valid], torch.zeros_like(aq[~valid]))


# ---- 4. train step with explicit keep-masks ----------------------------------------------------------------------------------------
def _train_parity(vqa, N, T, L, E, D, H, O, V, lens=None):
    m = _model(vqa, L, E, D, V=V, H=H, O=O).train()
    img, ids, lens = _inputs(N, L, D, T, V=V, lens=lens)
    m.set_keep_masks(**_masks(N, L, T, E, H, 5))
    logits, av, aq = m(img, ids, lens)
    wl, wv, wq = _loss_weights(logits, av, aq)
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    refs = {}
    for dt in (torch.float64, torch.float32):
        sd = _sd_leaves(m, dt)
        rm = {k: v.to(DEV) for k, v in m._seeds.keep.items()}
        rl, rav, raq = RL.forward(sd, img, ids, lens, masks=rm, p=m.drop_p, dtype=dt)
        ((rl * wl.to(dt)).sum() + (rav * wv.to(dt)).sum() + (raq * wq.to(dt)).sum()).backward()
        refs[dt] = (rl.detach(), rav.detach(), raq.detach(),
                    {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu() for k, v in sd.items()})
    rl, rav, raq, g64 = refs[torch.float64]
    errs = [rel_err(a.detach().cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
    print("train N=%d T=%d L=%d E=%d: rel_err logits %.2e av %.2e aq %.2e" % (N, T, L, E, *errs))
    assert max(errs) <= 1e-4
    gpu = {k: p.grad for k, p in m.named_parameters()}
    assert set(gpu) == set(g64)
    grad_parity(gpu, refs[torch.float32][3], g64, label="HieCoAttenLadder lengths N=%d T=%d L=%d E=%d" % (N, T, L, E))
    assert torch.equal(gpu["word_emb.weight"][PAD], torch.zeros(E, device=DEV))      # id 0 occurs only as padding


@pytest.mark.parametrize("T", [14, 22])
def test_model_train_masks_grads(vqa, T):
    _train_parity(vqa, 5, T, 50, 64, 96, 48, 30, 40)


def test_model_full_size(vqa):
    """config 4's shapes: B = 256, L = 196, img 2048, E = 512, T = 14, 1000 answers; seeded lengths in [1, 14]"""
    g = torch.Generator().manual_seed(21)
    _train_parity(vqa, 256, 14, 196, 512, 2048, 1024, 1000, 15881, lens=torch.randint(1, 15, (256,), generator=g))


# ---- 5. exact properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L,E,D", [(14, 50, 64, 96), (22, 50, 64, 96), (14, 196, 512, 256)])
def test_exact_properties(vqa, T, L, E, D):
    N, V = 5, 40
    m = _model(vqa, L, E, D, V=V).train()
    m.set_keep_masks(**_masks(N, L, T, E, 48, 5))
    img, ids, lens = _inputs(N, L, D, T, V=V)
    a = _step(m, img, ids, lens)
    # aq: zero on the padding, a distribution over the real words (at most 22 fp32 terms, each a few ulp: 1e-5)
    valid = RL.valid_mask(lens, T).unsqueeze(1).expand(N, 3, T)
    aq = a[2]
    assert torch.equal(aq[~valid], torch.zeros_like(aq[~valid]))
    assert float((aq.sum(2) - 1).abs().max()) <= 1e-5
    # the padding ids do not matter: logits and ALL parameter gradients bit-identical
    ids2 = torch.where(RL.valid_mask(lens, T), ids, torch.full_like(ids, 17))
    assert not torch.equal(ids, ids2)
    assert _same(a, _step(m, img, ids2, lens))
    # id 0 occurs only as padding: its embedding row gets exactly no gradient (a real word's row does)
    assert torch.equal(a[3]["word_emb.weight"][PAD], torch.zeros(E, device=DEV))
    assert float(a[3]["word_emb.weight"][int(ids[0, 0])].abs().max()) > 0
    # lengths 0 and T + 5 behave as 1 and T
    lo_hi = lens.clone()
    i1, iT = int((lens == 1).nonzero()[0]), int((lens == T).nonzero()[0])
    lo_hi[i1], lo_hi[iT] = 0, T + 5
    assert _same(a, _step(m, img, ids, lo_hi))
    assert _same(a, _step(m, img, ids, lens.to(torch.int32)))          # int32 lengths are taken as they are
    # and the unmasked model on the same padded batch is a different function
    assert not torch.equal(a[0], _step(m, img, ids, None)[0])


@pytest.mark.parametrize("T", [14, 22])
def test_full_lengths_are_the_two_argument_model(vqa, T):
    """lengths all T, train mode, in-kernel Philox masks under one seed: results and gradients bit-identical to q_length=None"""
    N, L, E, D = 4, 50, 64, 96
    m = _model(vqa, L, E, D).train()
    img, ids, _ = _inputs(N, L, D, T)
    full = torch.full((N,), T, dtype=torch.int64, device=DEV)
    torch.manual_seed(77)
    a = _step(m, img, ids, None)
    torch.manual_seed(77)
    b = _step(m, img, ids, full)
    assert _same(a, b)
    torch.manual_seed(78)
    assert not torch.equal(a[0], _step(m, img, ids, None)[0])            # (the seed does decide the masks)


def test_q_length_checks(vqa):
    N, T, L, E, D = 3, 5, 50, 64, 96
    m = _model(vqa, L, E, D).eval()
    img, ids, lens = _inputs(N, L, D, T)
    for bad in (lens[:2], lens.view(N, 1), lens.float(), lens.cpu(), lens.tolist()):
        with pytest.raises(vqa.VqfError):
            m(img, ids, bad)


# ---- 6. structure -----------------------------------------------------------------------------------------------------------------
def test_structure_full_size(vqa, monkeypatch):
    """config 4's shapes: the masked step launches what the unmasked step launches, its forward calls no torch math on the big
    tensors, and the lengths are never read on the host"""
    ops = vqa.ops
    N, T, L, E, D = 256, 14, 196, 512, 2048
    m = _model(vqa, L, E, D, V=15881, H=1024, O=1000).train()
    g = torch.Generator().manual_seed(21)
    img, ids, lens = _inputs(N, L, D, T, V=15881, lens=torch.randint(1, 15, (N,), generator=g))

    def counted(q_len):
        _step(m, img, ids, q_len)                          # warm-up (the library's first launches)
        torch.cuda.synchronize()
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            _step(m, img, ids, q_len)
            torch.cuda.synchronize()
        finally:
            ops.prof_enable(False)
        return {k: v[0] for k, v in ops.prof_report().items()}

    plain, masked = counted(None), counted(lens)
    assert plain == masked, {k: (plain.get(k), masked.get(k)) for k in set(plain) | set(masked) if plain.get(k) != masked.get(k)}
    assert masked.get("hie_affinity_levels") == 1 and masked.get("phrase_ngram_fwd") == 1 and masked.get("phrase_ngram_bwd") == 1

    def boom(*a, **k):
        raise AssertionError("torch math on the ladder's hot path")

    def guard(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError("a GPU tensor was read on the host (Tensor.%s)" % name)
            return real(self, *a, **k)
        return f

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize during the masked forward")

    for mod, name in ((torch.nn.functional, "conv1d"), (torch, "bmm"), (torch, "matmul"), (torch, "softmax"), (torch, "where"),
                      (torch, "masked_fill"), (torch.Tensor, "masked_fill"), (torch.Tensor, "masked_fill_")):
        monkeypatch.setattr(mod, name, boom)
    # no GPU tensor -- the lengths and whatever is computed from them included -- is read on the host during the masked forward
    # (the dropout seeds come from the CPU generator, _DropSeeds.next: a CPU tensor's .item(), no GPU read, and stays)
    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, guard(name))
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = m(img, ids, lens)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------
def test_two_masked_steps_bit_identical(vqa):
    N, T, L, E, D = 5, 9, 50, 64, 96
    outs = []
    for _ in range(2):
        m = _model(vqa, L, E, D).train()
        img, ids, lens = _inputs(N, L, D, T)
        torch.manual_seed(1234)
        outs.append([_step(m, img, ids, lens) for _ in range(2)])
    for a, b in zip(*outs):
        assert _same(a, b)
    assert not torch.equal(outs[0][0][0], outs[0][1][0])                 # the two steps drew different dropout masks
