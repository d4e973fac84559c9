"""HieCoAttenLadder with per-image region counts on the MI355X: forward((img, img_length), ids, q_length, img_index) against the
fp64 masked restatement (tests/hie_ladder_regions_ref.py, pinned on the CPU by tests/test_hie_ladder_regions_cpu.py), the exact
properties of the masking, the structure of the masked step (no host read of the counts, no extra launch) and its determinism.
Helpers and criteria as in tests/test_gpu_hie_ladder_lengths.py: rel_err <= 1e-4 on logits / av / aq, grad_parity with explicit
keep-masks.  Both co-attention modes, with and without q_length, with and without img_index; T = 22 takes the batched-GEMM route."""
import warnings

import pytest
import torch

import hie_ladder_regions_ref as RR
from golden_util import rel_err, grad_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 0
MODES = ("parallel", "alternating")
SHARED_IDX = [2, 0, 0, 2, 0, 2, 0]                      # U = 3, N = 7: image 1 without a question


def _shared_counts(L):
    """image 0: L - 1 regions, image 2: one; the image without a question carries L"""
    return torch.tensor([L - 1, L, 1], dtype=torch.int64)


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


def _model(vqa, L, E, D, coatt, V=40, H=48, O=30, seed=0, drop_p=0.5):
    torch.manual_seed(seed)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O, drop_p=drop_p,
                             coatt=coatt)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in m.parameters():                     # weights of a size that keeps every level's softmax away from one-hot
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    return m.to(DEV)


def _counts(U, L, seed=0):
    """always L - 1, 1, L and an odd value where U allows, then seeded values in [1, L]"""
    g = torch.Generator().manual_seed(seed + 11)
    base = [L - 1, 1, L, 7]
    extra = torch.randint(1, L + 1, (max(U - 4, 0),), generator=g).tolist()
    return torch.tensor((base + extra)[:U], dtype=torch.int64)


def _inputs(U, N, L, D, T, V=40, seed=0, counts=None):
    """img (U, L, D), right-padded ids (padding id 0), question lengths, region counts -- on the GPU"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(U, L, D, generator=g)
    ids = torch.randint(1, V, (N, T), generator=g)
    lens = torch.tensor(([min(2, T), 1, T] + torch.randint(1, T + 1, (max(N - 3, 0),), generator=g).tolist())[:N], dtype=torch.int64)
    ids = torch.where(torch.arange(T).unsqueeze(0) < lens.unsqueeze(1), ids, torch.full_like(ids, PAD))
    counts = _counts(U, L, seed) if counts is None else counts
    return img.to(DEV), ids.to(DEV), lens.to(DEV), counts.to(DEV)


def _masks(U, N, L, T, E, H, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=g) >= p).to(torch.uint8).to(DEV)
    return {"img": mk(U * L, E), "word": mk(N * T, E), "ans_w": mk(N, E), "ans_p": mk(N, 2 * E), "ans_s": mk(N, 2 * E),
            "ans_h": mk(N, H)}


def _sd_leaves(m, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}


def _loss_weights(logits, av, aq, seed=9):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(logits.shape, generator=g).to(DEV), torch.randn(av.shape, generator=g).to(DEV),
            torch.randn(aq.shape, generator=g).to(DEV))


def _call(m, img, ids, lens, counts, idx):
    feats = img if counts is None else (img, counts)
    if idx is not None:
        return m(feats, ids, lens, idx)
    return m(feats, ids, lens) if lens is not None else m(feats, ids)


def _step(m, img, ids, lens, counts, idx=None):
    """one forward + backward of a weighted sum of all three outputs -> (logits, av, aq, {name: grad})"""
    m.zero_grad()
    logits, av, aq = _call(m, img, ids, lens, counts, idx)
    wl, wv, wq = _loss_weights(logits, av, aq)
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    return logits.detach().clone(), av.detach().clone(), aq.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and set(a[3]) == set(b[3]) and \
        all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def _pad_regions(counts, L, idx=None):
    """(N, L) bool: the padded regions of every question's image"""
    pad = ~RR.region_mask(counts, L)
    return pad if idx is None else pad[idx]


# ---- eval forward, both routes (T <= 16 streaming, T > 16 batched GEMM) -----------------------------------------------------------
def _eval_case(vqa, U, N, T, L, E, D, idx):
    idx = None if idx is None else torch.tensor(idx, device=DEV)
    for coatt in MODES:
        m = _model(vqa, L, E, D, coatt).eval()
        img, ids, lens, counts = _inputs(U, N, L, D, T, counts=None if idx is None else _shared_counts(L))
        sd = {k: v.double() for k, v in m.state_dict().items()}
        pad = _pad_regions(counts, L, idx).unsqueeze(1).expand(N, 3, L)
        for ql in (None, lens):
            with torch.no_grad():
                logits, av, aq = _call(m, img, ids, ql, counts, idx)
                rl, rav, raq = RR.forward(sd, img.double(), ids, counts, ql, idx, coatt=coatt)
            assert logits.shape == (N, 30) and av.shape == (N, 3, L) and aq.shape == (N, 3, T)
            errs = [rel_err(a.cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
            print("eval %s U=%d N=%d T=%d L=%d E=%d counts=%s q_length=%s: rel_err logits %.2e av %.2e aq %.2e"
                  % (coatt, U, N, T, L, E, counts.tolist(), ql is not None, *errs))
            assert max(errs) <= 1e-4
            assert torch.equal(av[pad], torch.zeros_like(av[pad]))
            assert float((av.sum(2) - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [5, 14, 22])
@pytest.mark.parametrize("N", [1, 3, 5])
def test_model_eval_vs_fp64(vqa, N, T, L, E, D):
    _eval_case(vqa, N, N, T, L, E, D, None)


@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [14, 22])
def test_model_eval_shared_images_vs_fp64(vqa, T, L, E, D):
    _eval_case(vqa, 3, 7, T, L, E, D, SHARED_IDX)


# ---- train step with explicit keep-masks --------------------------------------------------------------------------------------------
def _train_parity(vqa, coatt, U, N, T, L, E, D, H, O, V, with_lens, idx=None, counts=None):
    idx = None if idx is None else torch.tensor(idx, device=DEV)
    m = _model(vqa, L, E, D, coatt, V=V, H=H, O=O).train()
    img, ids, lens, counts = _inputs(U, N, L, D, T, V=V, counts=counts)
    lens = lens if with_lens else None
    m.set_keep_masks(**_masks(U, N, L, T, E, H, 5))
    logits, av, aq = _call(m, img, ids, lens, counts, idx)
    wl, wv, wq = _loss_weights(logits, av, aq)
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    refs = {}
    for dt in (torch.float64, torch.float32):
        sd = _sd_leaves(m, dt)
        rm = {k: v.to(DEV) for k, v in m._seeds.keep.items()}
        rl, rav, raq = RR.forward(sd, img, ids, counts, lens, idx, masks=rm, p=m.drop_p, dtype=dt, coatt=coatt)
        ((rl * wl.to(dt)).sum() + (rav * wv.to(dt)).sum() + (raq * wq.to(dt)).sum()).backward()
        refs[dt] = (rl.detach(), rav.detach(), raq.detach(),
                    {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu() for k, v in sd.items()})
    rl, rav, raq, g64 = refs[torch.float64]
    errs = [rel_err(a.detach().cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
    print("train %s N=%d T=%d L=%d E=%d: rel_err logits %.2e av %.2e aq %.2e" % (coatt, N, T, L, E, *errs))
    assert max(errs) <= 1e-4
    gpu = {k: p.grad for k, p in m.named_parameters()}
    assert set(gpu) == set(g64)
    grad_parity(gpu, refs[torch.float32][3], g64,
                label="HieCoAttenLadder regions %s N=%d T=%d L=%d E=%d q_length=%s%s" % (coatt, N, T, L, E, with_lens,
                                                                                         "" if idx is None else " img_index"))


@pytest.mark.parametrize("with_lens", [False, True], ids=["no_q_length", "q_length"])
@pytest.mark.parametrize("coatt", MODES)
@pytest.mark.parametrize("T", [14, 22])
def test_model_train_masks_grads(vqa, T, coatt, with_lens):
    _train_parity(vqa, coatt, 5, 5, T, 50, 64, 96, 48, 30, 40, with_lens)


@pytest.mark.parametrize("coatt", MODES)
def test_model_train_masks_grads_shared_images(vqa, coatt):
    _train_parity(vqa, coatt, 3, 7, 14, 50, 64, 96, 48, 30, 40, True, idx=SHARED_IDX, counts=_shared_counts(50))


def test_model_full_size(vqa):
    """config 4's shapes: B = 256, L = 196, img 2048, E = 512, T = 14, 1000 answers; seeded counts in [10, 196]"""
    g = torch.Generator().manual_seed(23)
    _train_parity(vqa, "parallel", 256, 256, 14, 196, 512, 2048, 1024, 1000, 15881, True,
                  counts=torch.randint(10, 197, (256,), generator=g))


# ---- exact properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "img_index"])
@pytest.mark.parametrize("coatt", MODES)
@pytest.mark.parametrize("T,L,E,D", [(14, 50, 64, 96), (22, 50, 64, 96), (14, 196, 512, 256)])
def test_exact_properties(vqa, T, L, E, D, coatt, shared):
    U, N = (3, 7) if shared else (5, 5)
    idx = torch.tensor(SHARED_IDX, device=DEV) if shared else None
    m = _model(vqa, L, E, D, coatt).train()
    m.set_keep_masks(**_masks(U, N, L, T, E, 48, 5))
    img, ids, lens, counts = _inputs(U, N, L, D, T, counts=_shared_counts(L) if shared else None)
    a = _step(m, img, ids, lens, counts, idx)
    # av: zero on the padded regions, a distribution over the real ones (at most 196 fp32 terms, each a few ulp: 1e-5)
    pad = _pad_regions(counts, L, idx).unsqueeze(1).expand(N, 3, L)
    assert torch.equal(a[1][pad], torch.zeros_like(a[1][pad])) and float((a[1].sum(2) - 1).abs().max()) <= 1e-5
    # what the padded rows of img hold does not matter: outputs and ALL parameter gradients bit-identical
    g = torch.Generator().manual_seed(31)
    noise = (torch.randn(img.shape, generator=g) * 1e3).to(DEV)
    img2 = torch.where(RR.region_mask(counts, L).unsqueeze(2), img, noise)
    assert not torch.equal(img, img2)
    assert _same(a, _step(m, img2, ids, lens, counts, idx))
    assert float(a[3]["img_emb.weight"].abs().max()) > 0
    # counts 0 and L + 5 behave as 1 and L; int32 counts are taken as they are
    lo_hi = counts.clone()
    lo_hi[int((counts == 1).nonzero()[0])], lo_hi[int((counts == L).nonzero()[0])] = 0, L + 5
    assert _same(a, _step(m, img, ids, lens, lo_hi, idx))
    assert _same(a, _step(m, img, ids, lens, counts.to(torch.int32), idx))
    # and the model without counts on the same padded batch is a different function
    assert not torch.equal(a[0], _step(m, img, ids, lens, None, idx)[0])


@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "img_index"])
@pytest.mark.parametrize("coatt", MODES)
@pytest.mark.parametrize("T", [14, 22])
def test_full_counts_are_the_plain_call(vqa, T, coatt, shared):
    """counts all L, train mode, in-kernel Philox masks under one seed: results and gradients bit-identical to the plain tensor
    and to (img, None); two runs give equal bits"""
    U, N, L, E, D = (3, 7, 50, 64, 96) if shared else (4, 4, 50, 64, 96)
    idx = torch.tensor(SHARED_IDX, device=DEV) if shared else None
    m = _model(vqa, L, E, D, coatt).train()
    img, ids, lens, counts = _inputs(U, N, L, D, T, counts=_shared_counts(L) if shared else None)
    full = torch.full((U,), L, dtype=torch.int64, device=DEV)
    runs = []
    for c in (None, full, counts, counts):
        torch.manual_seed(77)
        runs.append(_step(m, img, ids, lens, c, idx))
    assert _same(runs[0], runs[1]) and _same(runs[2], runs[3]) and not torch.equal(runs[0][0], runs[2][0])
    torch.manual_seed(77)
    m.zero_grad()
    out = m((img, None), ids, lens, idx)
    assert all(torch.equal(x, y) for x, y in zip(out, runs[0][:3]))
    torch.manual_seed(78)
    assert not torch.equal(runs[2][0], _step(m, img, ids, lens, counts, idx)[0])        # (the seed does decide the masks)


def test_img_length_checks(vqa):
    N, T, L, E, D = 3, 5, 50, 64, 96
    m = _model(vqa, L, E, D, "parallel").eval()
    img, ids, lens, counts = _inputs(N, N, L, D, T)
    for bad in (counts[:2], counts.view(N, 1), counts.float(), counts.cpu(), counts.tolist()):
        with pytest.raises(vqa.VqfError, match="img_length"):
            m((img, bad), ids)
    for bad in ((img,), (img, counts, counts), [img]):
        with pytest.raises(vqa.VqfError, match="pair"):
            m(bad, ids)
    idx = torch.tensor([1, 1, 0], device=DEV)
    with pytest.raises(vqa.VqfError, match="img_length"):          # with img_index: one count per IMAGE
        m((img[:2], counts), ids, None, idx)
    ids_k, probs = vqa.predict(m, (img, counts), ids, lens, k=3)    # predict passes the pair through
    with torch.no_grad():
        ref = vqa.topk_answers(m((img, counts), ids, lens)[0], 3)
    assert torch.equal(ids_k, ref[0]) and torch.equal(probs, ref[1])


# ---- structure --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coatt", MODES)
def test_structure_full_size(vqa, monkeypatch, coatt):
    """config 4's shapes (the streaming route): the step with counts launches no more than the plain step, and no GPU tensor -- the
    counts and whatever is computed from them included -- is read on the host during its forward"""
    ops = vqa.ops
    N, T, L, E, D = 256, 14, 196, 512, 2048
    m = _model(vqa, L, E, D, coatt, V=15881, H=1024, O=1000).train()
    g = torch.Generator().manual_seed(23)
    img, ids, lens, counts = _inputs(N, N, L, D, T, V=15881, counts=torch.randint(10, 197, (N,), generator=g))

    def counted(c):
        _step(m, img, ids, lens, c)                          # warm-up (the library's first launches)
        torch.cuda.synchronize()
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            _step(m, img, ids, lens, c)
            torch.cuda.synchronize()
        finally:
            ops.prof_enable(False)
        return {k: v[0] for k, v in ops.prof_report().items()}

    plain, masked = counted(None), counted(counts)
    diff = {k: (plain.get(k), masked.get(k)) for k in set(plain) | set(masked) if plain.get(k) != masked.get(k)}
    assert sum(masked.values()) <= sum(plain.values()) and not diff, diff
    assert masked.get("zero_cols_len", 0) == 0

    def guard(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError("a GPU tensor was read on the host (Tensor.%s)" % name)
            return real(self, *a, **k)
        return f

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize during the forward with counts")

    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, guard(name))
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = m((img, counts), ids, lens)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]
