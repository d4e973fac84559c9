"""HieCoAttenLadder(coatt="alternating") on the MI355X: the guided-logits kernels (csrc/hie_ladder_alt.hip) alone against fp64,
the model against its fp64 restatement (tests/hie_ladder_alt_ref.py, pinned on the CPU by tests/test_hie_ladder_alt_cpu.py) with
and without question lengths, the exact properties of the masking, the structure of the step and its determinism.
Criteria as in tests/test_gpu_hie_ladder.py: rel_err <= 1e-4 on logits / av / aq, grad_parity with explicit keep-masks; the
kernels at the values that file uses for the same kind of quantity (5e-6 where the fast tanh enters, 1e-5 for sums over rows)."""
import warnings

import pytest
import torch

import hie_ladder_alt_ref as RA
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


def _rand(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).to(dtype)


# ---- 1. the guided-logits kernels -----------------------------------------------------------------------------------------------
KERNEL_SHAPES = [(2, 1, 64), (300, 37, 96), (3, 14, 512), (2, 196, 1024), (256, 196, 512), (5, 1023, 32)]


@pytest.mark.parametrize("N,S,E", KERNEL_SHAPES)
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("guided", [True, False])
@pytest.mark.parametrize("wide", [False, True])
def test_guided_logits_kernels(vqa, N, S, E, G, guided, wide):
    """fwd and bwd against fp64 over EVERY element; wide: Xh and dXh are column blocks (offset 4) of buffers with ldx = G E + 8"""
    ops = vqa.ops
    M, GE = N * S, G * E
    assert ops.guided_logits_supported(N, S, E, G)
    xh = _rand((M, GE), 1 + S, 1.5)
    gp = _rand((N, GE), 2 + S, 1.0) if guided else None
    w = _rand((G, E), 3 + S, 0.2)
    dl = _rand((M, G), 4 + S, 1.0)
    if wide:
        buf = torch.full((M, GE + 8), 7.0, device=DEV)
        buf[:, 4:4 + GE] = xh.to(DEV)
        xd = buf[:, 4:4 + GE]
        obuf = torch.full((M, GE + 8), 7.0, device=DEV)
        out = obuf[:, 4:4 + GE]
    else:
        xd, out, obuf = xh.to(DEV), None, None
    gd = None if gp is None else gp.to(DEV)
    wd, dld = w.to(DEV), dl.to(DEV)
    logits = ops.guided_logits_fwd(xd, gd, wd, N, S)
    assert logits.shape == (M, G)
    pre = xh.double().view(N, S, G, E)
    if guided:
        pre = pre + gp.double().view(N, 1, G, E)
    H = torch.tanh(pre)                                                        # (N, S, G, E)
    want = (H * w.double().view(1, 1, G, E)).sum(3).view(M, G)
    e_l = rel_err(logits.cpu().numpy(), want.numpy())
    dxh, dgp, dw = ops.guided_logits_bwd(dld, xd, gd, wd, N, S, out=out)
    dref = dl.double().view(N, S, G, 1) * w.double().view(1, 1, G, E) * (1 - H * H)
    e_x = rel_err(dxh.cpu().numpy(), dref.view(M, GE).numpy())
    e_g = rel_err(dgp.cpu().numpy(), dref.sum(1).view(N, GE).numpy())
    e_w = rel_err(dw.cpu().numpy(), (dl.double().view(N, S, G, 1) * H).sum((0, 1)).numpy())
    print("guided N=%d S=%d E=%d G=%d guided=%d wide=%d: rel_err logits %.2e dXh %.2e dgp %.2e dw %.2e"
          % (N, S, E, G, guided, wide, e_l, e_x, e_g, e_w))
    assert e_l <= 5e-6 and e_x <= 5e-6
    assert e_g <= 1e-5 and e_w <= 1e-5
    if wide:                                                                   # nothing written outside the column block
        assert dxh.data_ptr() == out.data_ptr()
        assert torch.equal(obuf[:, :4], torch.full_like(obuf[:, :4], 7.0)) and torch.equal(obuf[:, 4 + GE:], torch.full_like(obuf[:, 4 + GE:], 7.0))
    # the sums run in a fixed order: a second call gives the same bits
    keep = (dxh.clone(), dgp.clone(), dw.clone())
    again = ops.guided_logits_bwd(dld, xd, gd, wd, N, S, out=out)
    assert all(torch.equal(a, b) for a, b in zip(keep, again))
    assert torch.equal(logits, ops.guided_logits_fwd(xd, gd, wd, N, S))


def test_guided_logits_zero_dlogit_rows(vqa):
    """a row whose dlogits are zero (a padded question position) gets an exact zero dXh row and adds nothing to dgp / dw"""
    ops = vqa.ops
    N, S, E = 4, 9, 64
    xh, gp, w = _rand((N * S, E), 1, 1.5).to(DEV), _rand((N, E), 2).to(DEV), _rand((1, E), 3, 0.2).to(DEV)
    dl = _rand((N * S, 1), 4).to(DEV)
    dl.view(N, S)[:, 5:] = 0
    dxh, dgp, dw = ops.guided_logits_bwd(dl, xh, gp, w, N, S)
    assert torch.equal(dxh.view(N, S, E)[:, 5:], torch.zeros(N, 4, E, device=DEV))
    xh2 = xh.clone()
    xh2.view(N, S, E)[:, 5:] = 3.0                                              # what those rows hold does not matter
    dxh2, dgp2, dw2 = ops.guided_logits_bwd(dl, xh2, gp, w, N, S)
    assert torch.equal(dxh, dxh2) and torch.equal(dgp, dgp2) and torch.equal(dw, dw2)


def test_guided_logits_refuses_unsupported(vqa):
    ops = vqa.ops
    z = lambda *s: torch.zeros(s, device=DEV)
    for N, S, E in ((2, 1025, 64), (2, 5, 48), (2, 5, 1056)):
        assert not ops.guided_logits_supported(N, S, E, 1)
        with pytest.raises(vqa.VqfError):
            ops.guided_logits_fwd(z(N * S, E), None, z(1, E), N, S)
    with pytest.raises(vqa.VqfError):
        ops.guided_logits_fwd(z(10, 64), z(3, 64), z(1, 64), 2, 5)              # gp of the wrong shape


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(vqa, L, E, D, V=40, H=48, O=30, seed=0, drop_p=0.5, **kw):
    kw.setdefault("coatt", "alternating")
    torch.manual_seed(seed)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O, drop_p=drop_p, **kw)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in m.parameters():                     # weights of a size that keeps every step's softmax away from one-hot
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    return m.to(DEV)


def _lengths(N, T, seed=0):
    """always 2, 1 and T (clipped to T) where N allows, then seeded values in [1, T]"""
    g = torch.Generator().manual_seed(seed + 7)
    base = [min(2, T), 1, T]
    extra = torch.randint(1, T + 1, (max(N - 3, 0),), generator=g).tolist()
    return torch.tensor((base + extra)[:N], dtype=torch.int64)


def _inputs(N, L, D, T, V=40, seed=0, masked=False, lens=None):
    """img, ids, lengths on the GPU; masked: right-padded ids (padding id 0, real words 1 .. V - 1), else lengths None"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(N, L, D, generator=g)
    ids = torch.randint(1, V, (N, T), generator=g)
    if not masked:
        return img.to(DEV), ids.to(DEV), None
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


def _eval_parity(vqa, N, T, L, E, D, masked, **kw):
    m = _model(vqa, L, E, D, **kw).eval()
    img, ids, lens = _inputs(N, L, D, T, V=kw.get("V", 40), masked=masked)
    with torch.no_grad():
        logits, av, aq = m(img, ids, lens)
        sd = {k: v.double() for k, v in m.state_dict().items()}
        rl, rav, raq = RA.forward(sd, img.double(), ids, lens)
    assert logits.shape == (N, kw.get("O", 30)) and av.shape == (N, 3, L) and aq.shape == (N, 3, T)
    errs = [rel_err(a.cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
    print("eval N=%d T=%d L=%d E=%d masked=%d: rel_err logits %.2e av %.2e aq %.2e" % (N, T, L, E, masked, *errs))
    assert max(errs) <= 1e-4
    if masked:
        valid = RL.valid_mask(lens, T).unsqueeze(1).expand(N, 3, T)
        assert torch.equal(aq[~valid], torch.zeros_like(aq[~valid]))


# ---- 2. eval forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [1, 5, 14, 22])
@pytest.mark.parametrize("N", [1, 3, 5])
def test_model_eval_vs_fp64(vqa, N, T, L, E, D, masked):
    _eval_parity(vqa, N, T, L, E, D, masked)


@pytest.mark.parametrize("masked", [False, True])
def test_model_eval_full_size(vqa, masked):
    """config 4's shapes: B = 256, L = 196, img 2048, E = 512, T = 14, 1000 answers"""
    _eval_parity(vqa, 256, 14, 196, 512, 2048, masked, V=15881, H=1024, O=1000)


# ---- 3. train step with explicit keep-masks -----------------------------------------------------------------------------------------
def _train_parity(vqa, N, T, L, E, D, H, O, V, masked):
    m = _model(vqa, L, E, D, V=V, H=H, O=O).train()
    img, ids, lens = _inputs(N, L, D, T, V=V, masked=masked)
    m.set_keep_masks(**_masks(N, L, T, E, H, 5))
    logits, av, aq = m(img, ids, lens)
    wl, wv, wq = _loss_weights(logits, av, aq)
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    refs = {}
    for dt in (torch.float64, torch.float32):
        sd = _sd_leaves(m, dt)
        rm = {k: v.to(DEV) for k, v in m._seeds.keep.items()}
        rl, rav, raq = RA.forward(sd, img, ids, lens, masks=rm, p=m.drop_p, dtype=dt)
        ((rl * wl.to(dt)).sum() + (rav * wv.to(dt)).sum() + (raq * wq.to(dt)).sum()).backward()
        refs[dt] = (rl.detach(), rav.detach(), raq.detach(),
                    {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu() for k, v in sd.items()})
    rl, rav, raq, g64 = refs[torch.float64]
    errs = [rel_err(a.detach().cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
    print("train N=%d T=%d L=%d E=%d masked=%d: rel_err logits %.2e av %.2e aq %.2e" % (N, T, L, E, masked, *errs))
    assert max(errs) <= 1e-4
    gpu = {k: p.grad for k, p in m.named_parameters()}
    assert set(gpu) == set(g64) and all(g is not None for g in gpu.values())
    grad_parity(gpu, refs[torch.float32][3], g64, label="HieCoAttenLadder alternating N=%d T=%d L=%d E=%d masked=%d" % (N, T, L, E, masked))
    if masked:
        assert torch.equal(gpu["word_emb.weight"][PAD], torch.zeros(E, device=DEV))      # id 0 occurs only as padding


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("T", [14, 22])
def test_model_train_masks_grads(vqa, T, masked):
    _train_parity(vqa, 5, T, 50, 64, 96, 48, 30, 40, masked)


@pytest.mark.parametrize("masked", [False, True])
def test_model_full_size(vqa, masked):
    """config 4's shapes: B = 256, L = 196, img 2048, E = 512, T = 14, 1000 answers; lengths 2, 1, 14, then seeded in [1, 14]"""
    _train_parity(vqa, 256, 14, 196, 512, 2048, 1024, 1000, 15881, masked)


# ---- 4. exact properties of the masking -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L,E,D", [(14, 50, 64, 96), (22, 50, 64, 96), (14, 196, 512, 256)])
def test_exact_properties(vqa, T, L, E, D):
    N, V = 5, 40
    m = _model(vqa, L, E, D, V=V).train()
    m.set_keep_masks(**_masks(N, L, T, E, 48, 5))
    img, ids, lens = _inputs(N, L, D, T, V=V, masked=True)
    a = _step(m, img, ids, lens)
    valid = RL.valid_mask(lens, T).unsqueeze(1).expand(N, 3, T)
    aq = a[2]
    assert torch.equal(aq[~valid], torch.zeros_like(aq[~valid]))
    assert float((aq.sum(2) - 1).abs().max()) <= 1e-5                      # (at most 22 fp32 terms, each a few ulp)
    # the padding ids do not matter: outputs and ALL parameter gradients bit-identical
    ids2 = torch.where(RL.valid_mask(lens, T), ids, torch.full_like(ids, 17))
    assert not torch.equal(ids, ids2)
    assert _same(a, _step(m, img, ids2, lens))
    # id 0 occurs only as padding: its embedding row gets exactly no gradient (a real word's row does)
    assert torch.equal(a[3]["word_emb.weight"][PAD], torch.zeros(E, device=DEV))
    assert float(a[3]["word_emb.weight"][int(ids[0, 0])].abs().max()) > 0
    # lengths 0 and T + 5 behave as 1 and T; int32 lengths are taken as they are
    lo_hi = lens.clone()
    i1, iT = int((lens == 1).nonzero()[0]), int((lens == T).nonzero()[0])
    lo_hi[i1], lo_hi[iT] = 0, T + 5
    assert _same(a, _step(m, img, ids, lo_hi))
    assert _same(a, _step(m, img, ids, lens.to(torch.int32)))
    # and the unmasked model on the same padded batch is a different function
    assert not torch.equal(a[0], _step(m, img, ids, None)[0])


@pytest.mark.parametrize("T,L,E,D", [(11, 50, 64, 96), (14, 196, 512, 256)])
def test_pad_width_and_ids_do_not_matter(vqa, T, L, E, D):
    """the same questions padded to T and to T + 3 words, with other padding ids: every sample's outputs bit-identical"""
    N, V = 5, 40
    m = _model(vqa, L, E, D, V=V).eval()
    img, ids, lens = _inputs(N, L, D, T, V=V, masked=True)
    wide = torch.cat([ids, torch.full((N, 3), 23, dtype=ids.dtype, device=DEV)], 1)
    wide = torch.where(RL.valid_mask(lens, T + 3), wide, torch.full_like(wide, 23))
    with torch.no_grad():
        l0, av0, aq0 = m(img, ids, lens)
        l1, av1, aq1 = m(img, wide, lens)
    assert torch.equal(l0, l1) and torch.equal(av0, av1)
    assert torch.equal(aq0, aq1[:, :, :T]) and torch.equal(aq1[:, :, T:], torch.zeros(N, 3, 3, device=DEV))


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


def test_argument_checks(vqa):
    N, T, L, E, D = 3, 5, 50, 64, 96
    m = _model(vqa, L, E, D).eval()
    img, ids, lens = _inputs(N, L, D, T, masked=True)
    for bad in (lens[:2], lens.view(N, 1), lens.float(), lens.cpu(), lens.tolist()):
        with pytest.raises(vqa.VqfError):
            m(img, ids, bad)
    with pytest.raises(vqa.VqfError):
        m(img.double(), ids)
    with pytest.raises(vqa.VqfError):
        m(img, ids.int())
    m2 = _model(vqa, L, 1056, D).eval()                                     # E > 1024: the guided-logits kernels say no
    with pytest.raises(vqa.VqfError, match="1024"):
        m2(img, ids)


# ---- 5. structure ---------------------------------------------------------------------------------------------------------------
def test_structure_full_size(vqa, monkeypatch):
    """config 4's shapes, one forward and backward under the library profiler: no affinity / rank-T launch, ONE guided-logits
    launch per direction over the image rows (G = 3) and one per level and step over the question rows; the masked step launches
    what the unmasked one does; the forward calls no torch math on the big tensors"""
    ops = vqa.ops
    N, T, L, E, D = 256, 14, 196, 512, 2048
    m = _model(vqa, L, E, D, V=15881, H=1024, O=1000).train()
    img, ids, lens = _inputs(N, L, D, T, V=15881, masked=True)
    calls = {"fwd": [], "bwd": []}
    real_f, real_b = ops.guided_logits_fwd, ops.guided_logits_bwd

    def fwd(xh, gp, w, N_, S_):
        calls["fwd"].append((N_, S_, w.shape[0]))
        return real_f(xh, gp, w, N_, S_)

    def bwd(dl, xh, gp, w, N_, S_, out=None):
        calls["bwd"].append((N_, S_, w.shape[0]))
        return real_b(dl, xh, gp, w, N_, S_, out=out)

    monkeypatch.setattr(ops, "guided_logits_fwd", fwd)
    monkeypatch.setattr(ops, "guided_logits_bwd", bwd)

    def counted(q_len):
        _step(m, img, ids, q_len)                          # warm-up (the library's first launches)
        torch.cuda.synchronize()
        calls["fwd"].clear()
        calls["bwd"].clear()
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            _step(m, img, ids, q_len)
            torch.cuda.synchronize()
        finally:
            ops.prof_enable(False)
        return {k: v[0] for k, v in ops.prof_report().items()}, {k: list(v) for k, v in calls.items()}

    (plain, pc), (masked, mc) = counted(None), counted(lens)
    assert plain == masked, {k: (plain.get(k), masked.get(k)) for k in set(plain) | set(masked) if plain.get(k) != masked.get(k)}
    assert pc == mc
    for name, cnt in masked.items():
        assert not (cnt and (name.startswith("hie_affinity") or name.startswith("hie_rank_") or name == "hie_hv_fwd")), (name, masked)
    assert masked.get("guided_logits_fwd") == 7 and masked.get("guided_logits_bwd") == 7, masked
    for d in ("fwd", "bwd"):
        assert [c for c in mc[d] if c[1] == L] == [(N, L, 3)], mc[d]
        assert sorted(c for c in mc[d] if c[1] != L) == [(N, T, 1)] * 6, mc[d]
    assert masked.get("att_logits_fwd", 0) == 0 and masked.get("phrase_ngram_fwd") == 1 and masked.get("phrase_ngram_bwd") == 1

    def boom(*a, **k):
        raise AssertionError("torch math on the ladder's hot path")

    for mod, name in ((torch.nn.functional, "conv1d"), (torch, "bmm"), (torch, "matmul"), (torch, "softmax"),
                      (torch, "where"), (torch, "masked_fill"), (torch.Tensor, "masked_fill"), (torch.Tensor, "masked_fill_")):
        monkeypatch.setattr(mod, name, boom)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = m(img, ids, lens)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]


# ---- 6. determinism, and the default mode ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_two_steps_bit_identical(vqa, masked):
    N, T, L, E, D = 5, 9, 50, 64, 96
    outs = []
    for _ in range(2):
        m = _model(vqa, L, E, D).train()
        img, ids, lens = _inputs(N, L, D, T, masked=masked)
        torch.manual_seed(1234)
        outs.append([_step(m, img, ids, lens) for _ in range(2)])
    for a, b in zip(*outs):
        assert _same(a, b)
    assert not torch.equal(outs[0][0][0], outs[0][1][0])                 # the two steps drew different dropout masks


@pytest.mark.parametrize("masked", [False, True])
def test_parallel_mode_is_the_default_model(vqa, masked):
    """coatt="parallel" spelt out and coatt left at its default: the same parameters from the same seed, the same bits"""
    N, T, L, E, D = 5, 14, 50, 64, 96
    res = []
    for kw in ({"coatt": "parallel"}, None):
        torch.manual_seed(0)
        if kw is None:
            m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=40, embed_size=E, hidden_size=48, output_size=30)
        else:
            m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=40, embed_size=E, hidden_size=48, output_size=30, **kw)
        m = m.to(DEV).train()
        assert m.coatt_mode == "parallel" and sorted(n for n, _ in m.coatt[0].named_parameters()) == \
            ["Wb.weight", "Wq.weight", "Wv.weight", "whq.weight", "whv.weight"]
        img, ids, lens = _inputs(N, L, D, T, masked=masked)
        torch.manual_seed(55)
        res.append(_step(m, img, ids, lens))
    assert _same(*res)
