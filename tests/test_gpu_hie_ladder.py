"""HieCoAttenLadder on the MI355X: the new kernels (csrc/hie_ladder.hip, the G = 3 pooling / logit launches) against fp64,
the model against its fp64 restatement (tests/hie_ladder_ref.py), its structure and its determinism."""
import warnings

import pytest
import torch

import hie_ladder_ref as R
from golden_util import rel_err, grad_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


def _rand(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).to(dtype)


# ---- 1. phrase kernels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,E", [(3, 14, 512), (2, 1, 64), (5, 16, 96), (4, 22, 512), (256, 14, 512)])
def test_phrase_ngram_kernels(vqa, N, T, E):
    ops = vqa.ops
    Z = _rand((N * T, 6 * E), 1 + T, 1.5)
    b = _rand((3 * E,), 2 + T, 0.5)
    qp, idx = ops.phrase_ngram_fwd(Z.to(DEV), b.to(DEV), N, T)
    Zd, bd = Z.double().view(N, T, 6 * E), b.double()
    u = []
    for k in (1, 2, 3):
        acc = bd[(k - 1) * E:k * E].expand(N, T, E).clone()
        for j in range(k):
            blk = Zd[:, :, (k * (k - 1) // 2 + j) * E:(k * (k - 1) // 2 + j + 1) * E]
            acc[:, :T - j] += blk[:, j:]
        u.append(acc)
    u = torch.stack(u, 0)                                                # (3, N, T, E)
    want = torch.tanh(u.max(0).values).view(N * T, E)
    assert rel_err(qp.cpu().numpy(), want.numpy()) <= 1e-6
    top2 = u.sort(0, descending=True).values
    clear = (top2[0] - top2[1] > 1e-5).view(N * T, E)
    assert torch.equal(idx.cpu().long()[clear], u.argmax(0).view(N * T, E)[clear])
    # backward, given the kernel's own Qp and winners
    dq = _rand((N * T, E), 3 + T)
    dZ = ops.phrase_ngram_bwd(dq.to(DEV), qp, idx, N, T)
    du = (dq.double() * (1 - qp.cpu().double() ** 2)).view(N, T, E)
    win = idx.cpu().long().view(N, T, E)
    ref = torch.zeros(N, T, 6 * E, dtype=torch.float64)
    for k in (1, 2, 3):
        for j in range(k):
            c0 = (k * (k - 1) // 2 + j) * E
            ref[:, j:, c0:c0 + E] = torch.where(win[:, :T - j] == k - 1, du[:, :T - j], torch.zeros(()).double())
    assert rel_err(dZ.cpu().numpy(), ref.view(N * T, 6 * E).numpy()) <= 1e-6
    db = ops.colsum(dZ).cpu().double()
    dbr = ref.view(N * T, 6 * E).sum(0)
    for c0 in (0, E, 3 * E):
        assert rel_err(db[c0:c0 + E].numpy(), dbr[c0:c0 + E].numpy()) <= 2e-5


# ---- 2. multi-level affinity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,E,T", [(3, 50, 64, 14), (2, 196, 512, 14), (300, 37, 96, 5)])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_hie_affinity_levels(vqa, N, L, E, T, G, shared, epi):
    ops = vqa.ops
    for pairs in (1, 2):
        if not ops.hie_affinity_levels_supported(N, L, E, T, G, pairs):
            assert E == 512 and G == 3 and pairs == 2                 # the one shape the LDS cannot hold
            continue
        x = _rand((N * T, 2 * G * E), 10 + pairs, 0.5).to(DEV)        # level g's X at column offset g * 2E
        y = _rand((N * L, G * E), 20 + pairs, 0.5).to(DEV)            # level g's Y at g * E (or all at 0)
        x2 = _rand((N * T, G * E), 30, 0.5).to(DEV) if pairs == 2 else None
        y2 = _rand((N * L, G * E + 4), 40, 0.5).to(DEV) if pairs == 2 else None
        yprev = _rand((G, N, T, L), 50, 0.9).to(DEV) if epi == 2 else None
        lvy = 0 if shared else E
        out = ops.hie_affinity_levels(x, 2 * E, y, lvy, G, N, L, T, E, x2=x2, lvx2=E, y2=y2, lvy2=lvy, epi=epi, yprev=yprev)
        xd, yd = x.cpu().double(), y.cpu().double()
        for g in range(G):
            X = xd[:, 2 * g * E:2 * g * E + E].view(N, T, E)
            Y = yd[:, g * lvy:g * lvy + E].view(N, L, E)
            s = torch.bmm(X, Y.transpose(1, 2))
            if pairs == 2:
                X2 = x2.cpu().double()[:, g * E:(g + 1) * E].view(N, T, E)
                Y2 = y2.cpu().double()[:, g * lvy:g * lvy + E].view(N, L, E)
                s = s + torch.bmm(X2, Y2.transpose(1, 2))
            if epi == 1:
                s = torch.tanh(s)
            elif epi == 2:
                s = s * (1 - yprev.cpu().double()[g] ** 2)
            # (epi 1: the streaming passes' exp / rcp tanh, a few 1e-6 absolute, as in vqf_hie_affinity)
            assert rel_err(out[g].cpu().numpy(), s.numpy()) <= (5e-6 if epi == 1 else 2e-6), (g, pairs)
        if G == 1:                                                    # the same k order as vqf_hie_affinity: the same bits
            one = ops.hie_affinity(x[:, :E], y[:, :E], N, L, T, x2=None if x2 is None else x2[:, :E],
                                   y2=None if y2 is None else y2[:, :E], epi=epi, yprev=yprev)
            assert torch.equal(one.view(-1), out.view(-1))


def test_affinity_dynamic_lds_grows(vqa):
    """vqf_hie_affinity at E = 1024: one pair needs 64.25 KB of dynamic LDS, two pairs 128.5 KB.  The attribute set for the
    first launch must be raised for the second (common.h vqf_set_dyn_lds keeps the largest size per device)."""
    ops = vqa.ops
    N, L, E, T = 2, 40, 1024, 6
    x = _rand((N * T, E), 61, 0.3).to(DEV)
    y = _rand((N * L, E), 62, 0.3).to(DEV)
    x2 = _rand((N * T, E), 63, 0.3).to(DEV)
    y2 = _rand((N * L, E), 64, 0.3).to(DEV)
    one = ops.hie_affinity(x, y, N, L, T, epi=0)
    two = ops.hie_affinity(x, y, N, L, T, x2=x2, y2=y2, epi=0)
    torch.cuda.synchronize()
    xd, yd, x2d, y2d = (t.cpu().double().view(N, -1, E) for t in (x, y, x2, y2))
    r1 = torch.bmm(xd, yd.transpose(1, 2))
    r2 = r1 + torch.bmm(x2d, y2d.transpose(1, 2))
    assert rel_err(one.cpu().numpy(), r1.numpy()) <= 2e-6
    assert rel_err(two.cpu().numpy(), r2.numpy()) <= 2e-6


# ---- 3. G = 3 pooling and logits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,S,C", [(3, 196, 512), (256, 196, 512), (2, 14, 64)])
def test_glimpse_pool_and_logits_g3(vqa, N, S, C):
    ops = vqa.ops
    feat = _rand((N, S, C), 71, 1.0).to(DEV)
    hid = _rand((N * S, 3 * C), 72, 1.0).to(DEV)
    w = torch.zeros(3, 3 * C)
    for g in range(3):
        w[g, g * C:(g + 1) * C] = _rand((C,), 73 + g, 0.1)
    w = w.to(DEV)
    b = torch.zeros(3, device=DEV)
    logits = ops.att_logits_fwd(hid, w, b)
    ld = hid.cpu().double() @ w.cpu().double().t()
    assert rel_err(logits.cpu().numpy(), ld.numpy()) <= 1e-6
    wts, pooled = ops.glimpse_pool_fwd(feat, logits, False)
    sm = torch.softmax(logits.cpu().double().view(N, S, 3).transpose(1, 2), 2)          # (N, 3, S)
    pr = torch.bmm(sm, feat.cpu().double()).reshape(N, 3 * C)
    assert rel_err(wts.cpu().numpy(), sm.numpy()) <= 1e-6
    assert rel_err(pooled.cpu().numpy(), pr.numpy()) <= 1e-6
    # backward of the pool (with a gradient through the weights) and of the logits
    dp = _rand((N, 3 * C), 74).to(DEV)
    dw_extra = _rand((N, 3, S), 75).to(DEV)
    dl, dfeat = ops.glimpse_pool_bwd(dp, feat, wts, False, True, dwts=dw_extra)
    smd = wts.cpu().double()
    dwt = torch.bmm(dp.cpu().double().view(N, 3, C), feat.cpu().double().transpose(1, 2)) + dw_extra.cpu().double()
    dlr = smd * (dwt - (smd * dwt).sum(2, keepdim=True))                                 # (N, 3, S)
    dfr = torch.bmm(smd.transpose(1, 2), dp.cpu().double().view(N, 3, C))
    assert rel_err(dl.cpu().numpy(), dlr.transpose(1, 2).reshape(N * S, 3).numpy()) <= 1e-5
    assert rel_err(dfeat.cpu().numpy(), dfr.numpy()) <= 1e-6
    dhid, dw, db, _ = ops.att_logits_bwd(dl, hid, w, relu_mask=False)
    dld = dl.cpu().double()
    assert rel_err(dhid.cpu().numpy(), (dld @ w.cpu().double()).numpy()) <= 1e-6
    assert rel_err(dw.cpu().numpy(), (dld.t() @ hid.cpu().double()).numpy()) <= 1e-5
    # (a softmax gradient sums to zero over a sample: db is a sum of cancelling terms, bounded by their magnitude)
    assert float((db.cpu().double() - dld.sum(0)).abs().max()) <= 1e-6 * float(dld.abs().sum(0).max())


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _model(vqa, L, E, D, V=40, H=48, O=30, seed=0, drop_p=0.5):
    torch.manual_seed(seed)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O, drop_p=drop_p)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in m.parameters():                     # weights of a size that keeps every level's softmax away from one-hot
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    return m.to(DEV)


def _inputs(N, L, D, T, V=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, L, D, generator=g).to(DEV), torch.randint(0, V, (N, T), generator=g).to(DEV)


def _sd_leaves(m, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [1, 5, 14, 22])
@pytest.mark.parametrize("N", [1, 3, 5])
def test_model_eval_vs_fp64(vqa, N, T, L, E, D):
    m = _model(vqa, L, E, D).eval()
    img, ids = _inputs(N, L, D, T)
    with torch.no_grad():
        logits, av, aq = m(img, ids)
        sd = {k: v.double() for k, v in m.state_dict().items()}
        rl, rav, raq = R.forward(sd, img.double(), ids)
    assert logits.shape == (N, 30) and av.shape == (N, 3, L) and aq.shape == (N, 3, T)
    assert rel_err(logits.cpu().numpy(), rl.cpu().numpy()) <= 1e-4
    assert rel_err(av.cpu().numpy(), rav.cpu().numpy()) <= 1e-4
    assert rel_err(aq.cpu().numpy(), raq.cpu().numpy()) <= 1e-4


def _masks(N, L, T, E, H, seed, p=0.5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=g) >= p).to(torch.uint8).to(DEV)
    return {"img": mk(N * L, E), "word": mk(N * T, E), "ans_w": mk(N, E), "ans_p": mk(N, 2 * E), "ans_s": mk(N, 2 * E),
            "ans_h": mk(N, H)}


def _train_parity(vqa, N, T, L, E, D, H, O, V, masks):
    m = _model(vqa, L, E, D, V=V, H=H, O=O).train()
    img, ids = _inputs(N, L, D, T, V=V)
    if masks:
        m.set_keep_masks(**_masks(N, L, T, E, H, 5))
    logits, av, aq = m(img, ids)
    g = torch.Generator().manual_seed(9)
    wl = torch.randn(logits.shape, generator=g).to(DEV)
    wv = torch.randn(av.shape, generator=g).to(DEV)
    wq = torch.randn(aq.shape, generator=g).to(DEV)
    loss = (logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()
    loss.backward()
    refs = {}
    for dt in (torch.float64, torch.float32):
        sd = _sd_leaves(m, dt)
        rm = {k: v.to(DEV) for k, v in m._seeds.keep.items()} if masks else None
        rl, rav, raq = R.forward(sd, img, ids, masks=rm, p=m.drop_p, dtype=dt)
        rloss = (rl * wl.to(dt)).sum() + (rav * wv.to(dt)).sum() + (raq * wq.to(dt)).sum()
        rloss.backward()
        refs[dt] = (rl.detach(), rav.detach(), raq.detach(), {k: v.grad.detach().cpu() for k, v in sd.items()})
    rl, rav, raq, g64 = refs[torch.float64]
    assert rel_err(logits.detach().cpu().numpy(), rl.cpu().numpy()) <= 1e-4
    assert rel_err(av.detach().cpu().numpy(), rav.cpu().numpy()) <= 1e-4
    assert rel_err(aq.detach().cpu().numpy(), raq.cpu().numpy()) <= 1e-4
    gpu = {k: p.grad for k, p in m.named_parameters()}
    assert set(gpu) == set(g64)
    grad_parity(gpu, refs[torch.float32][3], g64, label="HieCoAttenLadder N=%d T=%d L=%d E=%d" % (N, T, L, E))


@pytest.mark.parametrize("T", [14, 22])
def test_model_train_masks_grads(vqa, T):
    _train_parity(vqa, 3, T, 50, 64, 96, 48, 30, 40, masks=True)


def test_model_full_size(vqa):
    """config 4's shapes: B = 256, L = 196, img 2048, E = 512, T = 14, 1000 answers"""
    _train_parity(vqa, 256, 14, 196, 512, 2048, 1024, 1000, 15881, masks=True)


# ---- 7. structure ------------------------------------------------------------------------------------------------------------
def test_structure_full_size_forward(vqa, monkeypatch):
    ops = vqa.ops
    N, T, L, E, D = 256, 14, 196, 512, 2048
    m = _model(vqa, L, E, D, V=15881, H=1024, O=1000).train()
    img, ids = _inputs(N, L, D, T, V=15881)
    m(img, ids)                                            # warm-up (the library's first launches)
    torch.cuda.synchronize()
    pools = []
    real_pool = ops.glimpse_pool_fwd

    def pool(feat, logits, unit, pooled_out=None):
        pools.append((tuple(feat.shape), logits.shape[1]))
        return real_pool(feat, logits, unit, pooled_out=pooled_out)

    def boom(*a, **k):
        raise AssertionError("torch math on the ladder's hot path")

    monkeypatch.setattr(ops, "glimpse_pool_fwd", pool)
    for mod, name in ((torch.nn.functional, "conv1d"), (torch, "bmm"), (torch, "matmul"), (torch, "softmax")):
        monkeypatch.setattr(mod, name, boom)
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            m(img, ids)
            torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    rep = ops.prof_report()
    assert rep.get("hie_affinity_levels", (0, 0))[0] == 1, rep
    assert rep.get("hie_affinity", (0, 0))[0] == 0, rep
    assert [p for p in pools if p[1] == 3] == [((N, L, E), 3)], pools
    assert rep.get("phrase_ngram_fwd", (0, 0))[0] == 1, rep
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]


# ---- 8. determinism ----------------------------------------------------------------------------------------------------------
def test_two_steps_bit_identical(vqa):
    N, T, L, E, D = 4, 9, 50, 64, 96
    outs = []
    for _ in range(2):
        m = _model(vqa, L, E, D).train()
        img, ids = _inputs(N, L, D, T)
        torch.manual_seed(1234)
        res = []
        for step in range(2):
            m.zero_grad()
            logits, av, aq = m(img, ids)
            (logits.square().sum() + av.sum() * 0.5 + aq.square().sum()).backward()
            res.append((logits.detach().clone(), [p.grad.clone() for p in m.parameters()]))
        outs.append(res)
    for (la, ga), (lb, gb) in zip(*outs):
        assert torch.equal(la, lb)
        assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    assert not torch.equal(outs[0][0][0], outs[0][1][0])                 # the two steps drew different dropout masks
