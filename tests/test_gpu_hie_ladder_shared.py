"""HieCoAttenLadder.forward(..., img_index) on the MI355X: U images shared by N questions.  (1) each grouped kernel alone against
fp64 over every element (guided logits fwd / bwd, glimpse pooling fwd / bwd, the row-block gather and its grouped sum), with the
exact properties of the grouped sums: equal bits on a second run, exact zeros for an image without a question, untouched margins
where the kernel takes a pitch; (2) the model in both coatt modes against its fp64 specification (tests/hie_ladder_shared_ref.py,
pinned on the CPU by tests/test_hie_ladder_shared_cpu.py) and against the existing path called on img[idx].
Criteria are those of tests/test_gpu_hie_ladder_alt.py: 5e-6 where the fast tanh enters, 1e-5 for sums over rows, rel_err <= 1e-4
on logits / av / aq, grad_parity with explicit keep-masks.  Indices here are always in range (out-of-range values: the CPU file)."""
import pytest
import torch

import hie_ladder_len_ref as RL
import hie_ladder_shared_ref as RS
from golden_util import rel_err, grad_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 0
K = 4          # questions of a group per pass in the grouped kernels (GL_GRP_Q, csrc/hie_ladder_alt.hip; GP_Q, csrc/attention.hip)


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def group_index(vqa):
    import importlib
    return importlib.import_module(vqa.__name__ + ".host.hie_ladder")._group_index


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


def _index(U, N, kind):
    if kind == "4/0/3":
        return torch.tensor([2, 0, 0, 2, 0, 2, 0])                             # unsorted; image 1 without a question
    if kind == "one":
        return torch.zeros(N, dtype=torch.int64)
    if kind == "reversed":
        return torch.arange(N - 1, -1, -1)
    if kind == "big":                                                           # image 1: 2 K + 1 questions (two full passes and a tail)
        return torch.tensor([1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1])
    return torch.randint(0, U, (N,), generator=torch.Generator().manual_seed(U * 100 + N))


# (U, N, L, E, index): groups of 4 / 0 / 3; every question on one image; the identity reversed; a group of 2 K + 1 > K; one larger
SHAPES = [(3, 7, 5, 32, "4/0/3"), (1, 6, 37, 96, "one"), (5, 5, 196, 64, "reversed"), (2, 2 * K + 3, 14, 512, "big"),
          (8, 40, 196, 512, "random")]
_IDS = ["%dx%dx%dx%d" % s[:4] for s in SHAPES]


def _groups(group_index, U, N, kind):
    idx = _index(U, N, kind)
    assert idx.shape == (N,) and int(idx.min()) >= 0 and int(idx.max()) < U
    i32, order, off = group_index(idx.to(DEV), U)
    empty = [u for u in range(U) if int((idx == u).sum()) == 0]
    return idx, i32, order, off, empty


@pytest.mark.parametrize("U,N,L,E,kind", SHAPES, ids=_IDS)
@pytest.mark.parametrize("wide", [False, True])
def test_guided_logits_grouped(vqa, group_index, U, N, L, E, kind, wide):
    """G = 3 (the model's use): fwd and bwd against fp64 over every element; wide: Xh and dXh are column blocks (offset 4) of
    buffers with a pitch of 3 E + 8"""
    ops, G = vqa.ops, 3
    GE = G * E
    idx, i32, order, off, empty = _groups(group_index, U, N, kind)
    if kind == "big":
        assert int((idx == 1).sum()) == 2 * K + 1 > K
    assert ops.guided_logits_grouped_supported(N, U, L, E, G)
    xh, gp, w, dl = _rand((U * L, GE), 1 + L, 1.5), _rand((N, GE), 2 + L), _rand((G, E), 3 + L, 0.2), _rand((N * L, G), 4 + L)
    if wide:
        buf = torch.full((U * L, GE + 8), 7.0, device=DEV)
        buf[:, 4:4 + GE] = xh.to(DEV)
        xd = buf[:, 4:4 + GE]
        obuf = torch.full((U * L, GE + 8), 7.0, device=DEV)
        out = obuf[:, 4:4 + GE]
    else:
        xd, out, obuf = xh.to(DEV), None, None
    gd, wd, dld = gp.to(DEV), w.to(DEV), dl.to(DEV)
    logits = ops.guided_logits_fwd_grouped(xd, gd, wd, i32, N, U, L)
    assert logits.shape == (N * L, G)
    H = torch.tanh(xh.double().view(U, L, G, E)[idx] + gp.double().view(N, 1, G, E))           # (N, L, G, E)
    want = (H * w.double().view(1, 1, G, E)).sum(3).view(N * L, G)
    e_l = rel_err(logits.cpu().numpy(), want.numpy())
    dxh, dgp, dw = ops.guided_logits_bwd_grouped(dld, xd, gd, wd, order, off, N, U, L, out=out)
    per_q = dl.double().view(N, L, G, 1) * w.double().view(1, 1, G, E) * (1 - H * H)           # (N, L, G, E)
    dxr = torch.zeros(U, L, G, E, dtype=torch.float64).index_add_(0, idx, per_q)
    e_x = rel_err(dxh.cpu().numpy(), dxr.view(U * L, GE).numpy())
    e_g = rel_err(dgp.cpu().numpy(), per_q.sum(1).view(N, GE).numpy())
    e_w = rel_err(dw.cpu().numpy(), (dl.double().view(N, L, G, 1) * H).sum((0, 1)).numpy())
    print("guided grouped U=%d N=%d L=%d E=%d wide=%d: rel_err logits %.2e dXh %.2e dgp %.2e dw %.2e" % (U, N, L, E, wide, e_l, e_x, e_g, e_w))
    assert e_l <= 5e-6 and e_x <= 5e-6
    assert e_g <= 1e-5 and e_w <= 1e-5
    for u in empty:                                                             # an image without a question: exact zero rows
        assert torch.equal(dxh.view(U, L, GE)[u], torch.zeros(L, GE, device=DEV))
    if wide:                                                                    # nothing written outside the column block
        assert dxh.data_ptr() == out.data_ptr()
        assert torch.equal(obuf[:, :4], torch.full_like(obuf[:, :4], 7.0)) and torch.equal(obuf[:, 4 + GE:], torch.full_like(obuf[:, 4 + GE:], 7.0))
    keep = (dxh.clone(), dgp.clone(), dw.clone())                               # fixed summation order: the same bits again
    again = ops.guided_logits_bwd_grouped(dld, xd, gd, wd, order, off, N, U, L, out=out)
    assert all(torch.equal(a, b) for a, b in zip(keep, again))
    assert torch.equal(logits, ops.guided_logits_fwd_grouped(xd, gd, wd, i32, N, U, L))


def test_guided_logits_grouped_identity_is_the_plain_kernel(vqa, group_index):
    """idx = arange(N): the forward gives the plain kernel's bits, the backward its values (one question per image)"""
    ops = vqa.ops
    N, L, E, G = 5, 37, 96, 3
    i32, order, off = group_index(torch.arange(N, device=DEV), N)
    xh, gp, w, dl = (_rand(s, i, sc).to(DEV) for i, (s, sc) in enumerate((((N * L, G * E), 1.5), ((N, G * E), 1.0), ((G, E), 0.2), ((N * L, G), 1.0))))
    assert torch.equal(ops.guided_logits_fwd_grouped(xh, gp, w, i32, N, N, L), ops.guided_logits_fwd(xh, gp, w, N, L))
    a = ops.guided_logits_bwd_grouped(dl, xh, gp, w, order, off, N, N, L)
    b = ops.guided_logits_bwd(dl, xh, gp, w, N, L)
    assert torch.equal(a[0], b[0])                                              # dXh: the same expression per element
    assert rel_err(a[1].cpu().numpy(), b[1].cpu().numpy()) <= 1e-5 and rel_err(a[2].cpu().numpy(), b[2].cpu().numpy()) <= 1e-5


@pytest.mark.parametrize("U,N,L,E,kind", SHAPES, ids=_IDS)
def test_glimpse_pool_grouped(vqa, group_index, U, N, L, E, kind):
    """G = 3: wts, pooled, dlogits and dfeat against fp64 over every element (sums over rows: 1e-5), with a gradient arriving
    through the returned weights as in the model"""
    ops, G = vqa.ops, 3
    idx, i32, order, off, empty = _groups(group_index, U, N, kind)
    assert ops.glimpse_pool_grouped_supported(N, U, L, E, G)
    feat, lg = _rand((U, L, E), 11 + L), _rand((N * L, G), 12 + L, 2.0)
    dp, dwx = _rand((N, G * E), 13 + L), _rand((N, G, L), 14 + L)
    fd, lgd, dpd, dwd = feat.to(DEV), lg.to(DEV), dp.to(DEV), dwx.to(DEV)
    wts, pooled = ops.glimpse_pool_fwd_grouped(fd, lgd, i32)
    assert wts.shape == (N, G, L) and pooled.shape == (N, G * E)
    f64 = feat.double().requires_grad_(True)
    l64 = lg.double().requires_grad_(True)
    a64 = torch.softmax(l64.view(N, L, G).transpose(1, 2), 2)                                   # (N, G, L)
    p64 = torch.matmul(a64, f64[idx]).reshape(N, G * E)
    ((p64 * dp.double()).sum() + (a64 * dwx.double()).sum()).backward()
    e_w, e_p = rel_err(wts.cpu().numpy(), a64.detach().numpy()), rel_err(pooled.cpu().numpy(), p64.detach().numpy())
    dlg, dfeat = ops.glimpse_pool_bwd_grouped(dpd, fd, wts, i32, order, off, True, dwts=dwd)
    assert dlg.shape == (N * L, G) and dfeat.shape == (U, L, E)
    e_l, e_f = rel_err(dlg.cpu().numpy(), l64.grad.numpy()), rel_err(dfeat.cpu().numpy(), f64.grad.numpy())
    print("pool grouped U=%d N=%d L=%d E=%d: rel_err wts %.2e pooled %.2e dlogits %.2e dfeat %.2e" % (U, N, L, E, e_w, e_p, e_l, e_f))
    assert max(e_w, e_p, e_l, e_f) <= 1e-5
    for u in empty:
        assert torch.equal(dfeat[u], torch.zeros(L, E, device=DEV))
    again = ops.glimpse_pool_bwd_grouped(dpd, fd, wts, i32, order, off, True, dwts=dwd)
    assert torch.equal(dlg, again[0]) and torch.equal(dfeat, again[1])
    w2, p2 = ops.glimpse_pool_fwd_grouped(fd, lgd, i32)
    assert torch.equal(wts, w2) and torch.equal(pooled, p2)
    # the per-question half is the plain kernel on the expanded tensor: the same bits
    w3, p3 = ops.glimpse_pool_fwd(fd[idx.to(DEV)].contiguous(), lgd, False)
    assert torch.equal(wts, w3) and torch.equal(pooled, p3)


@pytest.mark.parametrize("U,N,L,E,kind", SHAPES, ids=_IDS)
def test_row_block_gather_and_group_sum(vqa, group_index, U, N, L, E, kind):
    ops = vqa.ops
    idx, i32, order, off, empty = _groups(group_index, U, N, kind)
    v, dv = _rand((U, L, E), 21 + L), _rand((N, L, E), 22 + L)
    vd, dvd = v.to(DEV), dv.to(DEV)
    out = ops.row_block_gather(vd, i32)
    assert torch.equal(out, vd.index_select(0, idx.to(DEV)))                    # a copy: bit-exact
    back = ops.row_block_group_sum(dvd, order, off)
    want = torch.zeros(U, L, E, dtype=torch.float64).index_add_(0, idx, dv.double())
    e = rel_err(back.cpu().numpy(), want.numpy())
    print("group sum U=%d N=%d L=%d E=%d: rel_err %.2e" % (U, N, L, E, e))
    assert back.shape == (U, L, E) and e <= 1e-5
    for u in empty:
        assert torch.equal(back[u], torch.zeros(L, E, device=DEV))
    assert torch.equal(back, ops.row_block_group_sum(dvd, order, off))


def test_grouped_ops_refuse_bad_operands(vqa, group_index):
    ops = vqa.ops
    z = lambda *s: torch.zeros(s, device=DEV)
    i32, order, off = group_index(torch.tensor([1, 0, 1], device=DEV), 2)
    for bad in (i32.long(), i32[:2], i32.cpu()):
        with pytest.raises(vqa.VqfError):
            ops.guided_logits_fwd_grouped(z(10, 96), z(3, 96), z(3, 32), bad, 3, 2, 5)
    # the gather takes N from idx itself, so a shorter idx is a valid call; a wrong type, rank, layout or device is not
    assert ops.row_block_gather(z(2, 8), i32[:2]).shape == (2, 8)
    for bad in (i32.long(), i32.view(1, 3), torch.stack([i32, i32], 1)[:, 0], i32.cpu(), [1, 0, 1]):
        with pytest.raises(vqa.VqfError):
            ops.row_block_gather(z(2, 8), bad)
    with pytest.raises(vqa.VqfError):
        ops.row_block_group_sum(z(3, 8), order[:2], off)                        # here N comes from src: order must be (N,)
    with pytest.raises(vqa.VqfError):
        ops.guided_logits_fwd_grouped(z(10, 96), None, z(3, 32), i32, 3, 2, 5)  # the grouped step always has guidance rows
    with pytest.raises(vqa.VqfError):
        ops.guided_logits_bwd_grouped(z(15, 3), z(10, 96), z(3, 96), z(3, 32), order, off[:2], 3, 2, 5)
    with pytest.raises(vqa.VqfError):
        ops.row_block_gather(z(2, 6), i32)                                      # a block that is no multiple of 4 floats
    assert not ops.guided_logits_grouped_supported(3, 65536, 5, 32, 3)


# ---- the model ------------------------------------------------------------------------------------------------------------------
MODES = ["parallel", "alternating"]
U_, N_, T_, L_, E_, D_, H_, O_, V_ = 3, 7, 9, 50, 64, 96, 48, 30, 40
IDX = [2, 0, 0, 2, 0, 2, 0]                                                     # unsorted; image 1 without a question


def _model(vqa, coatt, L=L_, E=E_, D=D_, seed=0, drop_p=0.5):
    torch.manual_seed(seed)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=V_, embed_size=E, hidden_size=H_, output_size=O_, drop_p=drop_p, coatt=coatt)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in m.parameters():                     # weights of a size that keeps every step's softmax away from one-hot
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    return m.to(DEV)


def _inputs(masked, U=U_, N=N_, L=L_, D=D_, T=T_, seed=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(U, L, D, generator=g)
    ids = torch.randint(1, V_, (N, T), generator=g)
    if not masked:
        return img.to(DEV), ids.to(DEV), None
    lens = torch.tensor(([min(2, T), 1, T] + torch.randint(1, T + 1, (max(N - 3, 0),), generator=g).tolist())[:N])
    ids = torch.where(RL.valid_mask(lens, T), ids, torch.full_like(ids, PAD))
    return img.to(DEV), ids.to(DEV), lens.to(DEV)


def _masks(U, N, L, T, E, seed=5, p=0.5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(s, generator=g) >= p).to(torch.uint8).to(DEV)
    return {"img": mk(U * L, E), "word": mk(N * T, E), "ans_w": mk(N, E), "ans_p": mk(N, 2 * E), "ans_s": mk(N, 2 * E), "ans_h": mk(N, H_)}


def _loss_weights(outs, seed=9):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g).to(DEV) for o in outs]


def _step(m, img, ids, lens, idx):
    m.zero_grad()
    outs = m(img, ids, lens, img_index=idx)
    sum((o * w).sum() for o, w in zip(outs, _loss_weights(outs))).backward()
    return [o.detach().clone() for o in outs] + [{k: p.grad.clone() for k, p in m.named_parameters()}]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and set(a[3]) == set(b[3]) and all(torch.equal(a[3][k], b[3][k]) for k in a[3])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("coatt", MODES)
def test_model_train_step(vqa, coatt, masked):
    """train mode, drop_p = 0.5, explicit keep-masks (one 'img' mask per image): outputs against fp64, every parameter gradient
    by grad_parity; the existing path on img[idx] with the expanded mask meets the same criteria and agrees with the grouped call;
    the masking's exact properties hold; a second identical step gives the same bits"""
    m = _model(vqa, coatt).train()
    img, ids, lens = _inputs(masked)
    idx = torch.tensor(IDX, device=DEV)
    masks = _masks(U_, N_, L_, T_, E_)
    m.set_keep_masks(**masks)
    a = _step(m, img, ids, lens, idx)
    assert a[0].shape == (N_, O_) and a[1].shape == (N_, 3, L_) and a[2].shape == (N_, 3, T_)
    wl = _loss_weights(a[:3])
    refs = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in m.state_dict().items()}
        outs = RS.forward(sd, img, ids, idx, lens, masks=masks, p=m.drop_p, dtype=dt, coatt=coatt)
        sum((o * w.to(dt)).sum() for o, w in zip(outs, wl)).backward()
        refs[dt] = ([o.detach() for o in outs], {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu() for k, v in sd.items()})
    r64, g64 = refs[torch.float64]
    errs = [rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:3], r64)]
    print("shared train %s masked=%d: rel_err logits %.2e av %.2e aq %.2e" % (coatt, masked, *errs))
    assert max(errs) <= 1e-4
    assert set(a[3]) == set(g64)
    grad_parity(a[3], refs[torch.float32][1], g64, label="HieCoAttenLadder %s img_index masked=%d" % (coatt, masked))
    # the existing path on the expanded batch
    m.set_keep_masks(**RS.expand_masks(masks, idx, U_))
    b = _step(m, img[idx].contiguous(), ids, lens, None)
    errs_b = [rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(b[:3], r64)]
    assert max(errs_b) <= 1e-4
    assert max(rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:3], b[:3])) <= 1e-4
    grad_parity(b[3], refs[torch.float32][1], g64, label="HieCoAttenLadder %s expanded masked=%d" % (coatt, masked))
    if masked:
        assert torch.equal(a[3]["word_emb.weight"][PAD], torch.zeros(E_, device=DEV))     # id 0 occurs only as padding
        assert float(a[3]["word_emb.weight"][int(ids[0, 0])].abs().max()) > 0
        pad = ~RL.valid_mask(lens, T_).unsqueeze(1).expand(N_, 3, T_)
        assert torch.equal(a[2][pad], torch.zeros_like(a[2][pad]))                        # aq exactly zero on padding
    # determinism, the integer type, and img_index=None
    m.set_keep_masks(**masks)
    assert _same(a, _step(m, img, ids, lens, idx))
    assert _same(a, _step(m, img, ids, lens, idx.to(torch.int32)))


@pytest.mark.parametrize("coatt", MODES)
def test_no_index_is_the_existing_model(vqa, coatt):
    """img_index=None with (N, L, D) images: the call without the argument, bit for bit (explicit masks)"""
    m = _model(vqa, coatt).train()
    img, ids, lens = _inputs(True, U=N_)
    m.set_keep_masks(**_masks(N_, N_, L_, T_, E_))
    m.zero_grad()
    outs = m(img, ids, lens)
    sum((o * w).sum() for o, w in zip(outs, _loss_weights(outs))).backward()
    a = [o.detach().clone() for o in outs] + [{k: p.grad.clone() for k, p in m.named_parameters()}]
    assert _same(a, _step(m, img, ids, lens, None))


@pytest.mark.parametrize("coatt", MODES)
def test_model_eval_config_width(vqa, coatt):
    """L = 196, E = 512 (config 4's grid and width), N < U with a repeated image, eval mode, against fp64; predict() forwards
    the keyword"""
    U, N, L, E, D, T = 4, 3, 196, 512, 256, 14
    m = _model(vqa, coatt, L=L, E=E, D=D).eval()
    img, ids, lens = _inputs(True, U=U, N=N, L=L, D=D, T=T)
    idx = torch.tensor([3, 1, 3], device=DEV)
    with torch.no_grad():
        outs = m(img, ids, lens, img_index=idx)
        sd = {k: v.double() for k, v in m.state_dict().items()}
        ref = RS.forward(sd, img.double(), ids, idx, lens, coatt=coatt)
    errs = [rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(outs, ref)]
    print("shared eval %s: rel_err logits %.2e av %.2e aq %.2e" % (coatt, *errs))
    assert outs[0].shape == (N, O_) and outs[1].shape == (N, 3, L) and outs[2].shape == (N, 3, T) and max(errs) <= 1e-4
    ans, prob = vqa.predict(m, img, ids, lens, k=3, img_index=idx)
    assert torch.equal(ans[:, 0], outs[0].argmax(1))


def test_alternating_image_side_stays_at_u(vqa, monkeypatch):
    """alternating mode: no product and no grouped pass sees N*L rows -- the image side runs on U*L rows, forward and backward"""
    ops = vqa.ops
    m = _model(vqa, "alternating").train()
    img, ids, lens = _inputs(True)
    idx = torch.tensor(IDX, device=DEV)
    rows = []
    real_gemm, real_rows = ops.gemm, ops.gemm_rows

    def gemm(a, b, *args, **kw):
        rows.append(a.shape[0])
        return real_gemm(a, b, *args, **kw)

    def gemm_rows(a, b, *args, **kw):
        rows.append(a.shape[0])
        return real_rows(a, b, *args, **kw)

    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "gemm_rows", gemm_rows)
    for name in ("guided_logits_fwd", "guided_logits_bwd"):                     # the per-sample image passes are not used
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, **k: (rows.append(a[-2] * a[-1]), _r(*a, **k))[1])
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        _step(m, img, ids, lens, idx)
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    prof = {k: v[0] for k, v in ops.prof_report().items()}
    assert N_ * L_ not in rows and U_ * L_ in rows, rows
    assert prof.get("glimpse_dfeat_grouped") == 1 and prof.get("row_block_gather", 0) == 0, prof
    assert prof.get("guided_logits_fwd") == 7 and prof.get("guided_logits_bwd") == 7, prof


def test_argument_checks(vqa):
    m = _model(vqa, "alternating").eval()
    img, ids, lens = _inputs(True)
    idx = torch.tensor(IDX, device=DEV)
    for bad in (idx[:3], idx.view(N_, 1), idx.float(), idx.cpu(), IDX):
        with pytest.raises(vqa.VqfError):
            m(img, ids, lens, img_index=bad)
    with pytest.raises(vqa.VqfError):
        m(img, ids, lens)                                                       # (U, L, D) images without an index: N mismatch in q_length
