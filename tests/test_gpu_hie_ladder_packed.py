"""HieCoAttenLadder on packed region features, on the MI355X: forward(PackedRegions(rows, offsets, max_regions), ids, q_length,
img_index) is, by definition, the model on the unpacked copy (tests/mfb_packed_ref.unpack_rows) with the counts of the offsets.

Kernel level: vqf_tanh_dropout_unpack_fwd / vqf_tanh_dropout_pack_bwd hold the BITS of vqf_tanh_dropout_fwd / _bwd on the zero-padded
operands (the same arithmetic on the same values, so equality and no tolerance), exact zero padded rows, the host Philox mask of
tests/philox_ref.py at the padded indices, no dependence on what the padded rows of dy / y hold, and untouched guard rows for any
offsets.  Model level: the criteria of tests/test_gpu_hie_ladder_regions.py unchanged -- rel_err <= 1e-4 on logits / av / aq and
grad_parity with explicit keep-masks against tests/hie_ladder_regions_ref.py, train and eval, both co-attention modes -- and
equality of bits where the operands are the same (every count equal to L)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import hie_ladder_regions_ref as RR
import mfb_packed_ref as PR
import philox_ref as PX
from golden_util import rel_err, grad_parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PAD = 0
MODES = ("parallel", "alternating")
SHARED_IDX = [2, 0, 0, 2, 0, 2, 0]                      # U = 3, N = 7: image 1 without a question
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def ops(vqa):
    return vqa.ops


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------
# (U, L, E, counts): odd sizes, counts 1 and L, L = 1, one owner that needs a second trip of the kernel's grid-stride loop
# (64 chunks of 256 threads cover 16384 of an owner's L * E / 4 = 262144 vectors)
KSHAPES = [(5, 20, 64, [1, 20, 19, 7, 4]), (3, 196, 512, [5, 196, 195]), (6, 3, 32, [1, 3, 2, 3, 1, 2]), (2, 1, 32, [1, 1]),
           (3, 1024, 1024, [1024, 1, 513])]
KMASKS = [("keep", 0.5, 0), ("philox", 0.5, 77), ("philox", 0.3, (1 << 61) + 987654321), ("none", 0.0, 0)]


def _kcase(U, L, E, counts, kind, p, seed):
    """z (R, E) away from zero (so y == 0 says 'dropped'), dy (U*L, E), the offsets and the mask arguments -- on the GPU"""
    g = torch.Generator().manual_seed(U * 1000 + L)
    R = sum(counts)
    z = (torch.rand(R, E, generator=g) * 1.9 + 0.1) * (torch.randint(0, 2, (R, E), generator=g) * 2 - 1).float()
    dy = torch.randn(U * L, E, generator=g)
    off = PR.offsets_of(counts)
    keep = (torch.rand(U * L, E, generator=g) >= p).to(torch.uint8).to(DEV) if kind == "keep" else None
    margs = dict(keep=keep, seed=seed, p_drop=p)
    real = RR.region_mask(torch.tensor(counts), L).to(DEV)                       # (U, L) bool
    return z.to(DEV), dy.to(DEV), off, off.to(torch.int32).to(DEV), margs, real


@pytest.mark.parametrize("kind,p,seed", KMASKS, ids=[k[0] + ("" if k[0] != "philox" else "_p%g" % k[1]) for k in KMASKS])
@pytest.mark.parametrize("U,L,E,counts", KSHAPES, ids=["U%d_L%d_E%d" % s[:3] for s in KSHAPES])
def test_unpack_kernels_hold_the_bits_of_the_padded_pass(ops, U, L, E, counts, kind, p, seed):
    z, dy, off, roff, margs, real = _kcase(U, L, E, counts, kind, p, seed)
    R = z.shape[0]
    zpad = PR.unpack_rows(z, off, L)[0].view(U * L, E)
    yref = ops.tanh_dropout_fwd(zpad, None, **margs)
    y = ops.tanh_dropout_unpack_fwd(z, roff, U, L, **margs)
    assert y.shape == (U * L, E)
    y3, yref3 = y.view(U, L, E), yref.view(U, L, E)
    assert torch.equal(y3[real], yref3[real])                                    # the real rows: the bits of the padded pass
    assert torch.equal(y3[~real], torch.zeros_like(y3[~real]))                   # padded rows: exact zeros
    assert torch.equal(ops.tanh_dropout_unpack_fwd(z, roff, U, L, **margs), y)   # two runs give equal bits
    dzref = ops.tanh_dropout_bwd(dy, yref, **margs)
    dz = ops.tanh_dropout_pack_bwd(dy, y, roff, U, R, L, **margs)
    assert dz.shape == (R, E)
    assert torch.equal(dz, PR.pack_rows(dzref.view(U, L, E), counts))
    assert torch.equal(ops.tanh_dropout_pack_bwd(dy, y, roff, U, R, L, **margs), dz)
    # NaN in the padded rows of dy / y changes no dz bit
    nan = torch.full_like(y3, float("nan"))
    dyn = torch.where(real.unsqueeze(2), dy.view(U, L, E), nan).view(U * L, E).contiguous()
    yn = torch.where(real.unsqueeze(2), y3, nan).view(U * L, E).contiguous()
    assert torch.equal(ops.tanh_dropout_pack_bwd(dyn, yn, roff, U, R, L, **margs), dz)
    kept = (y3 != 0)[real].cpu().numpy()
    if kind == "philox":                                                         # the host mask at the PADDED flat indices
        host = PX.keep32((U * L, E), seed, p).reshape(U, L, E)[real.cpu().numpy()]
        assert kept.shape == host.shape and np.array_equal(kept, host)
        if kept.size >= 10000:                                                   # 10 % of 1 - p is >= 10 sigma from here on
            assert 0.9 * (1 - p) < kept.mean() < 1.1 * (1 - p)
    elif kind == "keep":
        assert np.array_equal(kept, margs["keep"].view(U, L, E)[real].cpu().numpy() != 0)
    else:
        assert kept.all()


def _raw_calls(vqa, z, dyb, yb, roff, keep, seed, p, U, R, L, E, ybuf, dzbuf, G):
    """the two entry points on guarded buffers: y / dz start G rows into ybuf / dzbuf"""
    lib = vqa.lib.load()
    ptr = lambda t, rows=0: ctypes.c_void_p(t.data_ptr() + rows * E * 4)
    kp = ctypes.c_void_p(keep.data_ptr()) if keep is not None else None
    st = vqa.ops._stream()
    assert lib.vqf_tanh_dropout_unpack_fwd(ptr(z), ptr(roff), kp, seed, p, U, R, L, E, ptr(ybuf, G), st) == 0
    assert lib.vqf_tanh_dropout_pack_bwd(ptr(dyb), ptr(yb), ptr(roff), kp, seed, p, U, R, L, E, ptr(dzbuf, G), st) == 0
    torch.cuda.synchronize()


BAD_OFFSETS = [("well_formed", None),
               ("negative", [-7, -2, 5, 9, 30, 31]),
               ("decreasing", [0, 20, 12, 3, 3, 31]),
               ("beyond_R", [0, 40, 90, 1 << 30, (1 << 31) - 1, 31]),
               ("counts_above_L", [0, 25, 26, 27, 28, 29]),
               ("int_extremes", [-(1 << 31), (1 << 31) - 1, -(1 << 31), 0, (1 << 31) - 1, -1])]


@pytest.mark.parametrize("name,offs", BAD_OFFSETS, ids=[b[0] for b in BAD_OFFSETS])
@pytest.mark.parametrize("kind,p,seed", [KMASKS[0], KMASKS[1]], ids=["keep", "philox"])
def test_guard_rows_stay_untouched_whatever_the_offsets_hold(vqa, ops, name, offs, kind, p, seed):
    """y and dz sit between guard rows filled with a sentinel; offsets that are negative, decreasing, beyond R or with counts above
    L are clamped by the documented rule (start = clamp(off[u], 0, R - 1), cnt = clamp(off[u+1] - off[u], 1, min(L, R - start))):
    nothing outside the tensors is written, and y is the padded pass on the clamped spans"""
    U, L, E, counts = KSHAPES[0]
    z, dy, off, roff, margs, _ = _kcase(U, L, E, counts, kind, p, seed)
    R, G = z.shape[0], 3
    if offs is not None:
        off = torch.tensor(offs, dtype=torch.int64)
        roff = off.to(torch.int32).to(DEV)
    ybuf = torch.full((U * L + 2 * G, E), SENTINEL, device=DEV)
    dzbuf = torch.full((R + 2 * G, E), SENTINEL, device=DEV)
    y_in = ops.tanh_dropout_fwd(dy, None, keep=None, seed=0, p_drop=0.0)          # any bounded y for the backward
    _raw_calls(vqa, z, dy, y_in, roff, margs["keep"], seed, p, U, R, L, E, ybuf, dzbuf, G)
    for buf, rows in ((ybuf, U * L), (dzbuf, R)):
        assert torch.equal(buf[:G], torch.full_like(buf[:G], SENTINEL)) and torch.equal(buf[G + rows:], torch.full_like(buf[:G], SENTINEL))
    spans = PR.clamped_spans(off, R, L)
    zpad = torch.zeros(U, L, E, device=DEV)
    for u, (start, cnt) in enumerate(spans):
        assert 0 <= start and 1 <= cnt and start + cnt <= R and cnt <= L
        zpad[u, :cnt] = z[start:start + cnt]
    assert torch.equal(ybuf[G:G + U * L], ops.tanh_dropout_fwd(zpad.view(U * L, E), None, **margs))
    if offs is None:
        assert not bool((dzbuf[G:G + R] == SENTINEL).any())                      # every real row written


# ---- model level -------------------------------------------------------------------------------------------------------------------------
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


def _shared_counts(L):
    """image 0: L - 1 regions, image 2: one; the image without a question carries L"""
    return torch.tensor([L - 1, L, 1], dtype=torch.int64)


def _inputs(vqa, U, N, L, D, T, V=40, seed=0, counts=None):
    """the packed batch, right-padded ids (padding id 0), question lengths -- on the GPU -- and the counts (CPU)"""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(U, L, D, generator=g)
    ids = torch.randint(1, V, (N, T), generator=g)
    lens = torch.tensor(([min(2, T), 1, T] + torch.randint(1, T + 1, (max(N - 3, 0),), generator=g).tolist())[:N], dtype=torch.int64)
    ids = torch.where(torch.arange(T).unsqueeze(0) < lens.unsqueeze(1), ids, torch.full_like(ids, PAD))
    counts = _counts(U, L, seed) if counts is None else counts
    packed = vqa.PackedRegions(PR.pack_rows(img, counts).to(DEV), PR.offsets_of(counts).to(DEV), L)
    return packed, ids.to(DEV), lens.to(DEV), counts


def _unpacked(packed):
    """the unpacked copy, by the independent helper: (img (U, L, D) zero-padded, counts (U,)) on the GPU"""
    img, counts = PR.unpack_rows(packed.rows, packed.offsets.cpu(), packed.max_regions)
    return img, counts.to(DEV)


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


def _call(m, feats, ids, lens, idx):
    if idx is not None:
        return m(feats, ids, lens, idx)
    return m(feats, ids, lens) if lens is not None else m(feats, ids)


def _step(m, feats, ids, lens, idx=None):
    """one forward + backward of a weighted sum of all three outputs -> (logits, av, aq, {name: grad})"""
    m.zero_grad()
    logits, av, aq = _call(m, feats, ids, lens, idx)
    wl, wv, wq = _loss_weights(logits, av, aq)
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    return logits.detach().clone(), av.detach().clone(), aq.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and set(a[3]) == set(b[3]) and \
        all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def _parity(vqa, coatt, U, N, T, L, E, D, with_lens, train, idx=None, counts=None, H=48, O=30, V=40):
    """the packed step against the fp64 / fp32 restatement on the unpacked copy: rel_err <= 1e-4 on the outputs, grad_parity"""
    idx = None if idx is None else torch.tensor(idx, device=DEV)
    m = _model(vqa, L, E, D, coatt, V=V, H=H, O=O).train(train)
    packed, ids, lens, counts = _inputs(vqa, U, N, L, D, T, V=V, counts=counts)
    lens = lens if with_lens else None
    m.set_keep_masks(**_masks(U, N, L, T, E, H, 5))
    logits, av, aq = _call(m, packed, ids, lens, idx)
    assert logits.shape == (N, O) and av.shape == (N, 3, L) and aq.shape == (N, 3, T)
    wl, wv, wq = _loss_weights(logits, av, aq)
    m.zero_grad()
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    img, rcounts = _unpacked(packed)
    assert rcounts.tolist() == counts.tolist()
    refs = {}
    for dt in (torch.float64, torch.float32):
        sd = _sd_leaves(m, dt)
        rm = {k: v.to(DEV) for k, v in m._seeds.keep.items()} if train else None
        rl, rav, raq = RR.forward(sd, img, ids, rcounts, lens, idx, masks=rm, p=m.drop_p, dtype=dt, coatt=coatt)
        ((rl * wl.to(dt)).sum() + (rav * wv.to(dt)).sum() + (raq * wq.to(dt)).sum()).backward()
        refs[dt] = (rl.detach(), rav.detach(), raq.detach(),
                    {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu() for k, v in sd.items()})
    rl, rav, raq, g64 = refs[torch.float64]
    errs = [rel_err(a.detach().cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
    tag = "%s %s U=%d N=%d T=%d L=%d E=%d q_length=%s%s" % (coatt, "train" if train else "eval", U, N, T, L, E, with_lens,
                                                           "" if idx is None else " img_index")
    print("packed %s: rel_err logits %.2e av %.2e aq %.2e" % (tag, *errs))
    assert max(errs) <= 1e-4
    pad = ~RR.region_mask(rcounts, L)
    pad = (pad if idx is None else pad[idx]).unsqueeze(1).expand(N, 3, L)
    assert torch.equal(av[pad], torch.zeros_like(av[pad]))                       # av: exact zeros on padding
    assert float((av.detach().sum(2) - 1).abs().max()) <= 1e-5
    gpu = {k: p.grad for k, p in m.named_parameters()}
    assert set(gpu) == set(g64)
    assert float(gpu["img_emb.weight"].abs().max()) > 0
    grad_parity(gpu, refs[torch.float32][3], g64, label="HieCoAttenLadder packed " + tag)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("coatt", MODES)
@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [14, 22])
@pytest.mark.parametrize("N", [1, 5])
def test_model_vs_fp64_on_the_unpacked_copy(vqa, N, T, L, E, D, coatt, train):
    for with_lens in (False, True):
        _parity(vqa, coatt, N, N, T, L, E, D, with_lens, train)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("coatt", MODES)
@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [14, 22])
def test_model_shared_images_vs_fp64(vqa, T, L, E, D, coatt, train):
    """U = 3 images, N = 7 questions: offsets are per IMAGE"""
    _parity(vqa, coatt, 3, 7, T, L, E, D, True, train, idx=SHARED_IDX, counts=_shared_counts(L))


@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "img_index"])
@pytest.mark.parametrize("coatt", MODES)
@pytest.mark.parametrize("T", [14, 22])
def test_full_counts_are_the_plain_call(vqa, T, coatt, shared):
    """every count equal to L: R = U L and the projection sees the plain call's operands, so outputs and EVERY gradient are
    bit-identical to the plain-tensor call (train mode, in-kernel Philox masks under one seed); int32 and int64 offsets are the
    same call; two runs give equal bits; the pair and plain calls keep their bits"""
    U, N, L, E, D = (3, 7, 50, 64, 96) if shared else (4, 4, 50, 64, 96)
    idx = torch.tensor(SHARED_IDX, device=DEV) if shared else None
    m = _model(vqa, L, E, D, coatt).train()
    full = torch.full((U,), L, dtype=torch.int64)
    packed, ids, lens, _ = _inputs(vqa, U, N, L, D, T, counts=full)
    img = packed.rows.view(U, L, D)
    P = vqa.PackedRegions
    cnt = (_shared_counts(L) if shared else _counts(U, L)).to(DEV)
    ragged = _inputs(vqa, U, N, L, D, T, counts=cnt.cpu())[0]
    feats = [img, packed, P(packed.rows, packed.offsets.to(torch.int32), L), (img, None), (img, full.to(DEV)),
             ragged, ragged, P(ragged.rows, ragged.offsets.to(torch.int32), L),
             (_unpacked(ragged)[0], cnt), (_unpacked(ragged)[0], cnt.to(torch.int32))]
    runs = []
    for f in feats:
        torch.manual_seed(77)
        runs.append(_step(m, f, ids, lens, idx))
    assert all(_same(runs[0], r) for r in runs[1:5])
    assert _same(runs[5], runs[6]) and _same(runs[5], runs[7]) and _same(runs[8], runs[9])
    assert not torch.equal(runs[0][0], runs[5][0])
    # ragged counts: the pair call on the unpacked copy draws the same masks and differs only by the summation order of the
    # img_emb products (R rows against U L): the outputs agree far inside the model-level bound
    assert max(rel_err(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(runs[5][:3], runs[8][:3])) <= 1e-4
    torch.manual_seed(78)
    assert not torch.equal(runs[5][0], _step(m, ragged, ids, lens, idx)[0])      # (the seed does decide the masks)


@pytest.mark.parametrize("coatt", MODES)
def test_padded_rows_of_v_are_zero_and_masks_stay_padded(vqa, coatt):
    """set_keep_masks(img=...) stays (U*L, E): flipping mask entries of PADDED rows changes nothing, flipping one of a real row does"""
    U = N = 4
    T, L, E, D = 14, 50, 64, 96
    m = _model(vqa, L, E, D, coatt).train()
    packed, ids, lens, counts = _inputs(vqa, U, N, L, D, T)
    masks = _masks(U, N, L, T, E, 48, 5)
    m.set_keep_masks(**masks)
    a = _step(m, packed, ids, lens)
    real = RR.region_mask(counts, L).to(DEV).view(U * L, 1)
    flipped = dict(masks, img=torch.where(real, masks["img"], 1 - masks["img"]))
    m.set_keep_masks(**flipped)
    assert _same(a, _step(m, packed, ids, lens))
    m.set_keep_masks(**dict(masks, img=1 - masks["img"]))
    assert not torch.equal(a[0], _step(m, packed, ids, lens)[0])


@pytest.mark.parametrize("coatt", MODES)
def test_predict_takes_the_packed_batch(vqa, coatt):
    U, N, T, L, E, D = 3, 7, 14, 50, 64, 96
    idx = torch.tensor(SHARED_IDX, device=DEV)
    m = _model(vqa, L, E, D, coatt).train()
    packed, ids, lens, _ = _inputs(vqa, U, N, L, D, T, counts=_shared_counts(L))
    ids_k, probs = vqa.predict(m, packed, ids, lens, k=3, img_index=idx)
    assert m.training
    with torch.no_grad():
        logits = m.eval()(packed, ids, lens, idx)[0]
    ref = vqa.topk_answers(logits, 3)
    assert torch.equal(ids_k, ref[0]) and torch.equal(probs, ref[1]) and torch.equal(ids_k[:, 0], logits.argmax(1))
    p5, ids5, lens5, _ = _inputs(vqa, 5, 5, L, D, T)
    m5 = _model(vqa, L, E, D, coatt)
    with torch.no_grad():
        assert torch.equal(vqa.predict(m5, p5, ids5, k=3)[0][:, 0], m5.eval()(p5, ids5)[0].argmax(1))


# ---- structure --------------------------------------------------------------------------------------------------------------------
# (U, N, counts) at L = 196.  The only launches that can depend on the ROW COUNT of the img_emb products are the fp32 GEMM's own: it
# splits K, with a separate splitk_reduce launch, from 32 K-tiles of 16 on (csrc/gemm_f32.hip), and the depth K of the img_emb weight
# gradient is the row count -- R packed, U L padded.  "same_side": both depths >= 497, the two steps must launch equally often.
# "straddle": R = 392 < 497 <= 588 = U L, the packed weight gradient is not split and the packed step may have that one launch less.
STRUCT = [("own_images", 5, 5, [195, 1, 196, 7, 150], True), ("img_index_same_side", 3, 7, [195, 196, 150], True),
          ("img_index_straddle", 3, 7, [195, 196, 1], False)]


@pytest.mark.parametrize("name,U,N,counts,same_side", STRUCT, ids=[c[0] for c in STRUCT])
@pytest.mark.parametrize("coatt", MODES)
def test_structure(vqa, monkeypatch, coatt, name, U, N, counts, same_side):
    """the packed step launches as many kernels as the pair step -- the unpack kernel and its backward in the place of one
    tanh_dropout_fwd / _bwd launch, everything else unchanged -- and no GPU tensor, the offsets and whatever is computed from them
    included, is read on the host during its forward"""
    ops = vqa.ops
    T, L, E, D = 14, 196, 512, 256
    assert (sum(counts) >= 497) == same_side and U * L >= 497
    idx = torch.tensor(SHARED_IDX, device=DEV) if N != U else None
    m = _model(vqa, L, E, D, coatt).train()
    packed, ids, lens, counts = _inputs(vqa, U, N, L, D, T, counts=torch.tensor(counts))
    pair = (_unpacked(packed)[0], counts.to(DEV))

    def counted(feats):
        _step(m, feats, ids, lens, idx)                      # warm-up (the library's first launches)
        torch.cuda.synchronize()
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            _step(m, feats, ids, lens, idx)
            torch.cuda.synchronize()
        finally:
            ops.prof_enable(False)
        return {k: v[0] for k, v in ops.prof_report().items()}

    a, b = counted(pair), counted(packed)
    diff = {k: (a.get(k, 0), b.get(k, 0)) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}
    print("launches pair %d packed %d; differing: %s" % (sum(a.values()), sum(b.values()), diff))
    if same_side:
        assert sum(a.values()) == sum(b.values())
    else:
        assert sum(a.values()) - 1 <= sum(b.values()) <= sum(a.values())
        sk = diff.pop("splitk_reduce", None)
        assert sk is None or sk[1] == sk[0] - 1
    assert diff == {"tanh_dropout_fwd": (a["tanh_dropout_fwd"], a["tanh_dropout_fwd"] - 1),
                    "tanh_dropout_bwd": (a["tanh_dropout_bwd"], a["tanh_dropout_bwd"] - 1),
                    "tanh_dropout_unpack_fwd": (0, 1), "tanh_dropout_pack_bwd": (0, 1)}

    def guard(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError("a GPU tensor was read on the host (Tensor.%s)" % name)
            return real(self, *a, **k)
        return f

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize during the packed forward")

    for name in ("item", "cpu", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, guard(name))
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = _call(m, packed, ids, lens, idx)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]
