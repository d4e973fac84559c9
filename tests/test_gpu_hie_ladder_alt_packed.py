"""HieCoAttenLadder(coatt="alternating", packed_coatt=True) on the MI355X: the image side of the alternating levels on the R packed
rows of a PackedRegions.

Kernel level: vqf_guided_logits_fwd_packed / _bwd_packed and vqf_glimpse_pool_bwd_packed_dfeat hold the BITS of the existing plain /
_grouped / _len / _grouped_len entry points run on the padded copy (junk behind every count there, so a row read past a count
shows): every output in padded coordinates compares equal, the packed outputs equal that run's real rows; and they meet the fp64
references of tests/hie_ladder_alt_packed_ref.py at the bounds tests/test_gpu_hie_ladder_alt.py uses for the same quantities
(rel_err <= 5e-6 on logits and dXh, <= 1e-5 on the sums dgp and dw).  dfeat is a sum of G <= 3 products per element, like dXh: 5e-6;
dlogits is a dot product over C with the softmax backward behind it, a sum like dgp: 1e-5.  vqf_tanh_dropout_packed_fwd / _bwd hold
the bits of the unpack / pack forms' real rows.  Model level: the criteria of tests/test_gpu_hie_ladder_packed.py, unchanged."""
import ctypes
import sys
import warnings

import pytest
import torch

import hie_ladder_alt_packed_ref as AP
import hie_ladder_regions_ref as RR
import mfb_packed_ref as PR
import test_gpu_hie_ladder_packed as TP
from golden_util import rel_err, grad_parity

pytestmark = pytest.mark.gpu

DEV = TP.DEV
SENTINEL = TP.SENTINEL
GROUP_IDX = [2, 0, 0, 2, 0, 2, 0, 0, 0]             # U = 3, N = 9: image 1 without a question, image 0 with six (two trips of four)


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def ops(vqa):
    return vqa.ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float()


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------
# (U, L, E, counts): ragged counts in one chunk; 4 backward chunks of 49 and 7 forward chunks with an owner whose later chunks are
# empty; the 768-thread block at G = 3 with a count that ends inside chunk 0; tiny L; L = 1
KCASES = [(5, 20, 64, [1, 20, 19, 7, 4]), (3, 196, 512, [5, 196, 195]), (2, 70, 1024, [70, 33]), (6, 3, 32, [1, 3, 2, 3, 1, 2]),
          (2, 1, 32, [1, 1])]
GCASES = [(20, 64, [7, 20, 1]), (196, 512, [5, 196, 195]), (70, 1024, [70, 33, 12])]          # grouped: U = 3 with GROUP_IDX


def _operands(U, N, L, E, G, counts, idx, guided):
    """padded copies with finite junk behind every count, their packed rows, and the rest -- on the GPU; the fp64 side on the CPU"""
    GE = G * E
    qcounts = counts if idx is None else [counts[i] for i in idx]
    xh_pad = RR.fill_rows(_rand((U, L, GE), 1 + L, 1.5), counts, "rand", seed=7)
    v_pad = RR.fill_rows(_rand((U, L, E), 2 + L), counts, "rand", seed=8)
    c = dict(xh=PR.pack_rows(xh_pad, counts), v=PR.pack_rows(v_pad, counts), xh_pad=xh_pad, v_pad=v_pad,
             gp=_rand((N, GE), 3 + L) if guided else None, w=_rand((G, E), 4 + L, 0.2), dpooled=_rand((N, GE), 5 + L),
             dwts=_rand((N, G, L), 6 + L), off=PR.offsets_of(counts), qcounts=qcounts)
    dl = _rand((N, L, G), 9 + L)
    c["dl_zero"] = RR.fill_rows(dl, qcounts, 0.0)                                 # what the padded kernels are handed
    c["dl_junk"] = RR.fill_rows(dl, qcounts, "rand", seed=10)                     # the packed kernels do not read behind a count
    c["real_q"] = RR.region_mask(torch.tensor(qcounts), L)
    return c


def _gpu(c):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    d["roff"] = c["off"].to(torch.int32).to(DEV)
    d["lens_q"] = torch.tensor(c["qcounts"], dtype=torch.int32, device=DEV)
    return d


def _check(tag, got, want, bound):
    e = rel_err(got.detach().cpu().numpy(), want.numpy())
    print("%s: rel_err %.2e / bound %.0e" % (tag, e, bound))
    assert e <= bound, tag


def _kernel_case(vqa, U, N, L, E, G, counts, idx, guided):
    ops = vqa.ops
    GE, R = G * E, sum(counts)
    c = _operands(U, N, L, E, G, counts, idx, guided)
    d = _gpu(c)
    tag = "U=%d N=%d L=%d E=%d G=%d guided=%d" % (U, N, L, E, G, guided)
    grp = None
    if idx is not None:
        grp = sys.modules[vqa.PackedRegions.__module__]._group_index(torch.tensor(idx, device=DEV), U)     # host/grouping.py
    gidx = None if grp is None else grp[0]
    real_q = d["real_q"]
    # -- forward: logits in padded coordinates
    lg = ops.guided_logits_fwd_packed(d["xh"], d["gp"], d["w"], d["roff"], N, L, idx=gidx)
    if grp is None:
        lg_pad = ops.guided_logits_fwd(d["xh_pad"].view(U * L, GE), d["gp"], d["w"], N, L)
    else:
        lg_pad = ops.guided_logits_fwd_grouped(d["xh_pad"].view(U * L, GE), d["gp"], d["w"], gidx, N, U, L)
    lg3, lgp3 = lg.view(N, L, G), lg_pad.view(N, L, G)
    assert torch.equal(lg3[real_q], lgp3[real_q])
    assert torch.equal(lg3[~real_q], torch.zeros_like(lg3[~real_q]))             # exact zeros behind each count
    assert torch.equal(ops.guided_logits_fwd_packed(d["xh"], d["gp"], d["w"], d["roff"], N, L, idx=gidx), lg)
    _check("logits " + tag, lg3, AP.guided_logits_fwd(c["xh"], c["gp"], c["w"], c["off"], N, L, idx), 5e-6)
    # -- the pooling backward with dfeat, on the weights of the packed forward (existing entry point)
    wts, _ = ops.glimpse_pool_fwd_packed(d["v"], lg, d["roff"], N, L, False, idx=gidx)
    dlv, dfeat = ops.glimpse_pool_bwd_packed_dfeat(d["dpooled"], d["v"], wts, d["roff"], False, grp=grp,
                                                   dwts=d["dwts"])
    if grp is None:
        dlv_pad, dfeat_pad = ops.glimpse_pool_bwd(d["dpooled"], d["v_pad"], wts, False, True, dwts=d["dwts"], lens=d["lens_q"])
    else:
        dlv_pad, dfeat_pad = ops.glimpse_pool_bwd_grouped(d["dpooled"], d["v_pad"], wts, grp[0], grp[1], grp[2], True, dwts=d["dwts"],
                                                          lens=d["lens_q"])
    assert dfeat.shape == (R, E) and torch.equal(dlv, dlv_pad)
    assert torch.equal(dfeat, PR.pack_rows(dfeat_pad, counts))
    again = ops.glimpse_pool_bwd_packed_dfeat(d["dpooled"], d["v"], wts, d["roff"], False, grp=grp, dwts=d["dwts"])
    assert torch.equal(again[0], dlv) and torch.equal(again[1], dfeat)
    dl64, df64 = AP.pool_bwd(c["dpooled"], c["dwts"], c["v"], wts.cpu(), c["off"], N, L, idx)
    _check("dlogits " + tag, dlv.view(N, L, G), dl64, 1e-5)
    _check("dfeat " + tag, dfeat, df64, 5e-6)
    # -- the guided-logits backward
    dxh, dgp, dw = ops.guided_logits_bwd_packed(d["dl_junk"].view(N * L, G), d["xh"], d["gp"], d["w"], d["roff"], N, L, grp=grp)
    if grp is None:
        dxh_pad, dgp_pad, dw_pad = ops.guided_logits_bwd(d["dl_zero"].view(N * L, G), d["xh_pad"].view(U * L, GE), d["gp"], d["w"], N, L)
    else:
        dxh_pad, dgp_pad, dw_pad = ops.guided_logits_bwd_grouped(d["dl_zero"].view(N * L, G), d["xh_pad"].view(U * L, GE), d["gp"],
                                                                  d["w"], grp[1], grp[2], N, U, L)
    assert dxh.shape == (R, GE)
    assert torch.equal(dgp, dgp_pad) and torch.equal(dw, dw_pad)
    assert torch.equal(dxh, PR.pack_rows(dxh_pad.view(U, L, GE), counts))
    if idx is not None:                                                          # image 1 has no question: exact zeros on its rows
        st, cnt = PR.clamped_spans(c["off"], R, L)[1]
        assert torch.equal(dxh[st:st + cnt], torch.zeros(cnt, GE, device=DEV))
        assert torch.equal(dfeat[st:st + cnt], torch.zeros(cnt, E, device=DEV))
    again = ops.guided_logits_bwd_packed(d["dl_junk"].view(N * L, G), d["xh"], d["gp"], d["w"], d["roff"], N, L, grp=grp)
    assert all(torch.equal(a, b) for a, b in zip(again, (dxh, dgp, dw)))
    x64, g64, w64 = AP.guided_logits_bwd(c["dl_zero"], c["xh"], c["gp"], c["w"], c["off"], N, L, idx)
    _check("dXh " + tag, dxh, x64, 5e-6)
    _check("dgp " + tag, dgp, g64, 1e-5)
    _check("dw " + tag, dw, w64, 1e-5)


@pytest.mark.parametrize("guided", [True, False], ids=["gp", "no_gp"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("U,L,E,counts", KCASES, ids=["U%d_L%d_E%d" % s[:3] for s in KCASES])
def test_packed_kernels_hold_the_bits_of_the_padded_kernels(vqa, U, L, E, counts, G, guided):
    _kernel_case(vqa, U, U, L, E, G, counts, None, guided)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("L,E,counts", GCASES, ids=["L%d_E%d" % s[:2] for s in GCASES])
def test_grouped_packed_kernels_hold_the_bits_of_the_grouped_kernels(vqa, L, E, counts, G):
    _kernel_case(vqa, 3, len(GROUP_IDX), L, E, G, counts, GROUP_IDX, True)


# ---- the packed tanh / dropout pass ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,p,seed", TP.KMASKS, ids=[k[0] + ("" if k[0] != "philox" else "_p%g" % k[1]) for k in TP.KMASKS])
@pytest.mark.parametrize("U,L,E,counts", TP.KSHAPES, ids=["U%d_L%d_E%d" % s[:3] for s in TP.KSHAPES])
def test_packed_tanh_dropout_holds_the_bits_of_the_unpack_forms(ops, U, L, E, counts, kind, p, seed):
    """row start + l equals, bit for bit, row u*L + l of vqf_tanh_dropout_unpack_fwd, and dz the output of vqf_tanh_dropout_pack_bwd"""
    z, dy, off, roff, margs, real = TP._kcase(U, L, E, counts, kind, p, seed)
    R = z.shape[0]
    y_pad = ops.tanh_dropout_unpack_fwd(z, roff, U, L, **margs)
    y = ops.tanh_dropout_packed_fwd(z, roff, U, L, **margs)
    assert y.shape == (R, E) and torch.equal(y, PR.pack_rows(y_pad.view(U, L, E), counts))
    assert torch.equal(ops.tanh_dropout_packed_fwd(z, roff, U, L, **margs), y)
    dz_pad = ops.tanh_dropout_pack_bwd(dy, y_pad, roff, U, R, L, **margs)
    dz = ops.tanh_dropout_packed_bwd(PR.pack_rows(dy.view(U, L, E), counts), y, roff, U, L, **margs)
    assert dz.shape == (R, E) and torch.equal(dz, dz_pad)
    assert torch.equal(ops.tanh_dropout_packed_bwd(PR.pack_rows(dy.view(U, L, E), counts), y, roff, U, L, **margs), dz)
    if kind != "none":
        assert bool((y == 0).any()) and bool((y != 0).any())


# ---- offsets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["own_images", "img_index"])
@pytest.mark.parametrize("name,offs", TP.BAD_OFFSETS, ids=[b[0] for b in TP.BAD_OFFSETS])
def test_guard_rows_stay_untouched_whatever_the_offsets_hold(vqa, ops, name, offs, grouped):
    """every output of the new entry points sits between guard rows filled with a sentinel; offsets that are negative, decreasing,
    beyond R or with counts above L are clamped by the documented rule: every return code is VQF_OK, nothing outside a tensor is
    written, and logits are the reference on the clamped spans"""
    U, L, E, counts = TP.KSHAPES[0]
    G, GD = 3, 3
    GE, R = G * E, sum(counts)
    idx = [4, 0, 0, 2, 4, 1, 0, 3] if grouped else None
    N = len(idx) if grouped else U
    c = _operands(U, N, L, E, G, counts, idx, True)
    d = _gpu(c)
    off = c["off"] if offs is None else torch.tensor(offs, dtype=torch.int64)
    roff = off.to(torch.int32).to(DEV)
    grp = None
    if grouped:
        grp = sys.modules[vqa.PackedRegions.__module__]._group_index(torch.tensor(idx, device=DEV), U)     # host/grouping.py
    lib = vqa.lib.load()
    st = ops._stream()
    P = lambda t, rows=0: ctypes.c_void_p(t.data_ptr() + rows * t.stride(0) * 4) if t is not None else None
    guarded = lambda rows, cols: torch.full((rows + 2 * GD, cols), SENTINEL, device=DEV)
    bufs = {"logits": guarded(N * L, G), "dlogits": guarded(N * L, G), "dfeat": guarded(R, E), "dxh": guarded(R, GE),
            "dgp": guarded(N, GE), "dw": guarded(G, E), "y": guarded(R, E), "dz": guarded(R, E)}
    rows_of = {"logits": N * L, "dlogits": N * L, "dfeat": R, "dxh": R, "dgp": N, "dw": G, "y": R, "dz": R}
    gi, go, gg = (None, None, None) if grp is None else grp
    wts = torch.softmax(_rand((N, G, L), 3), 2).to(DEV).contiguous()
    ws = ops.workspace(DEV, lib.vqf_guided_logits_bwd_packed_ws_bytes(N, U, L, E, G))
    keep = (_rand((U * L, E), 5) > 0).to(torch.uint8).to(DEV)
    assert lib.vqf_guided_logits_fwd_packed(P(d["xh"]), GE, P(d["gp"]), P(d["w"]), P(gi), P(roff), N, U, R, L, E, G,
                                            P(bufs["logits"], GD), st) == 0
    assert lib.vqf_glimpse_pool_bwd_packed_dfeat(P(d["dpooled"]), P(d["dwts"]), P(d["v"]), P(wts), P(gi), P(go), P(gg), P(roff), N, U, R,
                                                 L, E, G, 0, P(bufs["dlogits"], GD), P(bufs["dfeat"], GD), st) == 0
    assert lib.vqf_guided_logits_bwd_packed(P(d["dl_junk"]), P(d["xh"]), GE, P(d["gp"]), P(d["w"]), P(go), P(gg), P(roff), N, U, R, L, E, G,
                                            P(bufs["dxh"], GD), GE, P(bufs["dgp"], GD), P(bufs["dw"], GD), P(ws), ws.numel(), st) == 0
    assert lib.vqf_tanh_dropout_packed_fwd(P(d["v"]), P(roff), P(keep), 0, 0.5, U, R, L, E, P(bufs["y"], GD), st) == 0
    assert lib.vqf_tanh_dropout_packed_bwd(P(d["v"]), P(d["v"]), P(roff), P(keep), 0, 0.5, U, R, L, E, P(bufs["dz"], GD), st) == 0
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        rows = rows_of[k]
        assert torch.equal(buf[:GD], torch.full_like(buf[:GD], SENTINEL)), k
        assert torch.equal(buf[GD + rows:], torch.full_like(buf[:GD], SENTINEL)), k
    spans = PR.clamped_spans(off, R, L)
    assert all(0 <= s0 and 1 <= cnt <= L and s0 + cnt <= R for s0, cnt in spans)
    want = AP.guided_logits_fwd(c["xh"], c["gp"], c["w"], off, N, L, idx)
    _check("logits on clamped spans (%s)" % name, bufs["logits"][GD:GD + N * L].view(N, L, G), want, 5e-6)
    for k in ("logits", "dlogits", "dgp", "dw"):                                # padded coordinates: every element written
        assert not bool((bufs[k][GD:GD + rows_of[k]] == SENTINEL).any()), k
    if offs is None:
        for k in ("dfeat", "dxh", "y", "dz"):                                    # every real row written
            assert not bool((bufs[k][GD:GD + R] == SENTINEL).any()), k


# ---- model level -------------------------------------------------------------------------------------------------------------------------
def _model(vqa, L, E, D, packed_coatt, V=40, H=48, O=30, seed=0, drop_p=0.5):
    """TP._model (the same seeded weights) with the keyword"""
    torch.manual_seed(seed)
    m = vqa.HieCoAttenLadder(block_num=L, img_size=D, vocab_size=V, embed_size=E, hidden_size=H, output_size=O, drop_p=drop_p,
                             coatt="alternating", packed_coatt=packed_coatt)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (1.2 / (p[0].numel() if p.dim() > 1 else 8) ** 0.5))
    return m.to(DEV)


def _parity(vqa, U, N, T, L, E, D, with_lens, train, idx=None, counts=None, H=48, O=30, V=40):
    """TP._parity with packed_coatt=True: rel_err <= 1e-4 on the outputs against fp64 on the unpacked copy, grad_parity"""
    idx = None if idx is None else torch.tensor(idx, device=DEV)
    m = _model(vqa, L, E, D, True, V=V, H=H, O=O).train(train)
    packed, ids, lens, counts = TP._inputs(vqa, U, N, L, D, T, V=V, counts=counts)
    lens = lens if with_lens else None
    m.set_keep_masks(**TP._masks(U, N, L, T, E, H, 5))
    logits, av, aq = TP._call(m, packed, ids, lens, idx)
    assert logits.shape == (N, O) and av.shape == (N, 3, L) and aq.shape == (N, 3, T)
    wl, wv, wq = TP._loss_weights(logits, av, aq)
    m.zero_grad()
    ((logits * wl).sum() + (av * wv).sum() + (aq * wq).sum()).backward()
    img, rcounts = TP._unpacked(packed)
    refs = {}
    for dt in (torch.float64, torch.float32):
        sd = TP._sd_leaves(m, dt)
        rm = {k: v.to(DEV) for k, v in m._seeds.keep.items()} if train else None
        rl, rav, raq = RR.forward(sd, img, ids, rcounts, lens, idx, masks=rm, p=m.drop_p, dtype=dt, coatt="alternating")
        ((rl * wl.to(dt)).sum() + (rav * wv.to(dt)).sum() + (raq * wq.to(dt)).sum()).backward()
        refs[dt] = (rl.detach(), rav.detach(), raq.detach(),
                    {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().cpu() for k, v in sd.items()})
    rl, rav, raq, g64 = refs[torch.float64]
    errs = [rel_err(a.detach().cpu().numpy(), b.cpu().numpy()) for a, b in ((logits, rl), (av, rav), (aq, raq))]
    tag = "%s U=%d N=%d T=%d L=%d E=%d q_length=%s%s" % ("train" if train else "eval", U, N, T, L, E, with_lens,
                                                        "" if idx is None else " img_index")
    print("packed_coatt %s: rel_err logits %.2e av %.2e aq %.2e / bound 1e-4" % (tag, *errs))
    assert max(errs) <= 1e-4
    pad = ~RR.region_mask(rcounts, L)
    pad = (pad if idx is None else pad[idx]).unsqueeze(1).expand(N, 3, L)
    assert torch.equal(av[pad], torch.zeros_like(av[pad]))                       # av: exact zeros behind each count
    assert float((av.detach().sum(2) - 1).abs().max()) <= 1e-5
    gpu = {k: p.grad for k, p in m.named_parameters()}
    assert set(gpu) == set(g64)
    assert float(gpu["img_emb.weight"].abs().max()) > 0
    grad_parity(gpu, refs[torch.float32][3], g64, label="HieCoAttenLadder packed_coatt " + tag)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [14, 22])
@pytest.mark.parametrize("N", [1, 5])
def test_model_vs_fp64_on_the_unpacked_copy(vqa, N, T, L, E, D, train):
    for with_lens in (False, True):
        _parity(vqa, N, N, T, L, E, D, with_lens, train)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("L,E,D", [(50, 64, 96), (196, 512, 256)])
@pytest.mark.parametrize("T", [14, 22])
def test_model_shared_images_vs_fp64(vqa, T, L, E, D, train):
    _parity(vqa, 3, 7, T, L, E, D, True, train, idx=TP.SHARED_IDX, counts=TP._shared_counts(L))


@pytest.mark.parametrize("shared", [False, True], ids=["own_images", "img_index"])
def test_keyword_against_the_default_model(vqa, shared):
    """on a plain tensor and on the pair the keyword changes no bit; on a PackedRegions (in-kernel Philox masks under one seed: the
    same masks are drawn) the outputs agree to <= 1e-4 -- the order of the dwimg sum differs, so bit-equality is not claimed; int32
    and int64 offsets are the same call; two runs give equal bits"""
    T, L, E, D = 14, 50, 64, 96
    U, N = (3, 7) if shared else (4, 4)
    idx = torch.tensor(TP.SHARED_IDX, device=DEV) if shared else None
    cnt = TP._shared_counts(L) if shared else TP._counts(U, L)
    on, off = _model(vqa, L, E, D, True).train(), _model(vqa, L, E, D, False).train()
    packed, ids, lens, _ = TP._inputs(vqa, U, N, L, D, T, counts=cnt)
    img = TP._unpacked(packed)[0]
    p32 = vqa.PackedRegions(packed.rows, packed.offsets.to(torch.int32), L)

    def run(m, feats, seed=77):
        torch.manual_seed(seed)
        return TP._step(m, feats, ids, lens, idx)

    for feats in (img, (img, None), (img, cnt.to(DEV))):
        assert TP._same(run(on, feats), run(off, feats))
    a, b = run(on, packed), run(off, packed)
    assert TP._same(a, run(on, packed)) and TP._same(a, run(on, p32))
    errs = [rel_err(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[:3], b[:3])]
    gerr = max(rel_err(a[3][k].cpu().numpy(), b[3][k].cpu().numpy()) for k in a[3])
    print("packed_coatt on / off, one Philox seed: rel_err logits %.2e av %.2e aq %.2e, gradients %.2e" % (*errs, gerr))
    assert max(errs) <= 1e-4
    assert not torch.equal(a[0], run(on, packed, seed=78)[0])                    # (the seed does decide the masks)


def test_keep_masks_stay_padded(vqa):
    """set_keep_masks(img=...) stays (U*L, E): flipping mask entries of PADDED rows changes nothing, flipping those of real rows does"""
    U = N = 4
    T, L, E, D = 14, 50, 64, 96
    m = _model(vqa, L, E, D, True).train()
    packed, ids, lens, counts = TP._inputs(vqa, U, N, L, D, T)
    masks = TP._masks(U, N, L, T, E, 48, 5)
    m.set_keep_masks(**masks)
    a = TP._step(m, packed, ids, lens)
    real = RR.region_mask(counts, L).to(DEV).view(U * L, 1)
    m.set_keep_masks(**dict(masks, img=torch.where(real, masks["img"], 1 - masks["img"])))
    assert TP._same(a, TP._step(m, packed, ids, lens))
    m.set_keep_masks(**dict(masks, img=1 - masks["img"]))
    assert not torch.equal(a[0], TP._step(m, packed, ids, lens)[0])


def test_predict_takes_it(vqa):
    U, N, T, L, E, D = 3, 7, 14, 50, 64, 96
    idx = torch.tensor(TP.SHARED_IDX, device=DEV)
    m = _model(vqa, L, E, D, True).train()
    packed, ids, lens, _ = TP._inputs(vqa, U, N, L, D, T, counts=TP._shared_counts(L))
    ids_k, probs = vqa.predict(m, packed, ids, lens, k=3, img_index=idx)
    assert m.training
    with torch.no_grad():
        logits = m.eval()(packed, ids, lens, idx)[0]
    ref = vqa.topk_answers(logits, 3)
    assert torch.equal(ids_k, ref[0]) and torch.equal(probs, ref[1]) and torch.equal(ids_k[:, 0], logits.argmax(1))


# ---- structure --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,U,N,counts", [s[:4] for s in TP.STRUCT[:2]], ids=[s[0] for s in TP.STRUCT[:2]])
def test_structure(vqa, monkeypatch, name, U, N, counts):
    """the opt-in step beside the default packed step: the packed tanh kernels in the place of the unpack / pack ones, otherwise the
    same launches up to the split-K reductions of the products whose depth or row count changed; no VX-family product has more than R
    rows; the forward reads no GPU tensor on the host and never synchronises"""
    ops = vqa.ops
    T, L, E, D = 14, 196, 512, 256
    R = sum(counts)
    assert R < U * L
    idx = torch.tensor(TP.SHARED_IDX, device=DEV) if N != U else None
    on, off = _model(vqa, L, E, D, True).train(), _model(vqa, L, E, D, False).train()
    packed, ids, lens, _ = TP._inputs(vqa, U, N, L, D, T, counts=torch.tensor(counts))
    vx = {"VX": (0, 0, 3 * E, E), "dV+=dVX.W": (0, 1, E, 3 * E)}                 # (ta, tb, N, K) with M = rows; dW: K = rows

    def counted(m):
        TP._step(m, packed, ids, lens, idx)                 # warm-up (the library's first launches)
        torch.cuda.synchronize()
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            TP._step(m, packed, ids, lens, idx)
            torch.cuda.synchronize()
        finally:
            ops.prof_enable(False)
        shapes = {}
        for rows in (R, U * L):
            for k, (ta, tb, n_, k_) in vx.items():
                shapes[(k, rows)] = ops.prof_gemm(ta, tb, rows, n_, k_)[0]
            shapes[("dW=dVX^T.V", rows)] = ops.prof_gemm(1, 1, 3 * E, E, rows)[0]
        return {k: v[0] for k, v in ops.prof_report().items()}, shapes

    (a, sa), (b, sb) = counted(off), counted(on)
    diff = {k: (a.get(k, 0), b.get(k, 0)) for k in set(a) | set(b) if a.get(k, 0) != b.get(k, 0)}
    print("launches default %d packed_coatt %d; differing: %s" % (sum(a.values()), sum(b.values()), diff))
    print("VX-family products (name, rows): launches  default %s  packed_coatt %s" % (sa, sb))
    assert "tanh_dropout_unpack_fwd" not in b and "tanh_dropout_pack_bwd" not in b
    assert b["tanh_dropout_packed_fwd"] == 1 and b["tanh_dropout_packed_bwd"] == 1
    assert "tanh_dropout_packed_fwd" not in a and a["tanh_dropout_unpack_fwd"] == 1 and a["tanh_dropout_pack_bwd"] == 1
    for k in ("tanh_dropout_unpack_fwd", "tanh_dropout_pack_bwd", "tanh_dropout_packed_fwd", "tanh_dropout_packed_bwd"):
        diff.pop(k)
    sk = diff.pop("splitk_reduce", (0, 0))
    assert diff == {}                                        # nothing else differs ...
    assert abs(sk[0] - sk[1]) <= 3                           # ... but the split-K reductions of the three VX-family products
    for k in ("VX", "dV+=dVX.W", "dW=dVX^T.V"):
        assert sb[(k, U * L)] == 0 and sb[(k, R)] >= 1, (k, sb)   # none at U L rows, each at R
        assert sa[(k, R)] == 0, (k, sa)

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
        out = TP._call(on, packed, ids, lens, idx)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]
