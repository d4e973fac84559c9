"""The packed image side of HieCoAttenLadder's alternating co-attention (HieCoAttenLadder(coatt="alternating", packed_coatt=True)),
the part that needs no GPU: the fp64 references of tests/hie_ladder_alt_packed_ref.py against
hie_ladder_regions_ref.coattention_alt on the unpacked copy (values and, through autograd, every gradient of the image step), the
constructor keyword, the new entry points in the header, the binding table and the built library, and their argument checks on
pointers that are never dereferenced."""
import inspect
import os
import re

import pytest
import torch

import hie_ladder_alt_packed_ref as AP
import hie_ladder_alt_ref as RA
import hie_ladder_regions_ref as RR
import mfb_packed_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"vqf_tanh_dropout_packed_fwd": 11, "vqf_tanh_dropout_packed_bwd": 12, "vqf_guided_logits_packed_supported": 6,
       "vqf_guided_logits_fwd_packed": 14, "vqf_guided_logits_bwd_packed_ws_bytes": 5, "vqf_guided_logits_bwd_packed": 21,
       "vqf_glimpse_pool_bwd_packed_dfeat": 18}


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.build()
    return vqa_amd


# ---- the references against the model's restatement on the unpacked copy ------------------------------------------------------------
def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


@pytest.mark.parametrize("U,N,idx,counts", [(4, 4, None, [1, 9, 8, 3]), (3, 7, [2, 0, 0, 2, 0, 2, 0], [8, 9, 1])],
                         ids=["own_images", "img_index"])
def test_refs_are_the_image_step_of_coattention_alt_on_the_unpacked_copy(U, N, idx, counts):
    """one alternating level on (V zero-padded, counts): its v, av and the gradients of V, s and the img_* weights equal what the
    packed references give on the packed rows of V and Xh -- dV = dfeat + dXh img_x on the real rows, zero behind every count"""
    L, T, E, lvl = 9, 5, 8, 1
    pre = "coatt.%d." % lvl
    sd = {pre + k: _rand(s, 10 + j, 0.6).requires_grad_(True) for j, (k, s) in enumerate(
        (("sum_x.weight", (E, E)), ("sum_x.bias", (E,)), ("sum_h.weight", (1, E)), ("img_x.weight", (E, E)), ("img_x.bias", (E,)),
         ("img_g.weight", (E, E)), ("img_h.weight", (1, E)), ("que_x.weight", (E, E)), ("que_x.bias", (E,)),
         ("que_g.weight", (E, E)), ("que_h.weight", (1, E))))}
    off = PR.offsets_of(counts)
    rows = _rand((sum(counts), E), 1)
    Vu = PR.unpack_rows(rows, off, L)[0].requires_grad_(True)                    # (U, L, E), zeros behind each count
    Q = _rand((N, T, E), 2)
    rvalid = RR.region_mask(torch.tensor(counts), L)
    ix = None if idx is None else torch.tensor(idx)
    V = Vu if ix is None else Vu.index_select(0, ix)
    rv = rvalid if ix is None else rvalid.index_select(0, ix)
    v_lvl, _, av_lvl, _ = RR.coattention_alt(V, Q, None, rv, sd, lvl)
    # the level's image step with its summary as a leaf (coattention_alt's second line), so that the summary's gradient shows
    s = RA.attend(Q, None, sd, pre + "sum", None)[0].detach().requires_grad_(True)
    v, av = RA.attend(V, s, sd, pre + "img", rv)
    assert torch.equal(v, v_lvl) and torch.equal(av, av_lvl)
    cv, ca = _rand(v.shape, 3), _rand(av.shape, 4)
    ((v * cv).sum() + (av * ca).sum()).backward()
    # the same step on the packed rows
    wx, bx, wg, wh = (sd[pre + k].detach() for k in ("img_x.weight", "img_x.bias", "img_g.weight", "img_h.weight"))
    xh = rows @ wx.t() + bx                                                       # (R, E): G = 1
    gp = s.detach() @ wg.t()
    lg = AP.guided_logits_fwd(xh, gp, wh, off, N, L, idx)
    assert torch.equal(lg[~rv], torch.zeros_like(lg[~rv]))
    wts, pooled = AP.pool_fwd(rows, lg, off, N, L, idx)
    assert torch.allclose(pooled, v.detach(), rtol=1e-12, atol=1e-13) and torch.allclose(wts[:, 0], av.detach(), rtol=1e-12, atol=1e-13)
    dl, dfeat = AP.pool_bwd(cv, ca.unsqueeze(1), rows, wts, off, N, L, idx)
    assert torch.equal(dl[~rv], torch.zeros_like(dl[~rv]))
    dxh, dgp, dw = AP.guided_logits_bwd(dl, xh, gp, wh, off, N, L, idx)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-10, atol=1e-12)
    dV = dfeat + dxh @ wx
    assert close(dV, PR.pack_rows(Vu.grad, counts))
    real_u = rvalid.unsqueeze(2).expand_as(Vu.grad)
    assert torch.equal(Vu.grad[~real_u], torch.zeros_like(Vu.grad[~real_u]))
    if idx is not None:                                                          # image 1 has no question: exact zeros on its rows
        st, cnt = PR.clamped_spans(off, rows.shape[0], L)[1]
        assert torch.equal(dV[st:st + cnt], torch.zeros(cnt, E, dtype=torch.float64))
    assert close(dgp @ wg, s.grad) and close(dgp.t() @ s.detach(), sd[pre + "img_g.weight"].grad)
    assert close(dw, sd[pre + "img_h.weight"].grad) and close(dgp.sum(0), sd[pre + "img_x.bias"].grad)
    assert close(dxh.t() @ rows, sd[pre + "img_x.weight"].grad)


def test_refs_take_any_offsets_through_clamped_spans():
    """malformed offsets: every span the references touch lies inside the R rows, and the outputs keep their shapes"""
    N, L, E, R = 5, 20, 8, 31
    xh, gp, w = _rand((R, E), 1), _rand((N, E), 2), _rand((1, E), 3)
    for offs in ([-7, -2, 5, 9, 30, 31], [0, 20, 12, 3, 3, 31], [0, 40, 90, 1 << 30, (1 << 31) - 1, 31], [0, 25, 26, 27, 28, 29]):
        off = torch.tensor(offs)
        assert all(0 <= st and 1 <= c <= L and st + c <= R for st, c in PR.clamped_spans(off, R, L))
        lg = AP.guided_logits_fwd(xh, gp, w, off, N, L)
        dxh, dgp, dw = AP.guided_logits_bwd(_rand((N, L, 1), 4), xh, gp, w, off, N, L)
        assert lg.shape == (N, L, 1) and dxh.shape == (R, E) and dgp.shape == (N, E) and dw.shape == (1, E)
        assert torch.isfinite(lg).all() and torch.isfinite(dxh).all()


# ---- the constructor keyword -----------------------------------------------------------------------------------------------------------
def _model(vqa, **kw):
    return vqa.HieCoAttenLadder(img_size=12, vocab_size=20, embed_size=32, hidden_size=10, output_size=6, **kw)


def test_constructor_keyword(vqa):
    with pytest.raises(ValueError, match="packed_coatt"):
        _model(vqa, coatt="parallel", packed_coatt=True)
    with pytest.raises(ValueError, match="packed_coatt"):
        _model(vqa, packed_coatt=True)                                           # parallel is the default mode
    on, off, dflt = _model(vqa, coatt="alternating", packed_coatt=True), _model(vqa, coatt="alternating", packed_coatt=False), \
        _model(vqa, coatt="alternating")
    assert on.packed_coatt is True and off.packed_coatt is False and dflt.packed_coatt is False
    assert _model(vqa, coatt="parallel").packed_coatt is False
    assert list(on.state_dict()) == list(off.state_dict()) == list(dflt.state_dict())       # no new parameters
    assert [tuple(v.shape) for v in on.state_dict().values()] == [tuple(v.shape) for v in off.state_dict().values()]
    assert list(inspect.signature(vqa.HieCoAttenLadder.forward).parameters) == ["self", "img_features", "que_features", "q_length",
                                                                                "img_index"]
    assert inspect.signature(vqa.HieCoAttenLadder.__init__).parameters["packed_coatt"].default is False
    doc = vqa.HieCoAttenLadder.__doc__
    assert "packed_coatt" in doc and "ValueError" in doc[doc.index("packed_coatt"):]
    # the refusals of the packed call are unchanged by the keyword: none needs a GPU
    good = vqa.pack_region_features([torch.randn(k, 12).numpy() for k in (3, 10, 1, 7)])
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        on(good, torch.ones(4, 5, dtype=torch.long))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_library_agree_on_the_new_names_within_abi_7(vqa):
    txt = open(os.path.join(ROOT, "include", "vqa_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vqf_[a-z0-9_]+)\s*\(", txt))
    lib = vqa.lib.load()
    for name, nargs in NEW.items():
        assert name in declared and name in vqa.lib.SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(vqa.lib.SIGNATURES[name][1]) == len(decl.split(",")) == nargs, name
    assert lib.vqf_abi_version() == vqa.lib.ABI_VERSION == 7
    names = [lib.vqf_prof_kernel_name(i).decode() for i in range(lib.vqf_prof_num_kernels())]
    assert names.index("region_rows_stage") < names.index("tanh_dropout_packed_fwd") < names.index("tanh_dropout_packed_bwd")
    assert names.index("tanh_dropout_pack_bwd") == names.index("tanh_dropout_unpack_fwd") + 1 == names.index("region_rows_stage") - 1
    for fn in ("tanh_dropout_packed_fwd", "tanh_dropout_packed_bwd", "guided_logits_packed_supported", "guided_logits_fwd_packed",
               "guided_logits_bwd_packed", "glimpse_pool_bwd_packed_dfeat"):
        assert callable(getattr(vqa.ops, fn)), fn
    assert issubclass(vqa.functions.TanhDropPackedFn, torch.autograd.Function)


BADARG, ALIGN, UNSUPPORTED, WORKSPACE = -1, -2, -3, -4
FAKE = 4096                                       # never dereferenced: every call below is refused first


def test_supported_answers_without_a_gpu(vqa):
    lib = vqa.lib.load()
    sup = lib.vqf_guided_logits_packed_supported
    for ok in ((256, 256, 14000, 100, 512, 3), (1, 1, 1, 1, 32, 1), (65535, 65535, (1 << 29) - 1, 2, 1024, 3), (7, 3, 392, 196, 512, 3),
               (3, 3, 5, 1024, 64, 2)):
        assert sup(*ok) == 1 and vqa.ops.guided_logits_packed_supported(*ok), ok
        assert lib.vqf_guided_logits_grouped_supported(ok[0], ok[1], *ok[3:]) == 1
    for bad in ((2, 2, 0, 3, 32, 1), (2, 2, -1, 3, 32, 1), (2, 2, 1 << 29, 3, 32, 1), (2, 2, 5, 3, 1056, 1), (2, 2, 5, 1025, 32, 1),
                (2, 2, 5, 3, 32, 4), (2, 2, 5, 3, 32, 0), (2, 2, 5, 3, 48, 1), (2, 2, 5, 0, 32, 1), (0, 2, 5, 3, 32, 1), (2, 0, 5, 3, 32, 1),
                (65536, 2, 5, 3, 32, 1), (2, 65536, 5, 3, 32, 1)):
        assert sup(*bad) == 0 and not vqa.ops.guided_logits_packed_supported(*bad), bad
    assert lib.vqf_guided_logits_bwd_packed_ws_bytes(7, 3, 196, 512, 3) == lib.vqf_guided_logits_bwd_grouped_ws_bytes(7, 3, 196, 512, 3)
    assert lib.vqf_guided_logits_bwd_packed_ws_bytes(5, 5, 196, 512, 3) >= lib.vqf_guided_logits_bwd_ws_bytes(5, 196, 512, 3)
    assert lib.vqf_guided_logits_bwd_packed_ws_bytes(0, 3, 196, 512, 3) == 0


def test_argument_checks_need_no_gpu(vqa):
    lib = vqa.lib.load()
    big = 1 << 40

    def fwd(xh=FAKE, gp=FAKE, w=FAKE, idx=None, roff=FAKE, N=2, U=2, R=5, S=3, E=32, G=1, out=FAKE, ldx=None):
        return lib.vqf_guided_logits_fwd_packed(xh, G * E if ldx is None else ldx, gp, w, idx, roff, N, U, R, S, E, G, out, None)

    def bwd(dl=FAKE, xh=FAKE, gp=FAKE, w=FAKE, order=None, grp_off=None, roff=FAKE, N=2, U=2, R=5, S=3, E=32, G=1, dxh=FAKE, dgp=FAKE,
            dw=FAKE, ws=FAKE, wsb=big):
        return lib.vqf_guided_logits_bwd_packed(dl, xh, G * E, gp, w, order, grp_off, roff, N, U, R, S, E, G, dxh, G * E, dgp, dw, ws,
                                                wsb, None)

    def dfeat(dp=FAKE, dwx=None, feat=FAKE, wts=FAKE, idx=None, order=None, grp_off=None, roff=FAKE, N=2, U=2, R=5, S=3, C=32, G=1,
              dl=FAKE, df=FAKE):
        return lib.vqf_glimpse_pool_bwd_packed_dfeat(dp, dwx, feat, wts, idx, order, grp_off, roff, N, U, R, S, C, G, 0, dl, df, None)

    for f in (fwd, bwd, dfeat):
        assert f(roff=None) == BADARG and f(roff=FAKE + 2) == BADARG             # a null or misaligned roff
        assert f(R=0) == BADARG and f(R=-4) == BADARG
        assert f(U=3) == BADARG                                                  # the plain form: U must equal N
        assert f(S=1025) == UNSUPPORTED and f(G=4) == UNSUPPORTED
    for f in (fwd, bwd):                                                         # (the pooling has no bound on R: 64-bit row addresses)
        assert f(R=1 << 29) == UNSUPPORTED
        assert f(E=1056) == UNSUPPORTED and f(E=48) == UNSUPPORTED and f(N=65536, U=65536) == UNSUPPORTED
        assert f(xh=None) == BADARG and f(w=None) == BADARG
        assert f(xh=FAKE + 4) == ALIGN and f(gp=FAKE + 4) == ALIGN and f(w=FAKE + 8) == ALIGN
        # the query agrees with the calls
        for dims in ((2, 2, 1 << 29, 3, 32, 1), (2, 2, 5, 3, 1056, 1), (2, 2, 5, 1025, 32, 1), (2, 2, 5, 3, 32, 4)):
            assert lib.vqf_guided_logits_packed_supported(*dims) == 0
            assert f(N=dims[0], U=dims[1], R=dims[2], S=dims[3], E=dims[4], G=dims[5]) == UNSUPPORTED
    assert fwd(out=None) == BADARG and fwd(ldx=30) == BADARG and fwd(ldx=34) == BADARG
    assert fwd(idx=FAKE + 2, U=3) == BADARG                                      # a misaligned idx
    # the backward: exactly one of order / grp_off is an argument error; so are misaligned ones and a grouped call without gp
    assert bwd(order=FAKE, U=3) == BADARG and bwd(grp_off=FAKE, U=3) == BADARG
    assert bwd(order=FAKE + 2, grp_off=FAKE, U=3) == BADARG and bwd(order=FAKE, grp_off=FAKE + 2, U=3) == BADARG
    assert bwd(order=FAKE, grp_off=FAKE, gp=None, U=3) == BADARG
    assert bwd(dl=None) == BADARG and bwd(dxh=None) == BADARG and bwd(dgp=None) == BADARG and bwd(dw=None) == BADARG
    assert bwd(dxh=FAKE + 4) == ALIGN and bwd(dgp=FAKE + 4) == ALIGN and bwd(ws=FAKE + 4) == ALIGN
    assert bwd(ws=None) == WORKSPACE and bwd(wsb=16) == WORKSPACE
    assert bwd(order=FAKE, grp_off=FAKE, U=3, wsb=lib.vqf_guided_logits_bwd_packed_ws_bytes(2, 3, 3, 32, 1) - 1) == WORKSPACE
    # the pooling backward with dfeat
    assert dfeat(df=None) == BADARG
    assert dfeat(idx=FAKE, U=3) == BADARG and dfeat(idx=FAKE, order=FAKE, U=3) == BADARG and dfeat(idx=FAKE, grp_off=FAKE, U=3) == BADARG
    assert dfeat(order=FAKE, grp_off=FAKE) == BADARG                             # order / grp_off without idx
    assert dfeat(idx=FAKE, order=FAKE + 2, grp_off=FAKE, U=3) == BADARG
    assert dfeat(C=30) == UNSUPPORTED and dfeat(N=65536, U=65536) == UNSUPPORTED
    assert dfeat(dp=FAKE + 4) == ALIGN and dfeat(feat=FAKE + 4) == ALIGN and dfeat(df=FAKE + 8) == ALIGN
    # the packed tanh / dropout pass: the range and codes of the unpack forms
    tf = lambda z=FAKE, roff=FAKE, keep=None, p=0.0, U=2, R=5, L=3, E=8, y=FAKE: \
        lib.vqf_tanh_dropout_packed_fwd(z, roff, keep, 0, p, U, R, L, E, y, None)
    tb = lambda dy=FAKE, y=FAKE, roff=FAKE, keep=None, p=0.0, U=2, R=5, L=3, E=8, dz=FAKE: \
        lib.vqf_tanh_dropout_packed_bwd(dy, y, roff, keep, 0, p, U, R, L, E, dz, None)
    for f in (tf, tb):
        assert f(roff=None) == BADARG and f(roff=FAKE + 2) == BADARG and f(R=0) == BADARG and f(p=1.0) == BADARG
        assert f(E=6) == UNSUPPORTED and f(L=1025) == UNSUPPORTED and f(U=65536) == UNSUPPORTED and f(R=1 << 29) == UNSUPPORTED
        assert f(keep=FAKE + 2) == ALIGN
    assert tf(z=None) == BADARG and tf(y=FAKE + 8) == ALIGN and tb(y=None) == BADARG and tb(dz=FAKE + 8) == ALIGN
    # the wrappers refuse what they are handed before any pointer is taken
    with pytest.raises(vqa.VqfError, match="GPU tensors"):
        vqa.ops.tanh_dropout_packed_fwd(torch.zeros(5, 8), torch.zeros(3, dtype=torch.int32), 2, 3)
    with pytest.raises(vqa.VqfError):
        vqa.ops.guided_logits_fwd_packed(torch.zeros(5, 32), None, torch.zeros(1, 32), torch.zeros(3, dtype=torch.int32), 2, 3)
