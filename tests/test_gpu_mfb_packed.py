"""MFB / MHBCoAtt on packed region features (forward(PackedRegions(rows, offsets, max_regions), ...)) on the GPU.

Kernel level: vqf_mfb_fuse_*_packed / *_grouped_packed and vqf_glimpse_pool_*_packed are instantiations of the *_len kernels that
address P / dP / feat through row offsets, so on the shapes, operands and masks of tests/test_gpu_mfb_regions.py they must give the
BITS of the *_len / *_grouped_len entry points on the padded copy (the same operations in the same order: no tolerance); against
the fp64 restatement mfb_regions_ref.fuse_ref the margins are those of test_gpu_mfb_regions.test_mfb_fuse_len_fwd_bwd on these very
operands (1e-5 forward, 2e-5 backward).  Sentinel rows around P / dP and offsets that the kernels have to clamp show that nothing
outside the R rows is read or written.
Model level: the operands, the fp64 oracle (computed once, shared through that module's cache) and the MODEL_RUNS matrix of
tests/test_gpu_mfb_regions.py; output 1e-4, gradients golden_util.grad_parity.
"""
import warnings

import pytest
import torch

import recipe
import mfb_regions_ref as RR
import mfb_packed_ref as PR
import test_gpu_mfb_regions as TR
from cases import MHBCOATT_CASES, make_cfg
from golden_util import rel_err, grad_parity

pytestmark = pytest.mark.gpu

P_DROP = TR.P_DROP
KERNEL_SHAPES = TR.KERNEL_SHAPES
MASKS = ["keep_p0.1", "philox_p0.1", "no_dropout"]


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def ops(vqa):
    return vqa.ops


@pytest.fixture(scope="module")
def grouping(vqa):
    import importlib
    return importlib.import_module(vqa.__name__ + ".host.grouping")


def _i32(x):
    return torch.as_tensor(x).to(torch.int32).cuda()


def _setup(ops, grouping, U, N, L, O_, index, counts, mask):
    """the operands of test_gpu_mfb_regions on the GPU, padded and packed; the mask's keyword arguments and its fp64 keep mask"""
    c = TR._operands(U, N, L, O_, index, counts)
    cu = lambda t: t.float().cuda()
    c.update(gP=cu(c["P"]), gpb=cu(c["pb"]), gq=cu(c["q"]), grp=None if U is None else grouping._group_index(c["idx"].cuda(), U))
    owners = N if U is None else U
    c["owners"] = owners
    c["gPp"] = PR.pack_rows(c["gP"].view(owners, L, 5 * O_), c["lens_u"])           # the real rows of the padded P
    c["roff"] = _i32(PR.offsets_of(c["lens_u"]))
    c["gdY"] = cu(c["dY"])
    lq, lu = _i32(c["lens_q"]), _i32(c["lens_u"])
    c["lens"] = lq if U is None else (lq, lu)
    if mask == "keep_p0.1":
        kw, keep64 = dict(keep=c["keep"].cuda(), p_drop=P_DROP), c["keep"]
    elif mask == "philox_p0.1":
        kw = dict(seed=4321, p_drop=P_DROP)
        Pg = c["gP"] if U is None else c["gP"].view(U, L, -1)[c["grp"][0].long()].reshape(N * L, -1).contiguous()
        keep64 = (ops.mfb_fuse_fwd(Pg, c["gq"], N, L, O_, pbias=c["gpb"], want_zdrop=True, **kw)[3] != 0).to(torch.uint8).cpu()
    else:
        kw, keep64 = dict(), None
    return c, kw, keep64


def _fwd_packed(ops, c, N, L, O_, P=None, roff=None, normalise=True, **kw):
    return ops.mfb_fuse_fwd_packed(c["gPp"] if P is None else P, c["gq"], c["roff"] if roff is None else roff, N, L, O_,
                                   idx=None if c["grp"] is None else c["grp"][0], pbias=c["gpb"], normalise=normalise, **kw)


def _bwd_packed(ops, c, N, L, O_, Y, norm, inv, want_dbias=True, **kw):
    return ops.mfb_fuse_bwd_packed(c["gdY"], Y, norm, inv, c["gPp"], c["gq"], c["roff"], N, L, O_, grp=c["grp"], pbias=c["gpb"],
                                   want_dbias=want_dbias, **kw)


def _abi_fwd(ops, c, U, N, L, O_, kw, packed, P, offs_or_lens, R=None):
    """R and rowssq themselves through the C ABI -> (Rout, rowssq); packed: offs_or_lens = roff, else lens (lens_q, lens_u)"""
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    keep_p = None if "keep" not in kw else ptr(kw["keep"])
    seed, p = kw.get("seed", 0), kw.get("p_drop", 0.0)
    out, ssq = torch.full((N * L, O_), 7.0, device="cuda"), torch.full((N * L * 4,), 7.0, device="cuda")
    Pp = P if isinstance(P, int) else ptr(P)
    if packed and U is None:
        rc = lib.vqf_mfb_fuse_fwd_packed(Pp, ptr(c["gpb"]), ptr(c["gq"]), ptr(offs_or_lens), keep_p, seed, p, N, R, L, O_, ptr(out), ptr(ssq), st)
    elif packed:
        rc = lib.vqf_mfb_fuse_fwd_grouped_packed(Pp, ptr(c["gpb"]), ptr(c["gq"]), ptr(c["grp"][0]), ptr(offs_or_lens), keep_p, seed, p, N, U, R,
                                                 L, O_, ptr(out), ptr(ssq), st)
    elif U is None:
        rc = lib.vqf_mfb_fuse_fwd_len(Pp, ptr(c["gpb"]), ptr(c["gq"]), ptr(offs_or_lens), keep_p, seed, p, N, L, O_, ptr(out), ptr(ssq), st)
    else:
        rc = lib.vqf_mfb_fuse_fwd_grouped_len(Pp, ptr(c["gpb"]), ptr(c["gq"]), ptr(c["grp"][0]), ptr(offs_or_lens[0]), ptr(offs_or_lens[1]), keep_p,
                                              seed, p, N, U, L, O_, ptr(out), ptr(ssq), st)
    assert rc == 0
    torch.cuda.synchronize()
    return out, ssq


def _abi_bwd(ops, c, U, N, L, O_, kw, packed, Y, inv, P, dP, offs_or_lens, R=None):
    """the backward through the C ABI with given coefficients (no rowdot pass in front) -> (dq, db); dP is written in place"""
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    keep_p = None if "keep" not in kw else ptr(kw["keep"])
    seed, p = kw.get("seed", 0), kw.get("p_drop", 0.0)
    cA, cB = TR._pos((N,), 170).float().cuda(), TR._rand((N,), 171, 0.1).float().cuda()
    dq, db = torch.full((N, 5 * O_), 7.0, device="cuda"), torch.full((5 * O_,), 7.0, device="cuda")
    head = (ptr(c["gdY"]), ptr(Y), ptr(inv), ptr(cA), ptr(cB), P if isinstance(P, int) else ptr(P), ptr(c["gpb"]), ptr(c["gq"]))
    dPp = dP if isinstance(dP, int) else ptr(dP)
    if U is None:
        ws = ops.workspace(Y.device, lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O_))
        if packed:
            rc = lib.vqf_mfb_fuse_bwd_packed(*head, ptr(offs_or_lens), keep_p, seed, p, N, R, L, O_, dPp, ptr(dq), ptr(db), ptr(ws), ws.numel(), st)
        else:
            rc = lib.vqf_mfb_fuse_bwd_len(*head, ptr(offs_or_lens), keep_p, seed, p, N, L, O_, dPp, ptr(dq), ptr(db), ptr(ws), ws.numel(), st)
    else:
        g = c["grp"]
        ws = ops.workspace(Y.device, lib.vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O_))
        if packed:
            rc = lib.vqf_mfb_fuse_bwd_grouped_packed(*head, ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(offs_or_lens), keep_p, seed, p, N, U, R, L, O_,
                                                     dPp, ptr(dq), ptr(db), ptr(ws), ws.numel(), st)
        else:
            rc = lib.vqf_mfb_fuse_bwd_grouped_len(*head, ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(offs_or_lens[0]), ptr(offs_or_lens[1]), keep_p, seed,
                                                  p, N, U, L, O_, dPp, ptr(dq), ptr(db), ptr(ws), ws.numel(), st)
    assert rc == 0
    torch.cuda.synchronize()
    return dq, db


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("U,N,L,O_,index,counts", KERNEL_SHAPES)
def test_packed_fuse_gives_the_bits_of_the_len_forms(ops, grouping, U, N, L, O_, index, counts, mask):
    """fp64 errors measured on an MI355X (profiles/mfb_packed_parity.txt): forward <= 2.0e-7, backward <= 3.1e-7 over every shape and
    mask, against the margins 1e-5 / 2e-5."""
    c, kw, keep64 = _setup(ops, grouping, U, N, L, O_, index, counts, mask)
    owners, W5 = c["owners"], 5 * O_
    Rtot = c["gPp"].shape[0]
    assert Rtot == sum(counts)
    # ---- forward: Y / norm / inv with normalise both ways, then R and rowssq through the C ABI
    for normalise in (True, False):
        a = _fwd_packed(ops, c, N, L, O_, normalise=normalise, **kw)
        b = TR._fwd(ops, c, U, N, L, O_, c["lens"], normalise=normalise, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), normalise
    Y, norm, inv = _fwd_packed(ops, c, N, L, O_, **kw)
    Rp, sp = _abi_fwd(ops, c, U, N, L, O_, kw, True, c["gPp"], c["roff"], Rtot)
    Rl, sl = _abi_fwd(ops, c, U, N, L, O_, kw, False, c["gP"], c["lens"])
    assert torch.equal(Rp, Rl) and torch.equal(sp, sl)
    pad_q = ~RR.valid_mask(c["lens_q"], L).cuda()
    assert float(Rp.view(N, L, O_)[pad_q].abs().sum()) == 0.0 and float(sp.view(N, L, 4)[pad_q].abs().sum()) == 0.0
    # ---- backward
    dP, dq, db = _bwd_packed(ops, c, N, L, O_, Y, norm, inv, **kw)
    dPl, dql, dbl = TR._bwd(ops, c, U, N, L, O_, c["lens"], c["gdY"], Y, norm, inv, **kw)
    assert tuple(dP.shape) == (Rtot, W5)
    assert torch.equal(dP, PR.pack_rows(dPl.view(owners, L, W5), c["lens_u"]))       # the real rows of the padded dP
    assert torch.equal(dq, dql) and torch.equal(db, dbl)
    if U is not None:
        off = PR.offsets_of(c["lens_u"]).tolist()
        for u in range(U):
            if u not in index:
                assert float(dP[off[u]:off[u + 1]].abs().max()) == 0.0            # exact zeros for an image without a question
    dP2, dq2, db2 = _bwd_packed(ops, c, N, L, O_, Y, norm, inv, **kw)
    assert torch.equal(dP, dP2) and torch.equal(dq, dq2) and torch.equal(db, db2)    # a second run: the same bits
    dP3, dq3, db3 = _bwd_packed(ops, c, N, L, O_, Y, norm, inv, want_dbias=False, **kw)
    assert db3 is None and torch.equal(dP, dP3) and torch.equal(dq, dq3)
    Y2, norm2, inv2 = _fwd_packed(ops, c, N, L, O_, **kw)
    assert torch.equal(Y, Y2) and torch.equal(norm, norm2) and torch.equal(inv, inv2)
    # ---- fp64, on the unpacked operands
    ref = TR._reference(U, N, L, O_, index, counts, keep64, mask)
    e_f = (TR._rel(Y, ref["Y"]), TR._rel(norm, ref["norm"]))
    dP64 = PR.pack_rows(ref["dP"].view(owners, L, W5), c["lens_u"])
    e_b = (TR._rel(dP, dP64), TR._rel(dq, ref["dq"]), TR._rel(db, ref["db"]))
    print("packed %s N%d L%d O%d %s  fwd: Y %.2e norm %.2e | bwd: dP %.2e dq %.2e dbias %.2e"
          % ("plain" if U is None else "U%d" % U, N, L, O_, mask, *e_f, *e_b))
    assert max(e_f) <= 1e-5
    assert max(e_b) <= 2e-5


@pytest.mark.parametrize("U,N,L,O_,index,counts", KERNEL_SHAPES)
def test_packed_fuse_touches_nothing_outside_its_rows(ops, grouping, U, N, L, O_, index, counts):
    """P and dP with one sentinel row before and one after the R rows: a NaN in the sentinel rows of P reaches no output and the
    sentinel rows of dP stay as they were."""
    c, kw, _ = _setup(ops, grouping, U, N, L, O_, index, counts, "keep_p0.1")
    W5, Rtot = 5 * O_, c["gPp"].shape[0]
    Pg = torch.full((Rtot + 2, W5), float("nan"), device="cuda")
    Pg[1:-1] = c["gPp"]
    dPg = torch.full((Rtot + 2, W5), 7.0, device="cuda")
    inner = lambda t: t.data_ptr() + W5 * 4                                       # (a row is a multiple of 16 bytes)
    Rp, sp = _abi_fwd(ops, c, U, N, L, O_, kw, True, inner(Pg), c["roff"], Rtot)
    R0, s0 = _abi_fwd(ops, c, U, N, L, O_, kw, True, c["gPp"], c["roff"], Rtot)
    assert torch.equal(Rp, R0) and torch.equal(sp, s0) and bool(torch.isfinite(Rp).all()) and bool(torch.isfinite(sp).all())
    inv = TR._pos((N,), 172).float().cuda()
    dq, db = _abi_bwd(ops, c, U, N, L, O_, kw, True, R0, inv, inner(Pg), inner(dPg), c["roff"], Rtot)
    dP0 = torch.full((Rtot, W5), 7.0, device="cuda")
    dq0, db0 = _abi_bwd(ops, c, U, N, L, O_, kw, True, R0, inv, c["gPp"], dP0, c["roff"], Rtot)
    assert torch.equal(dPg[0], torch.full_like(dPg[0], 7.0)) and torch.equal(dPg[-1], torch.full_like(dPg[-1], 7.0))
    assert torch.equal(dPg[1:-1], dP0) and torch.equal(dq, dq0) and torch.equal(db, db0)
    assert all(bool(torch.isfinite(t).all()) for t in (dPg, dq, db))
    assert float(dP0.abs().max()) > 0.0 and not bool((dP0 == 7.0).all(1).any())     # every one of the R rows was written


@pytest.mark.parametrize("U,N,L,O_,index,counts", KERNEL_SHAPES)
def test_packed_fuse_clamps_what_the_offsets_hold(ops, grouping, U, N, L, O_, index, counts):
    """Offsets inside [0, R] with a count of 0 and a count above L on owners other than the last: the outputs are those of the *_len
    forms with the clamped counts at the same start rows (dP: on the rows exactly one owner has; a row two owners share is written by
    both, a row none has is not written)."""
    c, kw, _ = _setup(ops, grouping, U, N, L, O_, index, counts, "keep_p0.1")
    owners, W5 = c["owners"], 5 * O_
    anomalies = [[(0, 0), (1, L + 2)]] if owners >= 3 else [[(0, 0)], [(0, L + 2)]]
    for anomaly in anomalies:
        cnts = list(counts)
        for s, v in anomaly:
            cnts[s] = v
        off = PR.offsets_of(cnts)
        Rtot = int(off[-1])
        Pk = TR._pos((Rtot, W5), 160).float().cuda()
        spans = PR.clamped_spans(off, Rtot, L)
        # the padded copy: owner s holds the packed rows start .. start + cnt - 1
        Pl = torch.full((owners, L, W5), 3.0, device="cuda")
        for s, (st, cn) in enumerate(spans):
            Pl[s, :cn] = Pk[st:st + cn]
        Pl = Pl.view(owners * L, W5)
        lu = torch.tensor([cn for _, cn in spans])
        lens = _i32(lu) if U is None else (_i32(lu[c["idx"]]), _i32(lu))
        roff = _i32(off)
        Rp, sp = _abi_fwd(ops, c, U, N, L, O_, kw, True, Pk, roff, Rtot)
        Rl, sl = _abi_fwd(ops, c, U, N, L, O_, kw, False, Pl, lens)
        assert torch.equal(Rp, Rl) and torch.equal(sp, sl)
        inv = TR._pos((N,), 172).float().cuda()
        dPk, dPl = torch.full((Rtot, W5), 7.0, device="cuda"), torch.full((owners * L, W5), 7.0, device="cuda")
        dq, db = _abi_bwd(ops, c, U, N, L, O_, kw, True, Rp, inv, Pk, dPk, roff, Rtot)
        dql, dbl = _abi_bwd(ops, c, U, N, L, O_, kw, False, Rl, inv, Pl, dPl, lens)
        assert torch.equal(dq, dql) and torch.equal(db, dbl)
        have = torch.zeros(Rtot, dtype=torch.int64)
        for st, cn in spans:
            have[st:st + cn] += 1
        dPl = dPl.view(owners, L, W5)
        for s, (st, cn) in enumerate(spans):
            for l in range(cn):
                if int(have[st + l]) == 1:
                    assert torch.equal(dPk[st + l], dPl[s, l]), (s, l)
        none = (have == 0).cuda()
        assert torch.equal(dPk[none], torch.full_like(dPk[none], 7.0))


# ---- glimpse pooling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["per_sample", "idx"])
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "live"])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("N,S,C,counts", [(3, 20, 96, [7, 20, 1]), (2, 100, 2048, [37, 100]), (4, 1, 8, [1, 1, 1, 1])],
                         ids=["N3_S20_C96", "N2_S100_C2048", "N4_S1_C8"])
def test_packed_glimpse_pool_gives_the_bits_of_the_len_forms(ops, N, S, C, counts, G, unit, shared):
    U = N
    feat = TR._rand((U, S, C), 301).float().cuda()                                # the padded copy (finite values in the padding)
    logits = TR._rand((N * S, G), 302, 3.0).float().cuda()
    dpooled = TR._rand((N, G * C), 303).float().cuda()
    cu = torch.tensor(counts)
    idx = torch.tensor([N - 1, 0, 0, N - 1][:N]) if shared else None
    rows = PR.pack_rows(feat, cu)
    roff = _i32(PR.offsets_of(cu))
    lens_q = _i32(cu if idx is None else cu[idx])
    gidx = None if idx is None else _i32(idx)
    featq = feat if idx is None else feat[idx.cuda()].contiguous()                 # what each question pools
    wts, pooled = ops.glimpse_pool_fwd_packed(rows, logits, roff, N, S, unit, idx=gidx)
    wl, pl = ops.glimpse_pool_fwd(featq, logits, unit, lens=lens_q)
    assert torch.equal(wts, wl) and torch.equal(pooled, pl)
    pad = ~RR.valid_mask(cu if idx is None else cu[idx], S).cuda()                # (N, S)
    assert float(wts.permute(0, 2, 1)[pad].abs().sum()) == 0.0
    dl = ops.glimpse_pool_bwd_packed(dpooled, rows, wts, roff, unit, idx=gidx)
    dll, _ = ops.glimpse_pool_bwd(dpooled, featq, wl, unit, False, lens=lens_q)
    assert torch.equal(dl, dll)
    assert float(dl.view(N, S, G)[pad].abs().sum()) == 0.0
    if shared and not unit:                                                        # the grouped entry points themselves
        wg, pg = ops.glimpse_pool_fwd_grouped(feat, logits, gidx, lens=lens_q)
        assert torch.equal(wts, wg) and torch.equal(pooled, pg)
        order = torch.sort(idx, stable=True).indices
        grp_off = PR.offsets_of(torch.bincount(idx, minlength=U))
        dlg, _ = ops.glimpse_pool_bwd_grouped(dpooled, feat, wg, gidx, _i32(order), _i32(grp_off), False, lens=lens_q)
        assert torch.equal(dl, dlg)
    # sentinel rows around feat: NaN there reaches nothing
    guard = torch.full((rows.shape[0] + 2, C), float("nan"), device="cuda")
    guard[1:-1] = rows
    w2, p2 = ops.glimpse_pool_fwd_packed(guard[1:-1], logits, roff, N, S, unit, idx=gidx)
    assert torch.equal(w2, wts) and torch.equal(p2, pooled)
    assert torch.equal(ops.glimpse_pool_bwd_packed(dpooled, guard[1:-1], wts, roff, unit, idx=gidx), dl)


def test_packed_entry_points_return_the_stated_error_codes(vqa, ops, grouping):
    U, N, L, O_, R = 3, 7, 5, 8, 9
    z = lambda *s: torch.zeros(s, device="cuda")
    i32, order, off = grouping._group_index(torch.tensor([2, 0, 0, 2, 0, 2, 0]).cuda(), U)
    rq, ru = _i32([0, 1, 2, 3, 4, 5, 7, 9]), _i32([0, 1, 4, 9])
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    P, q, Rout, ssq = z(R, 5 * O_), z(N, 5 * O_), z(N * L, O_), z(N * L * 4)
    odd = _i32([0] + [0, 1, 2, 3, 4, 5, 7, 9])[1:]                  # 4-byte aligned; + 2 bytes below is not
    BADARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    assert lib.vqf_mfb_fuse_fwd_packed(ptr(P), None, ptr(q), None, None, 0, 0.0, N, R, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_packed(ptr(P), None, ptr(q), odd.data_ptr() + 2, None, 0, 0.0, N, R, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_packed(ptr(P), None, ptr(q), ptr(odd), None, 0, 0.0, N, 0, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_packed(ptr(P), None, ptr(q), ptr(odd), None, 0, 0.0, N, R, 1025, O_, ptr(Rout), ptr(ssq), st) == UNSUPPORTED
    assert lib.vqf_mfb_fuse_fwd_packed(ptr(P), None, ptr(q), ptr(odd), None, 0, 0.0, N, R, L, O_, ptr(Rout), ptr(ssq), st) == 0
    assert lib.vqf_mfb_fuse_fwd_grouped_packed(ptr(P), None, ptr(q), ptr(i32), None, None, 0, 0.0, N, U, R, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_grouped_packed(ptr(P), None, ptr(q), None, ptr(ru), None, 0, 0.0, N, U, R, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_grouped_packed(ptr(P), None, ptr(q), ptr(i32), ptr(ru), None, 0, 0.0, N, U, R, L, O_, ptr(Rout), ptr(ssq), st) == 0
    one, dq, ws, dP = z(N), z(N, 5 * O_), z(1 << 16), z(R, 5 * O_)
    head = (ptr(Rout), ptr(Rout), ptr(one), ptr(one), ptr(one), ptr(P), None, ptr(q))
    assert lib.vqf_mfb_fuse_bwd_packed(*head, None, None, 0, 0.0, N, R, L, O_, ptr(dP), ptr(dq), None, ptr(ws), ws.numel() * 4, st) == BADARG
    assert lib.vqf_mfb_fuse_bwd_packed(*head, ptr(rq), None, 0, 0.0, N, R, L, O_, ptr(dP), ptr(dq), None, ptr(ws), ws.numel() * 4, st) == 0
    need = lib.vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O_)
    assert 0 < need <= ws.numel() * 4
    g = head + (ptr(i32), ptr(order), ptr(off))
    tail = (None, 0, 0.0, N, U, R, L, O_, ptr(dP), ptr(dq), None, ptr(ws))
    assert lib.vqf_mfb_fuse_bwd_grouped_packed(*g, None, *tail, ws.numel() * 4, st) == BADARG
    assert lib.vqf_mfb_fuse_bwd_grouped_packed(*g, ptr(ru), *tail, need - 4, st) == WORKSPACE
    assert lib.vqf_mfb_fuse_bwd_grouped_packed(*g, ptr(ru), *tail, need, st) == 0
    torch.cuda.synchronize()
    # the wrappers: type, shape and device of roff
    for bad in (rq.long(), rq.cpu(), rq[:5], rq.float()):
        with pytest.raises(vqa.VqfError, match="roff"):
            ops.mfb_fuse_fwd_packed(P, q, bad, N, L, O_)
    with pytest.raises(vqa.VqfError, match="roff"):
        ops.glimpse_pool_fwd_packed(z(R, 8), z(N * L, 2), ru, N, L, False)
    with pytest.raises(vqa.VqfError):
        ops.mfb_fuse_fwd_packed(P.to(torch.bfloat16), q, rq, N, L, O_)


# ---- model level -------------------------------------------------------------------------------------------------------------------
def _packed(vqa, img, counts):
    """the PackedRegions of the padded batch (img (U, L, D), counts (U,) on the GPU)"""
    return vqa.PackedRegions(PR.pack_rows(img, counts.cpu()), PR.offsets_of(counts), img.shape[1])


@pytest.mark.parametrize("case,mhb,shared,attrs,live", TR.MODEL_RUNS)
def test_model_on_packed_regions_matches_the_masked_reference(vqa, case, mhb, shared, attrs, live):
    model, img, counts, q, tgt, idx = TR._model(vqa, case, mhb, shared, **attrs)
    packed = _packed(vqa, img, counts)
    kw = {} if idx is None else dict(img_index=idx)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out, grads = TR._step(model, mhb, packed, q, tgt, **kw)
    # no torch fallback on the packed path (MHBCoAtt's question LSTM at this hidden width is nn.LSTM whatever the image side is)
    assert not [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning) and "LSTM" not in str(w.message)]
    o_out, g32, g64 = TR._oracle(case, mhb, shared, live)
    err = rel_err(out.cpu().numpy(), o_out.numpy())
    print("packed output rel err %.2e" % err)
    assert out.shape[0] == q.shape[0]
    assert err <= 1e-4
    grad_parity(grads, g32, g64, label="packed %s %s%s" % (case["name"], attrs, " img_index" if shared else ""))
    if live or mhb:
        assert float(grads["img_conv1d.weight"].abs().max()) > 0.0
    # int32 offsets are the same call; a second step gives the same bits
    p32 = vqa.PackedRegions(packed.rows, packed.offsets.to(torch.int32), packed.max_regions)
    out32, grads32 = TR._step(model, mhb, p32, q, tgt, **kw)
    assert torch.equal(out, out32) and all(torch.equal(grads[k], grads32[k]) for k in grads)
    # against the pair call on the unpacked batch (the projection GEMM may route differently at another M: no bit identity)
    uimg, ulen = packed.unpack()
    assert torch.equal(ulen, counts) and torch.equal(uimg, torch.where(RR.valid_mask(counts.cpu(), img.shape[1]).cuda()[:, :, None], img,
                                                                         torch.zeros_like(img)))
    outp, _ = TR._step(model, mhb, uimg, q, tgt, img_length=ulen, **kw)
    e2 = rel_err(out.cpu().numpy(), outp.cpu().numpy())
    print("packed vs pair rel err %.2e" % e2)
    assert e2 <= 1e-4
    # a wider max_regions only adds zero rows to what stays padded (the masks are per (n, l): eval mode, no dropout)
    model.set_keep_masks()
    model.eval()
    with torch.no_grad():
        a = model.forward(packed, q, **kw)
        b = model.forward(vqa.PackedRegions(packed.rows, packed.offsets, packed.max_regions + 5), q, **kw)
        cc = model.forward((uimg, ulen), q, **kw)
    assert rel_err(b.cpu().numpy(), a.cpu().numpy()) <= 1e-4 and rel_err(a.cpu().numpy(), cc.cpu().numpy()) <= 1e-4


@pytest.mark.parametrize("mhb,shared,attrs", [(False, False, {}), (False, True, dict(unit_softmax=False)), (True, False, {}), (True, True, {})],
                         ids=["mfb", "mfb_live_img_index", "mhbcoatt", "mhbcoatt_img_index"])
def test_eval_mode_on_packed_regions_matches_the_masked_reference(vqa, mhb, shared, attrs):
    """eval mode (no dropout) against the fp64 restatement without masks; predict() forwards the PackedRegions as it is"""
    case = TR.MHB3 if mhb else TR.MFB3
    model, img, counts, q, tgt, idx = TR._model(vqa, case, mhb, shared, **attrs)
    model.set_keep_masks()
    model.eval()
    packed = _packed(vqa, img, counts)
    kw = {} if idx is None else dict(img_index=idx)
    with torch.no_grad():
        a = model.forward(packed, q, **kw)
    cfg = make_cfg(case)
    from golden_util import recipe_sd
    from oracle import ref_torch as O
    sd = {k: v.double() for k, v in recipe_sd(O.mfb_shapes(cfg, mhb=mhb), case["salt"]).items()}
    im, cn = img.cpu().double(), counts.cpu()
    if shared:
        im, cn = im[torch.tensor(TR.INDEX)], cn[torch.tensor(TR.INDEX)]
    if mhb:
        ref = RR.mhbcoatt_forward(sd, cfg, im, q.cpu(), cn)
    else:
        ref = RR.mfb_forward(sd, cfg, im, q.cpu(), cn, live_softmax=not attrs.get("unit_softmax", True))
    err = rel_err(a.cpu().numpy(), ref.float().numpy())
    print("packed eval rel err %.2e" % err)
    assert err <= 1e-4
    ids, probs = vqa.predict(model, packed, q, **kw)
    assert torch.equal(ids[:, 0], a.argmax(1)) and not model.training


@pytest.mark.parametrize("shared", [False, True], ids=["per_sample", "img_index"])
def test_pruned_mfb_on_packed_regions_is_bit_identical_to_faithful(vqa, shared):
    res = []
    for pruned in (False, True):
        model, img, counts, q, tgt, idx = TR._model(vqa, TR.MFB3, False, shared, pruned=pruned)
        kw = {} if idx is None else dict(img_index=idx)
        res.append(TR._step(model, False, _packed(vqa, img, counts), q, tgt, **kw))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_packed_path_allocates_no_padded_projection(vqa):
    """N = 64, L = 20, every count 2, Philox dropout: peak memory over forward + backward of MHBCoAtt.  The pair call holds P and dP,
    two (N*L, 5000) fp32 tensors; the packed call holds R/(N*L) of that, so it must be lower by at least one P's worth of padding."""
    case = dict(MHBCOATT_CASES[1], N=64, name="mem_packed_n64")
    cfg = make_cfg(case)
    N, L, D = 64, cfg.img_feature_dim, cfg.img_feature_channel
    assert L == 20
    model = vqa.MHBCoAtt(cfg)
    sd = {k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"])) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model = model.cuda().train()
    counts = torch.full((N,), 2, dtype=torch.int64, device="cuda")
    img = torch.from_numpy(recipe.img_features(N, L, D, case["salt"])).cuda()
    img[:, 2:] = 0.0
    packed = _packed(vqa, img, counts)
    R = packed.rows.shape[0]
    assert R == 2 * N
    q = torch.from_numpy(recipe.question_tokens(N, case["T"], cfg.q_vocab_size, case["salt"])).cuda()
    soft = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, case["salt"])).cuda()
    peak = {}
    for form in ("pair", "packed", "pair", "packed"):                  # twice: workspaces and streams exist from the first round on
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(3)
        out = model.forward(packed, q) if form == "packed" else model.forward((img, counts), q)
        torch.nn.KLDivLoss()(out, soft).backward()
        torch.cuda.synchronize()
        peak[form] = torch.cuda.max_memory_allocated() - base
        del out
    one = (N * L - R) * 5000 * 4
    print("peak bytes above the baseline: pair %d, packed %d, the padding of one P %d" % (peak["pair"], peak["packed"], one))
    assert peak["packed"] <= peak["pair"] - one
