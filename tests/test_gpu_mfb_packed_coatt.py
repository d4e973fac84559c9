"""MFB / MHBCoAtt packed_coatt (the co-attention head on the packed rows) on the GPU.

Kernel level: vqf_mfb_fuse_*_packed_rows, vqf_l2_*_packed and vqf_glimpse_pool_*_packed_rows are instantiations (or lane-for-lane
restatements) of their *_packed siblings that put the per-(image, region) rows at start + l instead of n L + l, so on the same
operands and masks they must give that sibling's BITS (row-wise outputs: its real rows) -- torch.equal, no tolerance.  Every output
is written between guard rows of a sentinel value, on valid offsets and on the malformed ones of
test_gpu_mfb_packed.test_packed_fuse_clamps_what_the_offsets_hold; the guards must come back untouched.
Model level: the operands, the fp64 oracle and the un-shared entries of MODEL_RUNS of tests/test_gpu_mfb_regions.py (plus MFB's
faithful form with fold_norm off); output 1e-4 against the oracle and against packed_coatt = False in the same process, gradients
golden_util.grad_parity.  Structure: no GEMM of a step has M or K = N L, co_att_conv1's three products have R rows.
"""
import warnings

import pytest
import torch

import recipe
import mfb_regions_ref as RR
import mfb_packed_ref as PR
import test_gpu_mfb_regions as TR
import test_gpu_mfb_packed as TP
from cases import make_cfg
from golden_util import recipe_sd, rel_err, grad_parity
from oracle import ref_torch as O

pytestmark = pytest.mark.gpu

SENT = 7.0
PLAIN_SHAPES = [p for p in TR.KERNEL_SHAPES if p.values[0] is None]          # the un-grouped entries
assert [p.id for p in PLAIN_SHAPES] == ["N5_L20_counts_1_L_Lm1_odd", "N3_L196_count_below_LS16", "N6_L3_O8_two_active_lanes", "N2_L1"]
MASKS = TP.MASKS


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


def _guarded(rows, width, g=4):
    """(buffer, inner view): `rows` rows of `width` floats between g guard rows of SENT on either side (the inner view stays 16-byte
    aligned: g * width * 4 bytes with g = 4)"""
    buf = torch.full((rows + 2 * g, width), SENT, device="cuda")
    return buf, buf[g:rows + g]


def _untouched(buf, rows, g=4):
    return bool((buf[:g] == SENT).all()) and bool((buf[rows + g:] == SENT).all())


def _mask_args(ops, kw):
    return (None if "keep" not in kw else ops._ptr(kw["keep"])), kw.get("seed", 0), kw.get("p_drop", 0.0)


def _rows_fwd_abi(ops, c, N, L, O_, kw, P, roff, R):
    """vqf_mfb_fuse_fwd_packed_rows + vqf_l2_group_norm_packed through the C ABI, every output between guards
    -> dict(R (R, O), ssq (R, 4), norm (N), inv (N), rowinv (R)) and the guard verdict"""
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    keep_p, seed, p = _mask_args(ops, kw)
    ob, out = _guarded(R, O_)
    sb, ssq = _guarded(R, 4)
    assert lib.vqf_mfb_fuse_fwd_packed_rows(ptr(P), ptr(c["gpb"]), ptr(c["gq"]), ptr(roff), keep_p, seed, p, N, R, L, O_, ptr(out),
                                            ptr(ssq), st) == 0
    nb, norm = _guarded(N, 1)
    ib, inv = _guarded(N, 1)
    rb, rowinv = _guarded(R, 1)
    assert lib.vqf_l2_group_norm_packed(ptr(ssq), ptr(roff), N, R, L, ptr(norm), ptr(inv), ptr(rowinv), st) == 0
    torch.cuda.synchronize()
    ok = _untouched(ob, R) and _untouched(sb, R) and _untouched(nb, N) and _untouched(ib, N) and _untouched(rb, R)
    return dict(R=out, ssq=ssq, norm=norm.view(N), inv=inv.view(N), rowinv=rowinv.view(R)), ok


def _coefs(N):
    """the coefficients test_gpu_mfb_packed._abi_bwd passes"""
    return TR._pos((N,), 170).float().cuda(), TR._rand((N,), 171, 0.1).float().cuda()


def _rows_bwd_abi(ops, c, N, L, O_, kw, dY, Y, inv, P, roff, R):
    """vqf_mfb_fuse_bwd_packed_rows through the C ABI with given coefficients -> (dP (R, 5 O), dq, db) and the guard verdict"""
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    keep_p, seed, p = _mask_args(ops, kw)
    cA, cB = _coefs(N)
    W5 = 5 * O_
    pb_, dP = _guarded(R, W5)
    qb, dq = _guarded(N, W5)
    bb, db = _guarded(1, W5)
    ws = ops.workspace(Y.device, lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O_))
    assert lib.vqf_mfb_fuse_bwd_packed_rows(ptr(dY), ptr(Y), ptr(inv), ptr(cA), ptr(cB), ptr(P), ptr(c["gpb"]), ptr(c["gq"]), ptr(roff),
                                            keep_p, seed, p, N, R, L, O_, ptr(dP), ptr(dq), ptr(db), ptr(ws), ws.numel(), st) == 0
    torch.cuda.synchronize()
    return (dP, dq, db.view(W5)), _untouched(pb_, R) and _untouched(qb, N) and _untouched(bb, 1)


# ---- the fusion and the reducers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("U,N,L,O_,index,counts", PLAIN_SHAPES)
def test_packed_rows_fuse_gives_the_bits_of_the_packed_forms(ops, grouping, U, N, L, O_, index, counts, mask):
    c, kw, _ = TP._setup(ops, grouping, None, N, L, O_, None, counts, mask)
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    cu, W5 = c["lens_u"], 5 * O_
    Rtot = c["gPp"].shape[0]
    pack = lambda t, w: PR.pack_rows(t.view(N, L, w), cu)
    # ---- forward: R, rowssq, norm, inv, rowinv through the C ABI
    Rl, sl = TP._abi_fwd(ops, c, None, N, L, O_, kw, True, c["gPp"], c["roff"], Rtot)              # the *_packed sibling: padded
    norm_l, inv_l = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    assert lib.vqf_l2_group_norm(ptr(sl), N, 4 * L, ptr(norm_l), ptr(inv_l), st) == 0
    f, ok = _rows_fwd_abi(ops, c, N, L, O_, kw, c["gPp"], c["roff"], Rtot)
    assert ok
    assert torch.equal(f["R"], pack(Rl, O_)) and torch.equal(f["ssq"], pack(sl, 4))
    assert torch.equal(f["norm"], norm_l) and torch.equal(f["inv"], inv_l)
    assert torch.equal(f["rowinv"], inv_l.repeat_interleave(cu.cuda()))                            # the inv of the row's owner
    # ---- the wrappers, normalise both ways
    for normalise in (True, False):
        Y, norm, inv = TP._fwd_packed(ops, c, N, L, O_, normalise=normalise, **kw)
        Yr, normr, invr, rowinv = ops.mfb_fuse_fwd_packed_rows(c["gPp"], c["gq"], c["roff"], N, L, O_, pbias=c["gpb"],
                                                                normalise=normalise, **kw)
        assert tuple(Yr.shape) == (Rtot, O_)
        assert torch.equal(Yr, pack(Y, O_)) and torch.equal(normr, norm) and torch.equal(invr, inv), normalise
        assert torch.equal(rowinv, inv.repeat_interleave(cu.cuda()))
    # ---- backward on the same dY / Y: given coefficients through the C ABI ...
    inv1 = TR._pos((N,), 172).float().cuda()
    dPl = torch.full((Rtot, W5), SENT, device="cuda")
    dql, dbl = TP._abi_bwd(ops, c, None, N, L, O_, kw, True, Rl, inv1, c["gPp"], dPl, c["roff"], Rtot)
    dYp = pack(c["gdY"], O_)
    (dP, dq, db), ok = _rows_bwd_abi(ops, c, N, L, O_, kw, dYp, f["R"].contiguous(), inv1, c["gPp"], c["roff"], Rtot)
    assert ok
    assert torch.equal(dP, dPl) and torch.equal(dq, dql) and torch.equal(db, dbl)
    # ... and through the wrappers: the rowdot + coef_packed path (Y normalised) and the coef_lin_packed path (lin given)
    Y, norm, inv = TP._fwd_packed(ops, c, N, L, O_, **kw)
    a = TP._bwd_packed(ops, c, N, L, O_, Y, norm, inv, **kw)
    b = ops.mfb_fuse_bwd_packed_rows(dYp, pack(Y, O_), norm, inv, c["gPp"], c["gq"], c["roff"], N, L, O_, pbias=c["gpb"],
                                     want_dbias=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    Rn, norm, inv = TP._fwd_packed(ops, c, N, L, O_, normalise=False, **kw)
    valid = RR.valid_mask(cu, L).cuda().view(N * L, 1)
    for G in (1, 2):
        dl = torch.where(valid, TR._rand((N * L, G), 180 + G).float().cuda(), torch.zeros((), device="cuda"))
        ln = TR._rand((N * L, G), 190 + G).float().cuda()
        a = TP._bwd_packed(ops, c, N, L, O_, Rn, norm, inv, lin=(dl, ln), **kw)
        b = ops.mfb_fuse_bwd_packed_rows(dYp, pack(Rn, O_), norm, inv, c["gPp"], c["gq"], c["roff"], N, L, O_, pbias=c["gpb"],
                                         want_dbias=True, lin=(pack(dl, G), pack(ln, G)), **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), G
    b2 = ops.mfb_fuse_bwd_packed_rows(dYp, pack(Rn, O_), norm, inv, c["gPp"], c["gq"], c["roff"], N, L, O_, pbias=c["gpb"],
                                      want_dbias=False, lin=(pack(dl, 2), pack(ln, 2)), **kw)
    assert b2[2] is None and torch.equal(b2[0], b[0]) and torch.equal(b2[1], b[1])                # a second run: the same bits


@pytest.mark.parametrize("U,N,L,O_,index,counts", PLAIN_SHAPES)
def test_packed_coef_reducers_give_the_bits_of_the_padded_ones(ops, U, N, L, O_, index, counts):
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    cu = torch.tensor(counts)
    R = int(cu.sum())
    roff = _i32(PR.offsets_of(cu))
    valid = RR.valid_mask(cu, L).cuda()
    norm = TR._pos((N,), 201).float().cuda()
    norm[0] = 0.0                                                                  # the clamp_min branch: coefB = 0
    inv = 1.0 / norm.clamp_min(1e-12)
    z = torch.zeros((), device="cuda")
    e = lambda: torch.empty(N, device="cuda")
    # coef: rowdot (N L) with exact zeros behind each count
    rd = torch.where(valid.view(-1), TR._rand((N * L,), 202).float().cuda(), z)
    cA, cB = e(), e()
    assert lib.vqf_l2_norm_bwd_coef(ptr(rd), ptr(norm), ptr(inv), N, L, ptr(cA), ptr(cB), st) == 0
    ab, a = _guarded(N, 1)
    bb, b = _guarded(N, 1)
    rdp = PR.pack_rows(rd.view(N, L), cu)
    assert lib.vqf_l2_norm_bwd_coef_packed(ptr(rdp), ptr(roff), ptr(norm), ptr(inv), N, R, L, ptr(a), ptr(b), st) == 0
    torch.cuda.synchronize()
    assert _untouched(ab, N) and _untouched(bb, N)
    assert torch.equal(a.view(N), cA) and torch.equal(b.view(N), cB) and float(cB[0]) == 0.0
    pa, pb = ops.l2_norm_bwd_coef_packed(rdp, roff, norm, inv, N, L)
    assert torch.equal(pa, cA) and torch.equal(pb, cB)
    # coef_lin: dlogits (N L, G) zero behind each count, lin anything finite there
    for G in (1, 2):
        dl = torch.where(valid.view(-1, 1), TR._rand((N * L, G), 203 + G).float().cuda(), z)
        ln = TR._rand((N * L, G), 213 + G, 3.0).float().cuda()
        cA, cB, un = e(), e(), e()
        assert lib.vqf_l2_norm_bwd_coef_lin(ptr(dl), ptr(ln), G, ptr(norm), ptr(inv), N, L, ptr(cA), ptr(cB), ptr(un), st) == 0
        bufs = [_guarded(N, 1) for _ in range(3)]
        dlp, lnp = PR.pack_rows(dl.view(N, L, G), cu), PR.pack_rows(ln.view(N, L, G), cu)
        assert lib.vqf_l2_norm_bwd_coef_lin_packed(ptr(dlp), ptr(lnp), G, ptr(roff), ptr(norm), ptr(inv), N, R, L, ptr(bufs[0][1]),
                                                   ptr(bufs[1][1]), ptr(bufs[2][1]), st) == 0
        torch.cuda.synchronize()
        assert all(_untouched(bf, N) for bf, _ in bufs)
        for got, want in zip(bufs, (cA, cB, un)):
            assert torch.equal(got[1].view(N), want), G
        w = ops.l2_norm_bwd_coef_lin_packed(dlp, lnp, roff, norm, inv, N, L)
        assert torch.equal(w[0], cA) and torch.equal(w[1], cB) and torch.equal(w[2], un)


@pytest.mark.parametrize("U,N,L,O_,index,counts", PLAIN_SHAPES)
def test_packed_rows_fuse_clamps_what_the_offsets_hold(ops, grouping, U, N, L, O_, index, counts):
    """The malformed offsets of test_packed_fuse_clamps_what_the_offsets_hold (a count of 0, a count above L): the guards of every
    output come back untouched, rows exactly one owner has hold the *_packed form's values for that owner, rows none has are not
    written, and dq / dbias -- which read no shared output -- are that form's bits."""
    c, kw, _ = TP._setup(ops, grouping, None, N, L, O_, None, counts, "keep_p0.1")
    W5 = 5 * O_
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    anomalies = [[(0, 0), (1, L + 2)]] if N >= 3 else [[(0, 0)], [(0, L + 2)]]
    for anomaly in anomalies:
        cnts = list(counts)
        for s, v in anomaly:
            cnts[s] = v
        off = PR.offsets_of(cnts)
        Rtot = int(off[-1])
        roff = _i32(off)
        spans = PR.clamped_spans(off, Rtot, L)
        have = torch.zeros(Rtot, dtype=torch.int64)
        for stt, cn in spans:
            have[stt:stt + cn] += 1
        none = (have == 0).cuda()
        Pk = TR._pos((Rtot, W5), 160).float().cuda()
        f, ok = _rows_fwd_abi(ops, c, N, L, O_, kw, Pk, roff, Rtot)
        assert ok
        Rl, sl = TP._abi_fwd(ops, c, None, N, L, O_, kw, True, Pk, roff, Rtot)
        Rl3, sl3 = Rl.view(N, L, O_), sl.view(N, L, 4)
        for s, (stt, cn) in enumerate(spans):
            for l in range(cn):
                if int(have[stt + l]) == 1:
                    assert torch.equal(f["R"][stt + l], Rl3[s, l]) and torch.equal(f["ssq"][stt + l], sl3[s, l]), (s, l)
        assert bool((f["R"][none] == SENT).all()) and bool((f["ssq"][none] == SENT).all()) and bool((f["rowinv"][none] == SENT).all())
        assert bool(torch.isfinite(f["norm"]).all()) and bool(torch.isfinite(f["inv"]).all())
        # backward: the padded dY / Y the *_packed form reads are the packed rows of each owner's span
        dYk, Yk = TR._rand((Rtot, O_), 161).float().cuda(), f["R"].contiguous()
        dYl, Yl = torch.zeros((N, L, O_), device="cuda"), torch.zeros((N, L, O_), device="cuda")
        for s, (stt, cn) in enumerate(spans):
            dYl[s, :cn], Yl[s, :cn] = dYk[stt:stt + cn], Yk[stt:stt + cn]
        inv1 = TR._pos((N,), 172).float().cuda()
        (dP, dq, db), ok = _rows_bwd_abi(ops, c, N, L, O_, kw, dYk, Yk, inv1, Pk, roff, Rtot)
        assert ok
        dPl = torch.full((Rtot, W5), SENT, device="cuda")
        dql, dbl = TP._abi_bwd(ops, dict(c, gdY=dYl.view(N * L, O_)), None, N, L, O_, kw, True, Yl.view(N * L, O_), inv1, Pk, dPl, roff, Rtot)
        assert torch.equal(dq, dql) and torch.equal(db, dbl)
        one = (have == 1).cuda()
        assert torch.equal(dP[one], dPl[one]) and bool((dP[none] == SENT).all())
        # the coefficient reducers on the same offsets
        bufs = [_guarded(N, 1) for _ in range(3)]
        dl = TR._rand((Rtot, 2), 162).float().cuda()
        assert lib.vqf_l2_norm_bwd_coef_lin_packed(ptr(dl), ptr(dl), 2, ptr(roff), ptr(f["norm"].contiguous()), ptr(f["inv"].contiguous()),
                                                   N, Rtot, L, ptr(bufs[0][1]), ptr(bufs[1][1]), ptr(bufs[2][1]), st) == 0
        assert lib.vqf_l2_norm_bwd_coef_packed(ptr(dl), ptr(roff), ptr(f["norm"].contiguous()), ptr(f["inv"].contiguous()), N, Rtot, L,
                                               ptr(bufs[0][1]), ptr(bufs[1][1]), st) == 0
        torch.cuda.synchronize()
        assert all(_untouched(bf, N) for bf, _ in bufs) and all(bool(torch.isfinite(v).all()) for _, v in bufs)


# ---- glimpse pooling ---------------------------------------------------------------------------------------------------------------
# the sets of test_packed_glimpse_pool_gives_the_bits_of_the_len_forms, and one that takes glimpse_pool_fwd_rows_kernel (C / 4 = 128
# threads per row, a power of two, and S >= 4 * 1024 / 128 rows)
POOL_SETS = [(3, 20, 96, [7, 20, 1]), (2, 100, 2048, [37, 100]), (4, 1, 8, [1, 1, 1, 1]), (3, 40, 512, [33, 40, 5])]
POOL_IDS = ["N3_S20_C96", "N2_S100_C2048", "N4_S1_C8", "N3_S40_C512_row_slots"]


def _pool_rows_abi(ops, rows, logits, dpooled, roff, N, S, C, G, unit, dwts=None):
    """the two packed-rows pooling entry points through the C ABI, outputs between guards -> (wts, pooled, dlogits (R, G)), verdict"""
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    R = rows.shape[0]
    wb, wts = _guarded(N, G * S)
    pb, pooled = _guarded(N, G * C)
    assert lib.vqf_glimpse_pool_fwd_packed_rows(ptr(rows), ptr(logits), None, ptr(roff), N, N, R, S, C, G, int(unit), ptr(wts), ptr(pooled),
                                                st) == 0
    db, dl = _guarded(R, G)
    assert lib.vqf_glimpse_pool_bwd_packed_rows(ptr(dpooled), ptr(dwts), ptr(rows), ptr(wts), None, ptr(roff), N, N, R, S, C, G, int(unit),
                                                ptr(dl), st) == 0
    torch.cuda.synchronize()
    return (wts.view(N, G, S), pooled, dl), _untouched(wb, N) and _untouched(pb, N) and _untouched(db, R)


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "live"])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("N,S,C,counts", POOL_SETS, ids=POOL_IDS)
def test_packed_rows_glimpse_pool_gives_the_bits_of_the_packed_forms(ops, N, S, C, counts, G, unit):
    feat = TR._rand((N, S, C), 301).float().cuda()
    logits = TR._rand((N * S, G), 302, 3.0).float().cuda()
    dpooled = TR._rand((N, G * C), 303).float().cuda()
    dwts = TR._rand((N, G, S), 304).float().cuda()
    cu = torch.tensor(counts)
    rows, roff = PR.pack_rows(feat, cu), _i32(PR.offsets_of(cu))
    lg = PR.pack_rows(logits.view(N, S, G), cu)
    wts, pooled = ops.glimpse_pool_fwd_packed(rows, logits, roff, N, S, unit)
    for dw in (None, dwts):
        dl = ops.glimpse_pool_bwd_packed(dpooled, rows, wts, roff, unit, dwts=dw)
        (w, p, d), ok = _pool_rows_abi(ops, rows, lg, dpooled, roff, N, S, C, G, unit, dwts=dw)
        assert ok
        assert torch.equal(w, wts) and torch.equal(p, pooled)
        assert torch.equal(d, PR.pack_rows(dl.view(N, S, G), cu))                 # the real rows of the padded dlogits
        w2, p2 = ops.glimpse_pool_fwd_packed_rows(rows, lg, roff, N, S, unit)
        assert torch.equal(w2, wts) and torch.equal(p2, pooled)
        assert torch.equal(ops.glimpse_pool_bwd_packed_rows(dpooled, rows, wts, roff, unit, dwts=dw), d)
    pad = ~RR.valid_mask(cu, S).cuda()
    assert float(w.permute(0, 2, 1)[pad].abs().sum()) == 0.0                       # wts: exact zeros behind each count


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "live"])
def test_packed_rows_glimpse_pool_clamps_what_the_offsets_hold(ops, unit):
    N, S, C, G = 4, 20, 96, 2
    for cnts in ([0, S + 2, 5, 3], [6, 0, 0, 1]):
        off = PR.offsets_of(cnts)
        R = int(off[-1])
        roff = _i32(off)
        spans = PR.clamped_spans(off, R, S)
        rows = TR._rand((R, C), 311).float().cuda()
        lg = TR._rand((R, G), 312, 3.0).float().cuda()
        dpooled = TR._rand((N, G * C), 313).float().cuda()
        (w, p, d), ok = _pool_rows_abi(ops, rows, lg, dpooled, roff, N, S, C, G, unit)
        assert ok
        logits = torch.zeros((N, S, G), device="cuda")                             # the padded logits the *_packed form reads
        have = torch.zeros(R, dtype=torch.int64)
        for n, (stt, cn) in enumerate(spans):
            logits[n, :cn] = lg[stt:stt + cn]
            have[stt:stt + cn] += 1
        wts, pooled = ops.glimpse_pool_fwd_packed(rows, logits.view(N * S, G), roff, N, S, unit)
        assert torch.equal(w, wts) and torch.equal(p, pooled)
        dl = ops.glimpse_pool_bwd_packed(dpooled, rows, wts, roff, unit).view(N, S, G)
        for n, (stt, cn) in enumerate(spans):
            for s in range(cn):
                if int(have[stt + s]) == 1:
                    assert torch.equal(d[stt + s], dl[n, s]), (n, s)
        none = (have == 0).cuda()
        assert bool((d[none] == SENT).all())


def test_packed_rows_entry_points_return_the_stated_error_codes(vqa, ops):
    N, L, O_, R, C, G = 7, 5, 8, 9, 8, 2
    z = lambda *s: torch.zeros(s, device="cuda")
    rq = _i32([0, 1, 2, 3, 4, 5, 7, 9])
    odd = _i32([0] + [0, 1, 2, 3, 4, 5, 7, 9])[1:]                  # 4-byte aligned; + 2 bytes below is not
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    P, q, Rout, ssq = z(R, 5 * O_), z(N, 5 * O_), z(R, O_), z(R * 4)
    BADARG, UNSUPPORTED, WORKSPACE = -1, -3, -4
    fwd = lib.vqf_mfb_fuse_fwd_packed_rows
    assert fwd(ptr(P), None, ptr(q), None, None, 0, 0.0, N, R, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert fwd(ptr(P), None, ptr(q), odd.data_ptr() + 2, None, 0, 0.0, N, R, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert fwd(ptr(P), None, ptr(q), ptr(odd), None, 0, 0.0, N, 0, L, O_, ptr(Rout), ptr(ssq), st) == BADARG
    assert fwd(ptr(P), None, ptr(q), ptr(odd), None, 0, 0.0, N, R, 1025, O_, ptr(Rout), ptr(ssq), st) == UNSUPPORTED
    assert fwd(ptr(P), None, ptr(q), ptr(odd), None, 0, 0.0, N, R, L, O_, ptr(Rout), ptr(ssq), st) == 0
    one, dq, db, ws, dP = z(N), z(N, 5 * O_), z(5 * O_), z(1 << 16), z(R, 5 * O_)
    head = (ptr(Rout), ptr(Rout), ptr(one), ptr(one), ptr(one), ptr(P), None, ptr(q))
    bwd = lib.vqf_mfb_fuse_bwd_packed_rows
    need = lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O_)
    assert 0 < need <= ws.numel() * 4
    assert bwd(*head, None, None, 0, 0.0, N, R, L, O_, ptr(dP), ptr(dq), ptr(db), ptr(ws), need, st) == BADARG
    assert bwd(*head, odd.data_ptr() + 2, None, 0, 0.0, N, R, L, O_, ptr(dP), ptr(dq), ptr(db), ptr(ws), need, st) == BADARG
    assert bwd(*head, ptr(rq), None, 0, 0.0, N, 0, L, O_, ptr(dP), ptr(dq), ptr(db), ptr(ws), need, st) == BADARG
    assert bwd(*head, ptr(rq), None, 0, 0.0, N, R, L, O_, ptr(dP), ptr(dq), ptr(db), ptr(ws), need - 4, st) == WORKSPACE
    assert bwd(*head, ptr(rq), None, 0, 0.0, N, R, L, O_, ptr(dP), ptr(dq), ptr(db), ptr(ws), need, st) == 0
    rinv = z(R)
    gn = lib.vqf_l2_group_norm_packed
    assert gn(ptr(ssq), None, N, R, L, ptr(one), ptr(one), ptr(rinv), st) == BADARG
    assert gn(ptr(ssq), odd.data_ptr() + 2, N, R, L, ptr(one), ptr(one), ptr(rinv), st) == BADARG
    assert gn(ptr(ssq), ptr(rq), N, 0, L, ptr(one), ptr(one), ptr(rinv), st) == BADARG
    assert gn(ptr(ssq), ptr(rq), N, R, L, ptr(one), ptr(one), ptr(rinv), st) == 0
    cA, cB, un, dl = z(N), z(N), z(N), z(R, G)
    assert lib.vqf_l2_norm_bwd_coef_packed(ptr(rinv), None, ptr(one), ptr(one), N, R, L, ptr(cA), ptr(cB), st) == BADARG
    assert lib.vqf_l2_norm_bwd_coef_packed(ptr(rinv), ptr(rq), ptr(one), ptr(one), N, 0, L, ptr(cA), ptr(cB), st) == BADARG
    assert lib.vqf_l2_norm_bwd_coef_packed(ptr(rinv), ptr(rq), ptr(one), ptr(one), N, R, L, ptr(cA), ptr(cB), st) == 0
    assert lib.vqf_l2_norm_bwd_coef_lin_packed(ptr(dl), ptr(dl), G, None, ptr(one), ptr(one), N, R, L, ptr(cA), ptr(cB), ptr(un), st) == BADARG
    assert lib.vqf_l2_norm_bwd_coef_lin_packed(ptr(dl), ptr(dl), G, ptr(rq), ptr(one), ptr(one), N, R, L, ptr(cA), ptr(cB), ptr(un), st) == 0
    feat, wts, pooled, dpool = z(R, C), z(N, G, L), z(N, G * C), z(N, G * C)
    pf, pb = lib.vqf_glimpse_pool_fwd_packed_rows, lib.vqf_glimpse_pool_bwd_packed_rows
    assert pf(ptr(feat), ptr(dl), None, None, N, N, R, L, C, G, 0, ptr(wts), ptr(pooled), st) == BADARG
    assert pf(ptr(feat), ptr(dl), None, odd.data_ptr() + 2, N, N, R, L, C, G, 0, ptr(wts), ptr(pooled), st) == BADARG
    assert pf(ptr(feat), ptr(dl), None, ptr(rq), N, N, 0, L, C, G, 0, ptr(wts), ptr(pooled), st) == BADARG
    assert pf(ptr(feat), ptr(dl), ptr(rq), ptr(rq), N, N, R, L, C, G, 0, ptr(wts), ptr(pooled), st) == BADARG           # idx given
    assert pf(ptr(feat), ptr(dl), None, ptr(rq), N, N, R, 1025, C, G, 0, ptr(wts), ptr(pooled), st) == UNSUPPORTED
    assert pf(ptr(feat), ptr(dl), None, ptr(rq), N, N, R, L, C, G, 0, ptr(wts), ptr(pooled), st) == 0
    assert pb(ptr(dpool), None, ptr(feat), ptr(wts), ptr(rq), ptr(rq), N, N, R, L, C, G, 0, ptr(dl), st) == BADARG       # idx given
    assert pb(ptr(dpool), None, ptr(feat), ptr(wts), None, None, N, N, R, L, C, G, 0, ptr(dl), st) == BADARG
    assert pb(ptr(dpool), None, ptr(feat), ptr(wts), None, ptr(rq), N, N, R, L, C, G, 0, ptr(dl), st) == 0
    torch.cuda.synchronize()
    # the wrappers: type, shape and device of roff, and the row counts of what is packed
    for bad in (rq.long(), rq.cpu(), rq[:5], rq.float()):
        with pytest.raises(vqa.VqfError, match="roff"):
            ops.mfb_fuse_fwd_packed_rows(P, q, bad, N, L, O_)
        with pytest.raises(vqa.VqfError, match="roff"):
            ops.glimpse_pool_fwd_packed_rows(feat, dl, bad, N, L, False)
    with pytest.raises(vqa.VqfError, match=r"\(R, G\)"):
        ops.glimpse_pool_fwd_packed_rows(feat, z(N * L, G), rq, N, L, False)      # padded logits
    with pytest.raises(vqa.VqfError, match=r"\(R, O\)"):
        ops.mfb_fuse_bwd_packed_rows(z(N * L, O_), z(N * L, O_), one, one, P, q, rq, N, L, O_)


# ---- model level -------------------------------------------------------------------------------------------------------------------
def _runs():
    runs = [(p.values, p.id) for p in TR.MODEL_RUNS if not p.values[2]]          # the un-shared entries
    runs.append(((TR.MFB3, False, False, dict(fold_norm=False), False), "mfb_unit_softmax_fold_norm_off"))
    return [pytest.param(*v, id=i) for v, i in runs]


RUNS = _runs()
assert len(RUNS) == 7 and {True, False, "same-stream"} == {p.values[3].get("overlap_streams", True) for p in RUNS}


@pytest.mark.parametrize("case,mhb,shared,attrs,live", RUNS)
def test_model_with_packed_coatt_matches_the_masked_reference(vqa, case, mhb, shared, attrs, live):
    model, img, counts, q, tgt, idx = TR._model(vqa, case, mhb, False, **attrs)
    assert model.packed_coatt is False
    packed = TP._packed(vqa, img, counts)
    out0, grads0 = TR._step(model, mhb, packed, q, tgt)                           # the default form, same model, same process
    grads0 = {k: v.clone() for k, v in grads0.items()}
    model.packed_coatt = True
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out, grads = TR._step(model, mhb, packed, q, tgt)
    assert not [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning) and "LSTM" not in str(w.message)]
    grads = {k: v.clone() for k, v in grads.items()}
    o_out, g32, g64 = TR._oracle(case, mhb, False, live)
    err, e0 = rel_err(out.cpu().numpy(), o_out.numpy()), rel_err(out.cpu().numpy(), out0.cpu().numpy())
    print("packed_coatt output rel err: oracle %.2e, packed_coatt=False %.2e" % (err, e0))
    assert out.shape[0] == q.shape[0]
    assert err <= 1e-4
    assert e0 <= 1e-4
    grad_parity(grads, g32, g64, label="packed_coatt %s %s" % (case["name"], attrs))
    if live or mhb:
        assert float(grads["img_conv1d.weight"].abs().max()) > 0.0 and float(grads["co_att_conv1.weight"].abs().max()) > 0.0
    assert set(grads) == set(grads0) and all(grads[k].shape == grads0[k].shape for k in grads)
    # a second step gives the same bits; int32 offsets are the same call
    out2, grads2 = TR._step(model, mhb, packed, q, tgt)
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    p32 = vqa.PackedRegions(packed.rows, packed.offsets.to(torch.int32), packed.max_regions)
    out32, grads32 = TR._step(model, mhb, p32, q, tgt)
    assert torch.equal(out, out32) and all(torch.equal(grads[k], grads32[k]) for k in grads)
    # keep 'm1' given at (N L, 5000) is honoured: other bits in its REAL rows change the output, other bits in its padded rows do not
    masks = dict(model._seeds.keep)
    real = RR.valid_mask(counts.cpu(), img.shape[1]).cuda().view(-1, 1)
    model.set_keep_masks(**dict(masks, m1=torch.where(real, masks["m1"], 1 - masks["m1"])))
    out3, _ = TR._step(model, mhb, packed, q, tgt)
    assert torch.equal(out, out3)
    model.set_keep_masks(**dict(masks, m1=torch.where(real, 1 - masks["m1"], masks["m1"])))
    out4, _ = TR._step(model, mhb, packed, q, tgt)
    assert torch.equal(out, out4) != bool(live or mhb)              # (under unit_softmax the fusion cannot reach MFB's logits)
    # eval mode: a max_regions five wider changes the result by at most 1e-4, and the pair call agrees
    model.set_keep_masks()
    model.eval()
    uimg, ulen = packed.unpack()
    with torch.no_grad():
        a = model.forward(packed, q)
        b = model.forward(vqa.PackedRegions(packed.rows, packed.offsets, packed.max_regions + 5), q)
        cc = model.forward((uimg, ulen), q)
    assert rel_err(b.cpu().numpy(), a.cpu().numpy()) <= 1e-4 and rel_err(a.cpu().numpy(), cc.cpu().numpy()) <= 1e-4


@pytest.mark.parametrize("mhb,attrs", [(False, {}), (False, dict(unit_softmax=False)), (True, {})], ids=["mfb", "mfb_live", "mhbcoatt"])
def test_eval_mode_with_packed_coatt_matches_the_masked_reference(vqa, mhb, attrs):
    """eval mode (no dropout) against the fp64 restatement without masks; predict() forwards the attribute's form; a batch delivered
    by RegionStager (int32 offsets) gives the bits of the same batch packed by hand"""
    case = TR.MHB3 if mhb else TR.MFB3
    model, img, counts, q, tgt, _ = TR._model(vqa, case, mhb, False, packed_coatt=True, **attrs)
    model.set_keep_masks()
    model.eval()
    packed = TP._packed(vqa, img, counts)
    with torch.no_grad():
        a = model.forward(packed, q)
    cfg = make_cfg(case)
    sd = {k: v.double() for k, v in recipe_sd(O.mfb_shapes(cfg, mhb=mhb), case["salt"]).items()}
    im, cn = img.cpu().double(), counts.cpu()
    if mhb:
        ref = RR.mhbcoatt_forward(sd, cfg, im, q.cpu(), cn)
    else:
        ref = RR.mfb_forward(sd, cfg, im, q.cpu(), cn, live_softmax=not attrs.get("unit_softmax", True))
    err = rel_err(a.cpu().numpy(), ref.float().numpy())
    print("packed_coatt eval rel err %.2e" % err)
    assert err <= 1e-4
    ids, probs = vqa.predict(model, packed, q)
    assert torch.equal(ids[:, 0], a.argmax(1)) and not model.training and model.packed_coatt
    feats = [img[i, :int(k)].cpu().numpy() for i, k in enumerate(counts.tolist())]
    staged, none = vqa.stage_regions(feats)
    assert none is None and isinstance(staged, vqa.PackedRegions) and torch.equal(staged.rows, packed.rows)
    staged = vqa.PackedRegions(staged.rows, staged.offsets, packed.max_regions)   # the stager's width is the largest count
    with torch.no_grad():
        s = model.forward(staged, q)
    assert torch.equal(s, a)


# ---- structure -----------------------------------------------------------------------------------------------------------------------
def _big(vqa, mhb, N, counts, **attrs):
    """a batch of N questions at the small case's widths: model, PackedRegions, questions, targets"""
    case = dict(TR.MHB3 if mhb else TR.MFB3, N=N, name="packed_coatt_n%d" % N)
    cfg = make_cfg(case)
    L, D = cfg.img_feature_dim, cfg.img_feature_channel
    model = (vqa.MHBCoAtt if mhb else vqa.MFB)(cfg)
    sd = {k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"])) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model = model.cuda().train()
    for k, v in attrs.items():
        setattr(model, k, v)
    counts = torch.as_tensor(counts, dtype=torch.int64, device="cuda")
    img = torch.from_numpy(recipe.img_features(N, L, D, case["salt"])).cuda()
    img = torch.where(RR.valid_mask(counts.cpu(), L).cuda()[:, :, None], img, torch.zeros_like(img))
    q = torch.from_numpy(recipe.question_tokens(N, case["T"], cfg.q_vocab_size, case["salt"])).cuda()
    tgt = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, case["salt"]) if mhb
                           else recipe.hard_answers(N, cfg.a_vocab_size, case["salt"])).cuda()
    return model, img, counts, TP._packed(vqa, img, counts), q, tgt, cfg


STRUCT = [
    pytest.param(False, dict(unit_softmax=False), id="mfb_live"),
    pytest.param(False, dict(unit_softmax=False, fold_norm=False, overlap_streams=False), id="mfb_live_fold_norm_off_one_node"),
    pytest.param(True, dict(overlap_streams="same-stream"), id="mhbcoatt_same_stream"),
]


@pytest.mark.parametrize("mhb,attrs", STRUCT)
def test_structure(vqa, mhb, attrs):
    """A step with packed_coatt = True beside the default packed step: no GEMM with M or K = N L (the default has co_att_conv1's three
    there), those three products at R rows, and not more launches than the default form up to split-K reductions.  With False the
    census is the default form's, launch for launch (the attribute set to False explicitly against a model that never had it set)."""
    ops = vqa.ops
    N = 16
    counts = [1, 20, 19, 7, 4, 3, 11, 2, 20, 5, 9, 1, 13, 6, 8, 17]
    model, img, cnt, packed, q, tgt, cfg = _big(vqa, mhb, N, counts, **attrs)
    L, T, R = cfg.img_feature_dim, q.shape[1], sum(counts)
    NL = N * L
    Hd = model.co_att_conv1.out_channels
    others = {N, T, N * T, 1000, 5000, Hd, cfg.hidden_dim, 2 * cfg.hidden_dim, cfg.img_feature_channel, 2 * cfg.img_feature_channel,
              cfg.emb_dim, cfg.a_vocab_size, 4 * cfg.hidden_dim, 512, 1024, 2}
    assert R < NL and NL not in others and R not in others                        # a GEMM extent equal to N L (or R) can only be the rows

    def counted():
        TR._step(model, mhb, packed, q, tgt)                                      # warm-up (the library's first launches)
        torch.cuda.synchronize()
        ops.prof_reset()
        ops.prof_enable(True)
        try:
            TR._step(model, mhb, packed, q, tgt)
            torch.cuda.synchronize()
        finally:
            ops.prof_enable(False)
        census = {k: v[0] for k, v in ops.prof_report().items()}
        by_rows = {}
        for rows in (R, NL):
            by_rows[rows] = dict(M=sum(ops.prof_shape(g, rows, -1, -1)[0] for g in range(4)),
                                 K=sum(ops.prof_shape(g, -1, -1, rows)[0] for g in range(4)),
                                 conv1=(ops.prof_gemm(0, 0, rows, Hd, 1000)[0], ops.prof_gemm(0, 1, rows, 1000, Hd)[0],
                                        ops.prof_gemm(1, 1, Hd, 1000, rows)[0]))
        return census, by_rows

    base, base_rows = counted()                                                   # the attribute as the constructor left it
    model.packed_coatt = False
    off, off_rows = counted()
    model.packed_coatt = True
    on, on_rows = counted()
    print("launches: default %d, packed_coatt %d; by rows default %s packed_coatt %s" % (sum(off.values()), sum(on.values()), off_rows, on_rows))
    assert off == base and off_rows == base_rows                                  # False: the default form, launch for launch
    # the default form has co_att_conv1's three products on N L rows (and the projection's two on R) ...
    assert off_rows[NL]["conv1"] == (1, 1, 1) and off_rows[R]["conv1"] == (0, 0, 0)
    assert off_rows[NL]["M"] >= 2 and off_rows[NL]["K"] >= 1
    # ... the opt-in form has no GEMM with M or K = N L, and the three at R rows
    assert on_rows[NL]["M"] == 0 and on_rows[NL]["K"] == 0, on_rows
    assert on_rows[R]["conv1"] == (1, 1, 1), on_rows
    assert on_rows[R]["M"] == off_rows[R]["M"] + off_rows[NL]["M"] and on_rows[R]["K"] == off_rows[R]["K"] + off_rows[NL]["K"]
    diff = {k: (off.get(k, 0), on.get(k, 0)) for k in set(off) | set(on) if off.get(k, 0) != on.get(k, 0)}
    print("differing launch counts (default, packed_coatt): %s" % diff)
    sk = diff.pop("splitk_reduce", (0, 0))
    assert diff == {}                                                              # the same kernels, as often
    assert sum(on.values()) - sk[1] <= sum(off.values()) - sk[0]                   # not more launches, up to split-K reductions
    assert abs(sk[0] - sk[1]) <= 4


# ---- memory --------------------------------------------------------------------------------------------------------------------------
def test_packed_coatt_allocates_no_padded_fusion_output(vqa):
    """N = 64, L = 20, every count 2, MHBCoAtt, Philox dropout, two rounds: the peak of forward + backward with packed_coatt = True
    must lie below the default packed form's by at least the padding of one Y, (N L - R) * 1000 * 4 bytes."""
    N = 64
    model, img, counts, packed, q, soft, cfg = _big(vqa, True, N, [2] * N)
    L = cfg.img_feature_dim
    R = packed.rows.shape[0]
    assert L == 20 and R == 2 * N
    peak = {}
    for form in (False, True, False, True):                                        # twice: workspaces and streams exist from the first round on
        model.packed_coatt = form
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(3)
        out = model.forward(packed, q)
        torch.nn.KLDivLoss()(out, soft).backward()
        torch.cuda.synchronize()
        peak[form] = torch.cuda.max_memory_allocated() - base
        del out
    one = (N * L - R) * 1000 * 4
    print("peak bytes above the baseline: packed %d, packed_coatt %d, the padding of one Y %d" % (peak[False], peak[True], one))
    assert peak[True] <= peak[False] - one


# ---- where the attribute does nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mhb,form", [(False, "tensor"), (False, "pair"), (False, "pruned_packed"), (True, "tensor"), (True, "pair")],
                         ids=["mfb_tensor", "mfb_pair", "mfb_pruned_packed", "mhbcoatt_tensor", "mhbcoatt_pair"])
def test_packed_coatt_changes_nothing_on_the_other_call_forms(vqa, mhb, form):
    res = []
    for flag in (False, True):
        attrs = dict(pruned=True) if form == "pruned_packed" else ({} if mhb else dict(unit_softmax=False))
        model, img, counts, q, tgt, _ = TR._model(vqa, TR.MHB3 if mhb else TR.MFB3, mhb, False, packed_coatt=flag, **attrs)
        if form == "tensor":
            res.append(TR._step(model, mhb, img, q, tgt))
        elif form == "pair":
            res.append(TR._step(model, mhb, img, q, tgt, img_length=counts))
        else:
            res.append(TR._step(model, mhb, TP._packed(vqa, img, counts), q, tgt))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_packed_coatt_refuses_img_index_on_the_gpu_too(vqa):
    for mhb in (False, True):
        model, img, counts, q, tgt, idx = TR._model(vqa, TR.MHB3 if mhb else TR.MFB3, mhb, True, packed_coatt=True)
        with pytest.raises(vqa.VqfError, match="packed_coatt.*img_index"):
            model.forward(TP._packed(vqa, img, counts), q, img_index=idx)
        model.packed_coatt = False
        assert model.forward(TP._packed(vqa, img, counts), q, img_index=idx).shape[0] == q.shape[0]
