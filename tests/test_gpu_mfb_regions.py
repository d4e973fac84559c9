"""MFB / MHBCoAtt with per-image region counts (forward((img, img_length), ...)) on the GPU.

Kernel level: vqf_mfb_fuse_fwd_len / _bwd_len and their grouped forms against the fp64 restatement tests/mfb_regions_ref.fuse_ref
over every element, with the criteria of test_gpu_mfb_shared.test_mfb_fuse_grouped_fwd_bwd (1e-5 on Y / norm, 2e-5 on dP / dq /
dbias; well-conditioned operands: one sign per pooling window); padded rows are exact zeros, lens = L gives the bits of the
entry points without lens, two runs give equal bits, and what the padded rows of P / dY / Y hold changes no output bit.
Model level: tests/mfb_regions_ref (pinned on the oracle by tests/test_mfb_regions_cpu.py) in fp32 / fp64, output 1e-4,
gradients golden_util.grad_parity, as test_gpu_mfb_shared applies them.
Shapes: the smallest at which the row walk can go wrong -- counts 1, L, L - 1, an odd count (splits the image pass's row
pair), and at L = 196 a count below the row split LS = 16, so that some workgroups own no real row.
"""
import numpy as np
import pytest
import torch

import recipe
import mfb_regions_ref as RR
from cases import MFB_CASES, MHBCOATT_CASES, make_cfg
from golden_util import recipe_sd, rel_err, grad_parity
from oracle import ref_torch as O

pytestmark = pytest.mark.gpu

P_DROP = 0.1
INV_KEEP64 = 1.0 - float(np.float32(P_DROP))          # the kernels scale kept elements by 1 / (1 - p) with p in fp32


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


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().double()


def _pos(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 + 0.9 * torch.rand(shape, generator=g, dtype=torch.float64)).float().double()


def _rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).cuda()


# (U, N, L, O, index, counts per image); U is None: the plain forms, counts per sample
KERNEL_SHAPES = [
    pytest.param(None, 5, 20, 1000, None, [1, 20, 19, 7, 4], id="N5_L20_counts_1_L_Lm1_odd"),
    pytest.param(None, 3, 196, 1000, None, [5, 196, 195], id="N3_L196_count_below_LS16"),
    pytest.param(None, 6, 3, 8, None, [1, 3, 2, 3, 1, 2], id="N6_L3_O8_two_active_lanes"),
    pytest.param(None, 2, 1, 1000, None, [1, 1], id="N2_L1"),
    pytest.param(3, 7, 20, 1000, [2, 0, 0, 2, 0, 2, 0], [7, 20, 1], id="U3_N7_L20_image1_unused"),
    pytest.param(3, 7, 196, 1000, [2, 0, 0, 2, 0, 2, 0], [5, 196, 195], id="U3_N7_L196_count_below_LS16"),
    pytest.param(3, 2, 3, 8, [2, 0], [2, 3, 1], id="U3_N2_L3_O8_N_below_U"),
    pytest.param(3, 7, 1, 1000, [2, 0, 0, 2, 0, 2, 0], [1, 1, 1], id="U3_N7_L1"),
]

_OPER = {}
_REF = {}


def _operands(U, N, L, O_, index, counts):
    """fp64 operands of one shape (computed once, never modified)"""
    key = (U, N, L, O_)
    if key not in _OPER:
        W5 = 5 * O_
        rows = (U if U is not None else N) * L
        gsign = torch.sign(_rand((N, O_), 156) + 1e-3).repeat_interleave(5, 1)
        _OPER[key] = dict(P=_pos((rows, W5), 150), pb=_pos((W5,), 157), q=_pos((N, W5), 151) * gsign, dY=_rand((N * L, O_), 154),
                          keep=(torch.rand((N * L, W5), generator=torch.Generator().manual_seed(153)) >= P_DROP).to(torch.uint8))
    c = dict(_OPER[key])
    lens_u = torch.tensor(counts)
    c["idx"] = None if U is None else torch.tensor(index)
    c["lens_u"] = lens_u
    c["lens_q"] = lens_u if U is None else lens_u[c["idx"]]
    return c


def _reference(U, N, L, O_, index, counts, keep, tag):
    """fp64: Y, norm, dP, dq, db of the masked fusion; once per (shape, mask)"""
    key = (U, N, L, O_, tag)
    if key in _REF:
        return _REF[key]
    c = _operands(U, N, L, O_, index, counts)
    P, pb, q = (c[k].clone().requires_grad_() for k in ("P", "pb", "q"))
    R, Y, norm, valid = RR.fuse_ref(P, pb, q, c["lens_q"], N, L, O_, keep=keep, p=1.0 - INV_KEEP64, idx=c["idx"], U=U)
    (Y * c["dY"]).sum().backward()
    _REF[key] = dict(Y=Y.detach(), R=R.detach(), norm=norm.detach(), dP=P.grad, dq=q.grad, db=pb.grad, valid=valid)
    return _REF[key]


def _fwd(ops, c, U, N, L, O_, lens, P=None, normalise=True, **kw):
    P = c["gP"] if P is None else P
    if U is None:
        return ops.mfb_fuse_fwd(P, c["gq"], N, L, O_, pbias=c["gpb"], normalise=normalise, lens=lens, **kw)[:3]
    return ops.mfb_fuse_fwd_grouped(P, c["gq"], c["grp"][0], N, U, L, O_, pbias=c["gpb"], normalise=normalise, lens=lens, **kw)


def _bwd(ops, c, U, N, L, O_, lens, dY, Y, norm, inv, P=None, want_dbias=True, **kw):
    P = c["gP"] if P is None else P
    if U is None:
        dP, dq, _, db = ops.mfb_fuse_bwd(dY, Y, norm, inv, P, c["gq"], N, L, O_, pbias=c["gpb"], want_dbias=want_dbias, lens=lens, **kw)
        return dP, dq, db
    g = c["grp"]
    return ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, c["gq"], g[0], g[1], g[2], N, U, L, O_, pbias=c["gpb"], want_dbias=want_dbias,
                                    lens=lens, **kw)


@pytest.mark.parametrize("mask", ["keep_p0.1", "philox_p0.1"])
@pytest.mark.parametrize("U,N,L,O_,index,counts", KERNEL_SHAPES)
def test_mfb_fuse_len_fwd_bwd(ops, grouping, U, N, L, O_, index, counts, mask):
    c = _operands(U, N, L, O_, index, counts)
    cu = lambda t: t.float().cuda()
    c.update(gP=cu(c["P"]), gpb=cu(c["pb"]), gq=cu(c["q"]), grp=None if U is None else grouping._group_index(c["idx"].cuda(), U))
    dY = cu(c["dY"])
    lq, lu = _i32(c["lens_q"]), _i32(c["lens_u"])
    lens = lq if U is None else (lq, lu)
    full = torch.full_like(lq, L) if U is None else (torch.full_like(lq, L), torch.full_like(lu, L))
    if mask == "keep_p0.1":
        kw = dict(keep=c["keep"].cuda(), p_drop=P_DROP)
        keep64 = c["keep"]
    else:
        # the masks of the real elements are what the plain kernel draws: read them off its dropped product (P, q != 0)
        kw = dict(seed=4321, p_drop=P_DROP)
        Pg = c["gP"] if U is None else c["gP"].view(U, L, -1)[c["grp"][0].long()].reshape(N * L, -1).contiguous()
        z = ops.mfb_fuse_fwd(Pg, c["gq"], N, L, O_, pbias=c["gpb"], want_zdrop=True, **kw)[3]
        keep64 = (z != 0).to(torch.uint8).cpu()
        if keep64.numel() >= 100000:
            assert abs(1.0 - keep64.float().mean().item() - P_DROP) < 5e-3
    ref = _reference(U, N, L, O_, index, counts, keep64, mask)
    pad_q = ~ref["valid"].cuda()                                                      # (N, L) padded rows per question
    pad_u = pad_q if U is None else ~RR.valid_mask(c["lens_u"], L).cuda()            # (U, L) per image

    # ---- forward
    Y, norm, inv = _fwd(ops, c, U, N, L, O_, lens, **kw)
    R = _fwd(ops, c, U, N, L, O_, lens, normalise=False, **kw)[0]
    e_y, e_n = _rel(Y, ref["Y"]), _rel(norm, ref["norm"])
    print("fwd len: Y %.2e norm %.2e" % (e_y, e_n))
    assert e_y <= 1e-5 and e_n <= 1e-5
    assert torch.equal(R.view(N, L, O_)[pad_q], torch.zeros_like(R.view(N, L, O_)[pad_q]))
    assert torch.equal(Y.view(N, L, O_)[pad_q], torch.zeros_like(Y.view(N, L, O_)[pad_q]))
    # R and rowssq themselves, through the C ABI: zero partials on padding; lens = L gives the plain entry point's bits
    lib, ptr = ops._lib(), ops._ptr
    keep_p = None if "keep" not in kw else ptr(kw["keep"])
    seed = kw.get("seed", 0)
    out = [torch.full((N * L, O_), 7.0, device="cuda") for _ in range(3)]
    ssq = [torch.full((N * L * 4,), 7.0, device="cuda") for _ in range(3)]
    st = ops._stream()
    if U is None:
        assert lib.vqf_mfb_fuse_fwd_len(ptr(c["gP"]), ptr(c["gpb"]), ptr(c["gq"]), ptr(lq), keep_p, seed, P_DROP, N, L, O_, ptr(out[0]),
                                        ptr(ssq[0]), st) == 0
        assert lib.vqf_mfb_fuse_fwd_len(ptr(c["gP"]), ptr(c["gpb"]), ptr(c["gq"]), ptr(full), keep_p, seed, P_DROP, N, L, O_, ptr(out[1]),
                                        ptr(ssq[1]), st) == 0
        assert lib.vqf_mfb_fuse_fwd(ptr(c["gP"]), ptr(c["gpb"]), ptr(c["gq"]), None, keep_p, seed, P_DROP, N, L, O_, ptr(out[2]),
                                    ptr(ssq[2]), None, st) == 0
    else:
        ix = c["grp"][0]
        assert lib.vqf_mfb_fuse_fwd_grouped_len(ptr(c["gP"]), ptr(c["gpb"]), ptr(c["gq"]), ptr(ix), ptr(lq), ptr(lu), keep_p, seed, P_DROP,
                                                N, U, L, O_, ptr(out[0]), ptr(ssq[0]), st) == 0
        assert lib.vqf_mfb_fuse_fwd_grouped_len(ptr(c["gP"]), ptr(c["gpb"]), ptr(c["gq"]), ptr(ix), ptr(full[0]), ptr(full[1]), keep_p, seed,
                                                P_DROP, N, U, L, O_, ptr(out[1]), ptr(ssq[1]), st) == 0
        assert lib.vqf_mfb_fuse_fwd_grouped(ptr(c["gP"]), ptr(c["gpb"]), ptr(c["gq"]), ptr(ix), keep_p, seed, P_DROP, N, U, L, O_,
                                            ptr(out[2]), ptr(ssq[2]), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0], R)
    sq = ssq[0].view(N, L, 4)
    assert torch.equal(sq[pad_q], torch.zeros_like(sq[pad_q]))
    assert torch.equal(out[1], out[2]) and torch.equal(ssq[1], ssq[2])
    # the real rows are the plain kernel's bits (same operations in the same order)
    assert torch.equal(out[0].view(N, L, O_)[~pad_q], out[2].view(N, L, O_)[~pad_q]) and torch.equal(sq[~pad_q], ssq[2].view(N, L, 4)[~pad_q])

    # ---- backward
    dP, dq, db = _bwd(ops, c, U, N, L, O_, lens, dY, Y, norm, inv, **kw)
    e = (_rel(dP, ref["dP"]), _rel(dq, ref["dq"]), _rel(db, ref["db"]))
    print("bwd len: dP %.2e dq %.2e dbias %.2e" % e)
    assert dP.shape == c["gP"].shape and dq.shape == (N, 5 * O_)
    assert max(e) <= 2e-5
    dPv = dP.view(-1, L, 5 * O_)
    assert torch.equal(dPv[pad_u], torch.zeros_like(dPv[pad_u]))
    if U is not None:
        for u in range(U):
            if u not in index:
                assert float(dPv[u].abs().max()) == 0.0
    # two runs: the same bits; without the bias gradient (the other instantiations): the same dP and dq
    dP2, dq2, db2 = _bwd(ops, c, U, N, L, O_, lens, dY, Y, norm, inv, **kw)
    assert torch.equal(dP, dP2) and torch.equal(dq, dq2) and torch.equal(db, db2)
    dP3, dq3, db3 = _bwd(ops, c, U, N, L, O_, lens, dY, Y, norm, inv, want_dbias=False, **kw)
    assert db3 is None and torch.equal(dP, dP3) and torch.equal(dq, dq3)
    Y2, norm2, inv2 = _fwd(ops, c, U, N, L, O_, lens, **kw)
    assert torch.equal(Y, Y2) and torch.equal(norm, norm2) and torch.equal(inv, inv2)

    # ---- lens = L everywhere: the bits of the forms without lens
    a = _fwd(ops, c, U, N, L, O_, full, **kw)
    b = _fwd(ops, c, U, N, L, O_, None, **kw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ga = _bwd(ops, c, U, N, L, O_, full, dY, *b, **kw)
    gb = _bwd(ops, c, U, N, L, O_, None, dY, *b, **kw)
    assert all(torch.equal(x, y) for x, y in zip(ga, gb))

    # ---- what the padded rows of P, dY and Y hold changes no output bit (they are never read).  The backward through the C ABI:
    # ops.mfb_fuse_bwd's own vqf_rowdot pass in front reads all of Y and dY (the models hand it the forward's zero rows)
    if bool(pad_q.any()):
        junk = lambda t, s: (torch.rand(t.shape, generator=torch.Generator().manual_seed(s)) * 8 - 4).cuda()
        P2 = torch.where(pad_u[:, :, None], junk(c["gP"], 1).view(-1, L, 5 * O_), c["gP"].view(-1, L, 5 * O_)).view_as(c["gP"]).contiguous()
        dYj = torch.where(pad_q[:, :, None], junk(dY, 2).view(N, L, O_), dY.view(N, L, O_)).view_as(dY).contiguous()
        Yj = torch.where(pad_q[:, :, None], junk(Y, 3).view(N, L, O_), Y.view(N, L, O_)).view_as(Y).contiguous()
        Y4, norm4, inv4 = _fwd(ops, c, U, N, L, O_, lens, P=P2, **kw)
        assert torch.equal(Y, Y4) and torch.equal(norm, norm4) and torch.equal(inv, inv4)
        cA, cB = _pos((N,), 170).float().cuda(), _rand((N,), 171, 0.1).float().cuda()
        got = []
        for Pi, dYi, Yi in ((c["gP"], dY, Y), (P2, dYj, Yj)):
            o = dict(dP=torch.full_like(c["gP"], 7.0), dq=torch.full((N, 5 * O_), 7.0, device="cuda"), db=torch.full((5 * O_,), 7.0, device="cuda"))
            if U is None:
                ws = ops.workspace(dY.device, lib.vqf_mfb_fuse_bwd_ws_bytes(N, L, O_))
                rc = lib.vqf_mfb_fuse_bwd_len(ptr(dYi), ptr(Yi), ptr(inv), ptr(cA), ptr(cB), ptr(Pi), ptr(c["gpb"]), ptr(c["gq"]), ptr(lq),
                                              keep_p, seed, P_DROP, N, L, O_, ptr(o["dP"]), ptr(o["dq"]), ptr(o["db"]), ptr(ws), ws.numel(), st)
            else:
                g = c["grp"]
                ws = ops.workspace(dY.device, lib.vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O_))
                rc = lib.vqf_mfb_fuse_bwd_grouped_len(ptr(dYi), ptr(Yi), ptr(inv), ptr(cA), ptr(cB), ptr(Pi), ptr(c["gpb"]), ptr(c["gq"]),
                                                      ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(lq), ptr(lu), keep_p, seed, P_DROP, N, U, L, O_,
                                                      ptr(o["dP"]), ptr(o["dq"]), ptr(o["db"]), ptr(ws), ws.numel(), st)
            assert rc == 0
            torch.cuda.synchronize()
            got.append(o)
        for k in ("dP", "dq", "db"):
            assert torch.equal(got[0][k], got[1][k]), k
        assert float(got[0]["dP"].abs().max()) > 0.0


def test_len_entry_points_return_the_stated_error_codes(vqa, ops, grouping):
    U, N, L, O_ = 3, 7, 5, 8
    z = lambda *s: torch.zeros(s, device="cuda")
    i32, order, off = grouping._group_index(torch.tensor([2, 0, 0, 2, 0, 2, 0]).cuda(), U)
    lq, lu = _i32([5, 1, 1, 5, 1, 5, 1]), _i32([1, 3, 5])
    lib, ptr, st = ops._lib(), ops._ptr, ops._stream()
    P, Pu, q, R, ssq = z(N * L, 5 * O_), z(U * L, 5 * O_), z(N, 5 * O_), z(N * L, O_), z(N * L * 4)
    odd = _i32([0] * 9)[1:]                                    # 4-byte aligned; + 2 bytes below is not
    BADARG, WORKSPACE = -1, -4
    assert lib.vqf_mfb_fuse_fwd_len(ptr(P), None, ptr(q), None, None, 0, 0.0, N, L, O_, ptr(R), ptr(ssq), st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_len(ptr(P), None, ptr(q), odd.data_ptr() + 2, None, 0, 0.0, N, L, O_, ptr(R), ptr(ssq), st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_len(ptr(P), None, ptr(q), ptr(odd), None, 0, 0.0, N, L, O_, ptr(R), ptr(ssq), st) == 0
    assert lib.vqf_mfb_fuse_fwd_grouped_len(ptr(Pu), None, ptr(q), ptr(i32), ptr(lq), None, None, 0, 0.0, N, U, L, O_, ptr(R), ptr(ssq),
                                            st) == BADARG
    assert lib.vqf_mfb_fuse_fwd_grouped_len(ptr(Pu), None, ptr(q), ptr(i32), None, ptr(lu), None, 0, 0.0, N, U, L, O_, ptr(R), ptr(ssq),
                                            st) == BADARG
    one = z(N)
    dq, ws, dP, dPu = z(N, 5 * O_), z(1 << 16), z(N * L, 5 * O_), z(U * L, 5 * O_)
    assert lib.vqf_mfb_fuse_bwd_len(ptr(R), ptr(R), ptr(one), ptr(one), ptr(one), ptr(P), None, ptr(q), None, None, 0, 0.0, N, L, O_,
                                    ptr(dP), ptr(dq), None, ptr(ws), ws.numel() * 4, st) == BADARG
    need = lib.vqf_mfb_fuse_bwd_grouped_ws_bytes(N, U, L, O_)
    assert 0 < need <= ws.numel() * 4
    args = (ptr(R), ptr(R), ptr(one), ptr(one), ptr(one), ptr(Pu), None, ptr(q), ptr(i32), ptr(order), ptr(off))
    tail = (None, 0, 0.0, N, U, L, O_, ptr(dPu), ptr(dq), None, ptr(ws))
    assert lib.vqf_mfb_fuse_bwd_grouped_len(*args, ptr(lq), None, *tail, ws.numel() * 4, st) == BADARG
    assert lib.vqf_mfb_fuse_bwd_grouped_len(*args, ptr(lq), ptr(lu), *tail, need - 4, st) == WORKSPACE
    assert lib.vqf_mfb_fuse_bwd_grouped_len(*args, ptr(lq), ptr(lu), *tail, need, st) == 0
    torch.cuda.synchronize()
    # the wrappers: type, shape and device of lens
    for bad in (lq.long(), lq.cpu(), lq[:5], lq.float()):
        with pytest.raises(vqa.VqfError, match="lens"):
            ops.mfb_fuse_fwd(P, q, N, L, O_, lens=bad)
        with pytest.raises(vqa.VqfError, match="lens"):
            ops.mfb_fuse_fwd_grouped(Pu, q, i32, N, U, L, O_, lens=(bad, lu))
    with pytest.raises(vqa.VqfError, match="lens"):
        ops.mfb_fuse_fwd_grouped(Pu, q, i32, N, U, L, O_, lens=lq)
    with pytest.raises(vqa.VqfError, match="lens"):
        ops.mfb_fuse_fwd_grouped(Pu, q, i32, N, U, L, O_, lens=(lq, lu[:2]))
    with pytest.raises(vqa.VqfError, match="lens"):
        ops.mfb_fuse_fwd(P.to(torch.bfloat16), q, N, L, O_, lens=lq)


# ---- model level -------------------------------------------------------------------------------------------------------------------
INDEX = [2, 0, 0, 2, 0, 2, 0]            # U = 3 images, 7 questions, image 1 unused, unsorted
COUNTS = [7, 20, 1]                      # per image (L = 20): an odd count, L, 1
COUNTS_SHARED = [7, 1, 19]               # with INDEX: odd, (unused) 1, L - 1
_ORACLE = {}


def _inputs(case, mhb, shared):
    cfg = make_cfg(case)
    U, T, L, D, H = case["N"], case["T"], cfg.img_feature_dim, cfg.img_feature_channel, cfg.hidden_dim
    assert U == 3 and L == 20
    N = len(INDEX) if shared else U
    s = case["salt"]
    img = torch.from_numpy(recipe.img_features(U, L, D, s))
    counts = torch.tensor(COUNTS_SHARED if shared else COUNTS)
    # the padded rows hold finite values that are NOT zero: they must not matter
    img = torch.where(RR.valid_mask(counts, L)[:, :, None], img, torch.from_numpy(recipe.sym_tensor((U, L, D), 2.0, 91)))
    q = torch.from_numpy(recipe.question_tokens(N, T, cfg.q_vocab_size, s))
    tgt = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, s) if mhb else recipe.hard_answers(N, cfg.a_vocab_size, s))
    m = dict(l=torch.from_numpy(recipe.keep_mask((N, T, H), 0.3, "l")), m1=torch.from_numpy(recipe.keep_mask((N * L, 5000), 0.1, "m1")),
             m2=torch.from_numpy(recipe.keep_mask((N, 5000), 0.1, "m2")), m3=torch.from_numpy(recipe.keep_mask((N, 5000), 0.1, "m3")))
    return cfg, img, counts, q, tgt, m, (N, T, L, H)


def _oracle(case, mhb, shared, live=False):
    """(out32, g32, g64) of the masked restatement (on img[idx], counts[idx] when shared) with the explicit masks; once per mode"""
    key = (case["name"], mhb, shared, live)
    if key in _ORACLE:
        return _ORACLE[key]
    cfg, img, counts, q, tgt, m, (N, T, L, H) = _inputs(case, mhb, shared)
    if shared:
        idx = torch.tensor(INDEX)
        img, counts = img[idx], counts[idx]
    drop = dict(m1=m["m1"].view(N, L, 5000), m2=m["m2"], m3=m["m3"], l=m["l"].permute(1, 0, 2) if mhb else m["l"])
    res = []
    for dt in (torch.float32, torch.float64):
        sd = {k: v.to(dt).requires_grad_(True) for k, v in recipe_sd(O.mfb_shapes(cfg, mhb=mhb), case["salt"]).items()}
        if mhb:
            out = RR.mhbcoatt_forward(sd, cfg, img.to(dt), q, counts, drop=drop)
            O.kldiv_loss(out, tgt.to(dt)).backward()
        else:
            out = RR.mfb_forward(sd, cfg, img.to(dt), q, counts, drop=drop, live_softmax=live)
            O.ce_loss(out, tgt).backward()
        res.append((out.detach(), {k: v.grad for k, v in sd.items()}))
    _ORACLE[key] = (res[0][0], res[0][1], res[1][1])
    return _ORACLE[key]


def _model(vqa, case, mhb, shared, **attrs):
    cfg, img, counts, q, tgt, m, (N, T, L, H) = _inputs(case, mhb, shared)
    model = (vqa.MHBCoAtt if mhb else vqa.MFB)(cfg)
    sd = {k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"])) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model = model.cuda().train()
    for k, v in attrs.items():
        setattr(model, k, v)
    masks = dict(m1=m["m1"].cuda(), m2=m["m2"].cuda(), l=m["l"].view(N * T, H).cuda())
    if mhb:
        masks["m3"] = m["m3"].cuda()
    model.set_keep_masks(**masks)
    idx = torch.tensor(INDEX, device="cuda") if shared else None
    return model, img.cuda(), counts.cuda(), q.cuda(), tgt.cuda(), idx


def _step(model, mhb, img, q, tgt, img_length=None, **kw):
    """one train step; img_length: the counts travel with the features, forward((img, img_length), q, ...)"""
    model.zero_grad(set_to_none=True)
    out = model.forward(img if img_length is None else (img, img_length), q, **kw)
    (torch.nn.KLDivLoss()(out, tgt) if mhb else torch.nn.CrossEntropyLoss()(out, tgt)).backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in model.named_parameters()}


MFB3, MFBM, MHB3 = MFB_CASES[2], MFB_CASES[4], MHBCOATT_CASES[1]
MODEL_RUNS = [
    pytest.param(MFB3, False, False, {}, False, id="mfb_unit_softmax"),
    pytest.param(MFB3, False, True, {}, False, id="mfb_unit_softmax_img_index"),
    pytest.param(MFB3, False, False, dict(unit_softmax=False), True, id="mfb_live_softmax"),
    pytest.param(MFB3, False, True, dict(unit_softmax=False, overlap_streams=False, fold_norm=False), True,
                 id="mfb_live_one_node_fold_norm_off_img_index"),
    pytest.param(MFBM, False, False, dict(unit_softmax=False, overlap_streams=False), True, id="mfb_multilayer_live_one_node"),
    pytest.param(MFBM, False, True, dict(unit_softmax=False, overlap_streams="same-stream"), True, id="mfb_multilayer_live_same_stream_img_index"),
    pytest.param(MHB3, True, False, {}, False, id="mhbcoatt_side_stream"),
    pytest.param(MHB3, True, True, {}, False, id="mhbcoatt_side_stream_img_index"),
    pytest.param(MHB3, True, False, dict(overlap_streams="same-stream"), False, id="mhbcoatt_same_stream"),
    pytest.param(MHB3, True, True, dict(overlap_streams=False), False, id="mhbcoatt_one_node_img_index"),
    pytest.param(MHB3, True, False, dict(overlap_streams=False, fold_norm=False), False, id="mhbcoatt_one_node_fold_norm_off"),
]


@pytest.mark.parametrize("case,mhb,shared,attrs,live", MODEL_RUNS)
def test_model_with_img_length_matches_the_masked_reference(vqa, case, mhb, shared, attrs, live):
    model, img, counts, q, tgt, idx = _model(vqa, case, mhb, shared, **attrs)
    kw = dict(img_length=counts) if idx is None else dict(img_index=idx, img_length=counts)
    out, grads = _step(model, mhb, img, q, tgt, **kw)
    o_out, g32, g64 = _oracle(case, mhb, shared, live)
    err = rel_err(out.cpu().numpy(), o_out.numpy())
    print("img_length output rel err %.2e" % err)
    assert out.shape[0] == q.shape[0]
    assert err <= 1e-4
    grad_parity(grads, g32, g64, label="img_length %s %s%s" % (case["name"], attrs, " img_index" if shared else ""))
    if live or mhb:
        assert float(grads["img_conv1d.weight"].abs().max()) > 0.0
    # the int32 form of the counts is the same call
    out32, grads32 = _step(model, mhb, img, q, tgt, **dict(kw, img_length=counts.to(torch.int32)))
    assert torch.equal(out, out32) and all(torch.equal(grads[k], grads32[k]) for k in grads)
    # other finite values in the padded rows of img_features: the same bits everywhere
    pad = ~RR.valid_mask(counts.cpu(), img.shape[1]).cuda()
    img2 = torch.where(pad[:, :, None], torch.from_numpy(recipe.sym_tensor(tuple(img.shape), 5.0, 92)).cuda(), img)
    assert not torch.equal(img, img2)
    out2, grads2 = _step(model, mhb, img2, q, tgt, **kw)
    assert torch.equal(out, out2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    # counts beyond L and below 1 are clamped on the device
    big = torch.where(counts == img.shape[1], counts + 50, counts)
    out3, _ = _step(model, mhb, img, q, tgt, **dict(kw, img_length=big))
    assert torch.equal(out, out3)


@pytest.mark.parametrize("mhb,shared,attrs", [(False, False, {}), (False, True, dict(unit_softmax=False)), (True, False, {}), (True, True, {})],
                         ids=["mfb", "mfb_live_img_index", "mhbcoatt", "mhbcoatt_img_index"])
def test_eval_logits_do_not_depend_on_the_pad_width(vqa, mhb, shared, attrs):
    """eval mode (no dropout): L -> L + 5 more padded rows leaves every sample's logits within 1e-4 relative; the plain call on the
    padded tensor does depend on it."""
    model, img, counts, q, tgt, idx = _model(vqa, MHB3 if mhb else MFB3, mhb, shared, **attrs)
    model.set_keep_masks()
    model.eval()
    U, L, D = img.shape
    wide = torch.cat((img, torch.from_numpy(recipe.sym_tensor((U, 5, D), 2.0, 93)).cuda()), 1).contiguous()
    kw = {} if idx is None else dict(img_index=idx)
    with torch.no_grad():
        a = model.forward((img, counts), q, **kw)
        b = model.forward((wide, counts), q, **kw)
        c = model.forward(img, q, **kw)
    for n in range(a.shape[0]):
        assert rel_err(b[n].cpu().numpy(), a[n].cpu().numpy()) <= 1e-4, n
    assert rel_err(c.cpu().numpy(), a.cpu().numpy()) > 1e-4
    ids, probs = vqa.predict(model, (img, counts), q, **kw)
    assert torch.equal(ids[:, 0], a.argmax(1)) and not model.training


@pytest.mark.parametrize("shared", [False, True], ids=["per_sample", "img_index"])
def test_pruned_mfb_with_img_length_is_bit_identical_to_faithful(vqa, shared):
    res = []
    for pruned in (False, True):
        model, img, counts, q, tgt, idx = _model(vqa, MFB3, False, shared, pruned=pruned)
        kw = dict(img_length=counts) if idx is None else dict(img_index=idx, img_length=counts)
        res.append(_step(model, False, img, q, tgt, **kw))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_img_length_none_is_the_existing_path(vqa, ops):
    """(img, None) runs the code path of the call with the plain tensor: equal bits for the output and every gradient and the same
    launches, per kernel; the call with counts launches the same kernels (the region-count forms are instantiations of them)."""
    for mhb in (True, False):
        model, img, counts, q, tgt, _ = _model(vqa, MHB3 if mhb else MFB3, mhb, False, **({} if mhb else dict(unit_softmax=False)))
        loss = torch.nn.KLDivLoss() if mhb else torch.nn.CrossEntropyLoss()
        reports, res = [], []
        for form in ("positional", "none", "counts"):
            model.zero_grad(set_to_none=True)
            ops.prof_reset(); ops.prof_enable(True)
            if form == "positional":
                out = model.forward(img, q)
            elif form == "none":
                out = model.forward((img, None), q, None, True, None) if mhb else model.forward((img, None), q, True, None)
            else:
                out = model.forward((img, counts), q)
            loss(out, tgt).backward()
            torch.cuda.synchronize()
            reports.append({k: v[0] for k, v in ops.prof_report().items()}); ops.prof_enable(False)
            res.append((out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
        assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])
        assert reports[0] == reports[1]
        nfuse = 3 if mhb else 2                      # the image fusion and the final blocks' (N, 5000) launches
        assert reports[0].get("mfb_fuse_fwd", 0) == nfuse and reports[0].get("mfb_fuse_bwd", 0) == nfuse
        assert reports[2] == reports[0]
        assert not torch.equal(res[2][0], res[0][0])


def test_img_length_refusals(vqa):
    model, img, counts, q, tgt, idx = _model(vqa, MFB3, False, True)
    N = q.shape[0]
    for bad in (counts.cpu(), counts.float(), counts[:2], counts.view(-1, 1), COUNTS_SHARED, torch.ones(N, dtype=torch.int64, device="cuda")):
        with pytest.raises(vqa.VqfError, match="img_length"):
            model.forward((img, bad), q, img_index=idx)
    for bad in ((img,), (img, counts, counts), (COUNTS_SHARED, counts)):
        with pytest.raises(vqa.VqfError, match="img_length"):
            model.forward(bad, q, img_index=idx)
    with pytest.raises(vqa.VqfError, match="img_length"):
        model.forward((img[idx].contiguous(), counts), q)                        # without img_index: one count per sample
    for dt in ("bf16", "bf16-img", "bf16-all", "bf16-att"):
        model.gemm_dtype = dt
        with pytest.raises(vqa.VqfError, match="img_length is fp32 only"):
            model.forward((img[idx].contiguous(), counts[idx]), q)
    model.gemm_dtype = "bf16"
    with pytest.raises(vqa.VqfError, match="img_length is fp32 only"):
        model.forward((img[idx].to(torch.bfloat16).contiguous(), counts[idx]), q)
    mh, img, counts, q, tgt, _ = _model(vqa, MHB3, True, False, gemm_dtype="bf16")
    with pytest.raises(vqa.VqfError, match="img_length is fp32 only"):
        mh.forward((img, counts), q)
    with pytest.raises(vqa.VqfError, match="img_length"):
        mh.forward((img, counts.cpu()), q)
