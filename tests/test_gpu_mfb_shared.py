"""MFB / MHBCoAtt with shared images (forward(..., img_index)) on the GPU.

Kernel level: vqf_mfb_fuse_fwd_grouped / _bwd_grouped against an fp64 evaluation of the plain fusion on the gathered tensor
P[idx], over every element, with the criteria of test_gpu_kernels.test_mfb_fuse_fwd_bwd (1e-5 on Y / norm, 2e-5 on dP / dq /
dbias; well-conditioned operands: one sign per pooling window).  Model level: the oracle on img[idx] (output 1e-4, gradients
golden_util.grad_parity against the oracle's fp32 / fp64 pair), the project's criteria, unchanged.  The memory condition: the
shared path allocates no (N*L, 5000) tensor.
"""
import numpy as np
import pytest
import torch

import recipe
from cases import MFB_CASES, MHBCOATT_CASES, make_cfg
from golden_util import recipe_sd, rel_err, grad_parity
from oracle import ref_torch as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vqa():
    import vqa_amd
    vqa_amd.lib.load()
    return vqa_amd


@pytest.fixture(scope="module")
def ops(vqa):
    return vqa.ops


@pytest.fixture(scope="module")
def group_index(vqa):
    import importlib
    return importlib.import_module(vqa.__name__ + ".host.grouping")._group_index


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


def _ssqrt(s):
    return torch.sqrt(torch.relu(s)) - torch.sqrt(torch.relu(-s))


# (U, N, L, O, index)
KERNEL_SHAPES = [
    pytest.param(3, 7, 5, 1000, [2, 0, 0, 2, 0, 2, 0], id="U3_N7_image1_empty_unsorted"),
    pytest.param(1, 6, 3, 8, [0] * 6, id="U1_N6_O8_two_active_lanes"),
    pytest.param(5, 5, 20, 1000, [4, 3, 2, 1, 0], id="U5_N5_reversed_identity"),
    pytest.param(2, 11, 196, 1000, [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0], id="U2_N11_L196_group_of_9"),
]

_REF = {}


def _kernel_case(U, N, L, O, index, use_keep):
    """Operands and the fp64 reference, computed once per (shape, mask) and shared (never modified)."""
    key = (U, N, L, O, tuple(index), use_keep)
    if key in _REF:
        return _REF[key]
    W5 = 5 * O
    idx = torch.tensor(index)
    P = _pos((U * L, W5), 150).requires_grad_()
    pb = _pos((W5,), 157).requires_grad_()
    gsign = torch.sign(_rand((N, O), 156) + 1e-3).repeat_interleave(5, 1)
    q = (_pos((N, W5), 151) * gsign).requires_grad_()
    keep = (torch.rand((N * L, W5), generator=torch.Generator().manual_seed(153)) >= 0.1).to(torch.uint8) if use_keep else None
    Pg = (P + pb).view(U, L, W5)[idx].reshape(N * L, W5)                   # the gathered tensor the kernels never make
    z = Pg * q.repeat_interleave(L, 0)
    if use_keep:
        z = z * (keep.double() / (1.0 - np.float32(0.1).astype(np.float64)))
    R = _ssqrt(z.view(N * L, O, 5).sum(2))
    Y = torch.nn.functional.normalize(R.view(N, -1)).view(N * L, O)
    dY = _rand((N * L, O), 154)
    (Y * dY).sum().backward()
    _REF[key] = dict(P=P.detach(), pb=pb.detach(), q=q.detach(), keep=keep, Y=Y.detach(), norm=R.detach().view(N, -1).norm(dim=1),
                     dY=dY, dP=P.grad, dq=q.grad, db=pb.grad, idx=idx)
    return _REF[key]


@pytest.mark.parametrize("use_keep", [True, False], ids=["keep_p0.1", "no_dropout"])
@pytest.mark.parametrize("U,N,L,O,index", KERNEL_SHAPES)
def test_mfb_fuse_grouped_fwd_bwd(ops, group_index, U, N, L, O, index, use_keep):
    c = _kernel_case(U, N, L, O, index, use_keep)
    cu = lambda t: t.float().cuda()
    i32, order, off = group_index(c["idx"].cuda(), U)
    assert ops.mfb_fuse_grouped_supported(N, U, L, O)
    keep = None if c["keep"] is None else c["keep"].cuda()
    pd = 0.1 if use_keep else 0.0
    P, pb, q, dY = cu(c["P"]), cu(c["pb"]), cu(c["q"]), cu(c["dY"])
    Y, norm, inv = ops.mfb_fuse_fwd_grouped(P, q, i32, N, U, L, O, keep=keep, p_drop=pd, pbias=pb)
    e_y, e_n = _rel(Y, c["Y"]), _rel(norm, c["norm"])
    print("fwd grouped: Y %.2e norm %.2e" % (e_y, e_n))
    assert e_y <= 1e-5 and e_n <= 1e-5
    dP, dq, db = ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, q, i32, order, off, N, U, L, O, keep=keep, p_drop=pd,
                                          want_dbias=True, pbias=pb)
    e = (_rel(dP, c["dP"]), _rel(dq, c["dq"]), _rel(db, c["db"]))
    print("bwd grouped: dP %.2e dq %.2e dbias %.2e" % e)
    assert dP.shape == (U * L, 5 * O) and dq.shape == (N, 5 * O)
    assert max(e) <= 2e-5
    # an image without a question: exact zero rows
    for u in range(U):
        if u not in index:
            assert float(dP.view(U, L, -1)[u].abs().max()) == 0.0
    # fixed summation order: a second run gives the same bits
    dP2, dq2, db2 = ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, q, i32, order, off, N, U, L, O, keep=keep, p_drop=pd,
                                             want_dbias=True, pbias=pb)
    assert torch.equal(dP, dP2) and torch.equal(dq, dq2) and torch.equal(db, db2)
    # without the bias gradient (the other instantiation of the image-owned pass): the same dP and dq
    dP3, dq3, db3 = ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, q, i32, order, off, N, U, L, O, keep=keep, p_drop=pd, pbias=pb)
    assert db3 is None and torch.equal(dP, dP3) and torch.equal(dq, dq3)


@pytest.mark.parametrize("N,L,O,pd,seed", [(5, 20, 1000, 0.0, 0), (3, 196, 1000, 0.1, 77), (6, 3, 8, 0.1, 5), (2, 1, 1000, 0.0, 0)])
def test_identity_index_gives_the_plain_forward_bits(ops, N, L, O, pd, seed):
    P = _rand((N * L, 5 * O), 160).float().cuda()
    q = _rand((N, 5 * O), 161).float().cuda()
    pb = _rand((5 * O,), 162).float().cuda()
    ident = torch.arange(N, dtype=torch.int32, device="cuda")
    for keep in (None, (torch.rand((N * L, 5 * O), generator=torch.Generator().manual_seed(163)) >= 0.1).to(torch.uint8).cuda()):
        kw = dict(keep=keep, seed=seed, p_drop=0.1 if keep is not None else pd, pbias=pb)
        for normalise in (True, False):
            R0, n0, i0, _ = ops.mfb_fuse_fwd(P, q, N, L, O, normalise=normalise, **kw)
            R1, n1, i1 = ops.mfb_fuse_fwd_grouped(P, q, ident, N, N, L, O, normalise=normalise, **kw)
            assert torch.equal(R0, R1) and torch.equal(n0, n1) and torch.equal(i0, i1)
    # R and rowssq themselves, through the C ABI
    lib, ptr = ops._lib(), ops._ptr
    out = [torch.empty((N * L, O), device="cuda") for _ in range(2)]
    ssq = [torch.empty(N * L * 4, device="cuda") for _ in range(2)]
    assert lib.vqf_mfb_fuse_fwd(ptr(P), ptr(pb), ptr(q), None, None, seed, pd, N, L, O, ptr(out[0]), ptr(ssq[0]), None, ops._stream()) == 0
    assert lib.vqf_mfb_fuse_fwd_grouped(ptr(P), ptr(pb), ptr(q), ptr(ident), None, seed, pd, N, N, L, O, ptr(out[1]), ptr(ssq[1]),
                                        ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1]) and torch.equal(ssq[0], ssq[1])


def test_grouped_philox_mask_is_per_question_and_shared_by_both_directions(ops, group_index):
    """In-kernel Philox keyed on the QUESTION's flat element index: the forward equals the plain forward on the gathered tensor
    with the same seed, and the backward regenerates the same masks -- dP is zero exactly where every question of the image
    dropped the element."""
    U, N, L, O, seed = 3, 5, 7, 1000, 4321
    index = [2, 0, 2, 2, 0]                                                # image 1 without a question, a group of three
    P = torch.ones((U * L, 5 * O), device="cuda")
    q = torch.ones((N, 5 * O), device="cuda")
    i32, order, off = group_index(torch.tensor(index).cuda(), U)
    Pg = P.view(U, L, -1)[i32.long()].reshape(N * L, -1).contiguous()
    Y0, n0, i0, z = ops.mfb_fuse_fwd(Pg, q, N, L, O, seed=seed, p_drop=0.1, want_zdrop=True)
    Y, norm, inv = ops.mfb_fuse_fwd_grouped(P, q, i32, N, U, L, O, seed=seed, p_drop=0.1)
    assert torch.equal(Y, Y0) and torch.equal(norm, n0)
    kept = (z != 0).view(N, L, -1)
    assert abs(1.0 - kept.float().mean().item() - 0.1) < 5e-3
    dY = torch.ones_like(Y) + 0.5 * torch.rand(Y.shape, generator=torch.Generator().manual_seed(9)).cuda()
    dP, dq, _ = ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, q, i32, order, off, N, U, L, O, seed=seed, p_drop=0.1)
    any_kept = torch.zeros((U, L, 5 * O), dtype=torch.bool, device="cuda")
    for n, u in enumerate(index):
        any_kept[u] |= kept[n]
    nz = (dP != 0).view(U, L, -1)
    assert float(dP.view(U, L, -1)[1].abs().max()) == 0.0
    # (an element whose gradient coefficient is exactly 0 would also read as dropped: none is expected, a handful tolerated
    #  as test_mfb_fuse_philox_dropout does)
    assert torch.equal(nz, any_kept) or float((nz ^ any_kept).float().mean()) < 1e-3
    assert not bool((nz & ~any_kept).any())                                  # never a gradient where every question dropped
    dPg, dq0, _, _ = ops.mfb_fuse_bwd(dY, Y, norm, inv, Pg, q, N, L, O, seed=seed, p_drop=0.1)
    assert torch.equal(dq, dq0)                                              # the question-owned pass is the plain kernel
    ref = torch.zeros_like(dP).view(U, L, -1).index_add_(0, i32.long(), dPg.view(N, L, -1))
    assert _rel(dP, ref.view(U * L, -1)) <= 1e-6


def test_grouped_wrappers_refuse_bad_operands(vqa, ops, group_index):
    U, N, L, O = 3, 7, 5, 8
    z = lambda *s: torch.zeros(s, device="cuda")
    i32, order, off = group_index(torch.tensor([2, 0, 0, 2, 0, 2, 0]).cuda(), U)
    P, q = z(U * L, 5 * O), z(N, 5 * O)
    ops.mfb_fuse_fwd_grouped(P, q, i32, N, U, L, O)
    bad_fwd = [dict(idx=i32.cpu()), dict(idx=i32.long()), dict(idx=i32[:5]), dict(P=z(U * L, 10 * O)[:, ::2]), dict(P=z(N * L, 5 * O)),
               dict(q=z(N + 1, 5 * O))]
    for b in bad_fwd:
        a = dict(P=P, q=q, idx=i32)
        a.update(b)
        with pytest.raises(vqa.VqfError):
            ops.mfb_fuse_fwd_grouped(a["P"], a["q"], a["idx"], N, U, L, O)
    Y, norm, inv = ops.mfb_fuse_fwd_grouped(P, q, i32, N, U, L, O)
    dY = z(N * L, O)
    ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, P, q, i32, order, off, N, U, L, O)
    for b in (dict(idx=i32.cpu()), dict(order=order.long()), dict(order=order[:5]), dict(off=off[:U]), dict(P=z(U * L, 10 * O)[:, ::2]),
              dict(off=off.cpu())):
        a = dict(P=P, idx=i32, order=order, off=off)
        a.update(b)
        with pytest.raises(vqa.VqfError):
            ops.mfb_fuse_bwd_grouped(dY, Y, norm, inv, a["P"], q, a["idx"], a["order"], a["off"], N, U, L, O)
    with pytest.raises(vqa.VqfError):
        ops.mfb_fuse_fwd_grouped(z(U * L, 5 * 1028), z(N, 5 * 1028), i32, N, U, L, 1028)      # O above the envelope


# ---- model level -------------------------------------------------------------------------------------------------------------------
INDEX = [2, 0, 0, 2, 0, 2, 0]            # U = 3 images, N' = 2 * 3 + 1 questions, image 1 unused, unsorted
_ORACLE = {}


def _inputs(case, mhb):
    cfg = make_cfg(case)
    U, T, L, D, H = case["N"], case["T"], cfg.img_feature_dim, cfg.img_feature_channel, cfg.hidden_dim
    assert U == 3
    N = 2 * U + 1
    s = case["salt"]
    img = torch.from_numpy(recipe.img_features(U, L, D, s))
    q = torch.from_numpy(recipe.question_tokens(N, T, cfg.q_vocab_size, s))
    tgt = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, s) if mhb else recipe.hard_answers(N, cfg.a_vocab_size, s))
    ml = torch.from_numpy(recipe.keep_mask((N, T, H), 0.3, "l"))
    m1 = torch.from_numpy(recipe.keep_mask((N * L, 5000), 0.1, "m1"))
    m2 = torch.from_numpy(recipe.keep_mask((N, 5000), 0.1, "m2"))
    m3 = torch.from_numpy(recipe.keep_mask((N, 5000), 0.1, "m3"))
    return cfg, img, q, tgt, dict(l=ml, m1=m1, m2=m2, m3=m3), (N, T, L, H)


def _oracle(case, mhb, live=False):
    """(out32, g32, g64) of the oracle on img[idx] with the explicit masks; once per (case, mode)."""
    key = (case["name"], mhb, live)
    if key in _ORACLE:
        return _ORACLE[key]
    cfg, img, q, tgt, m, (N, T, L, H) = _inputs(case, mhb)
    idx = torch.tensor(INDEX)
    drop = dict(m1=m["m1"].view(N, L, 5000), m2=m["m2"], m3=m["m3"], l=m["l"].permute(1, 0, 2) if mhb else m["l"])
    res = []
    for dt in (torch.float32, torch.float64):
        sd = {k: v.to(dt).requires_grad_(True) for k, v in recipe_sd(O.mfb_shapes(cfg, mhb=mhb), case["salt"]).items()}
        if mhb:
            out = O.mhbcoatt_forward(sd, cfg, img[idx].to(dt), q, drop=drop)
            O.kldiv_loss(out, tgt.to(dt)).backward()
        else:
            out = O.mfb_forward(sd, cfg, img[idx].to(dt), q, drop=drop, live_softmax=live)
            O.ce_loss(out, tgt).backward()
        res.append((out.detach(), {k: v.grad for k, v in sd.items()}))
    _ORACLE[key] = (res[0][0], res[0][1], res[1][1])
    return _ORACLE[key]


def _model(vqa, case, mhb, **attrs):
    cfg, img, q, tgt, m, (N, T, L, H) = _inputs(case, mhb)
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
    return model, img.cuda(), q.cuda(), tgt.cuda()


def _step(model, mhb, img, q, tgt, img_index):
    model.zero_grad(set_to_none=True)
    out = model.forward(img, q, img_index=img_index)
    (torch.nn.KLDivLoss()(out, tgt) if mhb else torch.nn.CrossEntropyLoss()(out, tgt)).backward()
    torch.cuda.synchronize()
    return out.detach(), {k: p.grad for k, p in model.named_parameters()}


MODEL_RUNS = [
    pytest.param(MFB_CASES[2], False, {}, False, id="mfb_small_n3"),
    pytest.param(MFB_CASES[4], False, {}, False, id="mfb_multilayer_small_n3"),
    pytest.param(MHBCOATT_CASES[1], True, {}, False, id="mhbcoatt_small_n3_side_stream"),
    pytest.param(MHBCOATT_CASES[1], True, dict(overlap_streams="same-stream"), False, id="mhbcoatt_same_stream"),
    pytest.param(MHBCOATT_CASES[1], True, dict(overlap_streams=False), False, id="mhbcoatt_one_node"),
    pytest.param(MHBCOATT_CASES[1], True, dict(fold_norm=False), False, id="mhbcoatt_fold_norm_off"),
    pytest.param(MFB_CASES[2], False, dict(unit_softmax=False), True, id="mfb_live_softmax"),
    pytest.param(MFB_CASES[2], False, dict(unit_softmax=False, overlap_streams=False, fold_norm=False), True,
                 id="mfb_live_softmax_one_node_fold_norm_off"),
    pytest.param(MFB_CASES[4], False, dict(unit_softmax=False, overlap_streams="same-stream"), True, id="mfb_multilayer_live_same_stream"),
]


@pytest.mark.parametrize("case,mhb,attrs,live", MODEL_RUNS)
def test_model_with_img_index_matches_the_oracle_on_gathered_images(vqa, case, mhb, attrs, live):
    model, img, q, tgt = _model(vqa, case, mhb, **attrs)
    idx = torch.tensor(INDEX, device="cuda")
    out, grads = _step(model, mhb, img, q, tgt, idx)
    o_out, g32, g64 = _oracle(case, mhb, live)
    err = rel_err(out.cpu().numpy(), o_out.numpy())
    print("img_index output rel err %.2e" % err)
    assert out.shape[0] == len(INDEX)
    assert err <= 1e-4
    grad_parity(grads, g32, g64, label="img_index %s %s" % (case["name"], attrs))
    if live or mhb:
        assert float(grads["img_conv1d.weight"].abs().max()) > 0.0
    # the int32 form of the index is the same call
    out32, grads32 = _step(model, mhb, img, q, tgt, idx.to(torch.int32))
    assert torch.equal(out, out32) and all(torch.equal(grads[k], grads32[k]) for k in grads)


def test_model_index_shapes_n_below_u_and_singletons(vqa):
    """N < U (most images unused), the identity and a permutation: each equals the model on the gathered tensor, which runs the
    plain kernels (1e-5: the fusion's bits are equal, only the pooling kernels differ)."""
    case = MHBCOATT_CASES[1]
    model, img, q, tgt = _model(vqa, case, True)
    model.set_keep_masks()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    for index in ([1, 1], [0, 1, 2], [2, 0, 1], [1]):
        n = len(index)
        idx = torch.tensor(index, device="cuda")
        with torch.no_grad():
            a = model.forward(img, q[:n], img_index=idx)
            b = model.forward(img[idx].contiguous(), q[:n])
        assert a.shape == b.shape and rel_err(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5, index


def test_pruned_mfb_with_img_index_is_bit_identical_to_faithful(vqa):
    case = MFB_CASES[2]
    idx = torch.tensor(INDEX, device="cuda")
    res = []
    for pruned in (False, True):
        model, img, q, tgt = _model(vqa, case, False, pruned=pruned)
        res.append(_step(model, False, img, q, tgt, idx))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        a, b = res[0][1][k], res[1][1][k]
        assert torch.equal(a, b), k


def test_img_index_none_is_the_existing_path(vqa, ops):
    """img_index=None runs the code path of the call without the argument: equal bits for the output and every gradient, the
    same launches, and none of the grouped kernels."""
    case = MHBCOATT_CASES[1]
    model, img, q, tgt = _model(vqa, case, True)
    imgg = img[torch.tensor(INDEX, device="cuda")].contiguous()
    reports = []
    res = []
    for form in ("positional", "none"):
        model.zero_grad(set_to_none=True)
        ops.prof_reset(); ops.prof_enable(True)
        out = model.forward(imgg, q) if form == "positional" else model.forward(imgg, q, None, True, None)
        torch.nn.KLDivLoss()(out, tgt).backward()
        torch.cuda.synchronize()
        reports.append({k: v[0] for k, v in ops.prof_report().items()}); ops.prof_enable(False)
        res.append((out.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])
    assert reports[0] == reports[1]
    assert reports[1].get("mfb_fuse_bwd_image", 0) == 0 and reports[1].get("row_block_gather", 0) == 0
    # and the shared call does launch them
    ops.prof_reset(); ops.prof_enable(True)
    model.zero_grad(set_to_none=True)
    out = model.forward(img, q, img_index=torch.tensor(INDEX, device="cuda"))
    torch.nn.KLDivLoss()(out, tgt).backward()
    torch.cuda.synchronize()
    rep = {k: v[0] for k, v in ops.prof_report().items()}; ops.prof_enable(False)
    assert rep.get("mfb_fuse_bwd_image", 0) == 1 and rep.get("mfb_fuse_fwd", 0) == 3 and rep.get("mfb_fuse_bwd", 0) == 3


def test_img_index_refusals(vqa):
    case = MFB_CASES[2]
    model, img, q, tgt = _model(vqa, case, False)
    idx = torch.tensor(INDEX, device="cuda")
    for bad in (idx.cpu(), idx.float(), idx[:5], idx.view(-1, 1), INDEX):
        with pytest.raises(vqa.VqfError, match="img_index"):
            model.forward(img, q, img_index=bad)
    for dt in ("bf16", "bf16-img", "bf16-all", "bf16-att"):
        model.gemm_dtype = dt
        with pytest.raises(vqa.VqfError, match="fp32 only"):
            model.forward(img, q, img_index=idx)
    model.gemm_dtype = "bf16"
    with pytest.raises(vqa.VqfError, match="fp32 only"):
        model.forward(img.to(torch.bfloat16), q, img_index=idx)
    mh, img, q, tgt = _model(vqa, MHBCOATT_CASES[1], True, gemm_dtype="bf16")
    with pytest.raises(vqa.VqfError, match="fp32 only"):
        mh.forward(img, q, img_index=idx)


def test_shared_path_allocates_no_per_question_projection(vqa):
    """U = 2, N = 16, L = 196, D = 96, Philox dropout: peak memory over forward + backward of MHBCoAtt.  The unshared path holds
    P and dP, two (N*L, 5000) fp32 tensors; the shared path holds U/N of that, so it must be lower by at least ONE such tensor."""
    case = dict(MHBCOATT_CASES[1], N=16, L=196, name="mem_n16")
    cfg = make_cfg(case)
    U, N, L, D = 2, 16, 196, cfg.img_feature_channel
    model = vqa.MHBCoAtt(cfg)
    sd = {k: torch.from_numpy(recipe.weight_for(k, tuple(v.shape), case["salt"])) for k, v in model.state_dict().items()}
    model.load_state_dict(sd)
    model = model.cuda().train()
    img = torch.from_numpy(recipe.img_features(U, L, D, case["salt"])).cuda()
    q = torch.from_numpy(recipe.question_tokens(N, case["T"], cfg.q_vocab_size, case["salt"])).cuda()
    soft = torch.from_numpy(recipe.soft_answers(N, cfg.a_vocab_size, case["salt"])).cuda()
    idx = torch.tensor([0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0], device="cuda")
    imgg = img[idx].contiguous()
    peak = {}
    for form in ("gathered", "shared", "gathered", "shared"):          # twice: workspaces and streams exist from the first round on
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(3)
        out = model.forward(img, q, img_index=idx) if form == "shared" else model.forward(imgg, q)
        torch.nn.KLDivLoss()(out, soft).backward()
        torch.cuda.synchronize()
        peak[form] = torch.cuda.max_memory_allocated() - base
        del out
    one = N * L * 5000 * 4
    print("peak bytes above the baseline: gathered %d, shared %d, one (N*L, 5000) fp32 tensor %d" % (peak["gathered"], peak["shared"], one))
    assert peak["shared"] <= peak["gathered"] - one
